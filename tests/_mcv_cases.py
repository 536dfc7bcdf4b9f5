"""The test problem of K-SPLIT (tests/test_mcv_cpu.py, tests/test_mcv_gpu.py) and its host splits, made once.

M = RandomState(0).negative_binomial(0.3, 0.3 / 1.8, size=(300, 700)) with the shapes planted at which the kernel can go wrong:

  counts    M[7, 11] = 100 000 (the wave-shared path, 25 000 Philox blocks), M[0, 0] = 65 and M[1, 1] = 64 (either side of the
            lane-sharing cut-off), M[2, 2] = 5 (one molecule into a second Philox block); 1 and 4 occur throughout
  rows      3 and 299 empty (the last row: a grid-stride edge), row 5 cut to exactly 64 stored entries and row 6 to 65 (either
            side of one ballot), row 8 to 1; the other rows hold about 290 (five ballots, the last one ragged)
  zeros     a handful of explicit stored zeros, in rows 0, 4, 9 and in the otherwise empty row 3

86 043 stored entries, 411 019 molecules, 16 404 entries with y = 2."""
import numpy as np

THRESHOLDS = (0, 1, 1 << 31, int(0.8 * 2 ** 32), 2 ** 32 - 1, 2 ** 32)
N, G = 300, 700
ZERO_ROWS = (0, 0, 3, 3, 4, 9, 9)       # rows that get an explicit stored zero (at their first columns without a count)

_cache = {}


def dense():
    if 'M' not in _cache:
        M = np.random.RandomState(0).negative_binomial(0.3, 0.3 / 1.8, size=(N, G)).astype(np.int64)
        M[7, 11], M[0, 0], M[1, 1], M[2, 2] = 100000, 65, 64, 5
        M[3] = 0
        M[299] = 0
        for r, k in ((5, 64), (6, 65), (8, 1)):
            nz = np.nonzero(M[r])[0]
            assert len(nz) > k
            M[r, nz[k:]] = 0
        M.setflags(write=False)
        _cache['M'] = M
    return _cache['M']


def csr():
    """(indptr int64, indices int32, values float32) of the problem, the explicit zeros stored."""
    if 'csr' not in _cache:
        M = dense()
        S = M > 0
        for r in ZERO_ROWS:
            S[r, np.nonzero(~S[r])[0][0]] = True
        indptr = np.zeros(N + 1, np.int64)
        np.cumsum(S.sum(axis=1), out=indptr[1:])
        rows, cols = np.nonzero(S)
        out = (indptr, cols.astype(np.int32), M[rows, cols].astype(np.float32))
        for a in out:
            a.setflags(write=False)
        assert (np.diff(indptr)[[3, 5, 6, 8, 299]] == [2, 64, 65, 1, 0]).all()
        _cache['csr'] = out
    return _cache['csr']


def host_split(threshold, seed, rows=None):
    """thin_counts_host of the problem (of its rows `rows`, handed over with their row ids), cached and read-only."""
    from dca_amd.mcv import thin_counts_host
    key = (threshold, seed, None if rows is None else tuple(rows))
    if key not in _cache:
        ip, ix, v = csr() if rows is None else take_rows(rows)
        out = thin_counts_host(ip, ix, v, None if rows is None else np.asarray(rows, np.int64), threshold, seed)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def take_rows(rows):
    """The CSR of the given rows of the problem, in that order."""
    ip, ix, v = csr()
    pieces = [np.arange(ip[r], ip[r + 1]) for r in rows]
    sel = np.concatenate(pieces) if pieces else np.zeros(0, np.int64)
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(p) for p in pieces], out=ptr[1:])
    return ptr, ix[sel], v[sel]


def to_dense(ptr, idx, val, n=None, G_=G):
    n = len(ptr) - 1 if n is None else n
    D = np.zeros((n, G_), np.int64)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    D[rows, idx] = val.astype(np.int64)
    return D
