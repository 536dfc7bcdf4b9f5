"""Building and filtering the resident CSR, without a GPU: what dcahip_csr_compress and dcahip_csr_subset compute, restated
in numpy and held against scipy (what is a stored entry: -0.0, NaN, subnormals; empty rows; a dropped column that empties a
row), and the host route of prep.upload_csr / prep._normalize_counts, which ops without the new entries keep taking."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from test_counts_resident_cpu import CsrOps

from dca_amd import io, prep
from dca_amd._anndata import AnnData
from oracle.cpu_ops import CpuRefOps


# ---------------------------------------------------------------------------------------------------- the restatement
def np_compress(X, base=0):
    """dcahip_csr_compress of the fp32 rows X: (indptr int64 from base, indices int32, values fp32).  Stored: every bit
    pattern but +0.0 and -0.0."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    keep = (X.view(np.uint32) << np.uint32(1)) != 0
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64) + base
    cols = np.nonzero(keep)[1].astype(np.int32)            # row-major: rows in order, columns ascending
    return indptr, cols, X[keep]


def np_subset(indptr, indices, values, n, G, rows=None, cols=None):
    """dcahip_csr_subset: the kept rows in order, their kept entries in order, columns renumbered by the prefix sum of the
    column mask."""
    rows = np.ones(n, bool) if rows is None else np.asarray(rows, bool)
    cols = np.ones(G, bool) if cols is None else np.asarray(cols, bool)
    newcol = np.where(cols, np.cumsum(cols) - 1, -1)
    out_ptr, out_idx, out_val = [0], [], []
    for r in np.nonzero(rows)[0]:
        a, b = indptr[r], indptr[r + 1]
        c = newcol[indices[a:b]]
        out_idx.append(c[c >= 0])
        out_val.append(values[a:b][c >= 0])
        out_ptr.append(out_ptr[-1] + int((c >= 0).sum()))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)       # noqa: E731
    return np.asarray(out_ptr, np.int64), cat(out_idx, np.int32), cat(out_val, np.float32)


def matrix(n, G, density, seed, special=True):
    rng = np.random.default_rng(seed)
    X = (rng.integers(1, 40, (n, G)) * (rng.random((n, G)) < density)).astype(np.float32)
    if special and n * G >= 12:
        flat = X.reshape(-1)
        k = rng.choice(n * G, 6, replace=False)
        flat[k[0]] = -0.0
        flat[k[1]] = np.nan
        flat[k[2]] = np.float32(1e-42)                      # subnormal: stored
        flat[k[3]] = np.inf
        flat[k[4]] = -3.5
        flat[k[5]] = np.frombuffer(np.uint32(0x7fc01234).tobytes(), np.float32)[0]       # a NaN with a payload
    if n > 2:
        X[1] = 0.0                                          # an empty row
        X[n - 1] = np.arange(1, G + 1)                      # a full row
    return X


def same_csr(got, S):
    ip, ix, v = got
    S = sp.csr_matrix(S)
    S.sort_indices()
    np.testing.assert_array_equal(ip, S.indptr.astype(np.int64))
    np.testing.assert_array_equal(ix, S.indices.astype(np.int32))
    np.testing.assert_array_equal(v.view(np.uint32), S.data.astype(np.float32).view(np.uint32))


SHAPES = [(60, 1001, 0.07), (40, 9001, 0.001), (24, 33001, 0.3), (1, 1, 1.0), (3000, 7, 1.0), (17, 64, 0.0)]


@pytest.mark.parametrize('n, G, density', SHAPES)
def test_compress_restatement_stores_what_scipy_stores(n, G, density):
    X = matrix(n, G, density, seed=n + G)
    same_csr(np_compress(X), sp.csr_matrix(X))
    ip, _, _ = np_compress(X, base=2 ** 33 + 5)
    assert ip[0] == 2 ** 33 + 5 and ip[-1] - ip[0] == sp.csr_matrix(X).nnz


def test_minus_zero_is_dropped_and_nan_kept():
    X = np.array([[0.0, -0.0, np.nan, 2.0], [-0.0, -0.0, 0.0, 0.0]], np.float32)
    ip, ix, v = np_compress(X)
    assert ip.tolist() == [0, 2, 2] and ix.tolist() == [2, 3] and np.isnan(v[0]) and v[1] == 2.0
    same_csr((ip, ix, v), sp.csr_matrix(X))


def masks(n, G, seed):
    rng = np.random.default_rng(seed)
    some_r, some_c = rng.random(n) < 0.6, rng.random(G) < 0.6
    ends_r, ends_c = np.ones(n, bool), np.ones(G, bool)
    ends_r[[0, n - 1]] = False
    ends_c[[0, G - 1]] = False
    return [(some_r, None), (None, some_c), (some_r, some_c), (ends_r, ends_c), (np.ones(n, bool), np.ones(G, bool)),
            (np.zeros(n, bool), None), (None, np.zeros(G, bool)), (np.zeros(n, bool), np.zeros(G, bool))]


@pytest.mark.parametrize('n, G, density', [(60, 1001, 0.07), (24, 3301, 0.3), (50, 7, 1.0), (30, 40, 0.0)])
def test_subset_restatement_equals_the_host_subset(n, G, density):
    X = matrix(n, G, density, seed=G)
    ip, ix, v = np_compress(X)
    for rows, cols in masks(n, G, seed=n):
        Xs = X[rows] if rows is not None else X
        Xs = Xs[:, cols] if cols is not None else Xs
        same_csr(np_subset(ip, ix, v, n, G, rows, cols), sp.csr_matrix(Xs))


def test_a_dropped_column_empties_a_row():
    X = np.zeros((3, 5), np.float32)
    X[0, 2] = 4.0
    X[1, [0, 2, 4]] = [1.0, 2.0, 3.0]
    cols = np.array([1, 1, 0, 1, 1], bool)
    ip, ix, v = np_subset(*np_compress(X), 3, 5, None, cols)
    assert ip.tolist() == [0, 0, 2, 2] and ix.tolist() == [0, 3] and v.tolist() == [1.0, 3.0]


# ---------------------------------------------------------------------------------------------------- the host route stays
def _count_calls(monkeypatch):
    calls = dict(dense_conversions=0, uploads=0)
    real_csr, real_upload = sp.csr_matrix, prep.upload_csr

    def csr_matrix(*a, **kw):
        if a and isinstance(a[0], np.ndarray) and a[0].ndim == 2:
            calls['dense_conversions'] += 1
        return real_csr(*a, **kw)

    def upload_csr(*a, **kw):
        calls['uploads'] += 1
        return real_upload(*a, **kw)
    monkeypatch.setattr(sp, 'csr_matrix', csr_matrix)
    monkeypatch.setattr(prep, 'upload_csr', upload_csr)
    return calls, real_csr


def test_ops_without_the_entries_are_not_capable():
    X = matrix(10, 9, 0.5, 1)
    assert not hasattr(CsrOps(), 'csr_compress') and not hasattr(CsrOps(), 'csr_subset')
    assert not prep.compress_capable(X, torch.device('cpu'), CsrOps())
    assert not prep.compress_capable(X, torch.device('cuda'), CsrOps())

    class WithEntry(CsrOps):
        def csr_compress(self, *a):
            raise AssertionError('not on a CPU device')
    assert not prep.compress_capable(X, torch.device('cpu'), WithEntry())
    assert prep.compress_capable(X, torch.device('cuda'), WithEntry())
    # float64 can round a non-zero to 0.0f, which the host route keeps as a stored zero: it stays on the host route
    assert not prep.compress_capable(X.astype(np.float64), torch.device('cuda'), WithEntry())
    assert not prep.compress_capable(sp.csr_matrix(X), torch.device('cuda'), WithEntry())
    # scipy.sparse refuses float16: no host arrays to equal, the host route (and its refusal) stays
    assert not prep.compress_capable(X.astype(np.float16), torch.device('cuda'), WithEntry())
    for dt in (np.int16, np.int32, np.int64, np.uint8, bool):
        assert prep.compress_capable(np.nan_to_num(X, posinf=0).astype(dt), torch.device('cuda'), WithEntry())


def test_upload_csr_of_a_dense_matrix_keeps_the_host_route(monkeypatch):
    X = matrix(60, 101, 0.1, 4)
    calls, real_csr = _count_calls(monkeypatch)
    got = prep.upload_csr(X, torch.device('cpu'), CsrOps())
    assert calls['dense_conversions'] == 1                  # scipy compresses it, as before
    want = prep.upload_csr(real_csr(X), torch.device('cpu'), CsrOps())
    for k in ('indptr', 'indices', 'values'):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), k     # (bits: X holds NaNs)
    assert got.indptr.dtype == torch.int64 and got.indices.dtype == torch.int32 and got.values.dtype == torch.float32
    same_csr((got.indptr.numpy(), got.indices.numpy(), got.values.numpy()), real_csr(X))
    # a float64 non-zero that rounds to 0.0f is a stored zero of the host route
    Z = np.array([[1e-60, 2.0], [0.0, 0.0]])
    z = prep.upload_csr(Z, torch.device('cpu'), CsrOps())
    assert z.indptr.tolist() == [0, 2, 2] and z.values.tolist() == [0.0, 2.0]


def _adata(X):
    n, G = X.shape
    return AnnData(X, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


@pytest.mark.parametrize('sparse', [False, True])
def test_normalize_counts_without_csr_subset_uploads_after_every_filter(monkeypatch, sparse):
    y = synth_counts(50, 30, 1).astype(np.float32)
    y[:, [3, 17]] = 0
    y[[5, 44], :] = 0
    calls, real_csr = _count_calls(monkeypatch)
    ops, dev = CsrOps(), torch.device('cpu')
    ad = io.read_dataset(_adata(real_csr(y) if sparse else y.copy()))
    ad, dd = prep._normalize_counts(ad, True, True, True, True, ops, dev, True, None)
    assert calls['uploads'] == 3                            # the matrix, without the empty genes, without the empty cells
    assert calls['dense_conversions'] == (0 if sparse else 3)
    assert (dd.n, dd.G) == (48, 28) == ad.X.shape
    kept = y[np.ix_(y.sum(1) >= 1, y.sum(0) >= 1)]
    same_csr((dd.csr.indptr.numpy(), dd.csr.indices.numpy(), dd.csr.values.numpy()), real_csr(kept))
    # the AnnData is what the dense form leaves
    b, db = prep.normalize_device(io.read_dataset(_adata(y.copy())), ops=CpuRefOps(), device='cpu')
    np.testing.assert_array_equal(np.asarray(ad.X).view(np.uint32), np.asarray(b.X).view(np.uint32))
    raw = ad.raw.X.toarray() if sp.issparse(ad.raw.X) else ad.raw.X
    np.testing.assert_array_equal(raw, b.raw.X)
    for k in ('n_counts', 'size_factors'):
        np.testing.assert_array_equal(ad.obs[k].values, b.obs[k].values)
    np.testing.assert_array_equal(ad.var['n_counts'].values, b.var['n_counts'].values)
    assert torch.equal(dd.sf, db.sf)


def test_residency_does_not_count_the_nonzeros_of_a_dense_matrix(monkeypatch):
    def no_count(*a, **kw):
        raise AssertionError('a pass over the dense host matrix')
    monkeypatch.setattr(np, 'count_nonzero', no_count)
    X = matrix(10, 9, 0.5, 1)
    assert prep._nnz(X) == 0 and prep._nnz(sp.csr_matrix(X)) == sp.csr_matrix(X).nnz
    assert prep.residency(X, torch.device('cpu'), CsrOps(), mode='auto') == 'dense'
    assert prep.residency(X, torch.device('cpu'), CsrOps(), mode='counts') == 'counts'
