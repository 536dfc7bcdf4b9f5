"""Sparse count matrices on the host side (no GPU): the row-chunk plan and the packing of prep.upload_sparse, and Matrix
Market input (sc.read_mtx through dca/io.py:58-59) down to the CLI's result files."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.io
import scipy.sparse as sp

from conftest import synth_counts
from dca_amd import io, prep


def _check_plan(indptr, nnz_cap, row_cap):
    n = len(indptr) - 1
    chunks = prep.plan_csr_chunks(indptr, nnz_cap, row_cap)
    covered = []
    for r0, r1 in chunks:
        assert r1 > r0
        assert r1 - r0 <= row_cap
        nnz = int(indptr[r1]) - int(indptr[r0])
        assert nnz <= nnz_cap or r1 - r0 == 1, (r0, r1, nnz)
        covered.extend(range(r0, r1))
    assert covered == list(range(n))             # every row in exactly one chunk, in order
    return chunks


def test_plan_respects_caps_and_covers_every_row():
    rng = np.random.default_rng(0)
    lens = rng.integers(0, 50, 1000)
    lens[[3, 4, 5, 100, 999]] = 0                                   # empty rows
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int32)
    for nnz_cap, row_cap in ((100, 7), (49, 1000), (1, 1), (10 ** 6, 64), (10 ** 6, 10 ** 6)):
        _check_plan(indptr, nnz_cap, row_cap)
    assert prep.plan_csr_chunks(indptr, 10 ** 6, 10 ** 6) == [(0, 1000)]


def test_plan_gives_a_row_denser_than_the_cap_a_chunk_of_its_own():
    indptr = np.array([0, 2, 3, 503, 505, 505, 506], np.int64)
    chunks = _check_plan(indptr, 10, 100)
    assert (2, 3) in chunks
    assert prep.plan_csr_chunks(np.array([0, 0, 0, 0]), 5, 2) == [(0, 2), (2, 3)]   # all-empty rows: row cap only
    assert prep.plan_csr_chunks(np.array([0]), 5, 2) == []


def test_plan_takes_int64_indptr_beyond_int32():
    lens = np.full(12, 400_000_000, np.int64)              # 4.8e9 entries in all: offsets past 2**31
    indptr = np.r_[0, np.cumsum(lens)]
    assert indptr[-1] > 2 ** 31
    chunks = _check_plan(indptr, 1_000_000_000, 100)
    assert chunks == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12)]
    assert all(int(indptr[r1] - indptr[r0]) < 2 ** 31 for r0, r1 in chunks)


def _pack(X, r0, r1):
    m_max = int(X.indptr[r1] - X.indptr[r0])
    ip = np.full(r1 - r0 + 1, -7, np.int32)
    ix = np.full(max(m_max, 1), -7, np.int32)
    vv = np.full(max(m_max, 1), np.nan, np.float32)
    m = prep.pack_csr_chunk(X, r0, r1, ip, ix, vv)
    return ip, ix[:m], vv[:m]


def _expand(ip, ix, vv, G):
    """What dcahip_csr_expand computes, for canonical chunks (host check of the packing only)."""
    rows = len(ip) - 1
    out = np.zeros((rows, G), np.float32)
    for r in range(rows):
        out[r, ix[ip[r]:ip[r + 1]]] = vv[ip[r]:ip[r + 1]]
    return out


@pytest.mark.parametrize('vdtype', [np.float64, np.int64, np.int32, np.float32])
@pytest.mark.parametrize('idtype', [np.int32, np.int64])
def test_pack_converts_indices_and_values(vdtype, idtype):
    rng = np.random.default_rng(1)
    dense = (rng.random((40, 33)) < 0.2) * rng.integers(1, 300, (40, 33))
    dense = dense.astype(vdtype)
    if vdtype == np.float64:
        dense = dense * (1 + 1e-9)                              # values that round when cast to fp32
    X = sp.csr_matrix(dense)
    X.indices = X.indices.astype(idtype)
    X.indptr = X.indptr.astype(idtype)
    for r0, r1 in ((0, 40), (5, 17), (39, 40)):
        ip, ix, vv = _pack(X, r0, r1)
        assert ip[0] == 0 and ix.dtype == np.int32 and vv.dtype == np.float32
        want = np.asarray(X[r0:r1].toarray(), dtype=np.float32)
        np.testing.assert_array_equal(_expand(ip, ix, vv, 33), want)


def test_pack_makes_a_non_canonical_chunk_canonical_without_touching_the_callers_matrix():
    # rows with unsorted columns and duplicates whose fp64 sum rounds differently from the sum of fp32 values
    data = np.array([0.1, 0.2, 0.3, 1.0, 1e-9, 2.0, 0.7, 0.7], np.float64)
    indices = np.array([4, 1, 4, 0, 0, 3, 2, 2], np.int32)
    indptr = np.array([0, 3, 5, 5, 8], np.int32)
    X = sp.csr_matrix((data, indices, indptr), shape=(4, 6))
    assert not X.has_canonical_format
    before = [a.copy() for a in (X.data, X.indices, X.indptr)]
    ip, ix, vv = _pack(X, 0, 4)
    for a, b in zip(before, (X.data, X.indices, X.indptr)):
        np.testing.assert_array_equal(a, b)
    assert ip.tolist() == [0, 2, 3, 3, 5] and ix.tolist() == [1, 4, 0, 2, 3]
    np.testing.assert_array_equal(_expand(ip, ix, vv, 6), np.asarray(X.toarray(), dtype=np.float32))
    ip, ix, vv = _pack(X, 1, 4)                                  # a chunk in the middle
    np.testing.assert_array_equal(_expand(ip, ix, vv, 6), np.asarray(X[1:4].toarray(), dtype=np.float32))


def test_csr_capable_needs_sparse_input_a_gpu_and_the_kernel():
    import torch
    from oracle.cpu_ops import CpuRefOps
    X = sp.csr_matrix(np.eye(3, dtype=np.float32))

    class WithKernel:
        def csr_expand(self, *a):
            raise AssertionError

    assert prep.csr_capable(X, torch.device('cuda'), WithKernel())
    assert not prep.csr_capable(X.toarray(), torch.device('cuda'), WithKernel())
    assert not prep.csr_capable(X, torch.device('cpu'), WithKernel())
    assert not prep.csr_capable(X, torch.device('cuda'), CpuRefOps())        # the CPU suite keeps today's path


def test_read_mtx(tmp_path):
    y = synth_counts(30, 12, 2)
    y[:, 5] = 0
    plain = str(tmp_path / 'x.mtx')
    scipy.io.mmwrite(plain, sp.coo_matrix(y.astype(np.int64)))
    import gzip
    import shutil
    with open(plain, 'rb') as src, gzip.open(plain + '.gz', 'wb') as dst:
        shutil.copyfileobj(src, dst)
    for f in (plain, plain + '.gz'):
        a = io.read_dataset(f, check_counts=True)
        assert sp.issparse(a.X) and a.X.format == 'csr' and a.X.dtype == np.float32
        np.testing.assert_array_equal(a.X.toarray(), y.astype(np.float32))
        assert list(a.obs_names) == [str(i) for i in range(30)] and list(a.var_names) == [str(i) for i in range(12)]
        b = io.read_dataset(f, transpose=True, test_split=True)
        assert b.shape == (12, 30) and list(b.obs_names) == [str(i) for i in range(12)]
        assert (b.obs['dca_split'] == 'test').sum() == 2


@pytest.mark.parametrize('flags', [['--nosizefactors'], []])
def test_cli_on_mtx_writes_what_it_writes_for_the_same_tsv(tmp_path, flags):
    """The CLI on a .mtx file (gene x cell, as a TSV without -t) against the same counts as a TSV whose names are the
    numbers read_mtx gives.  Without size factors every host step does the same arithmetic on the sparse and the dense
    matrix: the files are identical.  With them, the host restatement of normalize_per_cell scales a sparse matrix by
    the fp64 reciprocal of the factors (as scanpy's sparse branch does) and divides a dense one in fp32: the inputs differ
    in the last bits, and two epochs later the means by far less than the tolerance of tests/test_prep_gpu.py."""
    from dca_amd.__main__ import main
    from dca_amd.network import override_ops
    from oracle.cpu_ops import CpuRefOps
    n, G = 70, 24
    y = synth_counts(n, G, 5).astype(np.int64)
    f_tsv = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T, index=[str(i) for i in range(G)], columns=[str(j) for j in range(n)]).to_csv(f_tsv, sep='\t')
    f_mtx = str(tmp_path / 'counts.mtx')
    scipy.io.mmwrite(f_mtx, sp.coo_matrix(y.T))                # gene x cell, as the CLI expects without -t
    means = []
    for f, out in ((f_tsv, 'res_tsv'), (f_mtx, 'res_mtx')):
        out = str(tmp_path / out)
        with override_ops(CpuRefOps):
            main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8'] + flags)
        m = pd.read_csv(os.path.join(out, 'mean.tsv'), sep='\t', index_col=0)
        assert m.shape == (G, n)
        assert list(m.index.astype(str)) == [str(i) for i in range(G)]
        assert list(m.columns.astype(str)) == [str(j) for j in range(n)]
        means.append(m.values)
    if flags:
        np.testing.assert_array_equal(means[0], means[1])
    else:
        np.testing.assert_allclose(means[0], means[1], rtol=5e-3, atol=1e-4)
