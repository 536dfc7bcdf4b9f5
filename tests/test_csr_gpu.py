"""Sparse count matrices to the MI355X as CSR: dcahip_csr_expand through the C ABI, prep.upload_sparse, and every caller
(resident_counts, normalize_device, dca(), Engine.load_data) against the same matrix passed dense -- bit for bit, since
the device sees the same counts and every kernel after the upload is deterministic."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from dca_amd import io, prep
from dca_amd._anndata import AnnData

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _expand(ops, X, ld, Y=None):
    """One chunk: the whole CSR matrix X through ops.csr_expand into a NaN-filled [rows, ld] destination."""
    dev = torch.device('cuda')
    n, G = X.shape
    ip = torch.as_tensor(X.indptr.astype(np.int32), device=dev)
    ix = torch.as_tensor(X.indices.astype(np.int32), device=dev)
    vv = torch.as_tensor(np.asarray(X.data, dtype=np.float32), device=dev)
    if Y is None:
        Y = torch.full((n, ld), float('nan'), dtype=torch.float32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_expand(ip, ix, vv, X.nnz, n, G, Y, ld, st)
    torch.cuda.synchronize()
    return Y, int(st.item())


def _want(X, ld):
    n, G = X.shape
    w = np.zeros((n, ld), np.float32)
    w[:, :G] = np.asarray(X.toarray(), dtype=np.float32)
    return w


def _random_csr(n, G, density, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    d = (rng.random((n, G)) < density) * rng.integers(1, 500, (n, G))
    return sp.csr_matrix(d.astype(dtype))


@pytest.mark.parametrize('n,G', [(1, 1), (7, 5), (33, 203), (64, 1000), (5, 8064), (9, 20003), (3, 40001)])
def test_csr_expand_equals_toarray(ops, n, G):
    """G not a multiple of 4 (the scalar-store kernel), several LDS column segments (G > 8064), pad columns zero."""
    X = _random_csr(n, G, 0.07, n * 7 + G)
    for ld in sorted({G, (G + 3) // 4 * 4, G + 9}):
        Y, st = _expand(ops, X, ld)
        assert st == 0
        np.testing.assert_array_equal(_bits(Y), _want(X, ld).view(np.uint32))


def test_csr_expand_empty_rows_zero_matrix_dense_row_empty_chunk(ops):
    G = 9000
    X = _random_csr(40, G, 0.05, 3).tolil()
    X[[0, 5, 6, 39], :] = 0
    X[7, :] = np.arange(1, G + 1)                                # one fully dense row, across two segments
    X = X.tocsr()
    X.eliminate_zeros()
    for M in (X, sp.csr_matrix((12, G), dtype=np.float32), sp.csr_matrix((1, 3), dtype=np.float32)):
        Y, st = _expand(ops, M, (M.shape[1] + 3) // 4 * 4)
        assert st == 0
        np.testing.assert_array_equal(_bits(Y), _want(M, Y.shape[1]).view(np.uint32))
    # an empty chunk (no rows) launches nothing and touches nothing
    dev = torch.device('cuda')
    Y = torch.full((2, 8), float('nan'), device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_expand(torch.zeros(1, dtype=torch.int32, device=dev), None, None, 0, 0, 8, Y, 8, st)
    torch.cuda.synchronize()
    assert torch.isnan(Y).all() and int(st.item()) == 0


@pytest.mark.parametrize('src', [np.float64, np.int32, np.int64, np.float32])
def test_upload_sparse_in_several_chunks_equals_dense_upload(ops, src):
    X = _random_csr(300, 1001, 0.1, 5, dtype=src)
    X = X.multiply(1.0 + 1e-9).astype(src) if src == np.float64 else X   # fp64 values that round to fp32
    X = sp.csr_matrix(X)
    dev = torch.device('cuda')
    dense = prep._upload(np.asarray(X.toarray(), dtype=np.float32), dev)
    for nnz_cap, row_cap in ((1, 1), (2000, 7), (5000, 1000), (1 << 22, 1 << 14)):
        got = prep.upload_sparse(X, dev, ops, dense.shape[1], nnz_cap=nnz_cap, row_cap=row_cap)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(got), _bits(dense))
    # int64 indices / indptr (what scipy gives matrices beyond 2**31 entries) and a non-canonical matrix
    X64 = X.copy()
    X64.indices = X64.indices.astype(np.int64)
    X64.indptr = X64.indptr.astype(np.int64)
    np.testing.assert_array_equal(_bits(prep.upload_sparse(X64, dev, ops, dense.shape[1], nnz_cap=3000)), _bits(dense))


def test_upload_sparse_sums_duplicates_on_a_copy(ops):
    data = np.array([0.1, 0.2, 0.3, 1.0, 1e-9, 2.0, 0.7, 0.7], np.float64)
    indices = np.array([4, 1, 4, 0, 0, 3, 2, 2], np.int32)
    indptr = np.array([0, 3, 5, 5, 8], np.int32)
    X = sp.csr_matrix((data, indices, indptr), shape=(4, 6))
    before = [a.copy() for a in (X.data, X.indices, X.indptr)]
    got = prep.upload_sparse(X, torch.device('cuda'), ops, 8, nnz_cap=2)
    np.testing.assert_array_equal(_bits(got), _want(X, 8).view(np.uint32))
    for a, b in zip(before, (X.data, X.indices, X.indptr)):
        np.testing.assert_array_equal(a, b)


def _guarded(ops, indptr, indices, values, rows, G, ld, guard=3):
    """The kernel on a (possibly malformed) chunk, writing into rows guard .. guard + rows of one NaN-filled allocation:
    returns (status, the guard rows' bits untouched)."""
    dev = torch.device('cuda')
    buf = torch.full((rows + 2 * guard, ld), float('nan'), dtype=torch.float32, device=dev)
    ip = torch.as_tensor(np.asarray(indptr, np.int32), device=dev)
    ix = torch.as_tensor(np.asarray(indices, np.int32), device=dev)
    vv = torch.as_tensor(np.asarray(values, np.float32), device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.csr_expand(ip, ix, vv, len(indices), rows, G, buf[guard:guard + rows], ld, st)
    torch.cuda.synchronize()
    b = buf.cpu()
    return int(st.item()), bool(torch.isnan(b[:guard]).all() and torch.isnan(b[guard + rows:]).all()), b[guard:guard + rows]


# Every chunk below keeps all its arrays the lengths the call states; only the CONTENTS are wrong.  The kernel checks
# every index it is given before it reads or writes with it, so these can only be rejected.
@pytest.mark.parametrize('ld', [12, 10])
@pytest.mark.parametrize('case', ['column = G', 'column in the pad', 'column >= ld', 'column = INT32_MAX',
                                  'negative column', 'decreasing indptr', 'indptr > nnz', 'negative indptr'])
def test_malformed_chunks_are_reported_and_touch_nothing_outside_y(ops, case, ld):
    G = 9
    indptr = [0, 2, 4, 6]
    indices = [1, 3, 0, 8, 2, 5]
    values = [1, 2, 3, 4, 5, 6]
    if case == 'column = G':
        indices[3] = G
    elif case == 'column in the pad':
        indices[5] = 10 if ld > 10 else G
    elif case == 'column >= ld':
        indices[5] = ld + 100
    elif case == 'column = INT32_MAX':
        indices[5] = 2 ** 31 - 1
    elif case == 'negative column':
        indices[0] = -1
    elif case == 'decreasing indptr':
        indptr = [0, 4, 2, 6]
    elif case == 'indptr > nnz':
        indptr = [0, 2, 4, 1000]
    elif case == 'negative indptr':
        indptr = [0, -5, 4, 6]
    st, guards_ok, Y = _guarded(ops, indptr, indices, values, 3, G, ld)
    assert st > 0
    assert guards_ok
    assert not torch.isnan(Y).any()                    # every element of Y itself is written
    assert (Y[:, G:] == 0).all()                       # nothing lands in the pad


def test_malformed_sparse_matrix_raises(ops):
    dev = torch.device('cuda')
    bad_col = sp.csr_matrix((np.ones(3, np.float32), np.array([0, 7, 1], np.int32), np.array([0, 2, 3], np.int32)),
                            shape=(2, 5))                 # column 7 of a 5-column matrix (scipy does not check)
    with pytest.raises(ValueError, match='malformed'):
        prep.upload_sparse(bad_col, dev, ops, 8)
    neg_col = sp.csr_matrix((np.ones(2, np.float32), np.array([-1, 1], np.int32), np.array([0, 1, 2], np.int32)),
                            shape=(2, 5))
    with pytest.raises(ValueError, match='malformed'):
        prep.upload_sparse(neg_col, dev, ops, 8)
    bad_ptr = sp.csr_matrix((np.ones(3, np.float32), np.array([0, 1, 2], np.int32), np.array([0, 2, 3], np.int32)),
                            shape=(2, 5))
    bad_ptr.indptr = np.array([0, 3, 2], np.int32)
    with pytest.raises(ValueError, match='malformed'):
        prep.upload_sparse(bad_ptr, dev, ops, 8)


def _adata(X):
    n, G = X.shape
    return AnnData(X, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


def _formats(y):
    d = y.astype(np.float32)
    return {'csr': sp.csr_matrix(d), 'csc': sp.csc_matrix(d), 'coo': sp.coo_matrix(d)}


def test_resident_counts_sparse_equals_dense(ops):
    y = synth_counts(500, 301, 11)
    Yd, gd = prep.resident_counts(y.astype(np.float32), ops=ops)
    for name, X in _formats(y).items():
        Ys, gs = prep.resident_counts(X, ops=ops)
        np.testing.assert_array_equal(_bits(Ys), _bits(Yd), err_msg=name)
        np.testing.assert_array_equal(gs.view(np.uint32), gd.view(np.uint32), err_msg=name)


@pytest.mark.parametrize('fmt', ['csr', 'csc', 'coo'])
@pytest.mark.parametrize('filters', [True, False])
def test_normalize_device_sparse_equals_dense(ops, fmt, filters):
    y = synth_counts(400, 203, 12)
    if filters:
        y[:, [3, 17]] = 0
        y[[5, 44], :] = 0
    X = _formats(y)[fmt]
    if filters and fmt == 'coo':
        X = X.tocsr()                          # (the AnnData stand-in subsets rows / columns of indexable formats only)
    a, da = prep.normalize_device(io.read_dataset(_adata(y.astype(np.float32))), filter_min_counts=filters, ops=ops)
    # (read_dataset's count check slices rows: a COO matrix cannot be, in the reference's code either)
    b, db = prep.normalize_device(io.read_dataset(_adata(X), check_counts=fmt != 'coo'), filter_min_counts=filters,
                                  ops=ops)
    assert list(a.obs.index) == list(b.obs.index) and list(a.var.index) == list(b.var.index)
    np.testing.assert_array_equal(a.X.view(np.uint32), b.X.view(np.uint32))
    assert sp.issparse(b.raw.X)
    np.testing.assert_array_equal(a.raw.X, b.raw.X.toarray())
    for k in ('n_counts', 'size_factors'):
        np.testing.assert_array_equal(a.obs[k].values, b.obs[k].values)
    if filters:
        np.testing.assert_array_equal(a.var['n_counts'].values, b.var['n_counts'].values)
    for t in ('X', 'Y', 'sf'):
        np.testing.assert_array_equal(_bits(getattr(da, t)), _bits(getattr(db, t)), err_msg=t)


def _dca(X, batch_size):
    from dca_amd.api import dca
    ad = _adata(X)
    dca(ad, ae_type='zinb-conddisp', epochs=3, batch_size=batch_size, random_state=0, return_info=True)
    return ad


@pytest.mark.parametrize('batch_size', [32, 512])
def test_dca_on_csr_anndata_is_bit_identical_to_dense(batch_size):
    y = synth_counts(700, 150, 13)
    a = _dca(y.astype(np.float32), batch_size)
    b = _dca(sp.csr_matrix(y.astype(np.float32)), batch_size)
    np.testing.assert_array_equal(np.asarray(a.X).view(np.uint32), np.asarray(b.X).view(np.uint32))
    assert a.uns['dca_loss_history'] == b.uns['dca_loss_history']
    np.testing.assert_array_equal(a.raw.X, b.raw.X.toarray())


def test_dca_on_csr_never_densifies_on_the_host(monkeypatch):
    """The sparse counts reach the device without a dense host copy: every toarray / todense of scipy.sparse raises."""
    from scipy.sparse import _base, _compressed, _coo, _matrix

    def refuse(*a, **k):
        raise AssertionError('dense host copy of a sparse matrix')

    for cls in (_base._spbase, _compressed._cs_matrix, _coo._coo_base):
        monkeypatch.setattr(cls, 'toarray', refuse)
    for cls in (_base._spbase, _matrix.spmatrix):
        monkeypatch.setattr(cls, 'todense', refuse)
    y = synth_counts(300, 120, 14)
    X = sp.csr_matrix(y.astype(np.float32))
    with pytest.raises(AssertionError):
        X.toarray()
    ad = _dca(X, 32)
    assert np.isfinite(np.asarray(ad.X)).all() and sp.issparse(ad.raw.X)


def test_engine_load_data_sparse_equals_dense():
    from dca_amd.network import AE_types
    y = synth_counts(260, 97, 15).astype(np.float32)
    x = np.log1p(y)
    out_cols = np.array([1, 5, 6, 40, 96])
    sf = np.linspace(0.5, 2.0, 260).astype(np.float32)
    loaded = []
    for to in (np.asarray, sp.csr_matrix, sp.csc_matrix):
        net = AE_types['zinb-conddisp'](input_size=97, output_size=len(out_cols), hidden_size=(16, 4, 16))
        net.build()
        eng = net.engine
        eng.load_data(to(x), to(y[:, out_cols]), sf)
        torch.cuda.synchronize()
        loaded.append((_bits(eng.X), _bits(eng.Y), _bits(eng.sf)))
    for got in loaded[1:]:
        for g, w in zip(got, loaded[0]):
            np.testing.assert_array_equal(g, w)
    # sparse X with a dense Y, and the other way round
    for xx, yy in ((sp.csr_matrix(x), y[:, out_cols]), (x, sp.csr_matrix(y[:, out_cols]))):
        eng.load_data(xx, yy, sf)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(eng.X), loaded[0][0])
        np.testing.assert_array_equal(_bits(eng.Y), loaded[0][1])


def test_train_with_output_subset_on_sparse_raw_counts():
    """train(output_subset=...) feeds adata.raw.X[:, genes] (dca/train.py:85-87): with sparse raw counts that is a sparse
    matrix going through Engine.load_data.  Same loss history as the dense counts."""
    from dca_amd.network import AE_types
    from dca_amd.train import train
    y = synth_counts(400, 80, 16).astype(np.float32)
    genes = ['g3', 'g10', 'g11', 'g50', 'g79']
    hist = []
    for X in (y, sp.csr_matrix(y)):
        np.random.seed(0)                                # the per-epoch shuffles draw from numpy's global stream
        ad = io.normalize(io.read_dataset(_adata(X)))
        assert sp.issparse(ad.raw.X) == sp.issparse(X)
        net = AE_types['zinb-conddisp'](input_size=80, output_size=len(genes), hidden_size=(16, 4, 16))
        net.seed = 0
        net.build()
        h = train(ad, net, epochs=2, batch_size=32, output_subset=genes, verbose=False)
        assert np.isfinite(h.history['loss']).all()
        hist.append(h.history)
    assert hist[0] == hist[1]
