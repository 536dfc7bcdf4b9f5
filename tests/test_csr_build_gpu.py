"""Building and filtering the resident CSR on the MI355X: dcahip_csr_compress against the host route (scipy's compression
+ the CSR upload) and dcahip_csr_subset against the host subset + upload, all arrays bit for bit; normalize_device and dca()
in counts mode on a DENSE host matrix against the sparse one and the dense-resident run, with no scipy conversion of the
dense matrix and exactly one upload."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from test_csr_build_cpu import masks, matrix, np_compress, np_subset

from dca_amd import io, prep
from dca_amd._anndata import AnnData

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _same_bits(a, b, what=''):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.numel():
        w = torch.int64 if a.element_size() == 8 else torch.int32
        assert torch.equal(a.contiguous().view(w), b.contiguous().view(w)), what


def _same_csr(a, b):
    assert (a.n, a.G, a.nnz) == (b.n, b.G, b.nnz)
    for k in ('indptr', 'indices', 'values'):
        _same_bits(getattr(a, k), getattr(b, k), k)
    assert a.indptr.dtype == torch.int64 and a.indices.dtype == torch.int32 and a.values.dtype == torch.float32


def _count_compress_calls(ops, monkeypatch):
    calls = []
    real = ops.csr_compress
    monkeypatch.setattr(ops, 'csr_compress', lambda *a: (calls.append(a[2]), real(*a))[1], raising=False)
    return calls


# ---------------------------------------------------------------------------------------------------- csr_compress
SHAPES = [(60, 1001, 0.07), (40, 9001, 0.001), (24, 33001, 0.3), (1, 1, 1.0), (3000, 7, 1.0), (17, 64, 0.0),
          (33, 4100, 1.0)]


@pytest.mark.parametrize('dense_rows', [2048, 7, 1])
@pytest.mark.parametrize('n, G, density', SHAPES)
def test_upload_of_a_dense_matrix_equals_the_host_route(ops, monkeypatch, n, G, density, dense_rows):
    """Chunks of 2 048 rows (one chunk), of 7 (several, the last one short) and of ONE row (a row alone fills a chunk)."""
    X = matrix(n, G, density, seed=n + G)
    want = prep.upload_csr(sp.csr_matrix(X), DEV, ops)
    calls = _count_compress_calls(ops, monkeypatch)
    assert prep.compress_capable(X, DEV, ops)
    got = prep.upload_csr(X, DEV, ops, dense_rows=dense_rows)
    assert calls == [min(dense_rows, n - s) for s in range(0, n, dense_rows)]
    _same_csr(got, want)
    _same_csr(prep.upload_csr(X, DEV, ops, device_compress=False), want)
    assert len(calls) == -(-n // dense_rows)                # (the switch of the A/B: the host route, no kernel)


def test_a_matrix_of_zeros(ops):
    for X in (np.zeros((9, 130), np.float32), np.full((5, 77), -0.0, np.float32)):
        got = prep.upload_csr(X, DEV, ops, dense_rows=4)
        _same_csr(got, prep.upload_csr(sp.csr_matrix(X), DEV, ops))
        assert got.nnz == 0 and not got.indptr.any()


@pytest.mark.parametrize('dtype', [np.int16, np.int32, np.int64, np.uint8, bool])
def test_other_dtypes_on_the_device_route_equal_the_host_route(ops, monkeypatch, dtype):
    X = np.nan_to_num(matrix(50, 301, 0.2, 9), posinf=7).astype(dtype)
    if np.dtype(dtype).kind == 'i':
        X[2, 5] = -3
    if dtype == np.int64:
        X[4, 4] = 2 ** 40 + 1                               # rounds in fp32, on both routes alike
    calls = _count_compress_calls(ops, monkeypatch)
    got = prep.upload_csr(X, DEV, ops, dense_rows=16)
    assert len(calls) == 4
    _same_csr(got, prep.upload_csr(sp.csr_matrix(X), DEV, ops))


def test_float16_keeps_the_host_route_and_its_refusal(ops, monkeypatch):
    X = matrix(20, 33, 0.3, 2, special=False).astype(np.float16)
    calls = _count_compress_calls(ops, monkeypatch)
    with pytest.raises(ValueError, match='float16'):        # scipy.sparse does not take the dtype: as before
        prep.upload_csr(X, DEV, ops)
    assert calls == []


def test_float64_keeps_the_host_route_and_its_stored_zero(ops, monkeypatch):
    X = matrix(20, 33, 0.3, 2, special=False).astype(np.float64)
    X[3, 3] = 1e-60                                         # non-zero, 0.0f in fp32: a stored zero of the host route
    calls = _count_compress_calls(ops, monkeypatch)
    got = prep.upload_csr(X, DEV, ops)
    assert calls == []
    _same_csr(got, prep.upload_csr(sp.csr_matrix(X), DEV, ops))
    assert got.nnz == np.count_nonzero(X)


def _compress(ops, Xd, ld, rows, G, base, cap, pad=64):
    """The entry on its own, with guard words around every output."""
    guard_i, guard_f = -7777, -7777.0
    indptr = torch.full((rows + 1 + 2 * pad,), -5, dtype=torch.int64, device=DEV)
    indices = torch.full((cap + 2 * pad,), guard_i, dtype=torch.int32, device=DEV)
    values = torch.full((cap + 2 * pad,), guard_f, dtype=torch.float32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.csr_compress(Xd, ld, rows, G, base, indptr[pad:pad + rows + 1], indices[pad:pad + cap], values[pad:pad + cap], status)
    torch.cuda.synchronize()
    for t, g in ((indptr, -5), (indices, guard_i), (values, guard_f)):
        assert (t[:pad] == g).all() and (t[t.numel() - pad:] == g).all()
    return (indptr[pad:pad + rows + 1].cpu().numpy(), indices[pad:pad + cap].cpu().numpy(),
            values[pad:pad + cap].cpu().numpy(), int(status.item()))


@pytest.mark.parametrize('n, G, density', [(60, 1001, 0.07), (24, 33001, 0.3), (1, 1, 1.0), (300, 7, 1.0), (9, 1024, 0.5),
                                           (5, 1030, 1.0)])
@pytest.mark.parametrize('layout', ['ld=G', 'ld=r4(G)+8', 'shifted'])
def test_the_entry_with_every_row_layout_and_a_base_beyond_two_to_the_31(ops, n, G, density, layout):
    """ld = G (16-byte loads only when G is a multiple of 4), a padded ld whose pad columns hold NaNs (never interpreted),
    a matrix that starts 4 bytes off a 16-byte boundary; base = 2^31 + 12 345 on the indptr the chunk writes."""
    X = matrix(n, G, density, seed=G + n)
    ld = G if layout != 'ld=r4(G)+8' else prep._r4(G) + 8
    buf = torch.full((n * ld + 1,), float('nan'), dtype=torch.float32, device=DEV)
    off = 1 if layout == 'shifted' else 0
    Xd = buf[off:off + n * ld].view(n, ld)
    Xd[:, :G] = torch.from_numpy(X).to(DEV)
    base = 2 ** 31 + 12345
    ip, ix, v, bad = _compress(ops, Xd, ld, n, G, base, n * G)
    wp, wi, wv = np_compress(X, base)
    assert bad == 0
    np.testing.assert_array_equal(ip, wp)
    m = len(wi)
    np.testing.assert_array_equal(ix[:m], wi)
    np.testing.assert_array_equal(v[:m].view(np.uint32), wv.view(np.uint32))
    assert (ix[m:] == -7777).all()                          # nothing beyond the chunk's entries


def test_entries_beyond_the_capacity_are_counted_not_written(ops):
    X = np.arange(1, 41, dtype=np.float32).reshape(4, 10)
    ip, ix, v, bad = _compress(ops, torch.from_numpy(X).to(DEV), 10, 4, 10, 0, 25)
    assert bad == 15 and ip.tolist() == [0, 10, 20, 30, 40]
    np.testing.assert_array_equal(ix, (np.arange(25) % 10).astype(np.int32))
    np.testing.assert_array_equal(v, np.arange(1, 26, dtype=np.float32))


def test_arguments_the_entry_cannot_take(ops):
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    ip = torch.zeros(9, dtype=torch.int64, device=DEV)
    ix = torch.zeros(64, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    for ld, rows, G, base in ((7, 8, 8, 0), (8, 8, 0, 0), (8, 8, -1, 0), (8, 8, 8, -1), (40000, 70000, 40000, 0)):
        with pytest.raises(RuntimeError, match='-22'):
            ops.csr_compress(t, ld, rows, G, base, ip, ix, t, st)
    ops.csr_compress(t, 8, 0, 8, 0, ip, ix, t, st)          # no rows: nothing launched
    torch.cuda.synchronize()
    assert int(st.item()) == 0


# ---------------------------------------------------------------------------------------------------- csr_subset
def _host_subset_upload(ops, Xs):
    """upload_csr of the subset host matrix; a subset without columns (which no upload takes) straight from scipy."""
    S = sp.csr_matrix(Xs)
    if Xs.shape[1] > 0:
        return prep.upload_csr(S, DEV, ops)
    return prep.CsrCounts(torch.zeros(Xs.shape[0] + 1, dtype=torch.int64, device=DEV),
                          torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.float32, device=DEV),
                          Xs.shape[0], 0)


@pytest.mark.parametrize('n, G, density', [(60, 1001, 0.07), (24, 3301, 0.3), (50, 7, 1.0), (30, 40, 0.0), (700, 130, 0.6)])
def test_subset_equals_the_host_subset_and_upload(ops, n, G, density):
    """Row-only, column-only and both masks, the first / last row and column dropped, everything kept, nothing kept."""
    X = matrix(n, G, density, seed=G)
    csr = prep.upload_csr(sp.csr_matrix(X), DEV, ops)
    for rows, cols in masks(n, G, seed=n):
        Xs = X[rows] if rows is not None else X
        Xs = Xs[:, cols] if cols is not None else Xs
        got = prep.subset_csr(ops, csr, rows=rows, cols=cols)
        _same_csr(got, _host_subset_upload(ops, Xs))
        wp, wi, wv = np_subset(csr.indptr.cpu().numpy(), csr.indices.cpu().numpy(), csr.values.cpu().numpy(), n, G, rows, cols)
        np.testing.assert_array_equal(got.indptr.cpu().numpy(), wp)
        np.testing.assert_array_equal(got.indices.cpu().numpy(), wi)


def test_subset_of_a_compressed_dense_upload(ops):
    X = matrix(90, 2003, 0.1, 3)
    rows, cols = masks(90, 2003, 5)[2]
    got = prep.subset_csr(ops, prep.upload_csr(X, DEV, ops, dense_rows=32), rows=rows, cols=cols)
    _same_csr(got, prep.upload_csr(sp.csr_matrix(X[rows][:, cols]), DEV, ops))


def test_subset_counts_malformed_input_and_a_wrong_row_count(ops):
    X = matrix(12, 20, 0.5, 1, special=False)
    csr = prep.upload_csr(sp.csr_matrix(X), DEV, ops)
    bad = prep.CsrCounts(csr.indptr.clone(), csr.indices.clone(), csr.values, 12, 20)
    bad.indices[3] = 25                                      # a column outside [0, G)
    with pytest.raises(ValueError, match='malformed'):
        prep.subset_csr(ops, bad, rows=np.ones(12, bool))
    # the mask keeps 5 rows, the output was sized for 4
    keep = torch.zeros(12, dtype=torch.uint8, device=DEV)
    keep[:5] = 1
    out = (torch.zeros(5, dtype=torch.int64, device=DEV), torch.full((csr.nnz + 8,), -1, dtype=torch.int32, device=DEV),
           torch.zeros(csr.nnz + 8, dtype=torch.float32, device=DEV))
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.csr_subset(csr, keep, None, 4, out[0], out[1][:csr.nnz], out[2][:csr.nnz], torch.zeros(32, dtype=torch.int32, device=DEV),
                   st)
    torch.cuda.synchronize()
    assert int(st.item()) > 0 and (out[1][csr.nnz:] == -1).all()


# ---------------------------------------------------------------------------------------------------- K-PREP, dca()
def _adata(X):
    n, G = X.shape
    return AnnData(X, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                   var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


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
    return calls, real_csr, real_upload


def _host(x):
    return x.toarray() if sp.issparse(x) else np.asarray(x)


@pytest.mark.parametrize('filters', [True, False])
def test_normalize_device_in_counts_mode_on_a_dense_host_matrix(ops, monkeypatch, filters):
    """Zero-count genes and cells: with filter_min_counts the gene and the cell filter drop them, without it
    normalize_per_cell drops the cells.  One upload, no scipy conversion of the dense matrix, and the resident CSR, norm,
    size factors and the host AnnData of the sparse-host run and of the dense-resident run, bit for bit."""
    y = synth_counts(400, 203, 12).astype(np.float32)
    y[:, [0, 3, 17, 202]] = 0
    y[[0, 5, 44, 399], :] = 0
    calls, real_csr, real_upload = _count_calls(monkeypatch)
    S = real_csr(y)
    monkeypatch.setenv('DCA_AMD_RESIDENT', 'counts')
    a, da = prep.normalize_device(io.read_dataset(_adata(y.copy())), filter_min_counts=filters, ops=ops)
    assert calls == dict(dense_conversions=0, uploads=1)
    b, db = prep.normalize_device(io.read_dataset(_adata(S)), filter_min_counts=filters, ops=ops)
    monkeypatch.setenv('DCA_AMD_RESIDENT', 'dense')
    c, dc = prep.normalize_device(io.read_dataset(_adata(y.copy())), filter_min_counts=filters, ops=ops)
    assert da.csr is not None and db.csr is not None and dc.csr is None
    kept = y[y.sum(1) >= 1][:, y.sum(0) >= 1] if filters else y[y.sum(1) >= 1]
    assert a.X.shape == kept.shape and kept.shape[0] <= 396 and kept.shape[1] <= (199 if filters else 203)
    _same_csr(da.csr, db.csr)
    _same_csr(da.csr, real_upload(real_csr(kept), DEV, ops))
    for other, dd in ((b, db), (c, dc)):
        assert list(a.obs.index) == list(other.obs.index) and list(a.var.index) == list(other.var.index)
        np.testing.assert_array_equal(np.asarray(a.X).view(np.uint32), np.asarray(other.X).view(np.uint32))
        np.testing.assert_array_equal(_host(a.raw.X).view(np.uint32), _host(other.raw.X).astype(np.float32).view(np.uint32))
        assert list(a.obs.columns) == list(other.obs.columns) and list(a.var.columns) == list(other.var.columns)
        for k in a.obs.columns:
            np.testing.assert_array_equal(a.obs[k].values, other.obs[k].values, err_msg=k)
        for k in a.var.columns:
            np.testing.assert_array_equal(a.var[k].values, other.var[k].values, err_msg=k)
        _same_bits(da.sf, dd.sf, 'sf')
        assert da.norm['do_log'] == dd.norm['do_log']
        for k in ('fac', 'mean', 'std'):
            _same_bits(da.norm[k], dd.norm[k], k)
    np.testing.assert_array_equal(_host(a.raw.X), kept)


def _dca_counts(X, monkeypatch):
    from dca_amd.api import dca
    monkeypatch.setenv('DCA_AMD_RESIDENT', 'counts')
    ad = _adata(X)
    dca(ad, mode='denoise', epochs=3, return_info=True, random_state=1, verbose=False)
    return ad


def test_dca_in_counts_mode_on_a_dense_anndata_equals_the_sparse_one(ops, monkeypatch):
    y = synth_counts(400, 600, 12).astype(np.float32)
    calls, real_csr, _ = _count_calls(monkeypatch)
    compressed = _count_compress_calls(ops.__class__, monkeypatch)
    rd = _dca_counts(y.copy(), monkeypatch)
    assert calls == dict(dense_conversions=0, uploads=1) and len(compressed) == 1
    rs = _dca_counts(real_csr(y), monkeypatch)
    np.testing.assert_array_equal(np.asarray(rd.X).view(np.uint32), np.asarray(rs.X).view(np.uint32))
    assert sorted(rd.obsm) == sorted(rs.obsm)
    for k in rd.obsm:
        np.testing.assert_array_equal(np.asarray(rd.obsm[k]).view(np.uint32), np.asarray(rs.obsm[k]).view(np.uint32), err_msg=k)
    assert rd.uns['dca_loss_history'] == rs.uns['dca_loss_history']
