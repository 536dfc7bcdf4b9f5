"""K-SPLIT on the MI355X: dcahip_csr_thin against the numpy restatement of its draw (dca_amd.mcv.thin_counts_host, which
tests/test_mcv_cpu.py checks against its binomial moments), bit for bit; HipOps.csr_thin, split_counts and mcv() end to end.

The shapes (tests/_mcv_cases.py) are the smallest at which the kernel can go wrong:

  rows of 0, 1, 64, 65 and ~290 entries                ballot boundaries (one, exactly one, one + 1 entry, five ballots)
  counts of 1, 4, 5, 64, 65 and 100 000                Philox block boundary, the lane-sharing cut-off, the shared path
  explicit zeros in the input                          dropped from both parts
  first row (a count of 65) and last row (empty)       grid-stride edges
  n = 0, nnz = 0                                       an empty input returns 0

No test depends on where the kernel starts to share an entry between lanes: the host restatement knows no such line."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import _mcv_cases as C
from conftest import synth_counts
from _score_ref import oracle_score, assert_marginals_close
from dca_amd import io, mcv
from dca_amd._anndata import AnnData
from oracle import net_np as N

pytestmark = pytest.mark.gpu

EINVAL = -22
NAN_BYTE = 0xff                 # buffers handed over full of 0xff bytes: NaN as fp32, -1 as integers


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the cached cases are read-only)


def _poisoned(count, dtype):
    t = torch.empty(max(count, 1), dtype=dtype, device='cuda')
    t.view(torch.uint8).fill_(NAN_BYTE)
    return t


def _thin(ptr, idx, val, G, row_ids, threshold, seed, n=None, nnz=None, cap=None, **over):
    """One raw call of dcahip_csr_thin on host arrays: (rc, status, the six output tensors)."""
    from dca_amd import hip
    L, p = hip.lib(), hip.ptr
    n = len(ptr) - 1 if n is None else n
    nnz = len(idx) if nnz is None else nnz
    cap = nnz if cap is None else cap
    d = dict(indptr=_dev(ptr), indices=_dev(idx) if len(idx) else None, values=_dev(val) if len(val) else None,
             row_ids=None if row_ids is None else _dev(np.asarray(row_ids, np.int64)),
             pa=_poisoned(len(ptr), torch.int64), ia=_poisoned(cap, torch.int32), va=_poisoned(cap, torch.float32),
             pb=_poisoned(len(ptr), torch.int64), ib=_poisoned(cap, torch.int32), vb=_poisoned(cap, torch.float32),
             ws=_poisoned(int(L.dcahip_csr_thin_workspace_bytes(max(n, 0), max(nnz, 0))), torch.uint8),
             status=torch.zeros(1, dtype=torch.int32, device='cuda'))
    d.update(over)
    rc = L.dcahip_csr_thin(p(d['indptr']), p(d['indices']), p(d['values']), nnz, n, G, p(d['row_ids']), threshold, seed,
                           p(d['pa']), p(d['ia']), p(d['va']), p(d['pb']), p(d['ib']), p(d['vb']), cap, p(d['ws']),
                           p(d['status']), hip.stream())
    torch.cuda.synchronize()
    status = int(d['status'].item()) if d['status'] is not None else 0
    return rc, status, [d[k] for k in ('pa', 'ia', 'va', 'pb', 'ib', 'vb')]


def _assert_equals_host(out, ref, what):
    for k, name in enumerate(('indptr_a', 'indices_a', 'values_a', 'indptr_b', 'indices_b', 'values_b')):
        got = out[k].cpu().numpy()[:len(ref[k])]
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), (what, name)
    for k in (1, 2, 4, 5):                              # nothing behind a part's last entry was written
        tail = out[k].view(torch.uint8)[len(ref[k]) * 4:]
        assert bool((tail == NAN_BYTE).all()), (what, k)


@pytest.mark.parametrize('seed', [0, 2 ** 40 + 3])
@pytest.mark.parametrize('threshold', C.THRESHOLDS)
def test_kernel_equals_the_host_restatement(ops, threshold, seed):
    ptr, idx, val = C.csr()
    rc, status, out = _thin(ptr, idx, val, C.G, None, threshold, seed)
    assert rc == 0 and status == 0
    _assert_equals_host(out, C.host_split(threshold, seed), 'threshold %d seed %d' % (threshold, seed))


def test_kernel_takes_row_ids(ops):
    """A permuted subset of the rows with their cell ids draws what the whole matrix draws for those cells."""
    thr = C.THRESHOLDS[3]
    rows = list(dict.fromkeys(np.random.RandomState(1).permutation(C.N)[:97].tolist() + [7, 0, 299]))
    ptr, idx, val = C.take_rows(rows)
    rc, status, out = _thin(ptr, idx, val, C.G, rows, thr, 0)
    assert rc == 0 and status == 0
    _assert_equals_host(out, C.host_split(thr, 0, rows=rows), 'row ids')
    full = C.host_split(thr, 0)
    A = C.to_dense(*full[:3])
    got = C.to_dense(*(t.cpu().numpy()[:n] for t, n in zip(out[:3], (len(rows) + 1, int(out[0][-1]), int(out[0][-1])))))
    assert np.array_equal(got, A[rows])


def test_kernel_is_deterministic(ops):
    ptr, idx, val = C.csr()
    a = _thin(ptr, idx, val, C.G, None, C.THRESHOLDS[2], 9)[2]
    b = _thin(ptr, idx, val, C.G, None, C.THRESHOLDS[2], 9)[2]
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_kernel_empty_inputs(ops):
    none = np.zeros(0, np.int32), np.zeros(0, np.float32)
    rc, status, out = _thin(np.zeros(1, np.int64), *none, 5, None, 1 << 31, 0)         # n = 0: nothing is launched
    assert rc == 0 and status == 0 and bool((out[0].view(torch.uint8) == NAN_BYTE).all())
    rc, status, out = _thin(np.zeros(4, np.int64), *none, 5, None, 1 << 31, 0)         # three empty rows
    assert rc == 0 and status == 0
    assert out[0].tolist() == [0, 0, 0, 0] and out[3].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('bad', [0.5, -1.0, float(2 ** 25), float('nan')])
def test_bad_values_set_status_and_raise(ops, bad):
    from dca_amd.prep import CsrCounts
    ptr, idx, val = C.take_rows([0, 1, 2])
    val = val.copy()
    val[[3, 200]] = bad
    rc, status, out = _thin(ptr, idx, val, C.G, None, 1 << 31, 0)
    assert rc == 0 and status == 2
    with pytest.raises(ValueError, match='not counts'):
        ops.csr_thin(CsrCounts(_dev(ptr), _dev(idx), _dev(val), 3, C.G), None, 1 << 31, 0)


def test_malformed_csr_is_clamped_and_counted(ops):
    ptr, idx, val = (a.copy() for a in C.take_rows([0, 1, 2]))
    idx[5], idx[9] = -1, C.G                                      # two columns outside [0, G)
    ptr[3] = len(idx) + 1000                                      # the last row's end behind the arrays
    rc, status, out = _thin(ptr, idx, val, C.G, None, 1 << 31, 0)
    assert rc == 0 and status == 3
    pa, pb = out[0].cpu().numpy(), out[3].cpu().numpy()
    assert pa[0] == pb[0] == 0 and (np.diff(pa) >= 0).all() and (np.diff(pb) >= 0).all() and pa[3] <= len(idx) and pb[3] <= len(idx)


def test_argument_errors_launch_nothing(ops):
    ptr, idx, val = C.take_rows([0, 1, 2])

    def untouched(out):
        return all(bool((t.view(torch.uint8) == NAN_BYTE).all()) for t in out if t is not None)
    for kw in (dict(n=-1), dict(nnz=-1), dict(cap=-1), dict(G=0), dict(G=-3), dict(threshold=(1 << 32) + 1),
               dict(indptr=None), dict(indices=None), dict(values=None), dict(pa=None), dict(pb=None), dict(ia=None),
               dict(va=None), dict(ib=None), dict(vb=None), dict(ws=None), dict(status=None)):
        what = dict(kw)
        rc, _, out = _thin(ptr, idx, val, kw.pop('G', C.G), None, kw.pop('threshold', 1 << 31), 0, **kw)
        assert rc == EINVAL, what
        assert untouched(out), what
    rc, status, out = _thin(ptr, idx, val, C.G, None, 1 << 31, 0)                      # the same operands, complete: runs
    assert rc == 0 and status == 0 and not untouched(out[:1])


def test_workspace_query(ops):
    L = ops.L
    assert L.dcahip_csr_thin_workspace_bytes(5, 0) == 0 and L.dcahip_csr_thin_workspace_bytes(0, 0) == 0
    assert L.dcahip_csr_thin_workspace_bytes(5, 7) == 32 and L.dcahip_csr_thin_workspace_bytes(5, 1 << 33) == 1 << 35
    assert L.dcahip_csr_thin_workspace_bytes(-1, 7) == EINVAL and L.dcahip_csr_thin_workspace_bytes(5, -7) == EINVAL


# ---------------------------------------------------------------------------------------------------- the Python layers
def _adata(X, n, G):
    return AnnData(X, obs=pd.DataFrame(index=['c%d' % i for i in range(n)]), var=pd.DataFrame(index=['g%d' % i for i in range(G)]))


def test_ops_csr_thin_cuts_the_parts_to_their_size(ops):
    from dca_amd.prep import CsrCounts
    ptr, idx, val = C.csr()
    thr = C.THRESHOLDS[3]
    A, B = ops.csr_thin(CsrCounts(_dev(ptr), _dev(idx), _dev(val), C.N, C.G), None, thr, 0)
    ref = C.host_split(thr, 0)
    for part, r in ((A, ref[:3]), (B, ref[3:])):
        assert (part.n, part.G, part.nnz) == (C.N, C.G, len(r[1]))
        assert np.array_equal(part.indptr.cpu().numpy(), r[0]) and np.array_equal(part.indices.cpu().numpy(), r[1]) and \
            np.array_equal(part.values.cpu().numpy(), r[2])
    with pytest.raises(ValueError, match='threshold'):
        ops.csr_thin(A, None, (1 << 32) + 1, 0)


@pytest.mark.parametrize('form', ['sparse', 'dense'])
def test_split_counts_device_equals_host(ops, form):
    ptr, idx, val = C.csr()
    X = sp.csr_matrix((val.copy(), idx.copy(), ptr.copy()), shape=(C.N, C.G)) if form == 'sparse' else C.dense().astype(np.float32)
    fd, hd = mcv.split_counts(_adata(X, C.N, C.G), 0.8, seed=5, device=True)
    fh, hh = mcv.split_counts(_adata(X, C.N, C.G), 0.8, seed=5, device=False)
    for d, h in ((fd, fh), (hd, hh)):
        if form == 'sparse':
            assert np.array_equal(d.X.indptr, h.X.indptr) and np.array_equal(d.X.indices, h.X.indices) and \
                np.array_equal(d.X.data, h.X.data) and d.X.dtype == np.float32
        else:
            assert isinstance(d.X, np.ndarray) and np.array_equal(d.X, h.X)


def test_mcv_end_to_end_against_the_oracle():
    """mcv() on the device: the held-out likelihood of the fitted network, against the fp64 oracle on the fitted parameters,
    the held-out counts and the scaled size factors (the bars of tests/test_score_gpu.py)."""
    n, G, f, seed, hs = 200, 120, 0.8, 3, (16, 8, 16)
    ad = _adata(synth_counts(n, G, 8).astype(np.float32), n, G)
    res = mcv.mcv(ad, fraction=f, seed=seed, return_model=True, ae_type='zinb-conddisp', hidden_size=hs, epochs=2, verbose=False)
    net = res['model']
    # the evaluation set, by the documented recipe, on the host
    fit, held = mcv.split_counts(io.read_dataset(ad, copy=True), f, seed, device=False)
    genes = np.asarray(fit.X.sum(axis=0)).reshape(-1) > 0
    fit, held = fit[:, genes].copy(), held[:, genes].copy()
    cells = np.asarray(fit.X.sum(axis=1)).reshape(-1) > 0
    fit, held = fit[cells].copy(), held[cells].copy()
    assert (res['n_cells'], res['n_genes']) == fit.shape
    fit = io.normalize(fit, filter_min_counts=False)
    sf = np.asarray(fit.obs['size_factors'].values, np.float64) * ((1 - f) / f)
    p = {k: np.asarray(v, np.float64) for k, v in net.engine.get_params().items()}
    cell_ref, gene_ref = oracle_score(N.OracleAE('zinb-conddisp', p, hs, True, net.ridge), fit.X, held.X, sf)
    nn, GG = fit.shape
    assert_marginals_close(res['cell_nll'] * GG, res['gene_nll'] * nn, cell_ref, gene_ref, 'mcv')
    ref = cell_ref.sum() / (nn * GG)
    print('mcv_loss %.8f oracle %.8f rel %.2e' % (res['mcv_loss'], ref, abs(res['mcv_loss'] / ref - 1)))
    assert abs(res['mcv_loss'] - ref) <= 1e-5 * abs(ref)
