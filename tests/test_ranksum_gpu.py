"""The Wilcoxon rank-sum integers on the MI355X: dcahip_ranksum alone against tests/_ranksum_ref.rank_ref -- EQUALITY, no
tolerance: both sides are integers --, its invalid rows, its argument checks and its determinism; Engine.rank_sums on the
bits predict returns, in both residency modes; Autoencoder.group_stats(method='wilcoxon') end to end against
scipy.stats.mannwhitneyu."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine, run_single_step
from _ranksum_ref import rank_ref, order_of
from oracle import net_np as N

pytestmark = pytest.mark.gpu

EINVAL = -22
SENT = -777

# (g, n, ldx, K): the smallest case | .. | wave edges (63, 64, 65) | .. | many tiles | more rows than any grid | mostly empty
# groups | one row of the product's length
SHAPES = [(1, 1, 1, 1), (3, 2, 4, 2), (5, 63, 64, 3), (5, 64, 64, 3), (4, 65, 68, 2), (7, 1000, 1000, 5), (3, 4097, 4100, 4),
          (2, 20011, 20012, 7), (1500, 70, 72, 3), (2, 9000, 9000, 4096), (1, 70000, 70000, 16)]
FAMILIES = ['normal', 'ints', 'const', 'asc', 'desc', 'signed']
_SIGNED_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                         0x3F800000, 0x3F800001, 0xBF800000, 0xBF800001,           # differ in the lowest mantissa bit only
                         0x01234567, 0x21234567, 0x41234567, 0x61234567, 0xC1234567,   # differ in the top byte only
                         0x3F800100, 0x3F810000, 0xBF800100, 0xBF810000], dtype=np.uint32)
_cases = {}


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _values(family, g, n, rng):
    if family == 'normal':
        return rng.standard_normal((g, n)).astype(np.float32)
    if family == 'ints':                                   # runs of equal values that span tiles
        return rng.integers(0, 6, size=(g, n)).astype(np.float32)
    if family == 'const':
        return np.full((g, n), 1.5, np.float32)
    if family in ('asc', 'desc'):
        v = np.arange(n, dtype=np.float32) * 0.25 - 3.0
        return np.tile(v if family == 'asc' else v[::-1], (g, 1)).astype(np.float32)
    bits = rng.choice(_SIGNED_BITS, size=(g, n))
    some = rng.random((g, n)) < 0.25                       # a quarter of the cells: continuous values of both signs
    bits[some] = rng.standard_normal(int(some.sum())).astype(np.float32).view(np.uint32)
    return bits.view(np.float32)


def _codes_for(n, K, rng):
    """Random codes; from 30 cells on a tenth of the cells in no group; from K = 3 on group 1 is empty."""
    c = rng.integers(0, K, size=n).astype(np.int32)
    if K >= 3:
        c[c == 1] = 0
    if n >= 30:
        c[rng.permutation(n)[:n // 10]] = -1
    return c


def _modes(K):
    return sorted({-1, 0, K - 1} | ({1} if K >= 3 else set()))      # rest | ref 0 | ref K - 1 | ref = the empty group


def _case(family, shape):
    key = (family, shape)
    if key not in _cases:
        g, n, ldx, K = shape
        rng = np.random.default_rng(FAMILIES.index(family) * 100003 + n * 7 + K)
        x = _values(family, g, n, rng)
        order, gstart, counts = order_of(_codes_for(n, K, rng), K)
        _cases[key] = dict(x=x, order=order, gstart=gstart, counts=counts, ref={})
    return _cases[key]


def _ref(c, K, ref):
    if ref not in c['ref']:
        c['ref'][ref] = rank_ref(c['x'], c['order'], c['gstart'], K, ref)
    return c['ref'][ref]


def _run(ops, x, ldx, order, gstart, K, ref, pad=3):
    """One call: x [g, n] host fp32 goes into a [g, ldx] plane whose pad columns hold NaN, the plane sits inside a larger
    allocation; the outputs are preloaded with a sentinel, ldr = g + pad; the workspace holds garbage."""
    g, n = x.shape
    big = torch.full((g * ldx + 32,), float('nan'), dtype=torch.float32)
    plane = big[16:16 + g * ldx].view(g, ldx)
    plane[:, :n] = torch.from_numpy(np.ascontiguousarray(x))
    big = big.cuda()
    plane = big[16:16 + g * ldx].view(g, ldx)
    ldr = g + pad
    rank2 = torch.full((K, ldr), SENT, dtype=torch.int64, device='cuda')
    tie = torch.full((K, ldr), SENT, dtype=torch.int64, device='cuda')
    ws = torch.full((ops.ranksum_workspace_bytes(g, n),), 0xAB, dtype=torch.uint8, device='cuda')
    od = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).cuda()
    gs = torch.from_numpy(np.ascontiguousarray(gstart, dtype=np.int32)).cuda()
    ops.ranksum(plane, ldx, g, n, od, len(order), gs, K, ref, rank2, tie, ldr, ws)
    torch.cuda.synchronize()
    r2, t = rank2.cpu().numpy(), tie.cpu().numpy()
    assert (r2[:, g:] == SENT).all() and (t[:, g:] == SENT).all()          # columns >= g are not touched
    return r2[:, :g], t[:, :g]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_ld%d_k%d' % s)
@pytest.mark.parametrize('family', FAMILIES)
def test_kernel_equals_the_reference(ops, family, shape):
    g, n, ldx, K = shape
    c = _case(family, shape)
    for ref in _modes(K):
        want2, wantt = _ref(c, K, ref)
        got2, gott = _run(ops, c['x'], ldx, c['order'], c['gstart'], K, ref)
        np.testing.assert_array_equal(got2, want2, err_msg='rank2, ref %d' % ref)
        np.testing.assert_array_equal(gott, wantt, err_msg='tie, ref %d' % ref)
        if ref < 0 and len(c['order']):                      # the rank sums of all groups: 1 + 2 + .. + m, doubled
            m = len(c['order'])
            assert (got2.sum(axis=0) == m * (m + 1)).all()


@pytest.mark.parametrize('shape', [SHAPES[5], SHAPES[7]], ids=lambda s: '%dx%d_ld%d_k%d' % s)
def test_two_calls_give_equal_bits(ops, shape):
    g, n, ldx, K = shape
    c = _case('ints', shape)
    for ref in (-1, 0):
        a, b = _run(ops, c['x'], ldx, c['order'], c['gstart'], K, ref), _run(ops, c['x'], ldx, c['order'], c['gstart'], K, ref)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_no_labelled_cell_writes_zeros(ops):
    x = np.random.default_rng(0).standard_normal((3, 50)).astype(np.float32)
    for ref in (-1, 1):
        r2, t = _run(ops, x, 52, np.zeros(0, np.int32), np.zeros(4, np.int32), 3, ref)
        assert (r2 == 0).all() and (t == 0).all()


@pytest.mark.parametrize('shape', [SHAPES[4], SHAPES[6]], ids=lambda s: '%dx%d_ld%d_k%d' % s)
def test_nan_marks_its_row_alone_and_only_among_the_labelled_cells(ops, shape):
    g, n, ldx, K = shape
    c = _case('normal', shape)
    codes = np.full(n, -1)
    codes[c['order']] = np.repeat(np.arange(K), np.diff(c['gstart']))
    if (codes < 0).sum() == 0:                               # 65 cells: nobody is unlabelled yet
        codes[5] = -1
    order, gstart, _ = order_of(codes, K)
    free, used = int(np.flatnonzero(codes < 0)[0]), int(order[len(order) // 2])
    for ref in (-1, 0):
        clean = _run(ops, c['x'], ldx, order, gstart, K, ref)
        x = c['x'].copy()
        x[:, free] = np.nan                                   # a NaN in an unlabelled cell of every row: no effect
        same = _run(ops, x, ldx, order, gstart, K, ref)
        assert np.array_equal(same[0], clean[0]) and np.array_equal(same[1], clean[1])
        x[g - 1, used] = np.nan                               # a NaN in a labelled cell of the last row: that row is -1
        got = _run(ops, x, ldx, order, gstart, K, ref)
        for a, b in zip(got, clean):
            assert (a[:, g - 1] == -1).all() and np.array_equal(a[:, :g - 1], b[:, :g - 1])
        want = rank_ref(x, order, gstart, K, ref)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_an_order_entry_outside_the_cells_is_not_an_index(ops):
    """n and -1 in `order`: the rows are marked -1.  (The plane sits inside a larger allocation with pad columns, so the
    test is harmless for the device either way.)"""
    g, n, ldx, K = 4, 65, 68, 2
    c = _case('normal', (g, n, ldx, K))
    for bad in (n, -1, 10 ** 9):
        order = c['order'].copy()
        order[7] = bad
        for ref in (-1, 1):
            r2, t = _run(ops, c['x'], ldx, order, c['gstart'], K, ref)
            assert (r2 == -1).all() and (t == -1).all()


def test_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    L, p = hip.lib(), hip.ptr
    g, n, K, m = 3, 8, 2, 6
    x = torch.zeros(g, n, dtype=torch.float32, device='cuda')
    od = torch.arange(m, dtype=torch.int32, device='cuda')
    gs = torch.tensor([0, 3, 6], dtype=torch.int32, device='cuda')
    r2 = torch.full((K, g), SENT, dtype=torch.int64, device='cuda')
    t = torch.full((K, g), SENT, dtype=torch.int64, device='cuda')
    ws = torch.zeros(ops.ranksum_workspace_bytes(g, n), dtype=torch.uint8, device='cuda')

    def call(x_=x, ldx=n, g=g, n=n, od_=od, m=m, gs_=gs, K=K, ref=-1, r2_=r2, t_=t, ldr=g, ws_=ws):
        return L.dcahip_ranksum(p(x_), ldx, g, n, p(od_), m, p(gs_), K, ref, p(r2_), p(t_), ldr, p(ws_), hip.stream())
    assert call(x_=None) == EINVAL and call(gs_=None) == EINVAL and call(r2_=None) == EINVAL and call(t_=None) == EINVAL
    assert call(ws_=None) == EINVAL and call(od_=None) == EINVAL
    assert call(ldx=n - 1) == EINVAL and call(ldr=g - 1) == EINVAL and call(g=0) == EINVAL and call(n=0) == EINVAL
    assert call(m=-1) == EINVAL and call(m=n + 1) == EINVAL
    assert call(K=0) == EINVAL and call(K=4097) == EINVAL and call(ref=-2) == EINVAL and call(ref=K) == EINVAL
    assert call(n=2097152, ldx=2097152) == EINVAL
    q = L.dcahip_ranksum_workspace_bytes
    assert q(0, n) == EINVAL and q(g, 0) == EINVAL and q(g, 2097152) == EINVAL and q(g, 2097151) > 0
    assert q(20000, 68579) == q(512, 68579) and q(100000, 1000) == q(512, 1000)       # per workgroup, not per gene
    torch.cuda.synchronize()
    assert (r2 == SENT).all() and (t == SENT).all()
    assert call(od_=None, m=0) == 0                                      # no labelled cell needs no order: zeros
    torch.cuda.synchronize()
    assert (r2 == 0).all() and (t == 0).all()
    with pytest.raises(ValueError, match='4096'):
        ops.ranksum(x, n, g, n, od, m, gs, 4097, -1, r2, t, g, ws)
    with pytest.raises(ValueError, match='2097151'):
        ops.ranksum_workspace_bytes(g, 2097152)


# ---------------------------------------------------------------------------------------------------- Engine.rank_sums
HS = (12, 5, 12)


def _codes(n, K, seed=0):
    c = np.random.default_rng(seed).integers(0, K, size=n).astype(np.int32)
    c[::9] = -1
    return c


def _predicted(eng, n, chunk=64):
    """The fp32 matrix predict_chunk writes as 'mean', gene-major."""
    eng.reserve(chunk)
    x = np.concatenate([eng.predict_chunk(s, min(chunk, n - s), {'mean'})['mean'].cpu().numpy() for s in range(0, n, chunk)])
    return np.ascontiguousarray(x.T)


@pytest.mark.parametrize('ae', ['zinb-conddisp', 'normal', 'nb', 'zinb-shared'])
def test_engine_rank_sums_equal_the_reference_on_the_bits_predict_returns(ops, ae):
    """G = 21 in blocks of 7 genes with ragged chunks of 64 rows, against one block, against rank_ref on predict's bits."""
    n, G, K = 150, 21, 4
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    eng = make_engine(ops, ae, G, HS, True, 0.05 if ae.startswith('zinb') else 0.0, p, X, Y, sf)
    eng.load_data(X, None, sf)                                           # no targets
    codes = _codes(n, K)
    order, gstart, counts = order_of(codes, K)
    xt = _predicted(eng, n)
    for ref in (None, 2):
        want2, wantt = rank_ref(xt, order, gstart, K, -1 if ref is None else ref)
        one = eng.rank_sums(codes, K, reference=ref, chunk=150)
        blocks = eng.rank_sums(torch.as_tensor(codes).cuda(), K, reference=ref, gene_block=7, chunk=64)
        torch.cuda.synchronize()
        for res in (one, blocks):
            assert res['rank2'].is_cuda and res['rank2'].dtype == res['tie'].dtype == res['count'].dtype == torch.int64
            assert res['rank2'].shape == res['tie'].shape == (K, G)
            np.testing.assert_array_equal(res['count'].cpu().numpy(), counts)
            np.testing.assert_array_equal(res['rank2'].cpu().numpy(), want2)
            np.testing.assert_array_equal(res['tie'].cpu().numpy(), wantt)
    auto = eng.rank_sums(codes, K)                                       # the block size from the free memory: one block here
    np.testing.assert_array_equal(auto['rank2'].cpu().numpy(), rank_ref(xt, order, gstart, K, -1)[0])
    if ae != 'normal':
        sfd = np.asarray(sf, np.float32)
        lg = eng.rank_sums(codes, K, no_sf=True, log1p=True, gene_block=8, chunk=64)
        assert (lg['rank2'] >= 0).all() and int(lg['rank2'].sum()) == G * len(order) * (len(order) + 1)
        assert sfd.shape == (n,)


def test_rank_sums_leave_the_training_state_untouched(ops):
    n, G, ae = 150, 33, 'zinb-conddisp'
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    rows = np.random.RandomState(1).permutation(n)[:32]
    out = []
    for ranked in (False, True):
        eng = make_engine(ops, ae, G, HS, True, 0.05, p, X, Y, sf)
        eng.set_optimizer('rmsprop')
        if ranked:
            before = (eng.w.clone(), eng.ms.clone(), eng.acc.clone(), eng.cursor.clone(), [m.clone() for m in eng.mm],
                      [m.clone() for m in eng.mv])
            eng.rank_sums(_codes(n, 3), 3, gene_block=16, chunk=64)
            torch.cuda.synchronize()
            for a, b in zip(before, (eng.w, eng.ms, eng.acc, eng.cursor, eng.mm, eng.mv)):
                if isinstance(a, list):
                    assert all(torch.equal(x, y) for x, y in zip(a, b))
                else:
                    assert torch.equal(a, b)
        out.append(run_single_step(eng, rows))
    (l0, g0, p0), (l1, g1, p1) = out
    assert l0 == l1
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k


def test_counts_resident_rank_sums_equal_the_dense_ones(ops, monkeypatch):
    import scipy.sparse as sp
    from dca_amd import prep
    from dca_amd._anndata import AnnData
    from dca_amd.engine import Engine
    n, G, ae, K = 150, 33, 'zinb-conddisp', 3
    p = {k: np.asarray(v, np.float32) for k, v in N.init_params(ae, G, HS, batchnorm=True, seed=4).items()}
    codes = _codes(n, K)
    res = {}
    for form in ('dense', 'counts'):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        ad = AnnData(sp.csr_matrix(synth_counts(n, G, 11).astype(np.float32)),
                     obs=pd.DataFrame(index=['c%d' % i for i in range(n)]), var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
        ad, dd = prep.normalize_device(ad, filter_min_counts=False, ops=ops)
        assert (dd.csr is not None) == (form == 'counts')
        eng = Engine(ae, G, G, HS, True, 0.05, ops=ops)
        eng.set_params(p)
        if form == 'dense':
            eng.attach_device_data(dd.X, dd.Y, dd.sf, norm=dd.norm, compact=False)
        else:
            eng.attach_counts(dd.csr, dd.sf, dd.norm)
        res[form] = eng.rank_sums(codes, K, reference=1, log1p=True, no_sf=True, gene_block=20, chunk=64)
        torch.cuda.synchronize()
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    for k in ('rank2', 'tie', 'count'):
        assert torch.equal(res['dense'][k], res['counts'][k]), k
    assert int(res['dense']['rank2'].sum()) > 0


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('reference, tie_correct', [('rest', False), ('k1', True)])
def test_autoencoder_group_stats_wilcoxon_end_to_end(reference, tie_correct):
    """group_stats(method='wilcoxon') on the device against scipy.stats.mannwhitneyu on predict()'s matrix on the host: the
    device ranks the bits predict writes, so U is equal and z, p are float64 arithmetic on the same integers (1e-9)."""
    from scipy.stats import mannwhitneyu, norm
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G, K = 333, 130, 3
    np.random.seed(0)
    ad = AnnData(synth_counts(n, G, 4).astype(np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    ad = io.normalize(ad)
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    train(ad, net, epochs=2, early_stop=0, reduce_lr=0, verbose=False)
    codes = _codes(n, K)
    ad.obs['cluster'] = pd.Categorical([('k%d' % c) if c >= 0 else None for c in codes])
    assert net.group_stats(ad, 'cluster', reference=reference, method='wilcoxon', tie_correct=tie_correct) is None
    d = ad.uns['dca_groups']
    assert d['method'] == 'wilcoxon' and d['tie_correct'] is tie_correct
    x = np.asarray(net.predict(ad, copy=True).X, np.float32).astype(np.float64)
    inside = codes >= 0
    for k in range(K):
        if reference != 'rest' and k == 1:
            assert np.isnan(d['scores'][k]).all() and np.isnan(d['auroc'][k]).all()
            continue
        a = x[codes == k]
        b = x[inside & (codes != k)] if reference == 'rest' else x[codes == 1]
        U, pv = mannwhitneyu(a, b, use_continuity=False, method='asymptotic', axis=0)
        n1, n2 = len(a), len(b)
        np.testing.assert_array_equal(np.rint(2 * d['auroc'][k] * (n1 * n2)) / 2, U)       # U exactly: a multiple of 1 / 2
        if tie_correct:                                       # scipy always corrects for ties
            np.testing.assert_allclose(d['pvals'][k], pv, rtol=1e-9)
        else:                                                 # scanpy's formula: no tie term in the variance
            z = (U - n1 * n2 / 2) / np.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
            np.testing.assert_allclose(d['scores'][k], z, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(d['pvals'][k], 2 * norm.sf(np.abs(z)), rtol=1e-9)
