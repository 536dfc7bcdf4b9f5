"""Per-group moments of the denoised expression on the MI355X: dcahip_group_moments alone against fp64, against what
predict writes (the same bits), its determinism and its argument checks; Engine.group_moments in both residency modes;
Autoencoder.group_stats end to end (reference: tests/_groups_ref.py).

Bars of the kernel test, derived, not fitted.  The sums are taken in double, whose rounding (2^-53 per addition) is far
below every bar, so the bars are those of the fp32 element value x:
  * DCAHIP_NLL_MSE: x is one fp32 product (a * sf, or a itself): |x - ref| <= 2^-24 |x|, held at
    |S1 - ref| <= 2^-23 sum |x| and |S2 - ref| <= 2^-22 sum x^2;
  * otherwise expf (documented 1 ulp) and, with DCAHIP_GROUP_LOG1P, log1pf (2 ulp) come on top of the product; an ulp
    is at most 2^-23 relative and log1p does not amplify a relative error of its argument (x / ((1 + x) log1p x) <= 1):
    (1 + u) 2^-23 sum |x| on S1 and twice that on S2, u the summed ulp bounds (1 or 3).
The accumulators are ADDED to: `acc += S` rounds once at the accumulator's own magnitude, and the test, which preloads them
with small integers, adds half an ulp of the stored double to the bar of S."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine, run_single_step
from _groups_ref import MSE, NO_SF, LOG1P, elements, moments, abs_moments, two_pass_stats
from oracle import net_np as N

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


# ---------------------------------------------------------------------------------------------------- the kernel alone
# (B, G, lda, K): one element | the scalar path (lda % 4 != 0) | two 1024-gene segments with pad columns | a ragged last quad,
# an empty group, a group of one row, a fifth of the rows in no group | many groups: one slice, no workspace | one group:
# the most slices
SHAPES = [(1, 1, 1, 1), (3, 5, 5, 2), (37, 1030, 1032, 3), (70, 2051, 2052, 5), (300, 260, 260, 130), (513, 8, 8, 1)]
FLAGS = [0, NO_SF, LOG1P, NO_SF | LOG1P, MSE, MSE | NO_SF]
_cases = {}


def _codes_for(shape, rng):
    B, G, ld, K = shape
    if K == 5:                                   # group 2 empty, group 4 a single row, 14 of 70 rows in no group, shuffled
        c = rng.choice([0, 1, 3], size=B).astype(np.int32)
        c[rng.permutation(B)[:B // 5]] = -1
        c[np.flatnonzero(c >= 0)[7]] = 4
        assert (c == 2).sum() == 0 and (c == 4).sum() == 1 and (c == -1).sum() == 14
        return c
    c = rng.integers(0, K, size=B).astype(np.int32)
    if B >= 30:
        c[rng.permutation(B)[:B // 10]] = -1
    return c


def _case(flags, shape):
    """Operands of one call (host, fp32) and the fp64 moments -- made once per (flags, shape)."""
    key = (flags, shape)
    if key not in _cases:
        B, G, ld, K = shape
        rng = np.random.default_rng(1000 * flags + B)
        am = rng.uniform(-4.0, 4.0, size=(B, G)).astype(np.float32)
        for v in (20.0, -20.0, 20.0, -20.0):                         # both clips of the mean activation
            am[rng.integers(0, B), rng.integers(0, G)] = v
        sf = rng.uniform(0.3, 3.0, size=B).astype(np.float32)
        codes = _codes_for(shape, rng)
        x = elements(flags, am, sf)
        s1, s2, n = moments(x, codes, K)
        a1, a2 = abs_moments(x, codes, K)
        _cases[key] = dict(am=am, sf=sf, codes=codes, s1=s1, s2=s2, n=n, a1=a1, a2=a2)
    return _cases[key]


def _base(K, ldg):
    """Known accumulator contents: small integers, none of them zero."""
    return (1 + (torch.arange(K)[:, None] + torch.arange(ldg)[None, :]) % 8).to(torch.float64).cuda()


def _call(ops, c, flags, shape, codes=None):
    B, G, ld, K = shape
    am = torch.full((B, ld), float('nan'), dtype=torch.float32)
    am[:, :G] = torch.from_numpy(c['am'])
    am = am.cuda()
    sf = torch.from_numpy(c['sf']).cuda()
    cd = torch.from_numpy(c['codes'] if codes is None else codes).cuda()
    ldg = G + 2
    s1, s2 = _base(K, ldg), _base(K, ldg) + 1.0
    ws = torch.full((ops.group_moments_workspace_doubles(B, G, K),), float('nan'), dtype=torch.float64, device='cuda')
    ops.group_moments(am, ld, None if flags & NO_SF else sf, cd, B, G, K, flags, s1, s2, ldg, ws)
    torch.cuda.synchronize()
    return s1, s2


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_ld%d_k%d' % s)
@pytest.mark.parametrize('flags', FLAGS)
def test_kernel_against_fp64(ops, flags, shape):
    B, G, ld, K = shape
    c = _case(flags, shape)
    s1, s2 = _call(ops, c, flags, shape)
    base = _base(K, G + 2)
    assert torch.equal(s1[:, G:], base[:, G:]) and torch.equal(s2[:, G:], base[:, G:] + 1.0)   # ldg > G: the pad is not touched
    d1, d2 = (s1 - base)[:, :G].cpu().numpy(), (s2 - base - 1.0)[:, :G].cpu().numpy()
    assert np.isfinite(d1).all() and np.isfinite(d2).all()           # the NaN pad columns / workspace reached nothing
    u = 0 if flags & MSE else (3 if flags & LOG1P else 1)
    bar1 = (1 + u) * 2.0 ** -23 * c['a1'] if u else 2.0 ** -23 * c['a1']
    bar2 = 2 * (1 + u) * 2.0 ** -23 * c['a2'] if u else 2.0 ** -22 * c['a2']
    e1, e2 = np.abs(d1 - c['s1']), np.abs(d2 - c['s2'])
    # the bars are those of S; `acc += S` itself rounds once at the accumulator's magnitude (base + S, up to 9 here): half an
    # ulp of the stored double, which a sum of squares near 1e-10 (a clipped 1e-5 mean alone in its group) does feel.
    # (acc - base) is exact.
    r1 = 2.0 ** -53 * 2.0 ** np.floor(np.log2(np.abs(s1[:, :G].cpu().numpy())))     # |acc| in [2^k, 2^(k+1)): ulp 2^(k-52)
    r2 = 2.0 ** -53 * 2.0 ** np.floor(np.log2(np.abs(s2[:, :G].cpu().numpy())))
    print('flags %d %s: worst error / bar S1 %.3f, S2 %.3f (/ element bar alone: %.3f, %.3f)'
          % (flags, shape, (e1 / (bar1 + r1)).max(), (e2 / (bar2 + r2)).max(),
             (e1 / np.maximum(bar1, 1e-300))[c['n'] > 0].max(), (e2 / np.maximum(bar2, 1e-300))[c['n'] > 0].max()))
    assert (e1 <= bar1 + r1).all(), float((e1 / (bar1 + r1)).max())
    assert (e2 <= bar2 + r2).all(), float((e2 / (bar2 + r2)).max())
    empty = c['n'] == 0
    assert (d1[empty] == 0).all() and (d2[empty] == 0).all()            # an empty group keeps its accumulators


@pytest.mark.parametrize('flags', [0, NO_SF | LOG1P, MSE])
@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[4], SHAPES[5]], ids=lambda s: '%dx%d_ld%d_k%d' % s)
def test_kernel_is_deterministic(ops, flags, shape):
    c = _case(flags, shape)
    a1, a2 = _call(ops, c, flags, shape)
    b1, b2 = _call(ops, c, flags, shape)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)


@pytest.mark.parametrize('flags', [0, LOG1P])
@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3]], ids=lambda s: '%dx%d_ld%d_k%d' % s)
def test_nan_mean_reaches_the_sums_of_its_group_and_gene_only(ops, flags, shape):
    """One NaN pre-activation of the mean head at (row r, gene g), r in group k: the element is NaN, as it is in what
    heads_infer_kernel stores (the clip of mean_act keeps NaN, tests/test_heads_infer_gpu.py), so sum and sumsq are NaN at
    (k, g) and every other entry keeps the bits of the run without the NaN.  On the scalar and on the vector form, g the last
    gene (at 2051 the last valid column of a ragged quad)."""
    B, G, ld, K = shape
    c = _case(flags, shape)
    r = int(np.flatnonzero(c['codes'] >= 0)[-1])
    k, g = int(c['codes'][r]), G - 1
    am = c['am'].copy()
    am[r, g] = np.nan
    clean1, clean2 = _call(ops, c, flags, shape)
    nan1, nan2 = _call(ops, dict(c, am=am), flags, shape)
    hit = torch.zeros(K, G + 2, dtype=torch.bool, device='cuda')
    hit[k, g] = True
    for name, got, clean in (('sum', nan1, clean1), ('sumsq', nan2, clean2)):
        print('flags %d %s: %s[%d, %d] = %r (without the NaN %r)' % (flags, shape, name, k, g, got[k, g].item(), clean[k, g].item()))
        assert torch.equal(torch.isnan(got), hit), (name, got[k, g].item())
        assert torch.equal(got[~hit].view(torch.int64), clean[~hit].view(torch.int64)), name


@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[4]], ids=lambda s: '%dx%d_ld%d_k%d' % s)
def test_codes_outside_the_range_are_left_out(ops, shape):
    """A code of K, of 10^6 and of -7 behaves as -1 (the documented rule: such a row is in no group and its code is never an
    index)."""
    B, G, ld, K = shape
    c = _case(0, shape)
    rows = np.flatnonzero(c['codes'] >= 0)[[1, 5, 9, 13, 17, 21]]
    odd, out = c['codes'].copy(), c['codes'].copy()
    odd[rows] = [K, 10 ** 6, -7, K, 10 ** 6, -7]
    out[rows] = -1
    a1, a2 = _call(ops, c, 0, shape, codes=odd)
    b1, b2 = _call(ops, c, 0, shape, codes=out)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    r1, _ = _call(ops, c, 0, shape)
    assert not torch.equal(a1, r1)                                       # the rows were taken out of their groups


def test_kernel_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    L, p = hip.lib(), hip.ptr
    B, G, K = 3, 8, 2
    am = torch.zeros(B, G, dtype=torch.float32, device='cuda')
    sf = torch.ones(B, dtype=torch.float32, device='cuda')
    cd = torch.zeros(B, dtype=torch.int32, device='cuda')
    s1 = torch.full((K, G), 7.0, dtype=torch.float64, device='cuda')
    s2 = torch.full((K, G), 9.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(ops.group_moments_workspace_doubles(B, G, K), dtype=torch.float64, device='cuda')

    def call(B=B, G=G, K=K, am_=am, sf_=sf, cd_=cd, s1_=s1, s2_=s2, ws_=ws, lda=G, ldg=G, flags=0):
        return L.dcahip_group_moments(p(am_), lda, p(sf_), p(cd_), B, G, K, flags, p(s1_), p(s2_), ldg, p(ws_), hip.stream())
    assert call(B=0) == EINVAL and call(G=0) == EINVAL and call(K=0) == EINVAL and call(K=4097) == EINVAL
    assert call(am_=None) == EINVAL and call(cd_=None) == EINVAL and call(s1_=None) == EINVAL
    assert call(s2_=None) == EINVAL and call(ws_=None) == EINVAL and call(sf_=None) == EINVAL
    assert call(lda=G - 1) == EINVAL and call(ldg=G - 1) == EINVAL
    assert call(flags=MSE | LOG1P) == EINVAL and call(flags=MSE | LOG1P | NO_SF) == EINVAL
    q = L.dcahip_group_moments_workspace_doubles
    assert q(0, G, K) == 0 and q(B, 0, K) == 0 and q(B, G, 0) == 0 and q(B, G, 4097) == EINVAL
    assert q(4096, 20000, 16) > 0 and q(4096, 20000, 4096) > 0
    torch.cuda.synchronize()
    assert (s1 == 7.0).all() and (s2 == 9.0).all()
    assert call(sf_=None, flags=NO_SF) == 0                              # without the factor no sf is needed: runs
    torch.cuda.synchronize()
    assert (s1[0] == 7.0 + B).all() and (s1[1] == 7.0).all() and (s2[0] == 9.0 + B).all()      # exp(0) = 1, three rows of code 0


# ---------------------------------------------------------------------------------------------------- Engine.group_moments
HS = (12, 5, 12)


def _codes(n, K, seed=0):
    c = np.random.default_rng(seed).integers(0, K, size=n).astype(np.int32)
    c[::9] = -1
    return c


def test_engine_sums_the_same_bits_predict_writes(ops):
    """The sharp test: predict_chunk's fp32 `mean`, summed per group in float64 on the host, against Engine.group_moments --
    only the order of the double additions may differ (1e-12).  A kernel that restated the activation otherwise (another
    exp, a fused multiply) fails here and nowhere else."""
    n, G, ae, K = 150, 37, 'zinb-conddisp', 4
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    eng = make_engine(ops, ae, G, HS, True, 0.05, p, X, Y, sf)
    codes = _codes(n, K)
    eng.reserve(64)
    x = np.zeros((n, G))
    for s in range(0, n, 64):
        b = min(64, n - s)
        x[s:s + b] = eng.predict_chunk(s, b, {'mean'})['mean'].cpu().numpy().astype(np.float64)
    s1, s2, cnt = moments(x, codes, K)
    a1, a2 = abs_moments(x, codes, K)
    res = eng.group_moments(codes, K, chunk=64)
    torch.cuda.synchronize()
    assert res['sum'].is_cuda and res['sum'].dtype == res['sumsq'].dtype == torch.float64 and res['count'].dtype == torch.int64
    np.testing.assert_array_equal(res['count'].cpu().numpy(), cnt)
    e1, e2 = np.abs(res['sum'].cpu().numpy() - s1), np.abs(res['sumsq'].cpu().numpy() - s2)
    print('same bits: worst error / (1e-12 sum) S1 %.3g, S2 %.3g' % ((e1 / (1e-12 * a1)).max(), (e2 / (1e-12 * a2)).max()))
    assert (e1 <= 1e-12 * a1).all() and (e2 <= 1e-12 * a2).all()
    one = eng.group_moments(codes, K, chunk=150)                         # other chunks: other slices, the same sums
    assert (np.abs(one['sum'].cpu().numpy() - s1) <= 1e-12 * a1).all()
    assert (np.abs(one['sumsq'].cpu().numpy() - s2) <= 1e-12 * a2).all()
    again = eng.group_moments(torch.as_tensor(codes).cuda(), K, chunk=64)
    assert torch.equal(again['sum'], res['sum']) and torch.equal(again['sumsq'], res['sumsq'])


def test_engine_ragged_tail_with_more_slices_than_the_chunk(ops):
    """chunk = 100 rows take 50 slices of two rows, the 64-row tail 64 slices of one: the workspace is sized once, for the
    chunk, and the query is an upper bound that does not decrease with the rows (tests/test_groups_cpu.py), so the tail's
    partial sums fit.  Against predict's output, as above."""
    n, G, ae, K = 164, 37, 'zinb-conddisp', 4
    assert ops.group_moments_workspace_doubles(100, G, K) == ops.group_moments_workspace_doubles(64, G, K) == 2 * 64 * K * G
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    eng = make_engine(ops, ae, G, HS, True, 0.05, p, X, Y, sf)
    codes = _codes(n, K)
    eng.reserve(100)
    x = np.concatenate([eng.predict_chunk(s, min(100, n - s), {'mean'})['mean'].cpu().numpy().astype(np.float64)
                        for s in range(0, n, 100)])
    s1, s2, _ = moments(x, codes, K)
    a1, a2 = abs_moments(x, codes, K)
    res = eng.group_moments(codes, K, chunk=100)
    torch.cuda.synchronize()
    assert (np.abs(res['sum'].cpu().numpy() - s1) <= 1e-12 * a1).all()
    assert (np.abs(res['sumsq'].cpu().numpy() - s2) <= 1e-12 * a2).all()


@pytest.mark.parametrize('ae', ['normal', 'nb', 'zinb-shared'])
def test_engine_other_network_types(ops, ae):
    n, G, K = 150, 33, 3
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    eng = make_engine(ops, ae, G, HS, True, 0.0, p, X, Y, sf)
    eng.load_data(X, None, sf)                                           # no targets
    codes = _codes(n, K)
    eng.reserve(64)
    x = np.concatenate([eng.predict_chunk(s, min(64, n - s), {'mean'})['mean'].cpu().numpy().astype(np.float64)
                        for s in range(0, n, 64)])
    s1, s2, _ = moments(x, codes, K)
    a1, a2 = abs_moments(x, codes, K)
    res = eng.group_moments(codes, K, chunk=64)
    assert (np.abs(res['sum'].cpu().numpy() - s1) <= 1e-12 * a1).all()
    assert (np.abs(res['sumsq'].cpu().numpy() - s2) <= 1e-12 * a2).all()


def test_group_moments_leave_the_training_state_untouched(ops):
    n, G, ae = 150, 33, 'zinb-conddisp'
    X, Y, sf, p = make_problem(n, G, HS, ae, seed=6)
    rows = np.random.RandomState(1).permutation(n)[:32]
    out = []
    for grouped in (False, True):
        eng = make_engine(ops, ae, G, HS, True, 0.05, p, X, Y, sf)
        eng.set_optimizer('rmsprop')
        if grouped:
            before = (eng.w.clone(), eng.ms.clone(), eng.acc.clone(), eng.cursor.clone(), [m.clone() for m in eng.mm],
                      [m.clone() for m in eng.mv])
            eng.group_moments(_codes(n, 3), 3, chunk=64)
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


def test_counts_resident_group_moments_equal_the_dense_ones(ops, monkeypatch):
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
        res[form] = eng.group_moments(codes, K, log1p=True, no_sf=True, chunk=64)
        torch.cuda.synchronize()
        if form == 'counts':
            assert int(eng.gather_status.item()) == 0 and eng.X.shape[0] == 64 < n      # tiles, not the matrix
    monkeypatch.delenv('DCA_AMD_RESIDENT')
    for k in ('sum', 'sumsq', 'count'):
        assert torch.equal(res['dense'][k], res['counts'][k]), k
    assert float(res['dense']['sum'].abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------- end to end
def test_autoencoder_group_stats_end_to_end():
    """Autoencoder.group_stats(value='normalized', log1p=True) on the device against scipy's two-pass statistics of
    log1p(predict() / size factor) on the host.  eps = 6 * 2^-23 bounds the relative difference of the two element values
    (device: expf 1 ulp + log1pf 2 ulp, (1 + 3) ulp by the kernel test's rule; host route: predict's mean has 1 ulp of expf
    and half an ulp of the product, 1.5 -- together under 6).  Hence: mean to eps; variance to 4 eps rms(x) sd (its first
    order change under a perturbation d of the elements is 2 cov(x, d) <= 2 sd eps rms(x); a factor two to spare); the
    score to eps (|m1| + |m2|) / se + |t| times the larger relative variance bound."""
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G, K = 333, 530, 3
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
    x_before = np.array(ad.X, copy=True)
    assert net.group_stats(ad, 'cluster', value='normalized', log1p=True) is None
    np.testing.assert_array_equal(ad.X, x_before)
    d = ad.uns['dca_groups']
    assert list(d['names']) == ['k0', 'k1', 'k2'] and d['counts'].tolist() == [int((codes == k).sum()) for k in range(K)]
    sf = ad.obs['size_factors'].values.astype(np.float32).astype(np.float64)[:, None]
    x = np.log1p(np.asarray(net.predict(ad, copy=True).X, np.float64) / sf)
    ref = two_pass_stats(x, codes, K)
    eps = 6 * 2.0 ** -23
    assert (np.abs(d['mean'] - ref['mean']) <= eps * np.abs(ref['mean'])).all()
    inside = codes >= 0
    relvar = np.zeros((K, G))
    for k in range(K):
        for rows in (codes == k, inside & (codes != k)):
            v = x[rows].var(axis=0, ddof=1)
            relvar[k] = np.maximum(relvar[k], 4 * eps * np.sqrt((x[rows] ** 2).mean(axis=0)) / np.sqrt(v))
        rms, sd = np.sqrt((x[codes == k] ** 2).mean(axis=0)), np.sqrt(ref['var'][k])
        ev = np.abs(d['var'][k] - ref['var'][k])
        assert (ev <= 4 * eps * rms * sd).all(), float((ev / (4 * eps * rms * sd)).max())
        rest = inside & (codes != k)
        se = np.sqrt(ref['var'][k] / (codes == k).sum() + x[rest].var(axis=0, ddof=1) / rest.sum())
        tol = eps * (np.abs(ref['mean'][k]) + np.abs(x[rest].mean(axis=0))) / se + np.abs(ref['scores'][k]) * relvar[k]
        et = np.abs(d['scores'][k] - ref['scores'][k])
        print('group %d: worst variance error / bar %.3f, score error / bar %.3f' % (k, (ev / (4 * eps * rms * sd)).max(),
                                                                                    (et / tol).max()))
        assert (et <= tol).all(), float((et / tol).max())
    assert np.isfinite(d['pvals_adj']).all() and (d['pvals_adj'] >= d['pvals'] * (1 - 1e-12)).all() and (d['pvals_adj'] <= 1).all()
