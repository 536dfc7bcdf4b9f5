"""Gene-gene correlation of the denoised expression without a GPU: the error bound of tests/_gram_ref.py on the reference's
own arithmetic, dca_amd.genecorr.corr_from_moments against np.corrcoef, the launch plan restated in tests/_gram_ref.py
against libdcahip.so's workspace query, and the Python layers (Engine.gene_gram, Autoencoder.gene_correlation,
top_partners, `dca --genecorr`) on the CPU oracle extended with gram (tests/_gram_ref.GramRefOps)."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _gram_ref import (GramRefOps, SHAPES, VARIANTS, MAX_G, plan, boundary_shapes, case, int_case, gram_ref, gram_ref_fast,
                       bound, U, _up32)
from dca_amd import genecorr as GC
from dca_amd import io
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.engine import Engine
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 3, 8)
N, G = 90, 21
ALL_SHAPES = SHAPES + list(boundary_shapes())


# ---------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_bound_holds_for_plain_double_arithmetic(shape, variant):
    """The reference in plain float64, rows in ascending order, against the same sums in np.longdouble: inside E on the
    operands the GPU file uses -- correct double arithmetic alone meets the bar."""
    c = case(shape, variant)
    x = np.nan_to_num(c['x'], nan=0.0)                               # the rows that are out hold NaN; they are not used
    cols = np.arange(shape[1]) if c['cols'] is None else c['cols']
    rows = np.arange(shape[0]) if c['keep'] is None else np.flatnonzero(c['keep'])
    d = (x[np.ix_(rows, cols)].astype(np.float64) - c['shift'][None, :]).astype(np.longdouble)
    exact_cross = np.zeros((shape[1], shape[1]), np.longdouble)
    for r in range(len(rows)):
        exact_cross += np.outer(d[r], d[r])
    exact_dsum = d.sum(axis=0) if len(rows) else np.zeros(shape[1], np.longdouble)
    e_cross = np.abs((c['cross'].astype(np.longdouble) - exact_cross).astype(np.float64))
    e_dsum = np.abs((c['dsum'].astype(np.longdouble) - exact_dsum).astype(np.float64))
    assert (e_cross <= bound(c['absprod'], c['m'])).all() and (e_dsum <= bound(c['absd'], c['m'])).all()
    if c['m'] == 0:
        assert not c['cross'].any() and not c['dsum'].any()
    # the two evaluation orders of the reference agree inside the bound as well
    f = gram_ref_fast(x, c['cols'], c['keep'], c['shift'])
    assert (np.abs(f[0] - c['cross']) <= 2 * bound(c['absprod'], c['m'])).all()


def test_integer_case_is_exact_in_double():
    for shape in ALL_SHAPES:
        c = int_case(shape)
        assert np.abs(c['cross']).max() < 2 ** 53 and shape[0] * 72 * 72 < 2 ** 53
        assert (c['cross'].dtype == np.int64) == (shape[0] * shape[1] ** 2 <= 1e8)
        assert np.array_equal(c['cross'], c['cross'].T) and (np.asarray(c['cross'], np.float64) % 1 == 0).all()
        if shape[0] * shape[1] ** 2 <= 4e6:
            ref = gram_ref(c['x'], c['cols'], c['keep'], c['shift'])
            assert np.array_equal(ref[0], c['cross'].astype(np.float64)) and np.array_equal(ref[1], c['dsum'].astype(np.float64))


# ---------------------------------------------------------------------------------------------------- corr_from_moments
def _moments(x, shift):
    d = np.asarray(x, np.float64) - np.asarray(shift, np.float64)[None, :]
    return d.T @ d, d.sum(axis=0)


def test_corr_from_moments_against_corrcoef():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(200, 6)) @ rng.normal(size=(6, 6)) + rng.normal(size=6) * 3
    ref = np.corrcoef(x, rowvar=False)
    r = GC.corr_from_moments(*_moments(x, x[:64].mean(axis=0)), 200)
    assert r.dtype == np.float64 and r.shape == (6, 6)
    np.testing.assert_allclose(r, ref, rtol=0, atol=1e-13)
    assert (np.diagonal(r) == 1.0).all() and np.array_equal(r, r.T) and np.abs(r).max() <= 1.0
    cov = GC.cov_from_moments(*_moments(x, x[:64].mean(axis=0)), 200)
    np.testing.assert_allclose(cov, np.cov(x, rowvar=False), rtol=1e-12, atol=1e-14)


def test_corr_from_moments_constant_gene_and_few_cells():
    rng = np.random.default_rng(1)
    x = rng.uniform(1, 2, size=(50, 4))
    x[:, 2] = 0.75
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = np.corrcoef(x, rowvar=False)
    r = GC.corr_from_moments(*_moments(x, x.mean(axis=0)), 50)
    assert np.isnan(r[2]).all() and np.isnan(r[:, 2]).all() and np.isnan(ref[2]).all()         # numpy's convention
    keep = [0, 1, 3]
    np.testing.assert_allclose(r[np.ix_(keep, keep)], ref[np.ix_(keep, keep)], atol=1e-13)
    assert (np.diagonal(r)[keep] == 1.0).all()
    one = GC.corr_from_moments(*_moments(x[:1], x[0]), 1)
    assert one.shape == (4, 4) and np.isnan(one).all()
    assert np.isnan(GC.corr_from_moments(np.zeros((4, 4)), np.zeros(4), 0)).all()
    two = GC.corr_from_moments(*_moments(x[:2], x[:2].mean(axis=0)), 2)                       # two cells: r = +-1
    np.testing.assert_allclose(two[np.ix_(keep, keep)], np.corrcoef(x[:2][:, keep], rowvar=False), atol=1e-13)
    assert np.abs(np.abs(two[np.ix_(keep, keep)]) - 1).max() <= 4 * U and np.isnan(two[2]).all()
    with pytest.raises(ValueError, match='cross is'):
        GC.corr_from_moments(np.zeros((3, 4)), np.zeros(4), 5)


def test_what_the_shift_buys():
    """Mean 1e3, sd 1, 4096 cells.  With shift = 0 the two terms of cross - dsum dsum^T / n are 4e9 each and their difference
    4e3: the covariance keeps about six digits fewer than the moments have (1e6 = mean^2 / var), in DOUBLE -- the correlation
    is still good to ~1e-9 here, and would be lost altogether in fp32 (2^-24 * 1e6 > 1).  With the shift at a chunk's mean the
    terms are of the size of the covariance itself and nothing cancels."""
    rng = np.random.default_rng(2)
    n = 4096
    x = (1e3 + rng.normal(size=(n, 5)) @ rng.normal(size=(5, 5))).astype(np.float32).astype(np.float64)
    ref = np.corrcoef(x, rowvar=False)
    near = np.abs(GC.corr_from_moments(*_moments(x, x[:1024].mean(axis=0)), n) - ref).max()
    far = np.abs(GC.corr_from_moments(*_moments(x, np.zeros(5)), n) - ref).max()
    print('shift at a chunk mean: max |r - corrcoef| = %.3g; shift 0: %.3g' % (near, far))
    # bars: the three entries of C that r is made of, each an n-term double sum, (n + 4) 2^-53 sum |d| |d| of tests/_gram_ref.py,
    # over sqrt(C_ii C_jj): the ratio sum d^2 / C_ii is 1 + n offset^2 / C_ii -- about 1 with the shift near the mean, and
    # mean^2 / var with shift 0 (the genes' variances here are sums of five squared normals: 1e4 < ratio < 1e7)
    var = x.var(axis=0)
    ratio_near = (1 + (x[:1024].mean(axis=0) - x.mean(axis=0)) ** 2 / var).max()
    ratio_far = ((x ** 2).mean(axis=0) / var).max()
    assert ratio_near < 1.01 and 1e4 < ratio_far < 1e7
    assert near <= 3 * (n + 4) * U * ratio_near
    assert far <= 3 * (n + 4) * U * ratio_far
    cross, dsum = _moments(x, np.zeros(5))
    lost = np.abs(cross).max() / np.abs(cross - np.outer(dsum, dsum) / n).max()
    assert 1e4 < lost < 1e7                            # the cancellation itself: four to seven digits of the moments


# ---------------------------------------------------------------------------------------------------- the plan
def _query():
    from dca_amd import build
    L = ctypes.CDLL(build.build_hip(verbose=False))
    q = L.dcahip_gram_workspace_doubles
    q.restype, q.argtypes = ctypes.c_long, [ctypes.c_int] * 2
    return q


def test_restated_plan_against_the_workspace_query():
    """The library loads without a GPU: dcahip_gram_workspace_doubles (host arithmetic) against the plan as the comment above
    gram_kernel states it; more than one slice only where the triangle's tiles alone do not fill the chip (at most 682);
    at most 64 MiB; non-decreasing in B; enough for every row block of the call (its gathered image and its partial tiles)."""
    q = _query()
    assert q(10, 0) == q(10, MAX_G + 1) == q(0, 0) == -22 and q(0, 5) == q(-3, 5) == 0
    for g in (1, 5, 16, 17, 63, 64, 65, 130, 200, 512, 1984, 1985, 2048, 2304, 2305, 2816, 2817, 4096, 8191, MAX_G):
        last = 0
        for B in list(range(1, 200)) + [480, 481, 1000, 1024, 2047, 2048, 2049, 4096, 68579]:
            p = plan(B, g)
            w = q(B, g)
            assert w == p['ws'] and w >= last and w * 8 <= 64 << 20, (B, g, w, p)
            assert sum(p['blocks']) == B and max(p['blocks']) == p['blocks'][0] <= p['rows_max'] and p['rows_max'] % 32 == 0
            Gp = 64 * p['T']
            for b, (cap, rows_per, S) in zip(p['blocks'], p['slices']):
                assert 1 <= S <= cap <= p['capmax'] <= 64 and rows_per % 32 == 0 and (S - 1) * rows_per < b <= S * rows_per
                need = (S * (p['NT'] * 4096 + p['T'] * 64) if S > 1 else 0) + _up32(p['blocks'][0]) * Gp // 2
                assert w >= need, (B, g, b, w, need)
                if S > 1:
                    assert p['NT'] <= 682 and S * p['NT'] < 1536     # 1024 / NT to the nearest integer
            if p['NT'] > 682:
                assert p['capmax'] == 1
            last = w
    # the three shapes tools/bench_genecorr.py times: 36 tiles x 26 slices | two row blocks of 528 tiles x 2 slices | two row
    # blocks of 8256 tiles, one slice, the image alone fills the 64 MiB
    assert plan(4096, 512)['slices'] == [(28, 160, 26)] and plan(4096, 512)['blocks'] == [4096]
    assert plan(4096, 2048)['slices'] == [(2, 1024, 2)] * 2 and plan(4096, 2048)['blocks'] == [2048, 2048]
    assert plan(4096, 8192)['blocks'] == [2048, 2048] and plan(4096, 8192)['S'] == 1 and plan(4096, 8192)['NT'] == 8256
    assert plan(4096, 8192)['ws'] * 8 == 64 << 20
    assert plan(68579, 64, cols=False)['blocks'] == [68579]          # no cols: the plane is read in place, one row block
    multi, single = boundary_shapes()
    assert multi[1] + 1 == single[1] == 2305


# ---------------------------------------------------------------------------------------------------- Engine.gene_gram
def test_engine_gene_gram_against_predict():
    """On the CPU oracle: the moments of what predict_chunk writes, for chunks that do not divide n, a row range, a keep
    mask that empties the first chunk (shift = zeros) and the value forms."""
    n, g = 150, 13
    X, Y, sf, p = make_problem(n, g, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(GramRefOps(), 'zinb-conddisp', g, HS, True, 0.05, p, X, Y, sf)
    eng.load_data(X, None, sf)                                        # no targets: an inference pass
    eng.reserve(64)
    x = np.concatenate([eng.predict_chunk(s, min(64, n - s), {'mean'})['mean'].numpy().astype(np.float32)
                        for s in range(0, n, 64)])
    cols = np.array([7, 2, 11, 0, 5])
    res = eng.gene_gram(cols, chunk=64)
    assert res['count'] == n and res['cross'].dtype == res['dsum'].dtype == res['shift'].dtype == torch.float64
    assert res['cross'].shape == (5, 5) and res['dsum'].shape == res['shift'].shape == (5,)
    shift = res['shift'].numpy()
    np.testing.assert_allclose(shift, x[:64][:, cols].astype(np.float64).mean(axis=0), rtol=1e-14)
    ref = gram_ref(x, cols, None, shift)
    np.testing.assert_allclose(res['cross'].numpy(), ref[0], rtol=0, atol=float(bound(ref[2], n).max()) * 4)
    np.testing.assert_allclose(res['dsum'].numpy(), ref[1], rtol=0, atol=float(bound(ref[3], n).max()) * 4)
    np.testing.assert_allclose(GC.corr_from_moments(res['cross'].numpy(), res['dsum'].numpy(), n),
                               np.corrcoef(x[:, cols].astype(np.float64), rowvar=False), atol=1e-12)
    keep = np.ones(n, bool)
    keep[:70] = False                                                 # the first chunk keeps no row: shift = zeros
    keep[100::7] = False
    part = eng.gene_gram(torch.as_tensor(cols), keep=keep, r0=3, r1=141, chunk=64)
    inside = keep.copy()
    inside[:3] = False
    inside[141:] = False
    assert part['count'] == inside.sum() and not part['shift'].numpy().any()
    ref = gram_ref(x, cols, inside, np.zeros(5))
    np.testing.assert_allclose(part['cross'].numpy(), ref[0], rtol=1e-13)
    np.testing.assert_allclose(part['dsum'].numpy(), ref[1], rtol=1e-13)
    sfv = np.asarray(sf, np.float32).astype(np.float64)[:, None]
    lg = eng.gene_gram(cols, no_sf=True, log1p=True, chunk=150)
    v = np.log1p(x.astype(np.float64) / sfv)[:, cols]
    np.testing.assert_allclose(lg['shift'].numpy() + lg['dsum'].numpy() / n, v.mean(axis=0), rtol=1e-6)
    np.testing.assert_allclose(GC.corr_from_moments(lg['cross'].numpy(), lg['dsum'].numpy(), n), np.corrcoef(v, rowvar=False),
                               atol=1e-4)
    empty = eng.gene_gram(cols, r0=20, r1=20)
    assert empty['count'] == 0 and not empty['cross'].numpy().any()


def test_engine_gene_gram_refusals():
    X, Y, sf, p = make_problem(40, 9, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    cols = np.arange(9)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.gene_gram(cols)
    eng = make_engine(GramRefOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(ValueError, match='rows'):
        eng.gene_gram(cols, r1=41)
    for bad in (cols.astype(np.float32), cols.reshape(3, 3), np.zeros(0, np.int64)):
        with pytest.raises(ValueError, match='1-d integer array'):
            eng.gene_gram(bad)
    for bad in ([0, 9], [-1, 3]):
        with pytest.raises(ValueError, match='cols must lie in 0 .. 8'):
            eng.gene_gram(np.array(bad))
    with pytest.raises(ValueError, match='more than once'):
        eng.gene_gram(np.array([1, 4, 1]))
    with pytest.raises(ValueError, match='at most 8192'):
        eng.gene_gram(np.arange(8193) % 9)
    with pytest.raises(ValueError, match='one per cell'):
        eng.gene_gram(cols, keep=np.ones(39, bool))
    with pytest.raises(ValueError, match='one per cell'):
        eng.gene_gram(cols, keep=np.ones(40, np.float32))
    lin = make_engine(GramRefOps(), 'normal', 9, HS, True, 0.0, make_problem(40, 9, HS, 'normal', seed=6)[3], X, Y, sf)
    with pytest.raises(ValueError, match='log1p'):
        lin.gene_gram(cols, log1p=True)
    assert lin.gene_gram(cols)['count'] == 40                        # without log1p a linear mean is fine
    fresh = Engine('zinb-conddisp', 9, 9, HS, True, 0.05, ops=GramRefOps())
    with pytest.raises(ValueError, match='needs data'):
        fresh.gene_gram(cols)

    class TwoRanks:
        rank, world, dp = 0, 2, False
    eng.comm = TwoRanks()
    with pytest.raises(ValueError, match='data-parallel'):
        eng.gene_gram(cols)


# ---------------------------------------------------------------------------------------------------- gene_correlation
def _adata(n=N, g=G, seed=3):
    ad = AnnData(synth_counts(n, g, seed).astype(np.float32),
                 obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(g)]))
    ad = io.read_dataset(ad, copy=True)
    return io.normalize(ad, device=False)


def _fitted(ae_type, ad, subset=None, ridge=0.05):
    with override_ops(GramRefOps):
        net = AE_types[ae_type](input_size=ad.n_vars, output_size=len(subset) if subset else ad.n_vars, hidden_size=HS,
                                ridge=ridge)
        net.build()
        train(ad, net, epochs=2, batch_size=32, output_subset=subset, verbose=False)
    return net


@pytest.fixture(scope='module')
def fitted():
    ad = _adata()
    return ad, _fitted('zinb-conddisp', ad)


KEYS = ['genes', 'corr', 'mean', 'var', 'n_cells', 'value', 'log1p', 'groupby', 'group']


def test_gene_correlation_against_corrcoef_of_predict(fitted):
    ad, net = fitted
    ad = ad.copy()
    x = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float64)
    before = ad.X.copy()
    res = net.gene_correlation(ad, copy=True)
    assert res is not ad and 'dca_gene_corr' not in ad.uns
    assert net.gene_correlation(ad) is None
    np.testing.assert_array_equal(ad.X, before)
    for a in (res, ad):
        d = a.uns['dca_gene_corr']
        assert list(d) == KEYS and list(d['genes']) == ['g%d' % i for i in range(G)]
        assert d['n_cells'] == N and d['value'] == 'denoised' and d['log1p'] is False and d['groupby'] is None and d['group'] is None
        assert d['corr'].dtype == np.float64 and d['corr'].shape == (G, G)
        np.testing.assert_allclose(d['corr'], np.corrcoef(x, rowvar=False), atol=1e-6)         # the oracle's heads are fp64
        np.testing.assert_allclose(d['mean'], x.mean(axis=0), rtol=1e-6)
        np.testing.assert_allclose(d['var'], x.var(axis=0, ddof=1), rtol=1e-5)
        assert np.array_equal(d['corr'], d['corr'].T) and (np.diagonal(d['corr']) == 1).all()
    # genes= gives the order of the result; key_added names it
    order = ['g7', 'g2', 'g19', 'g0']
    net.gene_correlation(ad, genes=order, key_added='four')
    d4, idx = ad.uns['four'], [7, 2, 19, 0]
    assert list(d4['genes']) == order
    np.testing.assert_allclose(d4['corr'], ad.uns['dca_gene_corr']['corr'][np.ix_(idx, idx)], atol=1e-12)
    # one group's cells
    lab = np.array(['abc'[i % 3] if i % 10 else None for i in range(N)], dtype=object)
    ad.obs['cluster'] = pd.Categorical(lab)
    net.gene_correlation(ad, groupby='cluster', group='b', value='normalized', log1p=True)
    d = ad.uns['dca_gene_corr']
    rows = lab == 'b'
    sf = ad.obs['size_factors'].values.astype(np.float32).astype(np.float64)[:, None]
    v = np.log1p(x / sf)[rows]
    assert d['n_cells'] == rows.sum() and d['groupby'] == 'cluster' and d['group'] == 'b' and d['log1p'] is True
    np.testing.assert_allclose(d['corr'], np.corrcoef(v, rowvar=False), atol=1e-4)
    np.testing.assert_allclose(d['mean'], v.mean(axis=0), rtol=1e-5)
    net.gene_correlation(ad, groupby=lab, group='b', value='normalized', log1p=True, key_added='by_array')
    assert ad.uns['by_array']['groupby'] is None
    np.testing.assert_array_equal(ad.uns['by_array']['corr'], d['corr'])


def test_top_partners(fitted):
    ad, net = fitted
    ad = ad.copy()
    net.gene_correlation(ad)
    r = ad.uns['dca_gene_corr']['corr'][4]
    names, vals = GC.top_partners(ad, 'g4', n=5)
    order = [j for j in np.argsort(-np.abs(r), kind='stable') if j != 4][:5]
    assert list(names) == ['g%d' % j for j in order] and np.array_equal(vals, r[order])
    assert (np.diff(np.abs(vals)) <= 0).all() and 'g4' not in names
    assert len(GC.top_partners(ad, 'g4', n=1000)[0]) == G - 1
    with pytest.raises(ValueError, match="'nope' is not one of the 21 genes"):
        GC.top_partners(ad, 'nope')
    ad.uns['dca_gene_corr']['corr'][4, 6] = np.nan                   # a constant partner has no correlation: left out
    assert 'g6' not in GC.top_partners(ad, 'g4', n=1000)[0]


def test_gene_correlation_of_a_gene_subset_network():
    ad = _adata()
    cols = [17, 2, 9, 11, 0]
    subset = ['g%d' % i for i in cols]
    net = _fitted('zinb-conddisp', ad, subset=subset)
    with pytest.raises(ValueError, match='output_subset'):
        net.gene_correlation(ad)
    net.gene_correlation(ad, output_subset=subset)
    d = ad.uns['dca_gene_corr']
    x = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float64)
    assert list(d['genes']) == subset and d['corr'].shape == (5, 5)
    np.testing.assert_allclose(d['corr'], np.corrcoef(x, rowvar=False), atol=1e-6)
    net.gene_correlation(ad, genes=['g9', 'g17'], output_subset=subset)
    np.testing.assert_allclose(ad.uns['dca_gene_corr']['corr'][0, 1], d['corr'][2, 0], atol=1e-12)
    with pytest.raises(ValueError, match="'g3' is not a gene the network fits"):
        net.gene_correlation(ad, genes=['g9', 'g3'], output_subset=subset)


def test_gene_correlation_refusals(fitted):
    ad, net = fitted
    with pytest.raises(ValueError, match='value'):
        net.gene_correlation(ad, value='raw')
    with pytest.raises(ValueError, match="'gX' is not a gene"):
        net.gene_correlation(ad, genes=['g1', 'gX'])
    with pytest.raises(ValueError, match='more than once'):
        net.gene_correlation(ad, genes=['g1', 'g2', 'g1'])
    with pytest.raises(ValueError, match='at least one'):
        net.gene_correlation(ad, genes=[])
    with pytest.raises(ValueError, match='needs groupby'):
        net.gene_correlation(ad, group='a')
    with pytest.raises(ValueError, match='needs group'):
        net.gene_correlation(ad, groupby=np.zeros(N))
    with pytest.raises(ValueError, match="no column 'nope'"):
        net.gene_correlation(ad, groupby='nope', group='a')
    with pytest.raises(ValueError, match='89 labels for 90 cells'):
        net.gene_correlation(ad, groupby=np.zeros(89), group=0)
    with pytest.raises(ValueError, match="gene_correlation: no cell carries the label 'z'"):
        net.gene_correlation(ad, groupby=np.array(['a'] * N, dtype=object), group='z')
    lin = _fitted('normal', ad, ridge=0.0)
    with pytest.raises(ValueError, match="ae_type='normal'"):
        lin.gene_correlation(ad, log1p=True)
    lin.gene_correlation(ad)
    assert ad.uns['dca_gene_corr']['corr'].shape == (G, G)
    one = np.array(['a'] + ['b'] * (N - 1), dtype=object)            # a group of one cell: no correlation
    net.gene_correlation(ad, groupby=one, group='a')
    d = ad.uns['dca_gene_corr']
    assert d['n_cells'] == 1 and np.isnan(d['corr']).all() and np.isnan(d['var']).all() and np.isfinite(d['mean']).all()


def test_gene_limit_is_named():
    """More than 8192 genes: refused by name before anything runs (no fit needed: the check precedes the binding)."""
    n, g = 4, MAX_G + 1
    ad = AnnData(np.ones((n, g), np.float32), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(g)]))

    class Lay:
        G_out = g

    class Eng:
        lay, flags = Lay(), 0

    class Net:
        engine = Eng()
    with pytest.raises(ValueError, match='8193 genes \\(at most 8192'):
        GC.gene_correlation(Net(), ad)


# ---------------------------------------------------------------------------------------------------- command line
def _write_counts(tmp_path, n=64, g=18, seed=5):
    y = synth_counts(n, g, seed)
    genes = ['g%d' % i for i in range(g)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


BASE = ['--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8']


@pytest.mark.parametrize('log1p', [False, True])
def test_cli_genecorr_file(tmp_path, monkeypatch, log1p):
    f, genes, cells = _write_counts(tmp_path)
    listed = ['g11', 'g3', 'g7', 'g0', 'g3']                         # a name listed twice counts once
    gl = str(tmp_path / 'genes.txt')
    with open(gl, 'w') as fh:
        fh.write('\n'.join(listed) + '\n')
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].gene_correlation

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        seen['kw'], seen['d'] = kw, adata.uns['dca_gene_corr']
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'gene_correlation', spy)
    with override_ops(GramRefOps):
        main([f, out] + BASE + ['--genecorr', gl] + (['--genecorr-log1p'] if log1p else []))
    assert seen['kw']['value'] == ('normalized' if log1p else 'denoised') and seen['kw']['log1p'] is log1p
    order = ['g0', 'g3', 'g7', 'g11']                                # the order of the input's genes
    assert seen['kw']['genes'] == order
    t = pd.read_csv(os.path.join(out, 'gene_corr.tsv'), sep='\t', index_col=0)
    assert list(t.index) == list(t.columns) == order
    np.testing.assert_array_equal(t.values, np.array([[float('%.6f' % v) for v in row] for row in seen['d']['corr']]))
    assert (np.diagonal(t.values) == 1.0).all()
    assert os.path.exists(os.path.join(out, 'mean.tsv'))


def test_cli_genecorr_refusals(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    gl = str(tmp_path / 'genes.txt')
    with open(gl, 'w') as fh:
        fh.write('g1\nnot_a_gene\ng2\n')
    with override_ops(GramRefOps):
        with pytest.raises(ValueError, match="'not_a_gene' is not a gene of the input"):
            main([f, str(tmp_path / 'res'), '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--genecorr', gl])
    assert not os.path.exists(os.path.join(str(tmp_path / 'res'), 'mean.tsv'))       # refused before the fit
    with open(gl, 'w') as fh:
        fh.write('g1\ng2\n')
    with override_ops(GramRefOps):
        with pytest.raises(ValueError, match='--type normal'):
            main([f, str(tmp_path / 'res2'), '--type', 'normal', '-e', '1', '-s', '8,2,8', '--genecorr', gl,
                  '--genecorr-log1p'])
        with pytest.raises(ValueError, match='give --genecorr'):
            main([f, str(tmp_path / 'res3'), '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--genecorr-log1p'])
        sub = str(tmp_path / 'subset.txt')
        with open(sub, 'w') as fh:
            fh.write('g2\ng5\ng9\n')
        with pytest.raises(ValueError, match="'g1' is not a gene of --denoisesubset"):
            main([f, str(tmp_path / 'res4'), '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--denoisesubset', sub,
                  '--genecorr', gl])
