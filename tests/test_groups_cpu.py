"""Groups of cells compared on the denoised expression, the Python layers (Autoencoder.group_stats, Engine.group_moments,
dca_amd.groups, `dca --groupstats`) on the CPU oracle extended with group_moments (tests/_groups_ref.GroupRefOps)."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _groups_ref import GroupRefOps, moments, abs_moments, two_pass_stats, bh
from test_counts_resident_cpu import CsrOps
from dca_amd import groups as GR
from dca_amd import io
from dca_amd import prep as P
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.engine import Engine
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 3, 8)
N, G = 90, 21
STAT_RTOL, STAT_ATOL = 1e-9, 1e-12          # moment-based statistics against scipy's two-pass ones


def _adata(n=N, G=G, seed=3):
    ad = AnnData(synth_counts(n, G, seed).astype(np.float32),
                 obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    return io.normalize(ad, device=False)


def _codes(n=N, K=3, seed=0):
    """Three groups of unequal size in shuffled order, every ninth cell in no group."""
    c = np.random.default_rng(seed).integers(0, K, size=n).astype(np.int32)
    c[::9] = -1
    return c


def _labels(n=N, K=3):
    """The codes as integer labels, None where a cell is in no group."""
    return np.array([int(c) if c >= 0 else None for c in _codes(n, K)], dtype=object)


def _fitted(ae_type, ad, ops=GroupRefOps, subset=None, ridge=0.05):
    with override_ops(ops):
        net = AE_types[ae_type](input_size=ad.n_vars, output_size=len(subset) if subset else ad.n_vars, hidden_size=HS,
                                ridge=ridge)
        net.build()
        train(ad, net, epochs=2, batch_size=32, output_subset=subset, verbose=False)
    return net


class SpyOps(GroupRefOps):
    """Keeps the element matrix every group_moments call summed (the rows of the chunks, in order)."""
    seen = None

    def group_moments(self, a_mean, lda, sf, codes, B, G, K, flags, *rest):
        from _groups_ref import elements
        from oracle.cpu_ops import _mat, _vec
        if type(self).seen is not None:
            type(self).seen.append(elements(flags, _mat(a_mean, B, G, lda), _vec(sf, B)).copy())
        return super().group_moments(a_mean, lda, sf, codes, B, G, K, flags, *rest)


@pytest.fixture(scope='module')
def fitted():
    ad = _adata()
    return ad, _fitted('zinb-conddisp', ad, ops=SpyOps)


# ---------------------------------------------------------------------------------------------------- Engine.group_moments
@pytest.mark.parametrize('ae_type, subset', [('zinb-conddisp', None), ('nb', None), ('normal', None), ('zinb-shared', None),
                                             ('zinb-conddisp', ['g%d' % i for i in (17, 2, 9, 11, 0)])])
def test_engine_group_moments_against_predict(ae_type, subset):
    """The sums of what predict() writes (fp32), reduced in float64 on the host: predict rounds every element to fp32
    (2^-24 relative), so |S1 - ref| <= 2^-23 sum |x| and |S2 - ref| <= 2^-22 sum x^2 with a factor two to spare."""
    ad = _adata()
    net = _fitted(ae_type, ad, subset=subset)
    codes, K = _codes(), 3
    x = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float64)      # what predict() stores as adata.X
    assert x.shape == (N, len(subset) if subset else G)
    s1, s2, n = moments(x, codes, K)
    a1, a2 = abs_moments(x, codes, K)
    net._bind_inputs(ad)
    res = net.engine.group_moments(codes, K, chunk=64)
    assert res['sum'].dtype == res['sumsq'].dtype == torch.float64 and res['count'].dtype == torch.int64
    assert res['sum'].shape == res['sumsq'].shape == (K, x.shape[1]) and res['count'].shape == (K,)
    np.testing.assert_array_equal(res['count'].numpy(), n)
    assert (np.abs(res['sum'].numpy() - s1) <= 2.0 ** -23 * a1).all()
    assert (np.abs(res['sumsq'].numpy() - s2) <= 2.0 ** -22 * a2).all()
    # the mean without the size factor, and its log1p
    sf = ad.obs['size_factors'].values.astype(np.float32).astype(np.float64)[:, None]
    r2 = net.engine.group_moments(codes, K, no_sf=True, chunk=64)
    t1, _, _ = moments(x / sf, codes, K)
    np.testing.assert_allclose(r2['sum'].numpy(), t1, rtol=1e-6)
    if ae_type != 'normal':
        r3 = net.engine.group_moments(codes, K, no_sf=True, log1p=True, chunk=64)
        t1, t2, _ = moments(np.log1p(x / sf), codes, K)
        np.testing.assert_allclose(r3['sum'].numpy(), t1, rtol=1e-6)
        np.testing.assert_allclose(r3['sumsq'].numpy(), t2, rtol=1e-6)


def test_engine_group_moments_chunks_and_row_range():
    X, Y, sf, p = make_problem(150, 13, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(GroupRefOps(), 'zinb-conddisp', 13, HS, True, 0.05, p, X, Y, sf)
    eng.load_data(X, None, sf)                                        # no targets: an inference pass
    codes = _codes(150, 4)
    a, b = eng.group_moments(codes, 4, chunk=64), eng.group_moments(torch.as_tensor(codes), 4, chunk=150)
    for k in ('sum', 'sumsq'):
        assert (np.abs(a[k].numpy() - b[k].numpy()) <= 1e-12 * np.abs(b[k].numpy())).all()
    assert torch.equal(a['count'], b['count'])
    part = eng.group_moments(codes, 4, r0=40, r1=131, chunk=32)
    only = codes.copy()
    only[:40] = -1
    only[131:] = -1
    ref = eng.group_moments(only, 4, chunk=150)
    assert torch.equal(part['count'], ref['count'])
    np.testing.assert_allclose(part['sum'].numpy(), ref['sum'].numpy(), rtol=1e-12)


def test_engine_group_moments_refusals():
    X, Y, sf, p = make_problem(40, 9, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    codes = np.zeros(40, np.int32)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.group_moments(codes, 1)
    eng = make_engine(GroupRefOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(ValueError, match='rows'):
        eng.group_moments(codes, 1, r1=41)
    with pytest.raises(ValueError, match='4096'):
        eng.group_moments(codes, 4097)
    with pytest.raises(ValueError, match='one per cell'):
        eng.group_moments(codes[:39], 1)
    with pytest.raises(ValueError, match='one per cell'):
        eng.group_moments(codes.astype(np.float32), 1)
    for bad in (-2, 1):
        c = codes.copy()
        c[7] = bad
        with pytest.raises(ValueError, match='codes must lie'):
            eng.group_moments(c, 1)
    lin = make_engine(GroupRefOps(), 'normal', 9, HS, True, 0.0, make_problem(40, 9, HS, 'normal', seed=6)[3], X, Y, sf)
    with pytest.raises(ValueError, match='log1p'):
        lin.group_moments(codes, 1, log1p=True)
    fresh = Engine('zinb-conddisp', 9, 9, HS, True, 0.05, ops=GroupRefOps())
    with pytest.raises(ValueError, match='needs data'):
        fresh.group_moments(codes, 1)

    class TwoRanks:
        rank, world, dp = 0, 2, False
    eng.comm = TwoRanks()
    with pytest.raises(ValueError, match='data-parallel'):
        eng.group_moments(codes, 1)


def test_workspace_query_does_not_decrease_with_the_rows():
    """Engine.group_moments sizes the workspace once, for `chunk` rows, and the ragged last chunk is shorter: the query
    (host arithmetic of libdcahip.so, no GPU) must be non-decreasing in B for every G and K, and cover the slices a call of
    that shape uses (restated: rows_per = ceil(B / cap), S = ceil(B / rows_per), cap = min(64, B, ceil(1024 / (segments K)))
    with the segments of the 16-byte path or of the scalar path)."""
    import ctypes
    from dca_amd import build
    L = ctypes.CDLL(build.build_hip(verbose=False))
    q = L.dcahip_group_moments_workspace_doubles
    q.restype, q.argtypes = ctypes.c_int, [ctypes.c_int] * 3

    def used(B, g, K, V):
        nseg = ((g + V - 1) // V + 255) // 256
        cap = max(1, min(64, B, -(-1024 // (nseg * K))))
        rows_per = -(-B // cap)
        S = -(-B // rows_per)
        return 2 * S * K * g if S > 1 else 0
    assert q(100, 37, 4) >= q(64, 37, 4) == 2 * 64 * 4 * 37                # 50 slices of two rows | 64 of one
    for g, K in ((1, 1), (8, 1), (37, 4), (260, 130), (1030, 3), (5000, 10), (20000, 16), (20000, 4096), (300, 1000)):
        last = 0
        for B in list(range(1, 300)) + [960, 1000, 1984, 2000, 4095, 4096, 68579]:
            w = q(B, g, K)
            assert w >= last, (B, g, K, w, last)
            assert w >= max(used(B, g, K, 4), used(B, g, K, 1), 1), (B, g, K)
            last = w


def test_engine_group_moments_ragged_tail_shorter_than_the_chunk():
    X, Y, sf, p = make_problem(164, 13, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(GroupRefOps(), 'zinb-conddisp', 13, HS, True, 0.05, p, X, Y, sf)
    codes = _codes(164, 4)
    a, b = eng.group_moments(codes, 4, chunk=100), eng.group_moments(codes, 4, chunk=164)
    for k in ('sum', 'sumsq'):
        assert (np.abs(a[k].numpy() - b[k].numpy()) <= 1e-12 * np.abs(b[k].numpy())).all()


class GroupCsrOps(GroupRefOps, CsrOps):
    pass


def test_counts_resident_group_moments_equal_the_dense_ones():
    ops = GroupCsrOps()
    _, Y, sf, _ = make_problem(75, 18, (6, 3, 6), 'zinb-conddisp', True, seed=3)
    Ys = sp.csr_matrix(Y)
    n, g = Ys.shape
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    fac = torch.as_tensor(np.linspace(0.5, 1.5, n).astype(np.float32))
    norm = P.csr_norm(ops, csr, fac, True, True)
    Xd, Yd = torch.zeros(n, P._r4(g)), torch.zeros(n, P._r4(g))
    ops.csr_gather(csr, None, None, 0, n, None, norm['fac'], True, norm['mean'], norm['std'], Yd, Yd.shape[1], Xd,
                   Xd.shape[1], None, None)
    codes = _codes(n, 3)
    res = []
    for form in ('dense', 'counts'):
        eng = Engine('zinb-conddisp', g, g, (6, 3, 6), True, 0.0, ops=ops)
        eng.init_params(seed=7)
        if form == 'dense':
            eng.attach_device_data(Xd, Yd, torch.as_tensor(sf), norm=norm)
        else:
            eng.attach_counts(csr, torch.as_tensor(sf), norm)
        res.append(eng.group_moments(codes, 3, chunk=32))
    for k in ('sum', 'sumsq', 'count'):
        assert torch.equal(res[0][k], res[1][k]), k
    assert float(res[0]['sum'].abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------- group_stats
KEYS = ['groupby', 'names', 'counts', 'value', 'log1p', 'reference', 'mean', 'var', 'scores', 'pvals', 'pvals_adj',
        'logfoldchanges']
ARRAYS = KEYS[6:]


def test_group_stats_keys_dtypes_shapes_and_copy(fitted):
    ad, net = fitted
    ad = ad.copy()
    ad.obs['cluster'] = pd.Categorical(['abc'[c] if c >= 0 else None for c in _codes()])
    before = (ad.X.copy(), dict(ad.uns))
    res = net.group_stats(ad, 'cluster', copy=True)
    assert res is not ad and 'dca_groups' not in ad.uns and dict(ad.uns) == before[1]
    np.testing.assert_array_equal(ad.X, before[0])
    assert net.group_stats(ad, 'cluster') is None                   # in place, like predict
    for a in (res, ad):
        d = a.uns['dca_groups']
        assert list(d) == KEYS
        assert d['groupby'] == 'cluster' and list(d['names']) == ['a', 'b', 'c'] and d['value'] == 'denoised'
        assert d['log1p'] is False and d['reference'] == 'rest'
        assert d['counts'].dtype == np.int64 and d['counts'].tolist() == [int((_codes() == k).sum()) for k in range(3)]
        for k in ARRAYS:
            assert d[k].dtype == np.float64 and d[k].shape == (3, G) and np.isfinite(d[k]).all(), k
    for k in ARRAYS:
        np.testing.assert_array_equal(res.uns['dca_groups'][k], ad.uns['dca_groups'][k])


def test_group_stats_label_forms_nan_and_groups(fitted):
    ad, net = fitted
    ad = ad.copy()
    codes = _codes()
    strings = np.array(['abc'[c] if c >= 0 else None for c in codes], dtype=object)
    ad.obs['cat'] = pd.Categorical(strings)
    ad.obs['str'] = strings
    ad.obs['int'] = [float(c) if c >= 0 else np.nan for c in codes]
    out = {}
    for key in ('cat', 'str', 'int'):
        net.group_stats(ad, key)
        out[key] = ad.uns['dca_groups']
    net.group_stats(ad, strings)
    out['array'] = ad.uns['dca_groups']
    assert out['array']['groupby'] is None and list(out['int']['names']) == [0.0, 1.0, 2.0]
    for key in ('str', 'int', 'array'):
        assert out[key]['counts'].tolist() == out['cat']['counts'].tolist() and out[key]['counts'].sum() == (codes >= 0).sum()
        for k in ARRAYS:
            np.testing.assert_array_equal(out[key][k], out['cat'][k])
    # groups=: the cells of 'b' are left out of the rest as well -- the same as labelling them NaN
    net.group_stats(ad, 'str', groups=['a', 'c'])
    sub = ad.uns['dca_groups']
    without_b = strings.copy()
    without_b[strings == 'b'] = None
    net.group_stats(ad, without_b)
    assert list(sub['names']) == ['a', 'c']
    for k in ARRAYS:
        np.testing.assert_array_equal(sub[k], ad.uns['dca_groups'][k])
    np.testing.assert_array_equal(sub['mean'], out['cat']['mean'][[0, 2]])
    assert np.abs(sub['scores'] - out['cat']['scores'][[0, 2]]).max() > 1e-3
    np.testing.assert_allclose(sub['scores'][0], -sub['scores'][1], rtol=1e-9)        # two groups, each against the other


@pytest.mark.parametrize('value, log1p, reference', [('denoised', False, 'rest'), ('normalized', True, 'rest'),
                                                     ('normalized', True, 1)])
def test_group_stats_against_scipy_two_pass(fitted, value, log1p, reference):
    """scores / pvals from the moments against scipy.stats.ttest_ind on the element matrix itself: 1e-9 relative + 1e-12.
    numpy's own float64 moment formula is held to the same bar on the same data first (the cancellation in
    S2 - S1^2 / n costs (1 + mean^2 / var) eps: far inside it as long as no gene is constant in a group)."""
    ad, net = fitted
    codes, K = _codes(), 3
    SpyOps.seen = []
    net.group_stats(ad, _labels(), value=value, log1p=log1p, reference=reference)
    d = ad.uns['dca_groups']
    x = np.concatenate(SpyOps.seen)
    SpyOps.seen = None
    assert x.shape == (N, G)
    ref = two_pass_stats(x, codes, K, None if reference == 'rest' else reference)
    assert (ref['var'] > 0).all()                                    # no fitted gene is constant in a group
    own = GR.stats_from_moments(*moments(x, codes, K), log1p=log1p, reference=None if reference == 'rest' else reference)
    for got in (own, d):
        for k in ('mean', 'var', 'scores', 'pvals'):
            same_nan = np.isnan(got[k]) == np.isnan(ref[k])
            assert same_nan.all(), k
            ok = ~np.isnan(ref[k])
            err = np.abs(got[k][ok] - ref[k][ok])
            assert (err <= STAT_RTOL * np.abs(ref[k][ok]) + STAT_ATOL).all(), (k, float((err / np.abs(ref[k][ok])).max()))
    if reference != 'rest':
        assert np.isnan(d['scores'][reference]).all() and np.isfinite(np.delete(d['scores'], reference, axis=0)).all()
    # Benjamini-Hochberg against its direct restatement; the fold change against its formula
    for k in range(K):
        if k != reference:
            np.testing.assert_allclose(d['pvals_adj'][k], bh(d['pvals'][k]), rtol=1e-12)
    back = np.expm1 if log1p else (lambda a: a)
    for k in range(K):
        if k == reference:
            continue
        other = (codes >= 0) & (codes != k) if reference == 'rest' else codes == reference
        lfc = np.log2((back(x[codes == k].mean(axis=0)) + 1e-9) / (back(x[other].mean(axis=0)) + 1e-9))
        np.testing.assert_allclose(d['logfoldchanges'][k], lfc, rtol=1e-9, atol=1e-12)


def test_zero_t_denominator_gives_score_zero_and_p_one():
    """A gene that is constant in the group AND in the reference: t = 0 / 0 -> score 0, p 1 (also after BH)."""
    x = np.random.default_rng(0).uniform(1, 2, size=(12, 3))
    x[:, 1] = 0.25
    codes = np.array([0, 1] * 6)
    st = GR.stats_from_moments(*moments(x, codes, 2))
    assert (st['var'][:, 1] == 0).all() and (st['scores'][:, 1] == 0).all() and (st['pvals'][:, 1] == 1).all()
    assert (st['pvals_adj'][:, 1] == 1).all() and np.isfinite(st['scores']).all() and (st['scores'][:, 0] != 0).all()
    one = GR.stats_from_moments(*moments(x[:3], np.array([0, 0, 1]), 2))           # a group of one cell: no variance
    assert np.isnan(one['var'][1]).all() and np.isnan(one['scores']).all() and np.isfinite(one['mean']).all()


def test_group_stats_of_a_gene_subset_network():
    ad = _adata()
    cols = [17, 2, 9, 11, 0]
    subset = ['g%d' % i for i in cols]
    net = _fitted('zinb-conddisp', ad, subset=subset)
    with pytest.raises(ValueError, match='output_subset'):
        net.group_stats(ad, _codes().astype(object))
    net.group_stats(ad, _codes().astype(object), output_subset=subset)
    d = ad.uns['dca_groups']
    outside = np.setdiff1d(np.arange(G), cols)
    x = np.zeros((N, G))
    x[:, cols] = net._run_predict(ad, {'mean'})['mean']
    for k in ARRAYS:
        assert d[k].shape == (4, G) and np.isnan(d[k][:, outside]).all() and np.isfinite(d[k][:3][:, cols]).all(), k
    assert list(d['names']) == [-1, 0, 1, 2]                         # an integer label -1 is a label like any other
    np.testing.assert_allclose(d['mean'][1][cols], x[_codes() == 0].mean(axis=0)[cols], rtol=1e-6)
    np.testing.assert_allclose(d['pvals_adj'][0][cols], bh(d['pvals'][0][cols]), rtol=1e-12)   # over the fitted genes only


def test_rank_genes_groups_layout(fitted):
    ad, net = fitted
    ad = ad.copy()
    net.group_stats(ad, np.array(['abc'[c] if c >= 0 else None for c in _codes()], dtype=object))
    d = ad.uns['dca_groups']
    r = GR.rank_genes_groups(ad, n_genes=7)
    assert r is ad.uns['rank_genes_groups']
    assert set(r) == {'params', 'names', 'scores', 'pvals', 'pvals_adj', 'logfoldchanges'}
    assert r['params']['reference'] == 'rest' and r['params']['method'] == 't-test'
    for k in ('names', 'scores', 'pvals', 'pvals_adj', 'logfoldchanges'):
        assert r[k].dtype.names == ('a', 'b', 'c') and r[k].shape == (7,)
    for i, g in enumerate('abc'):
        order = np.argsort(-d['scores'][i], kind='stable')[:7]
        assert list(r['names'][g]) == ['g%d' % j for j in order]
        assert (np.diff(r['scores'][g]) <= 0).all()
        np.testing.assert_array_equal(r['pvals_adj'][g], d['pvals_adj'][i, order])
    net.group_stats(ad, np.array(['abc'[c] if c >= 0 else None for c in _codes()], dtype=object), reference='b')
    r = GR.rank_genes_groups(ad, n_genes=1000, key_added='against_b')
    assert r['names'].dtype.names == ('a', 'c') and r['names'].shape == (G,) and 'against_b' in ad.uns
    lone = np.array(['abc'[c] if c >= 0 else None for c in _codes()], dtype=object)
    lone[0] = 'z'                                                    # a group of one cell: no statistics of its own
    net.group_stats(ad, lone)
    r = GR.rank_genes_groups(ad, n_genes=5)
    assert r['names'].dtype.names == ('a', 'b', 'c', 'z') and r['names'].shape == (5,)
    assert np.isfinite(r['scores']['a']).all() and np.isnan(r['scores']['z']).all()
    assert list(r['names']['z']) == ['g%d' % j for j in range(5)]


def test_group_stats_refusals(fitted):
    ad, net = fitted
    labels = _labels()
    with pytest.raises(ValueError, match='89 labels for 90 cells'):
        net.group_stats(ad, labels[:89])
    with pytest.raises(ValueError, match='no group'):
        net.group_stats(ad, np.full(N, None, dtype=object))
    with pytest.raises(ValueError, match='at most 4096'):
        net.group_stats(_adata(4100, 5), np.arange(4100))
    with pytest.raises(ValueError, match="no column 'nope'"):
        net.group_stats(ad, 'nope')
    with pytest.raises(ValueError, match="'z'"):
        net.group_stats(ad, labels, groups=[0, 'z'])
    with pytest.raises(ValueError, match='reference label 7'):
        net.group_stats(ad, labels, reference=7)
    with pytest.raises(ValueError, match='value'):
        net.group_stats(ad, labels, value='raw')
    lin = _fitted('normal', ad, ridge=0.0)
    with pytest.raises(ValueError, match="ae_type='normal'"):
        lin.group_stats(ad, labels, log1p=True)
    lin.group_stats(ad, labels)                                     # without log1p a linear mean is fine
    assert np.isfinite(ad.uns['dca_groups']['scores']).all()
    one = np.where(_codes() == 0, 'only', None).astype(object)      # one group: its moments, no statistics
    net.group_stats(ad, one)
    d = ad.uns['dca_groups']
    assert np.isfinite(d['mean']).all() and np.isfinite(d['var']).all() and d['mean'].shape == (1, G)
    for k in ('scores', 'pvals', 'pvals_adj', 'logfoldchanges'):
        assert np.isnan(d[k]).all()


# ---------------------------------------------------------------------------------------------------- command line
def _write_counts(tmp_path, n=64, g=18, seed=5):
    y = synth_counts(n, g, seed)
    genes = ['g%d' % i for i in range(g)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


def test_cli_groupstats_files(tmp_path, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    listed = [(c, 'T' if i % 3 else 'B') for i, c in enumerate(cells) if i % 5]            # every fifth cell is not listed
    with open(lab, 'w') as fh:
        fh.writelines('%s\t%s\n' % cl for cl in listed)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].group_stats

    def spy(self, adata, groupby, **kw):
        r = real(self, adata, groupby, **kw)
        seen['kw'], seen['d'] = kw, adata.uns['dca_groups']
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'group_stats', spy)
    with override_ops(GroupRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--groupstats', lab])
    assert seen['kw']['value'] == 'normalized' and seen['kw']['log1p'] is True
    d = seen['d']
    sizes = pd.read_csv(os.path.join(out, 'group_sizes.tsv'), sep='\t', index_col=0)
    assert list(sizes.index) == ['B', 'T'] and list(sizes.columns) == ['cells']
    assert sizes['cells'].tolist() == [sum(1 for _, l in listed if l == g) for g in 'BT'] == d['counts'].tolist()
    mean = pd.read_csv(os.path.join(out, 'mean.tsv'), sep='\t', index_col=0)
    for key, fmt in (('mean', '%.6f'), ('var', '%.6f'), ('scores', '%.6f'), ('pvals_adj', '%.6e'), ('logfoldchanges', '%.6f')):
        t = pd.read_csv(os.path.join(out, 'group_%s.tsv' % key), sep='\t', index_col=0)
        assert list(t.columns) == ['B', 'T'] and list(t.index) == list(mean.index) == genes and t.shape == (18, 2)
        np.testing.assert_array_equal(t.values, np.array([[float(fmt % v) for v in row] for row in d[key].T]))
    for line in open(os.path.join(out, 'group_pvals_adj.tsv')).read().splitlines()[1:]:
        assert all('e' in v and len(v.split('e')[0].split('.')[1]) == 6 for v in line.split('\t')[1:]), line
    for line in open(os.path.join(out, 'group_scores.tsv')).read().splitlines()[1:]:
        assert all(len(v.split('.')[1]) == 6 for v in line.split('\t')[1:]), line


def test_cli_groupstats_unknown_cell(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\nnot_a_cell\tA\nalso_not\tB\n')
    with override_ops(GroupRefOps):
        with pytest.raises(ValueError, match="'not_a_cell' is not a cell"):
            main([f, str(tmp_path / 'res'), '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--groupstats', lab])
    assert not os.path.exists(os.path.join(str(tmp_path / 'res'), 'mean.tsv'))       # refused before the fit
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\nc1\tB\n')
    with override_ops(GroupRefOps):
        with pytest.raises(ValueError, match="'c1' is listed more than once"):
            main([f, str(tmp_path / 'res3'), '--type', 'zinb-conddisp', '-e', '1', '-s', '8,2,8', '--groupstats', lab])
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\n')
    with override_ops(GroupRefOps):
        with pytest.raises(ValueError, match='--type normal'):
            main([f, str(tmp_path / 'res2'), '--type', 'normal', '-e', '1', '-s', '8,2,8', '--groupstats', lab])
    assert not os.path.exists(os.path.join(str(tmp_path / 'res2'), 'mean.tsv'))


def test_cli_without_groupstats_writes_todays_files(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    with override_ops(GroupRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8'])
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'latent.tsv', 'mean.tsv', 'model.pickle']
