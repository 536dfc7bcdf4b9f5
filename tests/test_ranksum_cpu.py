"""The Wilcoxon rank-sum test between groups of cells, the Python layers (dca_amd.groups.wilcoxon_from_ranks,
Engine.rank_sums, Autoencoder.group_stats(method='wilcoxon'), `dca --groupstats-method wilcoxon`) on the CPU oracle extended
with ranksum (tests/_ranksum_ref.RankSumRefOps), and the two forms of the integer reference against each other."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
from scipy.stats import mannwhitneyu, norm

from helpers import make_problem, make_engine
from _groups_ref import GroupRefOps
from _kmeans_ref import KmeansRefOps
from _ranksum_ref import RankSumRefOps, rank_ref, rank_scan, order_of
from test_groups_cpu import _adata, _codes, _labels, _fitted, _write_counts, KEYS, ARRAYS, N, G, HS
from test_counts_resident_cpu import CsrOps
from dca_amd import groups as GR
from dca_amd import prep as P
from dca_amd.__main__ import main
from dca_amd.engine import Engine
from dca_amd.network import override_ops, AE_types
from oracle.cpu_ops import CpuRefOps


class RankOps(RankSumRefOps, GroupRefOps):
    name = 'cpu-oracle-groups-ranksum'


@pytest.fixture(scope='module')
def fitted():
    ad = _adata()
    return ad, _fitted('zinb-conddisp', ad, ops=RankOps)


# ---------------------------------------------------------------------------------------------------- the integer reference
def test_the_two_reference_forms_agree():
    """Brute force / scipy.stats.rankdata against the sorted-scan form (run bounds by scans, the tie identity of a reference
    comparison): heavy ties, -0.0 beside 0.0, +-inf, empty groups, unlabelled cells, NaN rows."""
    rng = np.random.default_rng(0)
    for trial in range(40):
        n, g, K = int(rng.integers(1, 90)), 4, int(rng.integers(1, 7))
        x = rng.integers(-2, 3, size=(g, n)).astype(np.float32)
        x[x == 0] = rng.choice(np.float32([0.0, -0.0]), size=int((x == 0).sum()))
        x[0, rng.integers(0, n)] = np.inf
        x[1, rng.integers(0, n)] = -np.inf
        x[3] = rng.standard_normal(n)
        if trial % 5 == 0:
            x[2, rng.integers(0, n)] = np.nan
        codes = rng.integers(-1, K, size=n)
        if K > 2:
            codes[codes == 1] = 0                                  # an empty group
        order, gstart, counts = order_of(codes, K)
        for ref in [-1] + list(range(K)):
            a, b = rank_ref(x, order, gstart, K, ref), rank_scan(x, order, gstart, K, ref)
            assert a[0].dtype == a[1].dtype == np.int64
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
            nan_row = np.isnan(x[:, order]).any(axis=1)
            assert ((a[0] == -1).all(axis=0) == nan_row).all() and ((a[1] == -1).all(axis=0) == nan_row).all()
            if ref < 0:
                m = len(order)
                assert (a[0][:, ~nan_row].sum(axis=0) == m * (m + 1)).all()
            else:
                assert (a[0][counts == 0] <= 0).all()             # an empty group: rank2 = 0 (or the row's -1)


# ---------------------------------------------------------------------------------------------------- wilcoxon_from_ranks
def _tied_sample(seed=1, n=70, g=9, K=3):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 5, size=(g, n)).astype(np.float32)
    x[0] = rng.standard_normal(n)                                  # one gene without ties
    codes = rng.integers(0, K, size=n)
    codes[::11] = -1
    return x, codes, order_of(codes, K)


@pytest.mark.parametrize('reference', [None, 2])
def test_statistics_equal_scipy_mannwhitneyu(reference):
    """U exactly; the p-value at rtol 1e-9 (float64 arithmetic on exact integers on both sides); scipy always applies the
    tie correction, so this is tie_correct=True."""
    K = 3
    x, codes, (order, gstart, counts) = _tied_sample()
    r2, tie = rank_ref(x, order, gstart, K, -1 if reference is None else reference)
    st = GR.wilcoxon_from_ranks(r2, tie, counts, reference, tie_correct=True)
    for k in ('scores', 'pvals', 'pvals_adj', 'auroc', 'U'):
        assert st[k].dtype == np.float64 and st[k].shape == (K, x.shape[0])
    for c in range(K):
        if c == reference:
            for k in ('scores', 'pvals', 'pvals_adj', 'auroc'):
                assert np.isnan(st[k][c]).all()
            continue
        a = x[:, codes == c].astype(np.float64)
        b = x[:, (codes >= 0) & (codes != c)] if reference is None else x[:, codes == reference]
        U, p = mannwhitneyu(a, b.astype(np.float64), use_continuity=False, method='asymptotic', axis=1)
        np.testing.assert_array_equal(st['U'][c], U)
        np.testing.assert_allclose(st['pvals'][c], p, rtol=1e-9)
        np.testing.assert_array_equal(st['auroc'][c], U / (a.shape[1] * b.shape[1]))
        assert (np.sign(st['scores'][c]) == np.sign(U - a.shape[1] * b.shape[1] / 2)).all()


def test_without_tie_correction_it_is_scanpys_formula():
    """scanpy, rank_genes_groups(method='wilcoxon', tie_correct=False): z = (R - n_c (N + 1) / 2) / sqrt(n_c n_rest (N + 1) / 12),
    p = 2 norm.sf(|z|); R the rank sum of the group among all N cells."""
    from scipy.stats import rankdata
    K = 3
    x, codes, (order, gstart, counts) = _tied_sample(seed=2)
    r2, tie = rank_ref(x, order, gstart, K, -1)
    st = GR.wilcoxon_from_ranks(r2, tie, counts, None, tie_correct=False)
    lab = codes >= 0
    Nn = int(lab.sum())
    ranks = rankdata(x[:, lab].astype(np.float64), axis=1)
    for c in range(K):
        nc = int((codes == c).sum())
        R = ranks[:, codes[lab] == c].sum(axis=1)
        z = (R - nc * (Nn + 1) / 2.0) / np.sqrt(nc * (Nn - nc) * (Nn + 1) / 12.0)
        np.testing.assert_allclose(st['scores'][c], z, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(st['pvals'][c], 2 * norm.sf(np.abs(z)), rtol=1e-12)
    corrected = GR.wilcoxon_from_ranks(r2, tie, counts, None, tie_correct=True)
    moved = st['scores'][:, 1:] != 0                                                         # a z of exactly 0 stays 0
    assert moved.sum() > 16 and (np.abs(corrected['scores'][:, 1:]) > np.abs(st['scores'][:, 1:]))[moved].all()   # ties shrink the variance
    np.testing.assert_array_equal(corrected['scores'][:, 0], st['scores'][:, 0])             # gene 0 has no ties


def test_zero_sigma_empty_side_and_nan_conventions():
    K = 3
    x = np.full((2, 12), 0.25, np.float32)                           # gene 0 constant: with the correction sigma = 0
    x[1] = np.arange(12)
    codes = np.array([0, 2] * 6)                                     # group 1 is empty
    order, gstart, counts = order_of(codes, K)
    for reference in (None, 2):
        r2, tie = rank_ref(x, order, gstart, K, -1 if reference is None else reference)
        st = GR.wilcoxon_from_ranks(r2, tie, counts, reference, tie_correct=True)
        assert st['scores'][0, 0] == 0 and st['pvals'][0, 0] == 1 and st['pvals_adj'][0, 0] == 1 and st['auroc'][0, 0] == 0.5
        assert np.isfinite(st['scores'][0, 1]) and st['scores'][0, 1] != 0
        for k in ('scores', 'pvals', 'pvals_adj', 'auroc'):
            assert np.isnan(st[k][1]).all(), k                       # the empty group
        plain = GR.wilcoxon_from_ranks(r2, tie, counts, reference, tie_correct=False)
        assert plain['scores'][0, 0] == 0 and plain['pvals'][0, 0] == 1          # U at its mean: z = 0 either way
    against_empty = GR.wilcoxon_from_ranks(*rank_ref(x, order, gstart, K, 1), counts, 1)
    assert all(np.isnan(against_empty[k]).all() for k in ('scores', 'pvals', 'auroc'))
    x[1, 3] = np.nan                                                 # a gene marked -1: NaN in that column alone
    r2, tie = rank_ref(x, order, gstart, K, -1)
    st = GR.wilcoxon_from_ranks(r2, tie, counts, None)
    assert np.isnan(st['scores'][:, 1]).all() and np.isnan(st['auroc'][:, 1]).all() and np.isfinite(st['scores'][[0, 2], 0]).all()
    one = GR.wilcoxon_from_ranks(*rank_ref(x[:1], order[:6], np.array([0, 6]), 1, -1), np.array([6]), None)
    assert np.isnan(one['scores']).all()                             # a single group: nothing to compare it with


# ---------------------------------------------------------------------------------------------------- Engine.rank_sums
@pytest.mark.parametrize('ae_type, subset', [('zinb-conddisp', None), ('nb', None), ('normal', None), ('zinb-shared', None),
                                             ('zinb-conddisp', ['g%d' % i for i in (17, 2, 9, 11, 0)])])
def test_engine_rank_sums_against_predict(ae_type, subset):
    """The oracle ops rank what the engine hands them; the reference ranks predict()'s output: equal integers, in one block
    and in blocks of 4 genes with ragged chunks."""
    ad = _adata()
    net = _fitted(ae_type, ad, ops=RankOps, subset=subset)
    codes, K = _codes(), 3
    x = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float32)
    order, gstart, counts = order_of(codes, K)
    net._bind_inputs(ad)
    for ref in (None, 1):
        want = rank_ref(np.ascontiguousarray(x.T), order, gstart, K, -1 if ref is None else ref)
        for kw in (dict(chunk=N), dict(gene_block=4, chunk=64)):
            res = net.engine.rank_sums(codes, K, reference=ref, **kw)
            assert res['rank2'].dtype == res['tie'].dtype == res['count'].dtype == torch.int64
            assert res['rank2'].shape == res['tie'].shape == (K, x.shape[1]) and res['count'].shape == (K,)
            np.testing.assert_array_equal(res['count'].numpy(), counts)
            np.testing.assert_array_equal(res['rank2'].numpy(), want[0])
            np.testing.assert_array_equal(res['tie'].numpy(), want[1])
    if ae_type != 'normal':
        sf = ad.obs['size_factors'].values.astype(np.float32)[:, None]
        res = net.engine.rank_sums(codes, K, no_sf=True, log1p=True, gene_block=5, chunk=64)
        m = len(order)
        assert (res['rank2'].numpy().sum(axis=0) == m * (m + 1)).all() and sf.shape == (N, 1)
    none = net.engine.rank_sums(np.full(N, -1, np.int32), K)
    assert not none['rank2'].any() and not none['tie'].any() and not none['count'].any()


def test_engine_rank_sums_refusals():
    X, Y, sf, p = make_problem(40, 9, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(GroupRefOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    codes = np.zeros(40, np.int32)
    with pytest.raises(NotImplementedError, match=GroupRefOps.name):
        eng.rank_sums(codes, 1)
    eng = make_engine(RankOps(), 'zinb-conddisp', 9, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(ValueError, match='4096'):
        eng.rank_sums(codes, 4097)
    with pytest.raises(ValueError, match='one per cell'):
        eng.rank_sums(codes[:39], 1)
    with pytest.raises(ValueError, match='one per cell'):
        eng.rank_sums(codes.astype(np.float32), 1)
    for bad in (-2, 1):
        c = codes.copy()
        c[7] = bad
        with pytest.raises(ValueError, match='codes must lie'):
            eng.rank_sums(c, 1)
    with pytest.raises(ValueError, match='reference group'):
        eng.rank_sums(codes, 2, reference=2)
    with pytest.raises(ValueError, match='gene_block'):
        eng.rank_sums(codes, 1, gene_block=0)
    lin = make_engine(RankOps(), 'normal', 9, HS, True, 0.0, make_problem(40, 9, HS, 'normal', seed=6)[3], X, Y, sf)
    with pytest.raises(ValueError, match='log1p'):
        lin.rank_sums(codes, 1, log1p=True)
    fresh = Engine('zinb-conddisp', 9, 9, HS, True, 0.05, ops=RankOps())
    with pytest.raises(ValueError, match='needs data'):
        fresh.rank_sums(codes, 1)

    class TwoRanks:
        rank, world, dp = 0, 2, False
    eng.comm = TwoRanks()
    with pytest.raises(ValueError, match='data-parallel'):
        eng.rank_sums(codes, 1)


class RankCsrOps(RankOps, CsrOps):
    pass


class RankKmeansOps(RankOps, KmeansRefOps):
    pass


def test_counts_resident_rank_sums_equal_the_dense_ones():
    ops = RankCsrOps()
    _, Y, sf, _ = make_problem(75, 18, (6, 3, 6), 'zinb-conddisp', True, seed=3)
    Ys = sp.csr_matrix(Y)
    n, g = Ys.shape
    csr = P.upload_csr(Ys, torch.device('cpu'), ops)
    fac = torch.as_tensor(np.linspace(0.5, 1.5, n).astype(np.float32))
    norm_ = P.csr_norm(ops, csr, fac, True, True)
    Xd, Yd = torch.zeros(n, P._r4(g)), torch.zeros(n, P._r4(g))
    ops.csr_gather(csr, None, None, 0, n, None, norm_['fac'], True, norm_['mean'], norm_['std'], Yd, Yd.shape[1], Xd,
                   Xd.shape[1], None, None)
    codes = _codes(n, 3)
    res = []
    for form in ('dense', 'counts'):
        eng = Engine('zinb-conddisp', g, g, (6, 3, 6), True, 0.0, ops=ops)
        eng.init_params(seed=7)
        if form == 'dense':
            eng.attach_device_data(Xd, Yd, torch.as_tensor(sf), norm=norm_)
        else:
            eng.attach_counts(csr, torch.as_tensor(sf), norm_)
        res.append(eng.rank_sums(codes, 3, reference=0, gene_block=7, chunk=32))
    for k in ('rank2', 'tie', 'count'):
        assert torch.equal(res[0][k], res[1][k]), k
    assert int(res[0]['rank2'].sum()) > 0


# ---------------------------------------------------------------------------------------------------- group_stats
WKEYS = KEYS + ['auroc', 'method', 'tie_correct']


def test_group_stats_wilcoxon_keys_dtypes_and_values(fitted):
    ad, net = fitted
    ad = ad.copy()
    codes = _codes()
    ad.obs['cluster'] = pd.Categorical(['abc'[c] if c >= 0 else None for c in codes])
    net.group_stats(ad, 'cluster')
    plain = ad.uns['dca_groups']
    assert list(plain) == KEYS                                       # the default stores what it stored
    res = net.group_stats(ad, 'cluster', method='wilcoxon', copy=True)
    d = res.uns['dca_groups']
    assert list(d) == WKEYS and d['method'] == 'wilcoxon' and d['tie_correct'] is False
    for k in ARRAYS + ['auroc']:
        assert d[k].dtype == np.float64 and d[k].shape == (3, G) and np.isfinite(d[k]).all(), k
    for k in ('mean', 'var', 'logfoldchanges'):                      # these still come from the moments
        np.testing.assert_array_equal(d[k], plain[k])
    assert np.abs(d['scores'] - plain['scores']).max() > 1e-3 and ((d['auroc'] >= 0) & (d['auroc'] <= 1)).all()
    x = np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float32).astype(np.float64)
    inside = codes >= 0
    for k in range(3):
        U, p = mannwhitneyu(x[codes == k], x[inside & (codes != k)], use_continuity=False, method='asymptotic', axis=0)
        np.testing.assert_array_equal(d['auroc'][k], U / ((codes == k).sum() * (inside & (codes != k)).sum()))
        np.testing.assert_allclose(d['pvals_adj'][k], GR.benjamini_hochberg(d['pvals'][k]), rtol=1e-12)
    net.group_stats(ad, 'cluster', method='wilcoxon', tie_correct=True, reference='b', value='normalized', log1p=True)
    d = ad.uns['dca_groups']
    assert d['tie_correct'] is True and np.isnan(d['scores'][1]).all() and np.isnan(d['auroc'][1]).all()
    assert np.isfinite(d['scores'][[0, 2]]).all() and np.isfinite(d['mean']).all()
    sfac = ad.obs['size_factors'].values.astype(np.float32)[:, None]
    xl = np.log1p(np.asarray(net._run_predict(ad, {'mean'})['mean'], np.float32) / sfac).astype(np.float64)
    _, p = mannwhitneyu(xl[codes == 0], xl[codes == 1], use_continuity=False, method='asymptotic', axis=0)
    assert np.median(np.abs(np.log(d['pvals'][0] / p))) < 0.5        # the same test (the host route rounds log1p differently)


def test_group_stats_wilcoxon_refusals_single_group_and_subset(fitted):
    ad, net = fitted
    labels = _labels()
    with pytest.raises(ValueError, match='method'):
        net.group_stats(ad, labels, method='logreg')
    with pytest.raises(ValueError, match='tie_correct'):
        net.group_stats(ad, labels, tie_correct=True)
    lin = _fitted('normal', ad, ops=RankOps, ridge=0.0)
    with pytest.raises(ValueError, match="ae_type='normal'"):
        lin.group_stats(ad, labels, log1p=True, method='wilcoxon')
    no_rank = _fitted('zinb-conddisp', ad, ops=GroupRefOps)
    with pytest.raises(NotImplementedError, match='ranksum'):
        no_rank.group_stats(ad, labels, method='wilcoxon')
    one = np.where(_codes() == 0, 'only', None).astype(object)
    net.group_stats(ad, one, method='wilcoxon')
    d = ad.uns['dca_groups']
    assert np.isfinite(d['mean']).all() and d['mean'].shape == (1, G)
    for k in ('scores', 'pvals', 'pvals_adj', 'logfoldchanges', 'auroc'):
        assert np.isnan(d[k]).all()
    cols = [17, 2, 9, 11, 0]
    subset = ['g%d' % i for i in cols]
    sub = _fitted('zinb-conddisp', ad, ops=RankOps, subset=subset)
    sub.group_stats(ad, labels, output_subset=subset, method='wilcoxon')
    d = ad.uns['dca_groups']
    outside = np.setdiff1d(np.arange(G), cols)
    for k in ARRAYS + ['auroc']:
        assert d[k].shape == (3, G) and np.isnan(d[k][:, outside]).all() and np.isfinite(d[k][:, cols]).all(), k


def test_rank_genes_groups_reports_the_method(fitted):
    ad, net = fitted
    ad = ad.copy()
    lab = np.array(['abc'[c] if c >= 0 else None for c in _codes()], dtype=object)
    net.group_stats(ad, lab)
    assert GR.rank_genes_groups(ad, n_genes=5)['params']['method'] == 't-test'
    net.group_stats(ad, lab, method='wilcoxon')
    d = ad.uns['dca_groups']
    r = GR.rank_genes_groups(ad, n_genes=7)
    assert r['params']['method'] == 'wilcoxon' and set(r) == {'params', 'names', 'scores', 'pvals', 'pvals_adj', 'logfoldchanges'}
    for i, g in enumerate('abc'):
        order = np.argsort(-d['scores'][i], kind='stable')[:7]
        assert list(r['names'][g]) == ['g%d' % j for j in order]


# ---------------------------------------------------------------------------------------------------- command line
BASE = ['--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8']


def _labels_file(tmp_path, cells):
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.writelines('%s\t%s\n' % (c, 'T' if i % 3 else 'B') for i, c in enumerate(cells) if i % 5)
    return lab


def test_cli_wilcoxon_files(tmp_path, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    lab = _labels_file(tmp_path, cells)
    seen = {}
    real = AE_types['zinb-conddisp'].group_stats

    def spy(self, adata, groupby, **kw):
        r = real(self, adata, groupby, **kw)
        seen['kw'], seen['d'] = kw, adata.uns['dca_groups']
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'group_stats', spy)
    out = str(tmp_path / 'res')
    with override_ops(RankOps):
        main([f, out] + BASE + ['--groupstats', lab, '--groupstats-method', 'wilcoxon', '--groupstats-tie-correct'])
    assert seen['kw']['method'] == 'wilcoxon' and seen['kw']['tie_correct'] is True and seen['kw']['log1p'] is True
    d = seen['d']
    for key, fmt in (('scores', '%.6f'), ('pvals_adj', '%.6e'), ('auroc', '%.6f'), ('mean', '%.6f')):
        t = pd.read_csv(os.path.join(out, 'group_%s.tsv' % key), sep='\t', index_col=0)
        assert list(t.columns) == ['B', 'T'] and list(t.index) == genes
        np.testing.assert_array_equal(t.values, np.array([[float(fmt % v) for v in row] for row in d[key].T]))
    # without the flag: today's files, no group_auroc.tsv, and no new argument reaches group_stats
    out2 = str(tmp_path / 'res2')
    with override_ops(RankOps):
        main([f, out2] + BASE + ['--groupstats', lab])
    assert 'method' not in seen['kw'] and 'tie_correct' not in seen['kw'] and list(seen['d']) == KEYS
    assert sorted(x for x in os.listdir(out2) if x.startswith('group_')) == [
        'group_logfoldchanges.tsv', 'group_mean.tsv', 'group_pvals_adj.tsv', 'group_scores.tsv', 'group_sizes.tsv', 'group_var.tsv']
    assert sorted(set(os.listdir(out)) - set(os.listdir(out2))) == ['group_auroc.tsv']
    out3 = str(tmp_path / 'res3')
    with override_ops(RankKmeansOps):
        main([f, out3] + BASE + ['--kmeans', '2', '--kmeansstats', '--groupstats-method', 'wilcoxon'])
    assert os.path.exists(os.path.join(out3, 'group_auroc.tsv')) and seen['kw']['tie_correct'] is False


def test_cli_wilcoxon_refusals_come_before_the_fit(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = _labels_file(tmp_path, cells)
    for i, (extra, msg) in enumerate([(['--groupstats-method', 'wilcoxon'], '--groupstats FILE or --kmeansstats'),
                                      (['--groupstats', lab, '--groupstats-tie-correct'], '--groupstats-method wilcoxon'),
                                      (['--groupstats', lab, '--groupstats-method', 't-test', '--groupstats-tie-correct'],
                                       '--groupstats-method wilcoxon')]):
        out = str(tmp_path / ('r%d' % i))
        with override_ops(RankOps):
            with pytest.raises(ValueError, match=msg):
                main([f, out] + BASE + extra)
        assert not os.path.exists(os.path.join(out, 'mean.tsv'))
    with pytest.raises(SystemExit):
        main([f, str(tmp_path / 'r9')] + BASE + ['--groupstats', lab, '--groupstats-method', 'logreg'])
