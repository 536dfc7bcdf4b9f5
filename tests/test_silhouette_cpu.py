"""The silhouette above the kernel -- dca_amd.silhouette, Engine.latent_silhouette, Autoencoder.silhouette, `dca --silhouette` --
on the CPU oracle extended with silhouette (tests/_silhouette_ref.SilhouetteRefOps), and the references themselves: the fp64
reference against scikit-learn, its conventions, the fp32 restatement against the float criterion on the cases of the GPU
test, and the exactness premise of the GPU test's integer cases."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _knn_ref import d2_ref, direct_fp32, clustered
from _kmeans_ref import int_data, kmeans_ref
from _groups_ref import GroupRefOps
from _silhouette_ref import (SilhouetteRefOps, silhouette_ref, silhouette_from_delta, delta_fp32,
                             assert_silhouette_close, edge_labels, float_labels, float_ref, EXACT, FLOAT_CASES, FLOAT_N)
from dca_amd import io
from dca_amd import silhouette as sil
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 4, 8)


class BothRefOps(SilhouetteRefOps, GroupRefOps):
    name = 'cpu-oracle-silhouette-groups'


# ---------------------------------------------------------------------------------------------------- the references
def test_reference_against_scikit_learn():
    metrics = pytest.importorskip('sklearn.metrics')
    for d, k in ((3, 5), (32, 12)):
        X = clustered(400, d)
        lab = kmeans_ref(X, k, n_init=1)['labels']
        lab[:3] = [0, 1, 2]
        ref = silhouette_ref(X, lab, k)
        X64 = X.astype(np.float64)
        np.testing.assert_allclose(ref['s'], metrics.silhouette_samples(X64, lab), rtol=0, atol=1e-6)   # sklearn: the Gram form
        assert abs(ref['mean'] - metrics.silhouette_score(X64, lab)) <= 1e-6
    X = np.random.RandomState(0).normal(size=(60, 4)).astype(np.float32)
    lab = np.random.RandomState(1).randint(0, 4, 60)
    lab[lab == 3] = 0
    lab[17] = 3                                                                # a singleton scores 0 there too
    got = silhouette_ref(X, lab, 4)
    np.testing.assert_allclose(got['s'], metrics.silhouette_samples(X.astype(np.float64), lab), rtol=0, atol=1e-6)
    assert got['s'][17] == 0.0


def test_reference_conventions():
    X = np.asarray([[0, 0], [0, 3], [4, 0], [4, 3], [10, 0], [7, 7]], np.float32)
    codes = np.asarray([0, 0, 1, 1, 3, -1], np.int32)                          # cluster 2 empty, 3 a singleton, one unlabelled
    r = silhouette_ref(X, codes, 5)
    assert r['counts'].tolist() == [2, 2, 0, 1, 0]
    assert r['a'][0] == 3.0 and r['b'][0] == (4.0 + 5.0) / 2 and r['nearest'][0] == 1
    assert r['s'][0] == (4.5 - 3.0) / 4.5
    assert r['s'][4] == 0.0 and r['a'][4] == 0.0 and r['b'][4] == (6.0 + math.sqrt(45.0)) / 2 and r['nearest'][4] == 1
    assert np.isnan([r['s'][5], r['a'][5], r['b'][5]]).all() and r['nearest'][5] == -1
    assert r['S'][0, 1] == 9.0 and (r['S'][:, 2] == 0).all()                   # the unlabelled point is no candidate either
    assert np.isnan(r['cluster_mean'][[2, 4]]).all() and r['cluster_mean'][3] == 0.0
    assert r['mean'] == r['s'][:5].sum() / 5
    # equal mean distances: the lowest cluster
    X = np.asarray([[0, 0], [-2, 0], [2, 0], [0, 1]], np.float32)
    assert silhouette_ref(X, [0, 1, 2, 0], 3)['nearest'][0] == 1
    # all points equal: every distance 0, max(a, b) = 0 -> s = 0
    X = np.tile(np.asarray([[1.5, -2.0, 3.0]], np.float32), (7, 1))
    r = silhouette_ref(X, [0, 1, 0, 1, 2, 2, 2], 3)
    assert (r['s'] == 0).all() and (r['a'] == 0).all() and (r['b'] == 0).all() and (r['nearest'] == [1, 0, 1, 0, 0, 0, 0]).all()
    # fewer than two non-empty clusters: b = inf, nearest = -1, s = NaN
    X = np.random.RandomState(0).normal(size=(9, 3)).astype(np.float32)
    r = silhouette_ref(X, [1] * 8 + [-1], 4)
    assert np.isinf(r['b'][:8]).all() and (r['nearest'] == -1).all() and np.isnan(r['s']).all() and np.isnan(r['mean'])
    assert np.isfinite(r['a'][:8]).all() and np.isnan(r['a'][8])
    r = silhouette_ref(X, [-1] * 9, 2)
    assert np.isnan(r['s']).all() and np.isnan(r['mean']) and r['counts'].tolist() == [0, 0]


@pytest.mark.parametrize('d,k', FLOAT_CASES)
def test_fp32_restatement_meets_the_float_criterion(d, k):
    """The kernel's arithmetic evaluated on the host (sequential fp32 direct form, np.sqrt in float32, double sums) on the
    float cases of tests/test_silhouette_gpu.py: the bounds are a property of the arithmetic, not of a device."""
    X = clustered(FLOAT_N, d)
    D = delta_fp32(X)
    for kind in ('random', 'kmeans'):
        codes = float_labels(d, k, kind)
        ref = float_ref(d, k, kind)
        got = silhouette_from_delta(D, codes, k)
        assert_silhouette_close(got, ref, d, codes, k, what='fp32 on the host %s' % kind)
        if kind == 'random':
            assert np.abs(ref['s']).max() < 0.5                                # random labels: s near 0, clusters nearly tied


@pytest.mark.parametrize('n,d,k', EXACT + [(2100, 5, 7)])
def test_exactness_premise_of_the_integer_cases(n, d, k):
    """What lets the GPU test ask for equal bits for every number of splits: on int_data the fp32 direct form is exact, and
    the per-cluster sums of the fp32 square roots are exact in double -- equal under a permutation of the candidates and
    equal to math.fsum (d2 <= 2^13, so a term is an fp32 value below 2^7 with granularity >= 2^-23, and 2^12 of them need 42
    bits)."""
    X, _ = int_data(n, d, k)
    assert (np.abs(X) <= 4).all() and (X == np.round(X)).all()
    d2 = direct_fp32(X, X)
    np.testing.assert_array_equal(d2.astype(np.float64), d2_ref(X, X))
    assert d2.max() <= 2.0 ** 13
    codes = edge_labels(n, k)
    D = np.sqrt(d2).astype(np.float64)
    r = silhouette_from_delta(D, codes, k)
    rs = np.random.RandomState(n + d + k)
    for c in np.flatnonzero(r['counts']):
        members = np.flatnonzero(codes == c)
        perm = rs.permutation(len(members))
        for i in range(0, n, max(1, n // 12)):
            vals = D[i, members]
            assert r['S'][i, c] == math.fsum(vals) == np.cumsum(vals)[-1] == np.cumsum(vals[perm])[-1]
    # the labels carry the edges they are meant to carry
    if n >= 8:
        assert (codes == -1).sum() == 2 and (codes >= k).sum() == 2 and r['counts'][0] >= 0.7 * n
        if k > 2:
            assert r['counts'][1] == 1 and r['counts'][k - 1] == 0
    assert (r['counts'] > 0).sum() >= 2
    if n > 5:
        assert (X[5] == X[2]).all() and (X[n - 1] == X[0]).all()              # the duplicated rows


# ---------------------------------------------------------------------------------------------------- the module
def test_silhouette_on_the_oracle_equals_the_reference():
    X = clustered(300, 5)
    ops = SilhouetteRefOps()
    names = np.asarray(['b', 'a', 'c'], dtype=object)[kmeans_ref(X, 3, n_init=1)['labels']]
    names[[4, 40]] = None
    names[9] = np.nan
    res = sil.silhouette(X, names, ops=ops)
    codes = np.asarray([{'a': 0, 'b': 1, 'c': 2}.get(v, -1) for v in names], np.int32)
    ref = silhouette_ref(X, codes, 3)
    assert res.names == ['a', 'b', 'c'] and isinstance(res.mean, float) and res.mean == ref['mean']
    for got, want, dt in ((res.samples, ref['s'], np.float64), (res.intra, ref['a'], np.float64),
                          (res.nearest_dist, ref['b'], np.float64), (res.nearest, ref['nearest'], np.int32),
                          (res.cluster_mean, ref['cluster_mean'], np.float64), (res.sizes, ref['counts'], np.int64)):
        assert isinstance(got, np.ndarray) and got.dtype == dt
        np.testing.assert_array_equal(got, want)
    assert np.isnan(res.samples[[4, 9, 40]]).all() and (res.nearest[[4, 9, 40]] == -1).all()
    # a pandas categorical and integer labels name the same clusters
    cat = sil.silhouette(X, pd.Categorical(names), ops=ops)
    np.testing.assert_array_equal(cat.samples, res.samples)
    shifted = sil.silhouette(X[codes >= 0], codes[codes >= 0] * 10 + 7, ops=ops)           # integer labels: sorted, not 0-based
    assert shifted.names == [7, 17, 27]
    np.testing.assert_array_equal(shifted.samples, res.samples[codes >= 0])
    # an int32 code tensor on the ops' device is passed through as it is: codes 0 .. max, anything else in no cluster
    ct = torch.from_numpy(codes)
    dev = sil.silhouette(torch.from_numpy(X), ct, ops=ops)
    assert dev.names == [0, 1, 2]
    np.testing.assert_array_equal(np.asarray(dev.samples), ref['s'])


def test_silhouette_refusals():
    ops = SilhouetteRefOps()
    X = clustered(50, 4)
    lab = np.arange(50) % 3
    for call, what in ((lambda: sil.silhouette(X, np.zeros(50, int), ops=ops), '1 distinct label'),
                       (lambda: sil.silhouette(X, [None] * 50, ops=ops), '0 distinct labels'),
                       (lambda: sil.silhouette(X[:, 0], lab, ops=ops), '2-d array'),
                       (lambda: sil.silhouette(X, lab[:49], ops=ops), '49 labels for 50 points'),
                       (lambda: sil.silhouette(X, lab.reshape(10, 5), ops=ops), '1-d array'),
                       (lambda: sil.silhouette(np.zeros((300, 2), np.float32), np.arange(300), ops=ops), 'at most 256'),
                       (lambda: sil.silhouette(np.zeros((50, 129), np.float32), lab, ops=ops), '1 .. 128 coordinates')):
        with pytest.raises(ValueError, match=what):
            call()
    Xb = X.copy()
    Xb[7, 1] = np.nan
    with pytest.raises(ValueError, match='1 coordinates are not finite'):
        sil.silhouette(Xb, lab, ops=ops)
    with pytest.raises(ValueError, match='1 cluster with points'):
        ops.silhouette(torch.from_numpy(X), torch.full((50,), 2, dtype=torch.int32), 4)


def test_check_silhouette_args_names_the_limit():
    sil.check_silhouette_args(0, 1, 2, 0)
    sil.check_silhouette_args((1 << 31) - 1, 128, 256, 64)
    for args, what in (((10, 4, 1), r'2 \.\. 256 \(got 1\)'), ((10, 4, 257), r'2 \.\. 256 \(got 257\)'),
                       ((10, 0, 3), r'1 \.\. 128 coordinates \(got 0\)'), ((10, 129, 3), r'1 \.\. 128 coordinates \(got 129\)'),
                       ((-1, 4, 3), r'2\^31 - 1 points \(got -1\)'), ((1 << 31, 4, 3), r'2\^31 - 1 points'),
                       ((10, 4, 3, -1), r'1 \.\. 64 \(got -1\)'), ((10, 4, 3, 65), r'1 \.\. 64 \(got 65\)')):
        with pytest.raises(ValueError, match='silhouette: .*' + what):
            sil.check_silhouette_args(*args)
    ops = SilhouetteRefOps()
    with pytest.raises(ValueError, match='silhouette'):
        ops.silhouette_workspace_bytes(10, 4, 3, 65)
    with pytest.raises(ValueError, match='silhouette'):
        ops.silhouette_splits(10, 4, 1)


def _blobs(n_per=40, d=4, seed=0):
    rs = np.random.RandomState(seed)
    centres = np.asarray([[0] * d, [20] * d, [-20] + [20] * (d - 1)], np.float64)
    return np.concatenate([c + rs.normal(0, 1, (n_per, d)) for c in centres]).astype(np.float32)


def test_choose_k_on_three_blobs():
    X = _blobs()
    ops = SilhouetteRefOps()
    res = sil.choose_k(X, [2, 3, 4, 5], n_init=2, seed=1, ops=ops)
    assert res.best_k == 3
    t = res.table
    assert list(t.columns) == ['k', 'inertia', 'silhouette', 'n_iter', 'converged', 'smallest_cluster']
    assert t['k'].tolist() == [2, 3, 4, 5] and (np.diff(t['inertia']) < 0).all()   # the inertia cannot choose k
    assert t['silhouette'].idxmax() == 1 and t['smallest_cluster'][1] == 40 and t['converged'].all()
    for row in t.itertuples():
        km = kmeans_ref(X, row.k, n_init=2, seed=1)
        assert row.inertia == km['inertia'] and row.silhouette == silhouette_ref(X, km['labels'], row.k)['mean']
    for ks, what in (([], 'no k'), ([1, 2], r'2 \.\. 256'), ([2, 121], '121 clusters of 120 points')):
        with pytest.raises(ValueError, match=what):
            sil.choose_k(X, ks, ops=ops)


# ---------------------------------------------------------------------------------------------------- through the model
def _adata(n=90, G=21, seed=3):
    ad = AnnData(synth_counts(n, G, seed).astype(np.float32),
                 obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                 var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
    ad = io.read_dataset(ad, copy=True)
    return io.normalize(ad, device=False)


def _fitted(ad, hidden=HS):
    net = AE_types['zinb-conddisp'](input_size=ad.n_vars, output_size=ad.n_vars, hidden_size=hidden, ridge=0.05)
    net.build()
    train(ad, net, epochs=2, batch_size=32, verbose=False)
    return net


def test_autoencoder_silhouette_keys_dtypes_and_values():
    ad = _adata()
    n, k = ad.n_obs, 4
    with override_ops(SilhouetteRefOps):
        net = _fitted(ad)
        net.cluster(ad, k, n_init=2, seed=4)
        before = (ad.X.copy(), sorted(ad.obs.columns), sorted(ad.uns.keys()))
        res = net.silhouette(ad, copy=True)
        assert res is not ad and sorted(ad.obs.columns) == before[1] and sorted(ad.uns.keys()) == before[2]
        assert net.silhouette(ad) is None                                      # in place, like predict
        np.testing.assert_array_equal(ad.X, before[0])
        lab = np.asarray(['t%d' % (i % 3) for i in range(n)], dtype=object)
        lab[[5, 6]] = None
        net.silhouette(ad, groupby=lab, key_added='by_type')
    Z = ad.obsm['X_dca']
    col = ad.obs['dca_kmeans']
    live = sorted(set(np.asarray(col).astype(str)))                            # the sorted labels: strings
    codes = np.asarray([live.index(v) for v in np.asarray(col).astype(str)], np.int32)
    ref = silhouette_ref(Z, codes, len(live))
    for a in (res, ad):
        np.testing.assert_array_equal(a.obsm['X_dca'], Z)
        assert a.obs['dca_silhouette'].dtype == np.float64
        np.testing.assert_array_equal(np.asarray(a.obs['dca_silhouette']), ref['s'])
        assert np.asarray(a.obs['dca_silhouette_nearest']).tolist() == [live[c] for c in ref['nearest']]
        u = a.uns['dca_silhouette']
        assert set(u) == {'groupby', 'names', 'sizes', 'cluster_mean', 'mean', 'params'}
        assert u['groupby'] == 'dca_kmeans' and list(u['names']) == live and u['params'] == {'metric': 'euclidean'}
        assert u['sizes'].dtype == np.int64 and u['cluster_mean'].dtype == np.float64 and isinstance(u['mean'], float)
        np.testing.assert_array_equal(u['sizes'], ref['counts'])
        np.testing.assert_array_equal(u['cluster_mean'], ref['cluster_mean'])
        assert u['mean'] == ref['mean']
    t = ad.uns['by_type']
    assert t['groupby'] is None and list(t['names']) == ['t0', 't1', 't2'] and t['sizes'].sum() == n - 2
    s = np.asarray(ad.obs['by_type'])
    assert np.isnan(s[[5, 6]]).all() and np.isfinite(np.delete(s, [5, 6])).all()
    near = np.asarray(ad.obs['by_type_nearest'], dtype=object)
    assert near[5] is None and near[6] is None and set(np.delete(near, [5, 6])) <= {'t0', 't1', 't2'}
    assert (np.delete(near, [5, 6]) != np.delete(lab, [5, 6])).all()


def test_autoencoder_silhouette_refusals():
    ad = _adata(n=40)
    with override_ops(SilhouetteRefOps):
        net = _fitted(ad)
        with pytest.raises(ValueError, match="no column 'dca_kmeans'"):
            net.silhouette(ad)
        with pytest.raises(ValueError, match='1 distinct label'):
            net.silhouette(ad, groupby=np.zeros(40, int))
        with pytest.raises(ValueError, match='39 labels for 40 cells'):
            net.silhouette(ad, groupby=np.arange(39) % 2)
        big = _adata(n=300)
        with pytest.raises(ValueError, match='300 distinct labels .at most 256'):
            net.silhouette(big, groupby=np.arange(300))
        assert 'dca_silhouette' not in ad.obs.columns

        class TwoRanks:
            rank, world, dp = 0, 2, False
        comm, net.engine.comm = net.engine.comm, TwoRanks()
        with pytest.raises(ValueError, match='data-parallel'):
            net.silhouette(ad, groupby=np.arange(40) % 2)
        with pytest.raises(ValueError, match='data-parallel'):
            net.engine.latent_silhouette(np.arange(40) % 2, 2)
        net.engine.comm = comm
        flat = _fitted(ad, hidden=())
        with pytest.raises(ValueError, match='No such layer'):
            flat.silhouette(ad, groupby=np.arange(40) % 2)
        with pytest.raises(ValueError, match='No such layer'):
            flat.engine.latent_silhouette(np.arange(40) % 2, 2)


def test_engine_latent_silhouette_and_ops_without_silhouette():
    n, G = 50, 9
    X, Y, sf, p = make_problem(n, G, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    codes = (np.arange(n) % 3).astype(np.int32)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.latent_silhouette(codes, 3)
    eng = make_engine(SilhouetteRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    w = eng.w.clone()
    lat, r = eng.latent_silhouette(codes, 3, chunk=50)
    np.testing.assert_array_equal(lat.numpy(), eng.latent_knn(5, chunk=50)[0].numpy())      # one definition of the latent loop
    ref = silhouette_ref(lat.numpy(), codes, 3)
    assert set(r) == {'s', 'a', 'b', 'nearest', 'counts', 'cluster_mean', 'mean'}
    np.testing.assert_array_equal(r['s'].numpy(), ref['s'])
    np.testing.assert_array_equal(r['nearest'].numpy(), ref['nearest'])
    assert (eng.w == w).all()
    r2 = eng.latent_silhouette(torch.from_numpy(codes), 3, chunk=50)[1]        # a tensor of codes is taken as well
    np.testing.assert_array_equal(r2['s'].numpy(), ref['s'])
    with pytest.raises(ValueError, match='49 codes for 50 cells'):
        eng.latent_silhouette(codes[:49], 3)
    with pytest.raises(ValueError, match=r'2 \.\. 256'):
        eng.latent_silhouette(codes, 1)


# ---------------------------------------------------------------------------------------------------- command line
def _write_counts(tmp_path, n=64, g=18, seed=5):
    y = synth_counts(n, g, seed)
    genes = ['g%d' % i for i in range(g)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


BASE = ['--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8']


def test_cli_silhouette_kmeans_writes_two_more_files(tmp_path, monkeypatch, capsys):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].silhouette

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        seen['kw'], seen['u'] = kw, adata.uns['dca_silhouette']
        seen['s'], seen['near'] = np.asarray(adata.obs['dca_silhouette']), np.asarray(adata.obs['dca_silhouette_nearest'])
        seen['lab'] = np.asarray(adata.obs['dca_kmeans']).astype(str)
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'silhouette', spy)
    with override_ops(SilhouetteRefOps):
        main([f, out] + BASE + ['--kmeans', '3', '--silhouette', 'kmeans'])
    assert seen['kw'] == {'groupby': 'dca_kmeans'}
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'kmeans_centers.tsv', 'kmeans_labels.tsv', 'latent.tsv',
                                       'mean.tsv', 'model.pickle', 'silhouette.tsv', 'silhouette_clusters.tsv']
    tab = pd.read_csv(os.path.join(out, 'silhouette.tsv'), sep='\t', index_col=0, dtype={'label': str, 'nearest': str})
    assert list(tab.index) == cells and list(tab.columns) == ['label', 'silhouette', 'nearest']
    assert tab['label'].tolist() == seen['lab'].tolist() and tab['nearest'].tolist() == [str(v) for v in seen['near']]
    np.testing.assert_array_equal(tab['silhouette'].values, np.array([float('%.6f' % v) for v in seen['s']]))
    for line in open(os.path.join(out, 'silhouette.tsv')).read().splitlines()[1:]:
        assert len(line.split('\t')) == 4 and len(line.split('\t')[2].split('.')[1]) == 6, line
    cl = pd.read_csv(os.path.join(out, 'silhouette_clusters.tsv'), sep='\t', index_col=0)
    assert [str(v) for v in cl.index] == [str(v) for v in seen['u']['names']] and cl['cells'].tolist() == seen['u']['sizes'].tolist()
    np.testing.assert_array_equal(cl['silhouette'].values, np.array([float('%.6f' % v) for v in seen['u']['cluster_mean']]))
    assert 'dca: mean silhouette %.6f (64 cells in %d clusters)' % (seen['u']['mean'], len(seen['u']['names'])) in capsys.readouterr().out


def test_cli_silhouette_groups_leaves_unlisted_cells_empty(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.write(''.join('%s\t%s\n' % (c, 'AB'[i % 2]) for i, c in enumerate(cells[:60])))
    out = str(tmp_path / 'res')
    with override_ops(BothRefOps):
        main([f, out] + BASE + ['--groupstats', lab, '--silhouette', 'groups'])
    tab = pd.read_csv(os.path.join(out, 'silhouette.tsv'), sep='\t', index_col=0)
    assert list(tab.index) == cells and tab['label'][:60].tolist() == ['A', 'B'] * 30 and tab['nearest'][:60].tolist() == ['B', 'A'] * 30
    assert tab.iloc[60:].isna().all().all() and tab['silhouette'][:60].notna().all()
    cl = pd.read_csv(os.path.join(out, 'silhouette_clusters.tsv'), sep='\t', index_col=0)
    assert list(cl.index) == ['A', 'B'] and cl['cells'].tolist() == [30, 30]


def test_cli_silhouette_refusals_come_before_the_fit(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\n')
    one = str(tmp_path / 'one.tsv')
    with open(one, 'w') as fh:
        fh.write('c1\tA\nc2\tA\n')
    cases = [(['--silhouette', 'kmeans'], 'give --kmeans'), (['--silhouette', 'groups'], 'give --groupstats'),
             (['--silhouette', 'kmeans', '--groupstats', lab], 'give --kmeans'),
             (['--silhouette', 'groups', '--kmeans', '3'], 'give --groupstats'),
             (['--silhouette', 'kmeans', '--kmeans', '1'], '1 distinct label'),
             (['--silhouette', 'groups', '--groupstats', one], '1 distinct label'),
             (['--silhouette', 'groups', '--groupstats', lab, '-s', '8,200,8'], '1 .. 128 coordinates')]
    with override_ops(BothRefOps):
        for i, (flags, what) in enumerate(cases):
            out = str(tmp_path / ('res%d' % i))
            with pytest.raises(ValueError, match=what):
                main([f, out] + BASE + flags)
            assert not os.path.exists(os.path.join(out, 'mean.tsv')), flags
        with pytest.raises(SystemExit):
            main([f, str(tmp_path / 'resx')] + BASE + ['--silhouette', 'leiden'])
