"""K-means above the kernels -- dca_amd.cluster, Engine.latent_kmeans, Autoencoder.cluster, `dca --kmeans` -- on the CPU oracle
extended with kmeans_seed / kmeans_step (tests/_kmeans_ref.KmeansRefOps), and the references themselves: the integer seeding's
properties, the whole loop against scikit-learn, and the margin condition of the GPU trajectory cases."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _knn_ref import clustered, d2_ref
from _kmeans_ref import (KmeansRefOps, seed_ref, step_ref, lloyd_ref, kmeans_ref, int_data, TRAJECTORY_CASES,
                         TRAJECTORY_GAP, SEED_TAG)
from _groups_ref import GroupRefOps
from dca_amd import io, cluster
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 4, 8)


class BothRefOps(KmeansRefOps, GroupRefOps):
    name = 'cpu-oracle-kmeans-groups'


# ---------------------------------------------------------------------------------------------------- the seeding reference
def test_seed_tag_is_the_kernels_and_apart_from_the_other_streams():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dca_amd', 'csrc', 'philox.hpp')).read()
    assert 'kPhiloxSeedTag = 0x%08Xu' % SEED_TAG in src
    assert SEED_TAG > 255 and SEED_TAG != 0x7468696E


def test_seed_ref_properties():
    X = clustered(400, 5, seed=2)
    a = seed_ref(X, 12, 7, 0)
    assert a == seed_ref(X, 12, 7, 0) and len(a) == 12 and all(0 <= r < 400 for r in a)
    assert a != seed_ref(X, 12, 8, 0) and a != seed_ref(X, 12, 7, 1) and a != seed_ref(X, 12, 7 + (1 << 32), 0)
    assert a[:5] == seed_ref(X, 5, 7, 0)                                   # round t does not depend on k
    Y = X.copy()
    Y[7] = Y[3] + 1.0                                                      # all points distinct: so are the rows drawn
    for seed in range(5):
        rows = seed_ref(Y, 40, seed, 0)
        assert len(set(rows)) == 40
    same = np.tile(X[:1], (50, 1))                                         # M = 0: uniform rows, no division by zero
    rows = seed_ref(same, 6, 3, 0)
    assert all(0 <= r < 50 for r in rows) and len(set(rows)) > 1
    two = np.concatenate([same[:25], same[:25] + 1.0])                     # after both values are drawn M = 0 again
    rows = seed_ref(two, 5, 1, 0)
    assert {r < 25 for r in rows[:2]} == {True, False}
    # a point is drawn in proportion to its squared distance: the far point of a tight cloud almost always comes second
    far = np.zeros((200, 2), np.float32)
    far[:, 0] = np.arange(200) * 1e-3
    far[123] = (100.0, 0.0)
    hits = sum(seed_ref(far, 2, s, 0)[1] == 123 or seed_ref(far, 2, s, 0)[0] == 123 for s in range(20))
    assert hits >= 19


def test_step_ref_ties_empty_clusters_and_reseeding():
    X = np.asarray([[0, 0], [2, 0], [2, 0], [10, 0]], np.float32)
    C = np.asarray([[1, 0], [1, 0], [50, 0]], np.float32)                  # 0 and 1 identical, 2 out of reach
    s = step_ref(X, C)
    assert s['labels'].tolist() == [0, 0, 0, 0] and s['counts'].tolist() == [4, 0, 0] and s['changed'] == 4
    assert s['reseeded'] == 1 and s['C_out'][1].tolist() == [10, 0] and s['C_out'][2].tolist() == [50, 0]
    assert s['C_out'][0].tolist() == [3.5, 0] and s['inertia'] == 1 + 1 + 1 + 81 and s['gap'] == 0.0
    s2 = step_ref(X, s['C_out'], s['labels'])
    assert s2['labels'].tolist() == [0, 0, 0, 1] and s2['changed'] == 1 and s2['reseeded'] == 1       # cluster 2 still empty
    assert s2['C_out'][2].tolist() == [0, 0]                               # the farthest point, the largest index among ties
    r = lloyd_ref(X, C)
    assert r['converged'] and r['reseeds'] == [1, 2] and sorted(r['counts'].tolist()) == [1, 1, 2]


def test_kmeans_ref_against_scikit_learn():
    sk = pytest.importorskip('sklearn.cluster')
    X = clustered(1500, 32)
    for k, seed in ((12, 0), (5, 1), (20, 2)):
        init = X[seed_ref(X, k, seed, 0)]
        ref = kmeans_ref(X, k, init=init)
        km = sk.KMeans(n_clusters=k, algorithm='lloyd', init=init.astype(np.float64), n_init=1, tol=0, max_iter=300).fit(
            X.astype(np.float64))
        ours = [frozenset(np.flatnonzero(ref['labels'] == c).tolist()) for c in range(k)]
        theirs = [frozenset(np.flatnonzero(km.labels_ == c).tolist()) for c in range(k)]
        assert set(ours) == set(theirs)                                    # the same partition
        assert abs(ref['inertia'] - km.inertia_) <= 1e-6 * km.inertia_
        assert (np.diff(ref['sizes']) <= 0).all() and ref['sizes'].sum() == 1500


@pytest.mark.parametrize('d,k,seed', TRAJECTORY_CASES)
def test_trajectory_cases_keep_their_margin(d, k, seed):
    """The condition under which tests/test_kmeans_gpu.py asks for the reference's labels, n_iter and sizes exactly: in the
    reference itself every point's second-nearest centre is at least 1e-3 (relative, squared distances) farther than its
    nearest, in every iteration, and the run takes more than one iteration."""
    X = clustered(1500, d)
    ref = lloyd_ref(X, X[seed_ref(X, k, seed, 0)])
    print('clustered(1500, %d) k=%d seed=%d: %d iterations, gap %.3g' % (d, k, seed, ref['n_iter'], ref['gap']))
    assert ref['converged'] and ref['n_iter'] > 1 and ref['gap'] >= TRAJECTORY_GAP


# ---------------------------------------------------------------------------------------------------- dca_amd.cluster
def test_cluster_kmeans_on_the_oracle_equals_the_reference_loop():
    X = clustered(300, 6, seed=4)
    ops = KmeansRefOps()
    res = cluster.kmeans(X, 7, n_init=4, seed=3, ops=ops)
    ref = kmeans_ref(X, 7, n_init=4, seed=3)
    assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.int32 and res.labels.shape == (300,)
    assert res.centers.dtype == np.float32 and res.centers.shape == (7, 6) and res.sizes.dtype == np.int64
    assert isinstance(res.inertia, float) and isinstance(res.n_iter, int) and res.converged is True
    np.testing.assert_array_equal(res.labels, ref['labels'])
    np.testing.assert_array_equal(res.centers, ref['centers'])
    np.testing.assert_array_equal(res.sizes, ref['sizes'])
    assert res.inertia == ref['inertia'] and res.n_iter == ref['n_iter']
    # numbered by size descending, ties by the number in the run; labels and centres permuted together
    assert (np.diff(res.sizes) <= 0).all() and (np.bincount(res.labels, minlength=7) == res.sizes).all()
    near = np.argmin(d2_ref(X, res.centers), axis=1)
    np.testing.assert_array_equal(near, res.labels)
    # the winner among the n_init runs: the lowest inertia, the first of equals
    singles = [lloyd_ref(X, X[seed_ref(X, 7, 3, j)])['inertia'] for j in range(4)]
    assert res.inertia == min(singles)
    one = cluster.kmeans(X, 7, n_init=1, seed=3, ops=ops)
    assert one.inertia == singles[0]
    # an explicit start: n_init is 1, whatever is asked for
    init = X[[5, 50, 100, 150, 200, 250, 299]]
    a = cluster.kmeans(X, 7, n_init=5, init=init, ops=ops)
    b = kmeans_ref(X, 7, init=init)
    np.testing.assert_array_equal(a.labels, b['labels'])
    # tensors in (with on_device), tensors out
    t = cluster.kmeans(torch.from_numpy(X), 7, n_init=1, seed=3, ops=ops, on_device=True)
    assert isinstance(t.labels, torch.Tensor) and t.labels.dtype == torch.int32 and t.sizes.dtype == torch.int64
    np.testing.assert_array_equal(t.labels.numpy(), one.labels)


def test_cluster_renumber():
    rank, order = cluster.renumber([3, 9, 3, 0, 9])
    assert order.tolist() == [1, 4, 0, 2, 3] and rank.tolist() == [2, 0, 3, 4, 1]


def test_cluster_kmeans_does_not_depend_on_the_check_interval_and_stops_at_max_iter(monkeypatch):
    X = clustered(300, 3, seed=4)
    ops = KmeansRefOps()
    full = cluster.kmeans(X, 9, n_init=1, seed=1, ops=ops)
    assert full.converged and full.n_iter > 2                           # so that max_iter = 2 below cuts the run
    monkeypatch.setattr(cluster, 'CHECK_EVERY', 1)
    each = cluster.kmeans(X, 9, n_init=1, seed=1, ops=ops)
    for a, b in zip(full, each):
        np.testing.assert_array_equal(a, b)
    cut = cluster.kmeans(X, 9, n_init=1, seed=1, max_iter=2, ops=ops)
    ref = kmeans_ref(X, 9, n_init=1, seed=1, max_iter=2)
    assert not cut.converged and cut.n_iter == 2 and cut.inertia == ref['inertia']
    np.testing.assert_array_equal(cut.labels, ref['labels'])
    np.testing.assert_array_equal(np.argmin(d2_ref(X, cut.centers), axis=1), cut.labels)    # the labels of the centres returned


def test_cluster_kmeans_refusals():
    X = clustered(40, 3)
    ops = KmeansRefOps()
    for k, what in ((0, '1 .. 256'), (257, '1 .. 256'), (41, '41 clusters of 40 points')):
        with pytest.raises(ValueError, match=what):
            cluster.kmeans(X, k, ops=ops)
    with pytest.raises(ValueError, match='1 .. 128 coordinates'):
        cluster.kmeans(np.zeros((300, 129), np.float32), 3, ops=ops)
    with pytest.raises(ValueError, match='2-d array'):
        cluster.kmeans(X[:, 0], 3, ops=ops)
    with pytest.raises(ValueError, match='init must be'):
        cluster.kmeans(X, 3, init=X[:4], ops=ops)
    with pytest.raises(ValueError, match='n_init and max_iter'):
        cluster.kmeans(X, 3, n_init=0, ops=ops)
    with pytest.raises(ValueError, match='seed'):
        cluster.kmeans(X, 3, seed=-1, ops=ops)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match='1 coordinates are not finite'):
        cluster.kmeans(bad, 3, ops=ops)
    with pytest.raises(ValueError, match='not finite'):
        cluster.kmeans(bad, 3, init=X[:3], ops=ops)
    assert cluster.kmeans(X, 40, n_init=1, ops=ops).sizes.sum() == 40      # k = n is allowed


def test_kmeans_predict_is_the_nearest_centre():
    X = clustered(120, 5, seed=1)
    ops = KmeansRefOps()
    res = cluster.kmeans(X, 6, n_init=2, ops=ops)
    new = clustered(30, 5, seed=1) + np.float32(0.01)
    labels, dist = cluster.kmeans_predict(new, res.centers, ops=ops)
    D = d2_ref(new, res.centers)
    assert labels.dtype == np.int32 and dist.dtype == np.float32 and labels.shape == dist.shape == (30,)
    np.testing.assert_array_equal(labels, np.argmin(D, axis=1))
    np.testing.assert_array_equal(dist, np.sqrt(D.min(axis=1).astype(np.float32)))
    own, _ = cluster.kmeans_predict(X, res.centers, ops=ops)
    np.testing.assert_array_equal(own, res.labels)


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


def test_autoencoder_cluster_keys_dtypes_values_and_group_stats():
    ad = _adata()
    n, k = ad.n_obs, 5
    with override_ops(BothRefOps):
        net = _fitted(ad)
        before = (ad.X.copy(), sorted(ad.obsm.keys()), sorted(ad.obs.columns), dict(ad.uns))
        res = net.cluster(ad, k, n_init=3, seed=4, copy=True)
        assert res is not ad and sorted(ad.obsm.keys()) == before[1] and sorted(ad.obs.columns) == before[2]
        assert dict(ad.uns) == before[3]
        assert net.cluster(ad, k, n_init=3, seed=4) is None                # in place, like predict
        np.testing.assert_array_equal(ad.X, before[0])
        lat = ad.copy()
        net.predict(lat, mode='latent')
        net.cluster(ad, 3, n_init=1, max_iter=50, key_added='coarse')
        net.group_stats(ad, 'dca_kmeans')                                  # no glue between the two
    ref = kmeans_ref(lat.obsm['X_dca'], k, n_init=3, seed=4)
    for a in (res, ad):
        np.testing.assert_array_equal(a.obsm['X_dca'], lat.obsm['X_dca'])
        col = a.obs['dca_kmeans']
        assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == ['0', '1', '2', '3', '4']
        np.testing.assert_array_equal(np.asarray(col).astype(int), ref['labels'])
        u = a.uns['dca_kmeans']
        assert set(u) == {'centers', 'inertia', 'n_iter', 'converged', 'sizes', 'params'}
        assert u['centers'].dtype == np.float32 and u['centers'].shape == (k, HS[1]) and u['sizes'].dtype == np.int64
        assert isinstance(u['inertia'], float) and isinstance(u['n_iter'], int) and isinstance(u['converged'], bool)
        assert u['params'] == {'n_clusters': k, 'n_init': 3, 'max_iter': 300, 'seed': 4}
        np.testing.assert_array_equal(u['centers'], ref['centers'])
        np.testing.assert_array_equal(u['sizes'], ref['sizes'])
        assert u['inertia'] == ref['inertia'] and u['n_iter'] == ref['n_iter']
    assert ad.uns['coarse']['params'] == {'n_clusters': 3, 'n_init': 1, 'max_iter': 50, 'seed': 0}
    assert list(ad.obs['coarse'].cat.categories) == ['0', '1', '2']
    g = ad.uns['dca_groups']
    assert g['groupby'] == 'dca_kmeans' and int(np.sum(g['counts'])) == n
    assert [str(x) for x in g['names']] == [str(c) for c in range(k) if ref['sizes'][c] > 0]
    np.testing.assert_array_equal(np.asarray(g['counts']), ref['sizes'][ref['sizes'] > 0])


def test_autoencoder_cluster_refusals():
    ad = _adata(n=40)
    with override_ops(KmeansRefOps):
        net = _fitted(ad)
        with pytest.raises(ValueError, match='41 clusters of 40 cells'):
            net.cluster(ad, 41)
        for k in (0, 257):
            with pytest.raises(ValueError, match='1 .. 256'):
                net.cluster(ad, k)
        assert 'dca_kmeans' not in ad.obs.columns

        class TwoRanks:
            rank, world, dp = 0, 2, False
        comm, net.engine.comm = net.engine.comm, TwoRanks()
        with pytest.raises(ValueError, match='data-parallel'):
            net.cluster(ad, 3)
        with pytest.raises(ValueError, match='data-parallel'):
            net.engine.latent_kmeans(3)
        net.engine.comm = comm
        flat = _fitted(ad, hidden=())
        with pytest.raises(ValueError, match='No such layer'):
            flat.cluster(ad, 3)
        with pytest.raises(ValueError, match='No such layer'):
            flat.engine.latent_kmeans(3)


def test_engine_latent_kmeans_chunks_and_ops_without_kmeans():
    n, G = 50, 9
    X, Y, sf, p = make_problem(n, G, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.latent_kmeans(3)
    eng = make_engine(KmeansRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    w = eng.w.clone()
    lat, res = eng.latent_kmeans(4, n_init=2, seed=1, chunk=50)
    lat_knn = eng.latent_knn(5, chunk=50)[0]
    np.testing.assert_array_equal(lat.numpy(), lat_knn.numpy())            # one definition of the latent loop
    lat7, _ = eng.latent_kmeans(4, n_init=2, seed=1, chunk=7)              # ragged chunks: the same rows
    np.testing.assert_allclose(lat7.numpy(), lat.numpy(), rtol=1e-6, atol=1e-7)
    ref = kmeans_ref(lat.numpy(), 4, n_init=2, seed=1)
    assert isinstance(res.labels, torch.Tensor) and res.labels.dtype == torch.int32
    np.testing.assert_array_equal(res.labels.numpy(), ref['labels'])
    np.testing.assert_array_equal(res.centers.numpy(), ref['centers'])
    assert (eng.w == w).all()
    with pytest.raises(ValueError, match='51 clusters of 50 cells'):
        eng.latent_kmeans(51)


# ---------------------------------------------------------------------------------------------------- command line
def _write_counts(tmp_path, n=64, g=18, seed=5):
    y = synth_counts(n, g, seed)
    genes = ['g%d' % i for i in range(g)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


BASE = ['--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8']


def test_cli_kmeans_files_and_kmeansstats(tmp_path, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].cluster

    def spy(self, adata, n_clusters, **kw):
        r = real(self, adata, n_clusters, **kw)
        seen['kw'], seen['u'], seen['lab'] = kw, adata.uns['dca_kmeans'], np.asarray(adata.obs['dca_kmeans']).astype(str)
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'cluster', spy)
    with override_ops(BothRefOps):
        main([f, out] + BASE + ['--kmeans', '3', '--kmeans-seed', '5', '--kmeansstats'])
    assert seen['kw'] == {'seed': 5}
    lines = open(os.path.join(out, 'kmeans_labels.tsv')).read().splitlines()
    assert [l.split('\t')[0] for l in lines] == cells and [l.split('\t')[1] for l in lines] == seen['lab'].tolist()
    assert all(len(l.split('\t')) == 2 for l in lines)                     # no header: the format --groupstats reads
    cen = pd.read_csv(os.path.join(out, 'kmeans_centers.tsv'), sep='\t', index_col=0)
    assert cen.shape == (3, 2) and list(cen.index) == [0, 1, 2]
    np.testing.assert_array_equal(cen.values, np.array([[float('%.6f' % v) for v in row] for row in seen['u']['centers']]))
    for line in open(os.path.join(out, 'kmeans_centers.tsv')).read().splitlines()[1:]:
        assert all(len(v.split('.')[1]) == 6 for v in line.split('\t')[1:]), line
    sizes = pd.read_csv(os.path.join(out, 'group_sizes.tsv'), sep='\t', index_col=0)
    live = [c for c in range(3) if seen['u']['sizes'][c] > 0]
    assert [int(g) for g in sizes.index] == live and sizes['cells'].tolist() == [int(seen['u']['sizes'][c]) for c in live]
    scores = pd.read_csv(os.path.join(out, 'group_scores.tsv'), sep='\t', index_col=0)
    assert list(scores.index) == genes and scores.shape == (18, len(live))
    # the labels file read back through --groupstats describes the same groups
    out2 = str(tmp_path / 'res2')
    with override_ops(BothRefOps):
        main([f, out2] + BASE + ['--groupstats', os.path.join(out, 'kmeans_labels.tsv')])
    assert open(os.path.join(out2, 'group_sizes.tsv')).read() == open(os.path.join(out, 'group_sizes.tsv')).read()
    assert open(os.path.join(out2, 'group_scores.tsv')).read() == open(os.path.join(out, 'group_scores.tsv')).read()


def test_cli_kmeans_alone_writes_two_more_files(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    with override_ops(KmeansRefOps):
        main([f, out] + BASE + ['--kmeans', '4'])
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'kmeans_centers.tsv', 'kmeans_labels.tsv', 'latent.tsv',
                                       'mean.tsv', 'model.pickle']


def test_cli_kmeans_refusals_come_before_the_fit(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\n')
    cases = [(['--kmeansstats'], 'give --kmeans'), (['--kmeans', '0'], '1 .. 256'), (['--kmeans', '257'], '1 .. 256'),
             (['--kmeans', '65'], '65 clusters of 64 cells'), (['--kmeans', '3', '--kmeans-seed', '-1'], '--kmeans-seed'),
             (['--kmeans', '3', '--kmeansstats', '--groupstats', lab], 'give one of them'),
             (['--kmeans', '3', '-s', '8,200,8'], '1 .. 128 coordinates')]
    with override_ops(BothRefOps):
        for i, (flags, what) in enumerate(cases):
            out = str(tmp_path / ('res%d' % i))
            with pytest.raises(ValueError, match=what):
                main([f, out] + BASE + flags)
            assert not os.path.exists(os.path.join(out, 'mean.tsv')), flags
        out = str(tmp_path / 'resn')
        with pytest.raises(ValueError, match='--type normal'):
            main([f, out, '--type', 'normal', '-e', '1', '-s', '8,2,8', '--kmeans', '3', '--kmeansstats'])
        assert not os.path.exists(os.path.join(out, 'mean.tsv'))
