"""Louvain above the kernels -- dca_amd.community, Engine.latent_louvain, Autoencoder.louvain, `dca --louvain` -- on the CPU
oracle extended with graph_symmetrize / louvain_level (tests/_louvain_ref.LouvainRefOps), and the integer reference itself:
its modularity against networkx, planted partitions, the quality of its rule against networkx's Louvain, the 128-bit scores,
ties, both sweep directions, the level's state machine and the final numbering."""
import os
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from helpers import make_problem, make_engine
from _louvain_ref import (LouvainRefOps, R, symmetrize_ref, canonical, sweep_ref, level_ref, relabel_ref, aggregate_ref,
                          louvain_ref, modularity_ref, q_int_ref, degrees_ref, fixture, fixture_ref, cliques, wide_case,
                          RefLevel, FIXTURES)
from dca_amd import io, community
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 4, 8)


def _nx_graph(indices):
    nx = pytest.importorskip('networkx')
    return nx, nx.from_scipy_sparse_array(community.knn_adjacency(indices))


def _sets(labels):
    labels = np.asarray(labels)
    return [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_symmetrize_ref_and_knn_adjacency_agree():
    idx = np.array([[1, 2], [0, -1], [2, 0], [-1, -1]], dtype=np.int32)         # a mutual pair, a self entry, an empty row
    rowptr, col, deg, bad = symmetrize_ref(idx)
    assert bad == 0 and rowptr.tolist() == [0, 4, 6, 8, 8] and deg.tolist() == [4, 2, 2, 0]
    assert col.tolist() == [1, 1, 2, 2, 0, 0, 0, 0]
    W = community.knn_adjacency(idx)
    assert W.dtype.kind == 'i' and W.shape == (4, 4)
    np.testing.assert_array_equal(W.toarray(), [[0, 2, 2, 0], [2, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]])
    assert symmetrize_ref(np.array([[5, 1], [0, -2]], dtype=np.int32))[3] == 2
    with pytest.raises(ValueError, match='outside 0 .. 1'):
        community.knn_adjacency(np.array([[5, 1], [0, -1]]))


@pytest.mark.parametrize('resolution', [0.5, 1.0, 2.0])
def test_modularity_ref_equals_networkx(resolution):
    idx, which = fixture('blobs600')
    nx, G = _nx_graph(idx)
    for labels in (which, np.arange(600) % 7, fixture_ref('blobs600')['labels']):
        q, twom = modularity_ref(idx, labels, resolution)
        want = nx.community.modularity(G, _sets(labels), weight='weight', resolution=resolution)
        assert abs(q / (twom * twom * R) - want) <= 1e-12, (q / (twom * twom * R), want)


def test_planted_partitions_are_recovered_exactly():
    idx, planted = cliques([5, 6, 7, 5, 9, 4])
    r = louvain_ref(idx)
    assert len(set(zip(r['labels'].tolist(), planted.tolist()))) == 6 and len(r['sizes']) == 6
    assert r['sizes'].tolist() == [9, 7, 6, 5, 5, 4]
    idx, which = fixture('blobs600')
    r = fixture_ref('blobs600')
    assert len(r['sizes']) == 6 and len(set(zip(r['labels'].tolist(), which.tolist()))) == 6


def test_quality_against_networkx_louvain():
    """The reference's modularity is at least 0.95 x the lowest of networkx's Louvain over seeds 0 .. 4 on the three
    fixtures.  Measured ratios: blobs600 1.0000 (0.830011 / 0.830011), blobs3000 1.0000 (0.916398 / 0.916398), one3000
    0.9694 (0.479972 / 0.495125).  The 5 % is room for a structureless graph."""
    for name in FIXTURES:
        idx, _ = fixture(name)
        nx, G = _nx_graph(idx)
        r = fixture_ref(name)
        ours = r['q_int'] / (r['twom'] ** 2 * R)
        theirs = min(nx.community.modularity(G, nx.community.louvain_communities(G, weight='weight', seed=s), weight='weight')
                     for s in range(5))
        print('%s: %.6f / %.6f = %.4f' % (name, ours, theirs, ours / theirs))
        assert ours >= 0.95 * theirs, (name, ours, theirs)


def test_scores_beyond_64_bits_are_decided_exactly():
    """Vertex 0's two scores are about 2^69 and differ by exactly 1 (2^-69 of their size): +1 moves, -1 stays.  A double
    rounds both to the same number, and a 64-bit integer wraps."""
    for sign in (1, -1):
        rowptr, col, wt, labels, g, T = wide_case(sign)
        ki = degrees_ref(rowptr, col, wt)
        M = T * R
        stay = 1000 * M - g * int(ki[0]) * int(ki[1])
        move = 1001 * M - g * int(ki[0]) * int(ki[2])
        assert move - stay == sign and abs(stay) > 1 << 64 and Fraction(1, abs(stay)) < Fraction(1, 1 << 64)
        assert float(move) == float(stay)                                  # what a double sees
        new, moved, inside, tot2 = sweep_ref(rowptr, col, wt, labels, g, 1, T)
        assert new[0] == (2 if sign > 0 else 0), sign
        assert q_int_ref(rowptr, col, wt, new, g)[1:3] == (inside, tot2)


def test_ties_go_to_the_lowest_id_and_both_parities():
    # a path 1 - 0 - 2 - 3 .. with vertex 0's neighbours 1 and 2 of equal degree: equal scores
    idx = np.array([[1, 2], [0, 3], [0, 4], [1, -1], [2, -1]], dtype=np.int32)
    rowptr, col, deg, _ = symmetrize_ref(idx)
    lab = np.arange(5)
    odd, moved, _, _ = sweep_ref(rowptr, col, None, lab, 1024, 1)
    assert odd[0] == 1                                                     # 1 and 2 tie for vertex 0: the lower id
    assert (odd >= lab).all() and moved > 0                                # an odd sweep only moves up
    even, moved, _, _ = sweep_ref(rowptr, col, None, lab, 1024, 0)
    assert (even <= lab).all() and moved > 0 and even[0] == 0              # an even sweep only moves down
    assert even[3] == 1 and even[4] == 2


def test_level_state_machine():
    idx, _ = fixture('blobs600')
    rowptr, col, _, _ = symmetrize_ref(idx)
    labels, q, sweeps = level_ref(rowptr, col, None, len(col), 1024, 1000)
    assert q == q_int_ref(rowptr, col, None, labels, 1024)[0]
    lev = RefLevel(rowptr, col, None, len(col), 1024, 1000, labels=labels, best_q=q)
    lev.sweep(0)
    lev.sweep(1)
    st = lev.read(1)
    assert st['done'] in (1, 2) and st['q'] == q and (lev._lab == labels).all()        # a finished level stays
    capped = level_ref(rowptr, col, None, len(col), 1024, 3)
    assert capped[2] == 3 and capped[1] < q
    # the discard rule: from a state whose next sweep lowers Q the labels stay and the level ends with code 1
    lev = RefLevel(rowptr, col, None, len(col), 1024, 1000, labels=labels, best_q=(q + 1) << 20)
    lev._lab = np.arange(600)                                               # singletons move, but cannot reach that Q
    lev.sweep(0)
    assert lev.read(0)['done'] == 1 and not lev.read(0)['kept'] and lev.read(0)['moved'] > 0


def test_relabel_and_aggregate_equal_the_reference():
    idx, _ = fixture('blobs600')
    rowptr, col, _, _ = symmetrize_ref(idx)
    labels, _, _ = level_ref(rowptr, col, None, len(col), 1024, 1000)
    cu_ref, nc_ref = relabel_ref(labels)
    cu, nc = community.relabel(torch.from_numpy(labels.astype(np.int32)))
    assert nc == nc_ref and (cu.numpy() == cu_ref).all()
    assert [int(np.flatnonzero(cu_ref == c)[0]) for c in range(nc)] == sorted(int(np.flatnonzero(cu_ref == c)[0]) for c in range(nc))
    want = aggregate_ref(rowptr, col, None, cu_ref, nc)
    got = community.aggregate(torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int32)), None, cu, nc)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.numpy().astype(np.int64), b)
    assert int(want[2].sum()) == len(col)                                  # 2m is kept
    again = aggregate_ref(*want, np.arange(nc) // 2, (nc + 1) // 2)        # weights and self-loops through a second level
    got2 = community.aggregate(got[0], got[1], got[2], torch.arange(nc) // 2, (nc + 1) // 2)
    for a, b in zip(got2, again):
        np.testing.assert_array_equal(a.numpy().astype(np.int64), b)


# ---------------------------------------------------------------------------------------------------- the module on the oracle
def test_louvain_on_the_oracle_equals_the_reference_and_numbering():
    ops = LouvainRefOps()
    for name in ('blobs600', 'one3000'):
        idx, _ = fixture(name)
        ref = fixture_ref(name)
        res, det = community.louvain(idx, ops=ops, details=True)
        assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.int32 and res.sizes.dtype == np.int64
        np.testing.assert_array_equal(res.labels, ref['labels'])
        np.testing.assert_array_equal(res.sizes, ref['sizes'])
        assert det['q_int'] == ref['q_int'] and res.level_sizes == ref['level_sizes'] and res.n_sweeps == ref['n_sweeps']
        assert res.n_levels == len(ref['level_sizes']) and res.resolution == 1.0
        assert res.modularity == ref['q_int'] / float(ref['twom'] ** 2 * R)
        # the final numbering: by size descending, ties by the lowest member
        np.testing.assert_array_equal(np.bincount(res.labels), res.sizes)
        firsts = [int(np.flatnonzero(res.labels == c)[0]) for c in range(len(res.sizes))]
        keys = list(zip((-res.sizes).tolist(), firsts))
        assert keys == sorted(keys)
        assert community.modularity(idx, res.labels, ops=ops) == res.modularity
    every = community.louvain(idx, ops=ops, check_every=1)
    np.testing.assert_array_equal(every.labels, res.labels)
    t = community.louvain(torch.from_numpy(idx), ops=ops, on_device=True)
    assert isinstance(t.labels, torch.Tensor) and t.labels.dtype == torch.int32 and isinstance(t.sizes, torch.Tensor)
    fine = community.louvain(idx, resolution=2.0, ops=ops)
    assert len(fine.sizes) >= len(res.sizes) and fine.resolution == 2.0
    assert community.louvain(idx, resolution=1.0004, ops=ops).resolution == 1.0       # quantised to 1/1024
    # a graph without edges: every vertex alone, nothing launched past the symmetrisation
    lone = community.louvain(np.full((5, 2), -1, np.int32), ops=ops)
    assert lone.labels.tolist() == [0, 1, 2, 3, 4] and lone.modularity == 0.0 and lone.n_levels == 0 and lone.n_sweeps == []


def test_louvain_refusals():
    ops = LouvainRefOps()
    idx, _ = fixture('blobs600')
    with pytest.raises(ValueError, match='2m must stay below 2\\^31'):
        community.check_louvain_args(1 << 26, 16)
    with pytest.raises(ValueError, match='2\\^31 - 1 vertices'):
        community.check_louvain_args(1 << 31, 1)
    for res in (0.0, 64.1, -1):
        with pytest.raises(ValueError, match='resolution must lie in 1/1024 .. 64'):
            community.louvain(idx, resolution=res, ops=ops)
    with pytest.raises(ValueError, match='max_levels and max_sweeps'):
        community.louvain(idx, max_levels=0, ops=ops)
    with pytest.raises(ValueError, match='max_levels and max_sweeps'):
        community.louvain(idx, max_sweeps=0, ops=ops)
    with pytest.raises(ValueError, match=r'\[n, k\] array'):
        community.louvain(idx[0], ops=ops)
    with pytest.raises(ValueError, match='integers'):
        community.louvain(idx.astype(np.float32), ops=ops)
    bad = idx.copy()
    bad[3, 2] = 600
    bad[7, 0] = -2
    with pytest.raises(ValueError, match='2 neighbour indices lie outside 0 .. 599'):
        community.louvain(bad, ops=ops)
    with pytest.raises(ValueError, match='one per row'):
        community.modularity(idx, np.zeros(5, int), ops=ops)
    with pytest.raises(ValueError, match='below 2\\^31'):
        community.check_level_args(10, 5, 1 << 31, 1024, 10)


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


def test_autoencoder_louvain_keys_dtypes_values_and_what_follows():
    ad = _adata()
    n, k = ad.n_obs, 6
    with override_ops(LouvainRefOps):
        net = _fitted(ad)
        before = (ad.X.copy(), sorted(ad.obsm.keys()), sorted(ad.obs.columns), dict(ad.uns))
        res = net.louvain(ad, n_neighbors=k, copy=True)
        assert res is not ad and sorted(ad.obsm.keys()) == before[1] and sorted(ad.obs.columns) == before[2]
        assert dict(ad.uns) == before[3]
        assert net.louvain(ad, n_neighbors=k) is None                      # in place, like predict
        np.testing.assert_array_equal(ad.X, before[0])
        nb = ad.copy()
        net.neighbors(nb, n_neighbors=k)
        net.louvain(ad, n_neighbors=k, resolution=2.0, key_added='fine')
        net.group_stats(ad, 'dca_louvain')                                 # no glue between them
        net.silhouette(ad, 'dca_louvain')
    ref = louvain_ref(nb.obsm['dca_knn_indices'])
    for a in (res, ad):
        for key in ('X_dca', 'dca_knn_indices', 'dca_knn_distances'):
            np.testing.assert_array_equal(a.obsm[key], nb.obsm[key])
        assert a.uns['dca_neighbors'] == nb.uns['dca_neighbors']
        col = a.obs['dca_louvain']
        assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == [str(c) for c in range(len(ref['sizes']))]
        np.testing.assert_array_equal(np.asarray(col).astype(int), ref['labels'])
        u = a.uns['dca_louvain']
        assert set(u) == {'modularity', 'sizes', 'level_sizes', 'n_levels', 'n_sweeps', 'params'}
        assert u['sizes'].dtype == np.int64 and isinstance(u['modularity'], float) and isinstance(u['n_levels'], int)
        np.testing.assert_array_equal(u['sizes'], ref['sizes'])
        assert u['modularity'] == ref['q_int'] / float(ref['twom'] ** 2 * R)
        assert u['level_sizes'] == ref['level_sizes'] and u['n_sweeps'] == ref['n_sweeps']
        assert u['params'] == {'n_neighbors': k, 'resolution': 1.0, 'max_levels': 32, 'max_sweeps': 1000}
    assert ad.uns['fine']['params']['resolution'] == 2.0
    g = ad.uns['dca_groups']
    assert g['groupby'] == 'dca_louvain' and int(np.sum(g['counts'])) == n
    np.testing.assert_array_equal(np.asarray(g['counts']), ref['sizes'])
    assert ad.uns['dca_silhouette']['groupby'] == 'dca_louvain'


def test_autoencoder_louvain_refusals():
    ad = _adata(n=40)
    with override_ops(LouvainRefOps):
        net = _fitted(ad)
        with pytest.raises(ValueError, match='only 39 others'):
            net.louvain(ad, n_neighbors=40)
        with pytest.raises(ValueError, match='1 .. 64'):
            net.louvain(ad, n_neighbors=0)
        with pytest.raises(ValueError, match='resolution must lie'):
            net.louvain(ad, resolution=100)
        assert 'dca_louvain' not in ad.obs.columns and 'X_dca' not in ad.obsm

        class TwoRanks:
            rank, world, dp = 0, 2, False
        comm, net.engine.comm = net.engine.comm, TwoRanks()
        with pytest.raises(ValueError, match='data-parallel'):
            net.louvain(ad)
        with pytest.raises(ValueError, match='data-parallel'):
            net.engine.latent_louvain(5)
        net.engine.comm = comm
        flat = _fitted(ad, hidden=())
        with pytest.raises(ValueError, match='No such layer'):
            flat.louvain(ad)


def test_engine_latent_louvain_and_ops_without_it():
    n, G = 50, 9
    X, Y, sf, p = make_problem(n, G, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.latent_louvain(5)
    eng = make_engine(LouvainRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    w = eng.w.clone()
    lat, idx, d2, res = eng.latent_louvain(5, chunk=50)
    lat_knn, idx_knn, _ = eng.latent_knn(5, chunk=50)
    np.testing.assert_array_equal(lat.numpy(), lat_knn.numpy())
    np.testing.assert_array_equal(idx.numpy(), idx_knn.numpy())
    assert isinstance(res.labels, torch.Tensor) and res.labels.dtype == torch.int32
    np.testing.assert_array_equal(res.labels.numpy(), louvain_ref(idx.numpy())['labels'])
    assert (eng.w == w).all()


# ---------------------------------------------------------------------------------------------------- command line
def _write_counts(tmp_path, n=64, g=18, seed=5):
    y = synth_counts(n, g, seed)
    genes = ['g%d' % i for i in range(g)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


BASE = ['--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8']


def test_cli_louvain_files_stats_and_silhouette(tmp_path, monkeypatch, capsys):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].louvain

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        seen['kw'], seen['u'], seen['lab'] = kw, adata.uns['dca_louvain'], np.asarray(adata.obs['dca_louvain']).astype(str)
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'louvain', spy)
    with override_ops(LouvainRefOps):
        main([f, out] + BASE + ['--louvain', '--louvain-resolution', '0.5', '--neighbors', '7', '--louvainstats',
                                '--silhouette', 'louvain'])
    assert seen['kw'] == {'n_neighbors': 7, 'resolution': 0.5}
    lines = open(os.path.join(out, 'louvain_labels.tsv')).read().splitlines()
    assert [l.split('\t')[0] for l in lines] == cells and [l.split('\t')[1] for l in lines] == seen['lab'].tolist()
    assert all(len(l.split('\t')) == 2 for l in lines)                     # no header: the format --groupstats reads
    said = capsys.readouterr().out
    assert 'dca: louvain: %d clusters, modularity %.6f (7 neighbours, resolution 0.5' % (len(seen['u']['sizes']),
                                                                                         seen['u']['modularity']) in said
    sizes = pd.read_csv(os.path.join(out, 'group_sizes.tsv'), sep='\t', index_col=0)
    assert sizes['cells'].tolist() == [int(s) for s in seen['u']['sizes']]
    assert os.path.exists(os.path.join(out, 'silhouette.tsv')) and os.path.exists(os.path.join(out, 'knn_indices.tsv'))
    out2 = str(tmp_path / 'res2')
    with override_ops(LouvainRefOps):
        main([f, out2] + BASE + ['--groupstats', os.path.join(out, 'louvain_labels.tsv')])
    assert open(os.path.join(out2, 'group_sizes.tsv')).read() == open(os.path.join(out, 'group_sizes.tsv')).read()


def test_cli_louvain_alone_defaults_to_15_neighbours(tmp_path, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].louvain

    def spy(self, adata, **kw):
        seen['kw'] = kw
        return real(self, adata, **kw)
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'louvain', spy)
    with override_ops(LouvainRefOps):
        main([f, out] + BASE + ['--louvain'])
    assert seen['kw'] == {'n_neighbors': 15, 'resolution': 1.0}
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'latent.tsv', 'louvain_labels.tsv', 'mean.tsv',
                                       'model.pickle']


def test_cli_louvain_refusals_come_before_the_fit(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    lab = str(tmp_path / 'labels.tsv')
    with open(lab, 'w') as fh:
        fh.write('c1\tA\nc2\tB\n')
    cases = [(['--louvainstats'], 'give --louvain'), (['--louvain-resolution', '2'], 'give --louvain'),
             (['--silhouette', 'louvain'], 'give --louvain'), (['--louvain', '--louvain-resolution', '65'], '1/1024 .. 64'),
             (['--louvain', '--neighbors', '64'], 'only 63 others'),
             (['--louvain', '--louvainstats', '--groupstats', lab], 'give one of them'),
             (['--louvain', '--louvainstats', '--kmeans', '3', '--kmeansstats'], 'give one of them'),
             (['--louvain', '-s', '8,200,8'], '1 .. 128 coordinates')]
    with override_ops(LouvainRefOps):
        for i, (flags, what) in enumerate(cases):
            out = str(tmp_path / ('res%d' % i))
            with pytest.raises(ValueError, match=what):
                main([f, out] + BASE + flags)
            assert not os.path.exists(os.path.join(out, 'mean.tsv')), flags
        out = str(tmp_path / 'resn')
        with pytest.raises(ValueError, match='--type normal'):
            main([f, out, '--type', 'normal', '-e', '1', '-s', '8,2,8', '--louvain', '--louvainstats'])
        assert not os.path.exists(os.path.join(out, 'mean.tsv'))
