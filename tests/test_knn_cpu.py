"""The neighbour search above the kernel -- Autoencoder.neighbors, Engine.latent_knn, dca_amd.neighbors, `dca --neighbors` --
on the CPU oracle extended with knn (tests/_knn_ref.KnnRefOps), and the reference and the float criterion themselves."""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import synth_counts
from helpers import make_problem, make_engine
from _knn_ref import KnnRefOps, knn_ref, assert_knn_close, clustered, direct_fp32, gram_fp32, knn_from_matrix, float_tol
from dca_amd import io, neighbors
from dca_amd._anndata import AnnData
from dca_amd.__main__ import main
from dca_amd.network import override_ops, AE_types
from dca_amd.train import train
from oracle.cpu_ops import CpuRefOps

HS = (8, 3, 8)


def test_reference_agrees_with_sklearn_brute_force():
    from sklearn.neighbors import NearestNeighbors
    rs = np.random.RandomState(0)
    X = rs.normal(size=(300, 7))
    Q = rs.normal(size=(41, 7))
    idx, d2 = knn_ref(Q, X, 9)
    dist, ind = NearestNeighbors(n_neighbors=9, algorithm='brute').fit(X).kneighbors(Q)
    np.testing.assert_array_equal(idx, ind)                   # random doubles: no ties
    np.testing.assert_allclose(np.sqrt(d2), dist, rtol=1e-12, atol=1e-12)
    # a self-search leaves the row out by index: sklearn's columns 1 .. k of k + 1 neighbours
    idx, d2 = knn_ref(X, X, 5, self_offset=0)
    dist, ind = NearestNeighbors(n_neighbors=6, algorithm='brute').fit(X).kneighbors(X)
    np.testing.assert_array_equal(ind[:, 0], np.arange(300))
    np.testing.assert_array_equal(idx, ind[:, 1:])
    np.testing.assert_allclose(np.sqrt(d2), dist[:, 1:], rtol=1e-12, atol=1e-12)


def test_reference_order_padding_and_self_exclusion():
    X = np.array([[0.], [1.], [1.], [3.], [0.]])
    idx, d2 = knn_ref(X, X, 6, self_offset=0)
    # row 0: its copy (row 4) at 0, then the tie of rows 1 and 2 by index, then row 3; two slots of padding
    assert idx[0].tolist() == [4, 1, 2, 3, -1, -1] and d2[0, :4].tolist() == [0., 1., 1., 9.] and np.isinf(d2[0, 4:]).all()
    assert idx[1].tolist() == [2, 0, 4, 3, -1, -1]
    idx, d2 = knn_ref(X[1:3], X, 2, self_offset=1)            # queries 0, 1 are rows 1, 2
    assert idx.tolist() == [[2, 0], [1, 0]]
    idx, d2 = knn_ref(X[1:3], X, 2, self_offset=-1)
    assert idx.tolist() == [[1, 2], [1, 2]] and (d2 == 0).all()


@pytest.mark.parametrize('d', [3, 32, 128])
def test_float_criterion_passes_the_direct_form_and_fails_the_gram_form(d):
    """The criterion discriminates: on clusters far from the origin the direct form in sequential fp32 meets it, the
    |a|^2 + |b|^2 - 2 a.b form in fp32 does not."""
    X = clustered(1500, d)
    k = 15
    full = knn_ref(X, X, k, self_offset=0, return_full=True)           # the fp64 reference, once for both forms
    idx, d2 = knn_from_matrix(direct_fp32(X, X), k, self_offset=0)
    worst = assert_knn_close(idx, d2, X, X, k, self_offset=0, what='direct fp32 d=%d' % d, ref=full)
    assert worst <= float_tol(d) / 2
    G = gram_fp32(X, X)
    ref = full[2]
    off = ~np.eye(len(X), dtype=bool) & (ref > 0)
    print('gram form d=%d: worst relative error %.3g, %d negative' % (d, float((np.abs(G - ref)[off] / ref[off]).max()),
                                                                      int((G < 0).sum())))
    idx, d2 = knn_from_matrix(G, k, self_offset=0)
    with pytest.raises(AssertionError):
        assert_knn_close(idx, d2, X, X, k, self_offset=0, what='gram fp32 d=%d' % d, ref=full)


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


def test_autoencoder_neighbors_keys_dtypes_values_and_copy():
    ad = _adata()
    n, k = ad.n_obs, 7
    with override_ops(KnnRefOps):
        net = _fitted(ad)
        before = (ad.X.copy(), sorted(ad.obsm.keys()), dict(ad.uns))
        res = net.neighbors(ad, n_neighbors=k, copy=True)
        assert res is not ad and sorted(ad.obsm.keys()) == before[1] and dict(ad.uns) == before[2]
        np.testing.assert_array_equal(ad.X, before[0])
        assert net.neighbors(ad, n_neighbors=k) is None            # in place, like predict
        np.testing.assert_array_equal(ad.X, before[0])
        lat = ad.copy()
        net.predict(lat, mode='latent')
    for a in (res, ad):
        assert a.obsm['X_dca'].dtype == np.float32 and a.obsm['X_dca'].shape == (n, HS[1])
        assert a.obsm['dca_knn_indices'].dtype == np.int32 and a.obsm['dca_knn_indices'].shape == (n, k)
        assert a.obsm['dca_knn_distances'].dtype == np.float32 and a.obsm['dca_knn_distances'].shape == (n, k)
        assert a.uns['dca_neighbors'] == {'n_neighbors': k, 'metric': 'euclidean', 'include_self': False}
        np.testing.assert_array_equal(a.obsm['X_dca'], lat.obsm['X_dca'])
    np.testing.assert_array_equal(res.obsm['dca_knn_indices'], ad.obsm['dca_knn_indices'])
    idx, d2 = knn_ref(ad.obsm['X_dca'], ad.obsm['X_dca'], k, self_offset=0)
    np.testing.assert_array_equal(ad.obsm['dca_knn_indices'], idx)
    np.testing.assert_array_equal(ad.obsm['dca_knn_distances'], np.sqrt(d2.astype(np.float32)))
    assert (ad.obsm['dca_knn_indices'] != np.arange(n)[:, None]).all()


def test_autoencoder_neighbors_refusals():
    ad = _adata(n=40)
    with override_ops(KnnRefOps):
        net = _fitted(ad)
        with pytest.raises(ValueError, match='n_neighbors = 40'):
            net.neighbors(ad, n_neighbors=40)                      # 39 other cells
        net.neighbors(ad, n_neighbors=39)
        assert (np.sort(ad.obsm['dca_knn_indices'], axis=1) ==
                np.array([np.delete(np.arange(40), i) for i in range(40)])).all()
        with pytest.raises(ValueError, match='1 .. 64'):
            net.neighbors(ad, n_neighbors=0)
        big = _adata(n=70)
        with pytest.raises(ValueError, match='1 .. 64'):
            net.neighbors(big, n_neighbors=65)

        class TwoRanks:
            rank, world, dp = 0, 2, False
        comm, net.engine.comm = net.engine.comm, TwoRanks()
        with pytest.raises(ValueError, match='data-parallel'):
            net.neighbors(ad, n_neighbors=5)
        with pytest.raises(ValueError, match='data-parallel'):
            net.engine.latent_knn(5)
        net.engine.comm = comm
        flat = _fitted(ad, hidden=())
        with pytest.raises(ValueError, match='No such layer'):
            flat.neighbors(ad, n_neighbors=5)
        with pytest.raises(ValueError, match='No such layer'):
            flat.engine.latent_knn(5)


def test_engine_latent_knn_chunks_and_ops_without_knn():
    n, G = 50, 9
    X, Y, sf, p = make_problem(n, G, HS, 'zinb-conddisp', seed=6)
    eng = make_engine(CpuRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    with pytest.raises(NotImplementedError, match=CpuRefOps.name):
        eng.latent_knn(5)
    eng = make_engine(KnnRefOps(), 'zinb-conddisp', G, HS, True, 0.05, p, X, Y, sf)
    w = eng.w.clone()
    lat, idx, d2 = eng.latent_knn(5, chunk=50)
    lat7, idx7, d27 = eng.latent_knn(5, chunk=7)               # ragged chunks: the same rows
    assert lat.shape == (n, HS[1]) and idx.shape == d2.shape == (n, 5)
    np.testing.assert_allclose(lat7.numpy(), lat.numpy(), rtol=1e-6, atol=1e-7)
    ridx, rd2 = knn_ref(lat.numpy(), lat.numpy(), 5, self_offset=0)
    np.testing.assert_array_equal(idx.numpy(), ridx)
    np.testing.assert_array_equal(d2.numpy(), rd2.astype(np.float32))
    assert (eng.w == w).all()
    with pytest.raises(ValueError, match='neighbours of 50 cells'):
        eng.latent_knn(50)


def test_module_knn_and_graph_round_trip():
    rs = np.random.RandomState(2)
    X = rs.normal(size=(30, 4))                               # float64 host input: taken as float32
    ops = KnnRefOps()
    idx, dist = neighbors.knn(X, 5, ops=ops)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == dist.shape == (30, 5)
    ridx, rd2 = knn_ref(X.astype(np.float32), X.astype(np.float32), 5, self_offset=0)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(dist, np.sqrt(rd2.astype(np.float32)))
    Q = rs.normal(size=(6, 4))
    qidx, qdist = neighbors.knn(X, 3, queries=Q, ops=ops)     # queries: nothing left out
    ridx, _ = knn_ref(Q.astype(np.float32), X.astype(np.float32), 3)
    np.testing.assert_array_equal(qidx, ridx)
    sidx, sdist = neighbors.knn(X, 1, queries=X, ops=ops)
    assert (sidx[:, 0] == np.arange(30)).all() and (sdist == 0).all()
    with pytest.raises(ValueError, match='1 .. 64'):
        neighbors.knn(X, 65, ops=ops)
    with pytest.raises(ValueError, match='1 .. 128'):
        neighbors.knn(np.zeros((4, 129)), 2, ops=ops)
    with pytest.raises(ValueError, match='not finite'):
        neighbors.knn(np.array([[0., 1.], [np.nan, 0.], [1., 1.]]), 1, ops=ops)

    g = neighbors.knn_graph(idx, dist)
    assert g.shape == (30, 30) and g.nnz == 150 and g.dtype == np.float32
    for i in range(30):
        row = g.indices[g.indptr[i]:g.indptr[i + 1]]
        assert row.tolist() == idx[i].tolist()                  # the neighbours in the order given
        np.testing.assert_array_equal(g.data[g.indptr[i]:g.indptr[i + 1]], dist[i])
    # short rows: the -1 / inf padding is dropped
    pidx, pdist = neighbors.knn(X[:4], 5, ops=ops)
    assert (pidx[:, 3:] == -1).all() and np.isinf(pdist[:, 3:]).all()
    g = neighbors.knn_graph(pidx, pdist)
    assert g.shape == (4, 4) and g.nnz == 12 and np.isfinite(g.data).all()
    assert (np.diff(g.indptr) == 3).all()
    g = neighbors.knn_graph(qidx, qdist, n_cols=30)
    assert g.shape == (6, 30) and g.nnz == 18
    with pytest.raises(ValueError, match='outside'):
        neighbors.knn_graph(qidx, qdist)                        # 6 columns cannot hold the atlas' indices
    with pytest.raises(ValueError, match='one shape'):
        neighbors.knn_graph(idx, dist[:, :3])


def _write_counts(tmp_path, n=64, G=18, seed=5):
    y = synth_counts(n, G, seed)
    genes = ['g%d' % i for i in range(G)]
    cells = ['c%d' % i for i in range(n)]
    f = str(tmp_path / 'counts.tsv')
    pd.DataFrame(y.T.astype(int), index=genes, columns=cells).to_csv(f, sep='\t')
    return f, genes, cells


def test_cli_neighbors_files(tmp_path, monkeypatch):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    seen = {}
    real = AE_types['zinb-conddisp'].neighbors

    def spy(self, adata, **kw):
        r = real(self, adata, **kw)
        seen['idx'], seen['dist'] = adata.obsm['dca_knn_indices'].copy(), adata.obsm['dca_knn_distances'].copy()
        return r
    monkeypatch.setattr(AE_types['zinb-conddisp'], 'neighbors', spy)
    with override_ops(KnnRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--neighbors', '5', '--testsplit'])
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'knn_distances.tsv', 'knn_indices.tsv', 'latent.tsv',
                                       'mean.tsv', 'model.pickle']
    idx = pd.read_csv(os.path.join(out, 'knn_indices.tsv'), sep='\t', index_col=0)
    dist = pd.read_csv(os.path.join(out, 'knn_distances.tsv'), sep='\t', index_col=0)
    assert list(idx.index) == list(dist.index) == cells
    assert idx.shape == dist.shape == (len(cells), 5)
    assert idx.values.dtype.kind == 'i' and idx.values.min() >= 0 and idx.values.max() < len(cells)
    np.testing.assert_array_equal(idx.values, seen['idx'])
    np.testing.assert_array_equal(dist.values, np.array([['%.6f' % v for v in r] for r in seen['dist']], dtype=np.float64))
    for line in open(os.path.join(out, 'knn_distances.tsv')).read().splitlines()[1:]:
        assert all(len(v.split('.')[1]) == 6 for v in line.split('\t')[1:]), line
    assert (idx.values != np.arange(len(cells))[:, None]).all()  # train and test cells alike, nobody its own neighbour


def test_cli_without_neighbors_writes_todays_files(tmp_path):
    f, genes, cells = _write_counts(tmp_path)
    out = str(tmp_path / 'res')
    with override_ops(KnnRefOps):
        main([f, out, '--type', 'zinb-conddisp', '-e', '2', '-s', '8,2,8', '--testsplit'])
    assert sorted(os.listdir(out)) == ['dispersion.tsv', 'dropout.tsv', 'latent.tsv', 'mean.tsv', 'model.pickle']


def test_new_entry_points_are_declared_and_bound():
    import ctypes as c
    from dca_amd import hip, build
    vp = c.c_void_p
    assert hip._SIGNATURES['dcahip_knn_splits'] == (c.c_int, [c.c_int] * 4)
    assert hip._SIGNATURES['dcahip_knn_workspace_bytes'] == (c.c_long, [c.c_int] * 5)
    assert hip._SIGNATURES['dcahip_knn'] == (c.c_int, [vp, c.c_long, c.c_int, vp, c.c_long, c.c_int, c.c_int, c.c_int,
                                                       c.c_long, c.c_int, vp, vp, c.c_long, vp, vp, vp])
    assert 'dcahip_knn.hip' in build.SOURCES


def _size_functions():
    import ctypes as c
    from dca_amd import build
    L = c.CDLL(build.build_hip(verbose=False))
    L.dcahip_knn_splits.restype, L.dcahip_knn_splits.argtypes = c.c_int, [c.c_int] * 4
    L.dcahip_knn_workspace_bytes.restype, L.dcahip_knn_workspace_bytes.argtypes = c.c_long, [c.c_int] * 5
    return L


def test_split_choice_and_workspace_are_pure_functions_of_the_shape():
    """Host side of K-NEIGHBOURS (no launch): the split count fills about 1 536 workgroups when the query blocks (256 queries;
    128 from k = 33 up) are few and keeps at least 1 024 candidates per split, at most 64; the workspace holds one sorted
    list per (split, query) and, when d is not an unroll width, the zero-padded candidates."""
    L = _size_functions()
    r16 = lambda x: (x + 15) // 16 * 16

    def want_splits(nq, n, k):
        threads = 128 if k > 32 else 256
        qb = (nq + threads - 1) // threads
        return max(1, min((1536 + qb - 1) // qb, n // 1024, 64))
    shapes = [(68579, 68579, 32, 15), (1000000, 1000000, 32, 15), (100, 1500000, 32, 15), (1031, 1031, 32, 15),
              (5000, 5000, 10, 64), (1, 1, 1, 1), (300, 100000, 128, 33), (2000, 40000, 50, 32)]
    for nq, n, d, k in shapes:
        s = L.dcahip_knn_splits(nq, n, d, k)
        assert s == want_splits(nq, n, k) == L.dcahip_knn_splits(nq, n, d, k), (nq, n, d, k, s)
        dp = next(w for w in (8, 16, 32, 64, 128) if w >= d)
        for splits in (0, 1, 7, 64):
            S = splits or s
            want = r16(S * nq * k * 8) + (r16(n * dp * 4) if dp != d else 0)
            assert L.dcahip_knn_workspace_bytes(nq, n, d, k, splits) == want, (nq, n, d, k, splits)
    assert L.dcahip_knn_splits(68579, 68579, 32, 15) == 6 and L.dcahip_knn_splits(1000000, 1000000, 32, 15) == 1
    EINVAL = -22
    for bad in ((10, 10, 32, 0), (10, 10, 32, 65), (10, 10, 0, 5), (10, 10, 129, 5), (-1, 10, 32, 5), (10, -1, 32, 5)):
        assert L.dcahip_knn_splits(*bad) == EINVAL and L.dcahip_knn_workspace_bytes(*bad, 0) == EINVAL, bad
    assert L.dcahip_knn_workspace_bytes(10, 10, 32, 5, 65) == EINVAL and L.dcahip_knn_workspace_bytes(10, 10, 32, 5, -1) == EINVAL


def test_scan_kernels_stay_inside_their_budget():
    """One lane holds a query's coordinates in registers and its list in LDS: no scratch at any width, at most 64 KiB of
    LDS per workgroup, and the distance loop of the d = 32 form on packed fp32 instructions (16 fused multiply-adds per
    candidate)."""
    import re
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(root, 'dca_amd', 'csrc', 'dcahip_knn.hip')
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'k.s')
        out = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.join(root, 'include'),
                              '--cuda-device-only', '-S', src, '-o', asm, '-Rpass-analysis=kernel-resource-usage'],
                             capture_output=True, text=True, check=True).stderr
        text = open(asm).read()
    names = re.findall(r'Function Name: (\S+)', out)
    scratch = [int(x) for x in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', out)]
    lds = [int(x) for x in re.findall(r'LDS Size \[bytes/block\]: (\d+)', out)]
    assert len(names) == len(scratch) == len(lds)
    seen = 0
    for nme, s, l in zip(names, scratch, lds):
        if 'knn_' in nme:
            assert s == 0 and l <= 65536, (nme, s, l)
            seen += 'knn_scan_kernel' in nme
    assert seen == 15                                           # d padded to 8 / 16 / 32 / 64 / 128 x k to 16 / 32 / 64
    m = re.search(r'^(_Z\w*knn_scan_kernelILi32ELi16E\w*):', text, re.M)
    body = text[m.end():text.index('s_endpgm', m.end())]
    assert body.count('v_pk_fma_f32') >= 16, body.count('v_pk_fma_f32')
