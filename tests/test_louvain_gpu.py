"""K-LOUVAIN on the device (dcahip_graph_symmetrize / dcahip_louvain_begin / dcahip_louvain_sweep, HipOps.graph_symmetrize /
louvain_level, dca_amd.community, Autoencoder.louvain) against the integer reference of tests/_louvain_ref.py, by equality:
the symmetrised graph canonicalised, single sweeps of both directions from every kind of state, the discard rule, the
aggregation, the whole run (labels, level sizes, the integer Q; two runs; every check interval) and the model on dense and
counts-resident data.  No tolerance anywhere."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from _louvain_ref import (R, symmetrize_ref, canonical, sweep_ref, level_ref, relabel_ref, aggregate_ref, louvain_ref,
                          q_int_ref, degrees_ref, fixture, fixture_ref, cliques, wide_case, FIXTURES, RefLevel)

pytestmark = pytest.mark.gpu

EINVAL = -22
LOW = -(1 << 120)            # a best Q every sweep exceeds


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).cuda()


# ---------------------------------------------------------------------------------------------------- the graph
def _indices(n, k, seed):
    """Random neighbours with -1 padding, self entries, all-padding rows and forced mutual pairs."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, n, (n, k)).astype(np.int32)
    idx[rs.rand(n, k) < 0.2] = -1
    idx[rs.rand(n) < 0.1] = -1                                  # rows of degree 0 (unless somebody points at them)
    rows = rs.randint(0, n, max(1, n // 4))
    idx[rows, rs.randint(0, k, len(rows))] = rows               # self entries
    for a, b in rs.randint(0, n, (max(1, n // 4), 2)):          # mutual pairs
        idx[a, 0], idx[b, 0] = b, a
    return idx


def _check_symmetrize(ops, idx):
    rowptr, col, deg = ops.graph_symmetrize(_dev(idx))
    want = symmetrize_ref(idx)
    assert want[3] == 0
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and deg.dtype == torch.int32
    np.testing.assert_array_equal(rowptr.cpu().numpy(), want[0])
    np.testing.assert_array_equal(deg.cpu().numpy(), want[2])
    assert col.numel() == len(want[1])
    np.testing.assert_array_equal(canonical(rowptr.cpu().numpy(), col.cpu().numpy())[1], want[1])


@pytest.mark.parametrize('k', [1, 15, 64])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 1000])
def test_symmetrize_equals_the_reference(ops, n, k):
    _check_symmetrize(ops, _indices(n, k, 7 * n + k))


def test_symmetrize_hubs_empty_graph_and_more_than_one_scan_chunk(ops):
    idx = _indices(1000, 15, 1)
    idx[100:200, 3] = 5                                         # in-degree above 64
    _check_symmetrize(ops, idx)
    idx = _indices(1500, 4, 2)
    idx[200:1400, 1] = 7                                        # in-degree above 1 000
    assert symmetrize_ref(idx)[2][7] > 1000
    _check_symmetrize(ops, idx)
    _check_symmetrize(ops, np.full((70, 3), -1, np.int32))      # no edge at all
    _check_symmetrize(ops, _indices(4999, 3, 3))                # three scan chunks of 2 048 rows, the last one ragged
    rowptr, col, deg = ops.graph_symmetrize(torch.zeros(0, 4, dtype=torch.int32, device='cuda'))
    assert rowptr.tolist() == [0] and col.numel() == 0 and deg.numel() == 0


def test_symmetrize_out_of_range_entries_raise_and_limits_launch_nothing(ops):
    idx = _indices(300, 5, 4)
    idx[3, 2], idx[7, 0], idx[299, 4] = 300, -2, 1 << 30
    with pytest.raises(ValueError, match='3 neighbour indices lie outside 0 .. 299'):
        ops.graph_symmetrize(_dev(idx))
    with pytest.raises(ValueError, match='2m must stay below 2\\^31'):
        ops.graph_symmetrize_workspace_bytes(1 << 26, 16)
    with pytest.raises(ValueError, match='int32'):
        ops.graph_symmetrize(_dev(idx.astype(np.int64)))
    L = ops.L
    z = torch.zeros(64, dtype=torch.int64, device='cuda')
    p = z.data_ptr()
    assert L.dcahip_graph_symmetrize_workspace_bytes(-1, 3) == EINVAL and L.dcahip_graph_symmetrize_workspace_bytes(5, 0) == EINVAL
    for args in ((p, 2, 4, 3, p, p, 24, p, p, p), (p, 3, 4, 3, p, p, 23, p, p, p), (p, 3, 4, 0, p, p, 24, p, p, p),
                 (p, 3, -1, 3, p, p, 24, p, p, p), (None, 3, 4, 3, p, p, 24, p, p, p), (p, 16, 1 << 26, 16, p, p, 1 << 40, p, p, p)):
        assert L.dcahip_graph_symmetrize(*args, None) == EINVAL, args
    assert L.dcahip_louvain_sweep(4, 0, p, p, None, p, p, p, p, p, 10, 0, 0, 5, p, None) == EINVAL           # g = 0
    assert L.dcahip_louvain_sweep(4, 0, p, p, None, p, p, p, p, p, 1 << 31, 1024, 0, 5, p, None) == EINVAL   # 2m
    assert L.dcahip_louvain_sweep(4, 0, p, p, None, p, p, p, p, p, 10, 1024, 0, 0, p, None) == EINVAL        # max_sweeps
    assert L.dcahip_louvain_begin(4, 0, p, p, None, p, p, p, 10, 65537, p, None) == EINVAL
    torch.cuda.synchronize()
    assert int(z.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------- one sweep
def _graph_from_edges(n, edges):
    """CSR (rowptr, col, wt) of an undirected weighted graph from (a, b, w) triples; a == b is a self-loop, stored once."""
    rows = [[] for _ in range(n)]
    for a, b, w in edges:
        rows[a].append((b, w))
        if a != b:
            rows[b].append((a, w))
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    return rowptr, np.array([c for r in rows for c, _ in r], np.int64), np.array([w for r in rows for _, w in r], np.int64)


def _one_sweep(ops, rowptr, col, wt, labels, g, parity, twom=None, best_q=LOW):
    """Sweep `parity` on the device from `labels` against sweep_ref: the labels decided, the three sums, kept or not."""
    twom = int(len(col) if wt is None else np.asarray(wt).sum()) if twom is None else twom
    lev = ops.louvain_level(_dev(rowptr, np.int64), _dev(col, np.int32), None if wt is None else _dev(wt, np.int32), twom, g,
                            1000, labels=_dev(labels, np.int32), best_q=best_q)
    np.testing.assert_array_equal(lev.ki.cpu().numpy(), degrees_ref(rowptr, col, wt))
    lev.sweep(parity)
    st = lev.read(parity)
    new, moved, inside, tot2 = sweep_ref(rowptr, col, wt, labels, g, parity, twom)
    np.testing.assert_array_equal(lev.labels_new.cpu().numpy(), new)
    assert (st['moved'], st['inside'], st['tot2']) == (moved, inside, tot2)
    q = twom * R * inside - g * tot2
    assert st['kept'] == (moved > 0 and q > best_q) and st['sweeps'] == 1
    np.testing.assert_array_equal(lev.labels.cpu().numpy(), new if st['kept'] else labels)
    if st['kept']:
        assert st['q'] == q
        tot = np.zeros(len(labels), np.int64)
        np.add.at(tot, new, degrees_ref(rowptr, col, wt))
        np.testing.assert_array_equal(lev.tot.cpu().numpy(), tot)
    return st, new


@pytest.fixture(scope='module')
def graph1000():
    rowptr, col, deg, _ = symmetrize_ref(_indices(1000, 15, 11))
    return rowptr, col


@pytest.mark.parametrize('parity', [0, 1])
@pytest.mark.parametrize('start', ['singletons', 'random', 'few', 'converged'])
def test_one_sweep_equals_the_reference(ops, graph1000, start, parity):
    rowptr, col = graph1000
    if start == 'converged':                                    # a level that ended idle (the random graph's ends on a discard)
        rowptr, col = symmetrize_ref(fixture('blobs600')[0])[:2]
    n = len(rowptr) - 1
    rs = np.random.RandomState(5)
    for g in (1024, 300)[:1 if start == 'converged' else 2]:
        if start == 'converged':
            lev = RefLevel(rowptr, col, None, len(col), g, 1000)
            for s in range(1000):
                lev.sweep(s)
            assert lev.done == 2
            labels = lev._lab
        else:
            labels = {'singletons': np.arange(n), 'random': rs.randint(0, n, n), 'few': rs.randint(0, 20, n) * 37}[start]
        st, new = _one_sweep(ops, rowptr, col, None, labels, g, parity)
        if start in ('singletons', 'random'):
            assert st['moved'] > 0 and st['kept']
        if start == 'converged':
            assert st['moved'] == 0 and st['idle'] == 1 and not st['kept'] and st['done'] == 0


@pytest.mark.parametrize('parity', [0, 1])
def test_one_sweep_on_degrees_0_1_64_65_700_with_weights(ops, parity):
    """A star of 700 leaves (its row is read again past the 256 entries a wave keeps in registers, once per neighbouring
    community), vertices of degree 64 and 65 (one entry per lane, and one more), a leaf of degree 1, an isolated vertex,
    weights 1 .. 5 and self-loops."""
    rs = np.random.RandomState(9)
    n = 704
    edges = [(0, i, int(rs.randint(1, 6))) for i in range(1, 701)]
    edges += [(701, i, int(rs.randint(1, 6))) for i in range(1, 65)] + [(702, i, int(rs.randint(1, 6))) for i in range(100, 165)]
    edges += [(0, 0, 40), (701, 701, 7), (5, 5, 3)]
    rowptr, col, wt = _graph_from_edges(n, edges)
    deg = np.diff(rowptr)
    assert deg[0] == 701 and deg[701] == 65 and deg[702] == 65 and deg[700] == 1 and deg[703] == 0 and deg[200] == 1
    assert deg[1] == 2 and (deg == 64).sum() == 0
    rowptr2, col2, wt2 = _graph_from_edges(n, [e for e in edges if e[:2] != (701, 701)])      # degree 64 exactly
    assert np.diff(rowptr2)[701] == 64
    for labels in (np.arange(n), rs.randint(0, n, n), rs.randint(0, 5, n) + 300, np.full(n, 9)):
        _one_sweep(ops, rowptr, col, wt, labels, 1024, parity)
        _one_sweep(ops, rowptr2, col2, wt2, labels, 2048, parity)


@pytest.mark.parametrize('sign', [1, -1])
def test_scores_beyond_64_bits_on_a_coarse_graph(ops, sign):
    """Weights near 2^30 and self-loops: vertex 0's two scores are about 2^69 and differ by exactly 1."""
    rowptr, col, wt, labels, g, T = wide_case(sign)
    st, new = _one_sweep(ops, rowptr, col, wt, labels, g, 1, twom=T)
    assert new[0] == (2 if sign > 0 else 0)
    _one_sweep(ops, rowptr, col, wt, labels, g, 0, twom=T)
    _one_sweep(ops, rowptr, col, wt, np.arange(4), 65536, 1, twom=T)
    _one_sweep(ops, rowptr, col, wt, np.arange(4), 1, 0, twom=T)


@pytest.mark.parametrize('parity', [0, 1])
def test_exact_ties_go_to_the_lowest_id(ops, parity):
    idx = np.array([[1, 2], [0, 3], [0, 4], [1, -1], [2, -1]], dtype=np.int32)
    rowptr, col, _, _ = symmetrize_ref(idx)
    st, new = _one_sweep(ops, rowptr, col, None, np.arange(5), 1024, parity)
    assert new[0] == (1 if parity else 0)
    n = 130                                                     # a ring lattice: every vertex sees four equal candidates
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 2) % n], axis=1).astype(np.int32)
    rowptr, col, _, _ = symmetrize_ref(ring)
    st, new = _one_sweep(ops, rowptr, col, None, np.arange(n), 1024, parity)
    assert st['moved'] >= n - 4
    if parity == 0:
        assert (new[2:n - 2] == np.arange(n - 4)).all()         # the lowest of i-2, i-1 (the last two also see 0 and 1)


@pytest.mark.parametrize('seed,parity', [(7, 1), (11, 0)])
def test_a_sweep_that_lowers_q_is_discarded_and_ends_the_level(ops, seed, parity):
    idx = np.random.RandomState(seed).randint(0, 30, (30, 10)).astype(np.int32)
    rowptr, col, _, _ = symmetrize_ref(idx)
    lab = np.arange(30)
    q0 = q_int_ref(rowptr, col, None, lab, 1024)[0]
    new, moved, inside, tot2 = sweep_ref(rowptr, col, None, lab, 1024, parity)
    assert moved > 0 and len(col) * R * inside - 1024 * tot2 < q0               # the premise
    lev = ops.louvain_level(_dev(rowptr), _dev(col, np.int32), None, len(col), 1024, 1000)
    lev.sweep(parity)
    st = lev.read(parity)
    assert st['done'] == 1 and not st['kept'] and st['q'] == q0 and st['moved'] == moved and st['sweeps'] == 1
    np.testing.assert_array_equal(lev.labels.cpu().numpy(), lab)
    np.testing.assert_array_equal(lev.labels_new.cpu().numpy(), new)
    keep = (lev.labels_new.clone(), lev.tot.clone(), lev.tot_new.clone())
    for s in range(parity + 1, parity + 4):                     # past the end: exact no-ops
        lev.sweep(s)
    again = lev.read(parity + 3)
    assert (again['done'], again['sweeps'], again['q']) == (1, 1, q0)
    assert torch.equal(lev.labels_new, keep[0]) and torch.equal(lev.tot, keep[1]) and torch.equal(lev.tot_new, keep[2])
    np.testing.assert_array_equal(lev.labels.cpu().numpy(), lab)


def test_max_sweeps_ends_a_level(ops, graph1000):
    rowptr, col = graph1000
    want = level_ref(rowptr, col, None, len(col), 1024, 3)
    lev = ops.louvain_level(_dev(rowptr), _dev(col, np.int32), None, len(col), 1024, 3)
    for s in range(6):
        lev.sweep(s)
    st = lev.read(5)
    assert (st['done'], st['sweeps'], st['q']) == (3, 3, want[1])
    np.testing.assert_array_equal(lev.labels.cpu().numpy(), want[0])


# ---------------------------------------------------------------------------------------------------- aggregation
def test_aggregation_equals_the_reference(graph1000):
    from dca_amd import community
    rowptr, col = graph1000
    labels = level_ref(rowptr, col, None, len(col), 1024, 1000)[0]
    cu_ref, nc = relabel_ref(labels)
    cu, nc_dev = community.relabel(_dev(labels, np.int32))
    assert nc_dev == nc and cu.is_cuda
    np.testing.assert_array_equal(cu.cpu().numpy(), cu_ref)
    want = aggregate_ref(rowptr, col, None, cu_ref, nc)
    got = community.aggregate(_dev(rowptr), _dev(col, np.int32), None, cu, nc)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.cpu().numpy().astype(np.int64), b)
    labels2 = level_ref(*want, len(col), 1024, 1000)[0]         # a second level: weights and self-loops in
    cu2_ref, nc2 = relabel_ref(labels2)
    cu2, _ = community.relabel(_dev(labels2, np.int32))
    for a, b in zip(community.aggregate(*got, cu2, nc2), aggregate_ref(*want, cu2_ref, nc2)):
        np.testing.assert_array_equal(a.cpu().numpy().astype(np.int64), b)


# ---------------------------------------------------------------------------------------------------- the whole run
def _assert_run(res, det, ref):
    np.testing.assert_array_equal(res.labels.cpu().numpy() if isinstance(res.labels, torch.Tensor) else res.labels, ref['labels'])
    assert det['q_int'] == ref['q_int'] and det['twom'] == ref['twom']
    assert res.level_sizes == ref['level_sizes'] and res.n_sweeps == ref['n_sweeps'] and res.n_levels == len(ref['level_sizes'])
    np.testing.assert_array_equal(res.sizes.cpu().numpy() if isinstance(res.sizes, torch.Tensor) else res.sizes, ref['sizes'])
    assert res.modularity == ref['q_int'] / float(ref['twom'] ** 2 * R)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_the_whole_run_equals_the_reference(ops, name):
    from dca_amd import community
    idx, _ = fixture(name)
    ref = fixture_ref(name)
    res, det = community.louvain(idx, ops=ops, details=True)
    assert isinstance(res.labels, np.ndarray) and res.labels.dtype == np.int32
    _assert_run(res, det, ref)
    assert community.modularity(idx, res.labels, ops=ops) == res.modularity


def test_two_runs_every_check_interval_resolutions_and_device_input(ops):
    from dca_amd import community
    idx, _ = fixture('blobs600')
    ref = fixture_ref('blobs600')
    dev_idx = _dev(idx)
    first, det = community.louvain(dev_idx, ops=ops, details=True)
    assert isinstance(first.labels, torch.Tensor) and first.labels.is_cuda and first.labels.dtype == torch.int32
    assert first.sizes.is_cuda
    _assert_run(first, det, ref)
    for every in (None, 1, 5, 64):
        res, det = community.louvain(dev_idx, ops=ops, check_every=every, details=True)
        assert torch.equal(res.labels, first.labels) and det == dict(q_int=ref['q_int'], twom=ref['twom'], g=1024)
        assert res.n_sweeps == first.n_sweeps and res.level_sizes == first.level_sizes
    for resolution in (0.5, 2.0):
        res, det = community.louvain(idx, resolution=resolution, ops=ops, details=True)
        _assert_run(res, det, louvain_ref(idx, resolution))
    res, det = community.louvain(idx, max_levels=1, max_sweeps=4, ops=ops, details=True)
    _assert_run(res, det, louvain_ref(idx, max_levels=1, max_sweeps=4))
    ci, planted = cliques([5, 6, 7, 5, 9, 4])
    res, det = community.louvain(ci, ops=ops, details=True)
    _assert_run(res, det, louvain_ref(ci))
    assert len(set(zip(res.labels.tolist(), planted.tolist()))) == 6
    lone = community.louvain(np.full((5, 2), -1, np.int32), ops=ops)
    assert lone.labels.tolist() == [0, 1, 2, 3, 4] and lone.modularity == 0.0 and lone.n_levels == 0
    km = np.arange(600) % 7
    assert community.modularity(idx, km, ops=ops) == q_int_ref(*symmetrize_ref(idx)[:2], None, km, 1024)[0] / float(ref['twom'] ** 2 * R)


# ---------------------------------------------------------------------------------------------------- through the model
def test_autoencoder_louvain_dense_and_counts_resident_then_group_stats(ops, monkeypatch):
    import scipy.sparse as sp
    from dca_amd import io, community
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G, k = 300, 200, 10
    y = synth_counts(n, G, 4).astype(np.float32)

    def adata(form):
        monkeypatch.setenv('DCA_AMD_RESIDENT', form)
        ad = AnnData(sp.csr_matrix(y), obs=pd.DataFrame(index=['c%d' % i for i in range(n)]),
                     var=pd.DataFrame(index=['g%d' % i for i in range(G)]))
        ad = io.normalize(io.read_dataset(ad, copy=True))
        dd = getattr(ad, '_dca_device', None)
        assert dd is not None and (dd.csr is not None) == (form == 'counts')
        return ad
    np.random.seed(0)
    dense = adata('dense')
    net = AE_types['zinb-conddisp'](input_size=G, hidden_size=(64, 32, 64))
    net.build()
    train(dense, net, epochs=2, early_stop=0, reduce_lr=0, verbose=False)
    w = net.engine.w.clone()
    assert net.louvain(dense, n_neighbors=k) is None
    assert torch.equal(net.engine.w, w)
    net.group_stats(dense, 'dca_louvain')                       # follows with no glue
    counts = adata('counts')
    net.louvain(counts, n_neighbors=k)
    assert net.engine.csr is not None and int(net.engine.gather_status.item()) == 0
    nb = adata('dense')
    net.neighbors(nb, n_neighbors=k)
    for key in ('X_dca', 'dca_knn_indices', 'dca_knn_distances'):
        assert dense.obsm[key].tobytes() == nb.obsm[key].tobytes() == counts.obsm[key].tobytes()
    lab = np.asarray(dense.obs['dca_louvain']).astype(int)
    np.testing.assert_array_equal(lab, np.asarray(counts.obs['dca_louvain']).astype(int))
    res = community.louvain(nb.obsm['dca_knn_indices'], ops=ops)
    np.testing.assert_array_equal(lab, res.labels)
    ref = louvain_ref(nb.obsm['dca_knn_indices'])
    np.testing.assert_array_equal(lab, ref['labels'])
    u = dense.uns['dca_louvain']
    assert u['modularity'] == res.modularity == counts.uns['dca_louvain']['modularity']
    np.testing.assert_array_equal(u['sizes'], ref['sizes'])
    g = dense.uns['dca_groups']
    assert g['groupby'] == 'dca_louvain' and int(np.sum(g['counts'])) == n
