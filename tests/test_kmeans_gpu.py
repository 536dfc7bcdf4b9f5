"""K-MEANS on the MI355X: dcahip_kmeans_step and dcahip_kmeans_seed through HipOps against the host references
(tests/_kmeans_ref.py) -- bit for bit on integer coordinates, where every fp32 operation is exact and integer-valued doubles
sum exactly in any order; to the float criterion of the neighbour search on clusters far from the origin --, their
determinism and the no-op after convergence, whole trajectories where the reference's own decisions have a margin, empty
clusters, the refusals, and Autoencoder.cluster on dense and counts-resident data.

Bars on float data, tol = _knn_ref.float_tol(d) = 2 (d + 3) 2^-24 (twice the first-order bound of the fp32 direct form):
every point's centre is within (1 + tol) of its nearest in the reference's distances, every d2 within tol relative, the
inertia within n tol relative, a centre within 1 ulp of float32(double mean), the sums within (n - 1) 2^-53 sum|x| (a
double accumulation of n terms in any order)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from _knn_ref import float_tol, d2_ref
from _kmeans_ref import (seed_ref, step_ref, lloyd_ref, kmeans_ref, int_data, clustered, TRAJECTORY_CASES)

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A device array of `count` elements inside a larger one filled with a canary."""
    PAD = 16

    def __init__(self, count, dtype, canary):
        self.count, self.canary = count, canary
        self.buf = torch.full((count + 2 * self.PAD,), canary, dtype=dtype, device='cuda')
        self.ptr = self.buf.data_ptr() + self.PAD * self.buf.element_size()

    def get(self):
        return self.buf[self.PAD:self.PAD + self.count].cpu().numpy()

    def put(self, a):
        self.buf[self.PAD:self.PAD + self.count] = _dev(a).reshape(-1)

    def untouched(self):
        b = self.buf.cpu().numpy()
        return (b[:self.PAD] == self.canary).all() and (b[self.PAD + self.count:] == self.canary).all()


def _raw_step(ops, X, C, prev, it=1, state0=0, pads=(3, 2, 5, 1)):
    """dcahip_kmeans_step through the C entry with non-trivial leading dimensions and canaries around every output."""
    from dca_amd import hip
    n, d = X.shape
    k = C.shape[0]
    ldx, ldc, ldco, lds = (d + p for p in pads)
    Xp = torch.full((n, ldx), 99.0, device='cuda'); Xp[:, :d] = _dev(X)
    Cp = torch.full((k, ldc), -77.0, device='cuda'); Cp[:, :d] = _dev(C)
    out = dict(C_out=Guarded(k * ldco, torch.float32, -5.0), labels=Guarded(n, torch.int32, -9),
               d2=Guarded(n, torch.float32, -3.0), counts=Guarded(k, torch.int32, -11),
               sums=Guarded(k * lds, torch.float64, -13.0), inertia=Guarded(1, torch.float64, -15.0),
               changed=Guarded(1, torch.int32, -17), reseeded=Guarded(1, torch.int32, -19),
               state=Guarded(1, torch.int32, -21), status=Guarded(1, torch.int32, -23))
    out['labels'].put(np.asarray(prev, np.int32))
    out['state'].put(np.asarray([state0], np.int32))
    out['status'].put(np.zeros(1, np.int32))
    nbytes = ops.kmeans_workspace_bytes(n, d, k)
    ws = Guarded(nbytes, torch.uint8, 0xA5)
    o = out
    rc = ops.L.dcahip_kmeans_step(Xp.data_ptr(), ldx, n, d, k, Cp.data_ptr(), ldc, o['C_out'].ptr, ldco, o['labels'].ptr,
                                  o['d2'].ptr, o['counts'].ptr, o['sums'].ptr, lds, o['inertia'].ptr, o['changed'].ptr,
                                  o['reseeded'].ptr, o['state'].ptr, it, ws.ptr, o['status'].ptr, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for name, g in list(out.items()) + [('ws', ws)]:
        assert g.untouched(), name
    assert (Xp[:, d:] == 99.0).all() and (Cp[:, d:] == -77.0).all()
    res = {name: g.get() for name, g in out.items()}
    res['C_pad'] = res['C_out'].reshape(k, ldco)[:, d:]
    res['C_out'] = res['C_out'].reshape(k, ldco)[:, :d]
    res['sums_pad'] = res['sums'].reshape(k, lds)[:, d:]
    res['sums'] = res['sums'].reshape(k, lds)[:, :d]
    return res


# ---------------------------------------------------------------------------------------------------- one step, exact
# (n, d, k): every n of {1, 2, 63, 64, 65, 255, 256, 257, 1031} (around a wave and the 256-point tile; five tiles), every d of
# {1, 2, 3, 31, 32, 33, 128} (around the pad widths), every k of {1, 2, 15, 16, 17, 64, 255, 256}; k * pad(d) <= 5120 keeps
# the sums in LDS (with 32 .. 1 accumulator copies), above they go through the workspace: (1031, 32, 256), (1031, 128, 256),
# (257, 128, 255), (256, 33, 255), (255, 128, 64); k > n in (1, 1, 2), (2, 3, 17), (63, 2, 64); more than one staged chunk of
# centres from k * pad(d) > 4096
STEP = [(1, 1, 1), (1, 1, 2), (2, 2, 2), (2, 3, 17), (63, 2, 64), (64, 31, 16), (65, 32, 17), (255, 128, 64), (256, 33, 255),
        (257, 128, 255), (257, 3, 15), (1031, 1, 256), (1031, 32, 16), (1031, 32, 256), (1031, 128, 256), (1031, 31, 1)]


@pytest.mark.parametrize('n,d,k', STEP)
def test_one_step_on_integer_coordinates_equals_the_reference_bit_for_bit(ops, n, d, k):
    X, C = int_data(n, d, k)
    prev = np.random.RandomState(n + d + k).randint(-1, k, n).astype(np.int32)
    ref = step_ref(X, C, prev)
    got = _raw_step(ops, X, C, prev, it=4)
    np.testing.assert_array_equal(got['labels'], ref['labels'])
    np.testing.assert_array_equal(got['d2'].view(np.uint32), ref['d2'].astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(got['counts'], ref['counts'])
    np.testing.assert_array_equal(got['sums'], ref['sums'])
    assert got['inertia'][0] == ref['inertia'] and got['changed'][0] == ref['changed']
    assert got['reseeded'][0] == ref['reseeded'] and got['status'][0] == 0
    np.testing.assert_array_equal(got['C_out'].view(np.uint32), ref['C_out'].view(np.uint32))
    assert (got['C_pad'] == -5.0).all() and (got['sums_pad'] == -13.0).all()
    assert got['state'][0] == (4 if ref['changed'] == 0 and not ref['reseeded'] else 0)
    # the labels and distances of the neighbour search, bit for bit
    idx, kd2 = ops.knn(_dev(X), _dev(C), 1)
    np.testing.assert_array_equal(idx.cpu().numpy()[:, 0], got['labels'])
    np.testing.assert_array_equal(kd2.cpu().numpy()[:, 0].view(np.uint32), got['d2'].view(np.uint32))


def test_the_state_word_keeps_the_first_converged_iteration(ops):
    X, C = int_data(257, 3, 1)                                # one cluster: nothing is empty, nothing re-seeded
    prev = np.zeros(257, np.int32)
    assert _raw_step(ops, X, C, prev, it=7, state0=0)['state'][0] == 7
    assert _raw_step(ops, X, C, prev, it=7, state0=3)['state'][0] == 3            # already set: left alone
    prev[100] = -1
    assert _raw_step(ops, X, C, prev, it=7, state0=0)['state'][0] == 0            # a label changed


# ---------------------------------------------------------------------------------------------------- seeding, exact
SEED = [(1, 1, 1), (2, 2, 2), (63, 3, 17), (64, 31, 2), (65, 32, 17), (255, 33, 256), (256, 128, 17), (257, 1, 256),
        (1031, 32, 17), (1031, 128, 2), (1031, 3, 256), (2, 2, 17)]


@pytest.mark.parametrize('n,d,k', SEED)
def test_seeding_on_integer_coordinates_equals_the_integer_reference(ops, n, d, k):
    X, _ = int_data(n, d, 1, seed=1)
    Xp = torch.full((n, d + 3), 50.0, device='cuda')
    Xp[:, :d] = _dev(X)
    for seed, init in ((0, 0), (0, 3), ((1 << 40) + 12345, 0), ((1 << 63) + 5, 7)):
        rows, C = ops.kmeans_seed(Xp[:, :d], k, seed, init)
        want = seed_ref(X, k, seed, init)
        np.testing.assert_array_equal(rows.cpu().numpy(), np.asarray(want, np.int32))
        np.testing.assert_array_equal(C.cpu().numpy(), X[want])


def test_seeding_identical_points_draws_uniform_rows(ops):
    X = np.tile(np.asarray([[1.0, -2.0, 3.0]], np.float32), (65, 1))
    rows, C = ops.kmeans_seed(_dev(X), 5, 11, 2)
    want = seed_ref(X, 5, 11, 2)
    np.testing.assert_array_equal(rows.cpu().numpy(), np.asarray(want, np.int32))
    assert len(set(want)) > 1 and (C.cpu().numpy() == X[:5]).all()


# ---------------------------------------------------------------------------------------------------- determinism
def _buffers(n, d, k):
    f = dict(device='cuda')
    return dict(labels=torch.full((n,), -1, dtype=torch.int32, **f), d2=torch.empty(n, dtype=torch.float32, **f),
                counts=torch.zeros(k, dtype=torch.int32, **f), sums=torch.zeros(k, d, dtype=torch.float64, **f),
                inertia=torch.zeros(1, dtype=torch.float64, **f), info=torch.zeros(3, dtype=torch.int32, **f),
                status=torch.zeros(1, dtype=torch.int32, **f))


def _step(ops, Xt, C_in, C_out, b, it, ws):
    ops.kmeans_step(Xt, C_in, C_out, b['labels'], b['d2'], b['counts'], b['sums'], b['inertia'], b['info'], it, ws, b['status'])


def _snapshot(b, C):
    torch.cuda.synchronize()
    return {name: t.cpu().numpy().copy() for name, t in list(b.items()) + [('C', C)]}


def _same_bits(a, b):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


@pytest.mark.parametrize('n,d,k', [(1031, 32, 16), (1031, 32, 256), (700, 5, 40)])
def test_two_calls_give_the_same_bits_and_converged_steps_are_no_ops(ops, n, d, k):
    X = clustered(n, d, seed=3)
    Xt = _dev(X)
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device='cuda')
    C0 = ops.kmeans_seed(Xt, k, 5, 0, ws=ws)[1]
    snaps = []
    for _ in range(2):
        b, C = _buffers(n, d, k), C0.clone()
        _step(ops, Xt, C, C, b, 1, ws)
        _step(ops, Xt, C, C, b, 2, ws)
        snaps.append(_snapshot(b, C))
    _same_bits(*snaps)
    it = 2
    while int(b['info'][2].item()) == 0 and it < 300:
        it += 1
        _step(ops, Xt, C, C, b, it, ws)
    assert int(b['info'][2].item()) == it
    at = _snapshot(b, C)
    for extra in range(3):
        _step(ops, Xt, C, C, b, it + 1 + extra, ws)
    _same_bits(at, _snapshot(b, C))


@pytest.mark.parametrize('d,k,max_iter', [(3, 12, 300), (32, 40, 300), (3, 12, 3)])
def test_the_result_does_not_depend_on_how_often_the_state_is_read(ops, d, k, max_iter):
    from dca_amd import cluster
    X = clustered(1500, d, seed=1)
    Xt = _dev(X)
    ws = torch.empty(max(ops.kmeans_workspace_bytes(1500, d, k), 16), dtype=torch.uint8, device='cuda')
    C0 = ops.kmeans_seed(Xt, k, 1, 0, ws=ws)[1]
    runs = [cluster.lloyd(ops, Xt, C0.clone(), max_iter, ws, check_every=e) for e in (1, 8, 5)]
    for r in runs[1:]:
        assert r[2:5] == runs[0][2:5]                         # inertia, n_iter, converged
        for a, b in zip((r[0], r[1], r[5]), (runs[0][0], runs[0][1], runs[0][5])):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert runs[0][4] == (max_iter == 300) and (max_iter == 300 or runs[0][3] == 3)


# ---------------------------------------------------------------------------------------------------- float data
@pytest.mark.parametrize('d,k', [(3, 5), (32, 12), (128, 40)])
def test_float_data_every_point_at_the_returned_state(ops, d, k):
    from dca_amd import cluster
    n = 1500
    X = clustered(n, d)
    Xt = _dev(X)
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device='cuda')
    C = ops.kmeans_seed(Xt, k, 0, 0, ws=ws)[1]
    labels, C, inertia, n_iter, conv, counts = cluster.lloyd(ops, Xt, C, 300, ws)
    assert conv and n_iter >= 2
    b = _buffers(n, d, k)
    b['labels'].copy_(labels)
    _step(ops, Xt, C, C.clone(), b, n_iter + 1, ws)            # the no-op after convergence: d2 and sums of that state
    s = _snapshot(b, C)
    assert s['info'][0] == 0 and s['info'][1] == 0
    np.testing.assert_array_equal(s['labels'], labels.cpu().numpy())
    tol = float_tol(d)
    D = d2_ref(X, s['C'])
    own = D[np.arange(n), s['labels']]
    assert (own <= D.min(axis=1) * (1 + tol)).all()
    err = np.abs(s['d2'].astype(np.float64) - own)
    print('worst relative error of d2 %.2e (tol %.2e)' % (float((err / np.maximum(own, 1e-300)).max()), tol))
    assert (err <= tol * own).all()
    assert abs(s['inertia'][0] - own.sum()) <= n * tol * own.sum() and s['inertia'][0] == inertia
    X64 = X.astype(np.float64)
    np.testing.assert_array_equal(s['counts'], np.bincount(s['labels'], minlength=k))
    for c in range(k):
        members = X64[s['labels'] == c]
        if len(members):
            mean = (members.sum(axis=0) / len(members)).astype(np.float32)
            assert (np.abs(s['C'][c] - mean) <= np.spacing(np.abs(mean))).all(), c
        else:
            assert (s['sums'][c] == 0).all()
    total = np.abs(X64).sum(axis=0)
    fp64 = np.zeros((k, d))
    np.add.at(fp64, s['labels'], X64)
    assert (np.abs(s['sums'] - fp64) <= (n - 1) * 2.0 ** -53 * total).all()


# ---------------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize('d,k,seed', TRAJECTORY_CASES)
def test_trajectories_with_a_margin_equal_the_reference(ops, d, k, seed):
    """The cases whose every decision has a relative margin >= 1e-3 in the reference itself (asserted in
    tests/test_kmeans_cpu.py): more than 200 float_tol(3), far above a 1-ulp centre difference at coordinates of about 50.
    The start is the reference's k-means++ draw (on float data the device's own draw sees fp32 distances)."""
    from dca_amd import cluster
    X = clustered(1500, d)
    init = X[seed_ref(X, k, seed, 0)]
    ref = kmeans_ref(X, k, init=init)
    got = cluster.kmeans(X, k, init=init, ops=ops)
    assert got.n_iter == ref['n_iter'] and got.converged and ref['converged']
    np.testing.assert_array_equal(got.labels, ref['labels'])
    np.testing.assert_array_equal(got.sizes, ref['sizes'])
    assert got.labels.dtype == np.int32 and got.centers.dtype == np.float32 and got.sizes.dtype == np.int64
    assert abs(got.inertia - ref['inertia']) <= 1500 * float_tol(d) * ref['inertia']


# ---------------------------------------------------------------------------------------------------- empty clusters
def _sites():
    rs = np.random.RandomState(4)
    pts = set()
    while len(pts) < 10:
        pts.add(tuple(2 * rs.randint(-2, 3, 4)))
    P = np.asarray(sorted(pts), np.float32)
    return np.repeat(P, 3, axis=0), P


def test_empty_clusters_are_reseeded_one_per_iteration(ops):
    X, P = _sites()
    n, d, k = X.shape[0], 4, 12
    C0 = np.full((k, d), 40.0, np.float32)                     # clusters 10, 11: out of reach
    C0[:8] = P[:8] + np.asarray([0.5, 0, 0, 0], np.float32)
    C0[8], C0[9] = C0[0], C0[1]                                # the duplicated pairs (0, 8) and (1, 9)
    ref = lloyd_ref(X, C0)
    assert ref['converged'] and len(ref['reseeds']) >= 2 and ref['reseeds'] == list(range(1, len(ref['reseeds']) + 1))
    Xt = _dev(X)
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device='cuda')
    b, C = _buffers(n, d, k), _dev(C0)
    Cr, prev = C0, None
    for it in range(1, ref['n_iter'] + 1):
        s = step_ref(X, Cr, prev)
        _step(ops, Xt, C, C, b, it, ws)
        g = _snapshot(b, C)
        np.testing.assert_array_equal(g['labels'], s['labels'])
        np.testing.assert_array_equal(g['counts'], s['counts'])
        np.testing.assert_array_equal(g['sums'], s['sums'])
        assert g['info'][0] == s['changed'] and g['info'][1] == s['reseeded']
        np.testing.assert_array_equal(g['C'].view(np.uint32), s['C_out'].view(np.uint32))
        if it == 1:
            assert s['counts'][8] == 0 and s['counts'][9] == 0 and s['reseeded'] == 1      # the higher of a pair is empty
            far = int(np.flatnonzero(s['d2'] == s['d2'].max()).max())
            np.testing.assert_array_equal(g['C'][8], X[far])                               # the lowest empty cluster
            np.testing.assert_array_equal(g['C'][9], C0[9])
        assert g['info'][2] == (it if it == ref['n_iter'] else 0)                          # a re-seeding is not convergence
        Cr, prev = s['C_out'], s['labels']
    np.testing.assert_array_equal(g['labels'], ref['labels'])
    np.testing.assert_array_equal(g['C'].view(np.uint32), ref['centers'].view(np.uint32))


def test_identical_points_converge_without_reseeding(ops):
    from dca_amd import cluster
    X = np.tile(np.asarray([[3.0, 1.0]], np.float32), (200, 1))
    res = cluster.kmeans(X, 3, n_init=2, seed=9, ops=ops)
    assert res.converged and res.n_iter == 2 and res.sizes.tolist() == [200, 0, 0] and res.inertia == 0.0
    assert (res.labels == 0).all() and (res.centers == X[:3]).all()


# ---------------------------------------------------------------------------------------------------- refusals
def test_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    n, d, k = 50, 8, 5
    X = _dev(np.random.RandomState(0).normal(size=(n, d)).astype(np.float32))
    C = X[:k].clone()
    out = dict(C_out=torch.full((k, d), -5.0, device='cuda'), labels=torch.full((n,), -9, dtype=torch.int32, device='cuda'),
               d2=torch.full((n,), -3.0, device='cuda'), counts=torch.full((k,), -11, dtype=torch.int32, device='cuda'),
               sums=torch.full((k, d), -13.0, dtype=torch.float64, device='cuda'),
               inertia=torch.full((1,), -15.0, dtype=torch.float64, device='cuda'),
               info=torch.full((3,), -17, dtype=torch.int32, device='cuda'), rows=torch.full((256,), -19, dtype=torch.int32, device='cuda'),
               Cs=torch.full((256, d), -21.0, device='cuda'))
    keep = {name: t.clone() for name, t in out.items()}
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    st = torch.zeros(1, dtype=torch.int32, device='cuda')
    L = ops.L

    def step(n=n, d=d, k=k, ldx=d, ldc=d, ldco=d, lds=d, it=1, **null):
        p = lambda name, t: None if name in null else t.data_ptr()
        i = out['info'].data_ptr()
        return L.dcahip_kmeans_step(p('X', X), ldx, n, d, k, p('C', C), ldc, p('C_out', out['C_out']), ldco,
                                    p('labels', out['labels']), p('d2', out['d2']), p('counts', out['counts']),
                                    p('sums', out['sums']), lds, p('inertia', out['inertia']),
                                    None if 'changed' in null else i, None if 'reseeded' in null else i + 4,
                                    None if 'state' in null else i + 8, it, p('ws', ws), p('status', st), hip.stream())

    def seed(n=n, d=d, k=k, ldx=d, ldc=d, init=0, **null):
        p = lambda name, t: None if name in null else t.data_ptr()
        return L.dcahip_kmeans_seed(p('X', X), ldx, n, d, k, 1, init, p('rows', out['rows']), p('Cs', out['Cs']), ldc,
                                    p('ws', ws), p('status', st), hip.stream())
    for bad in (dict(k=0), dict(k=257), dict(d=0), dict(d=129), dict(n=-1), dict(ldx=d - 1), dict(ldc=d - 1)):
        assert step(**bad) == EINVAL and seed(**bad) == EINVAL, bad
    assert step(ldco=d - 1) == EINVAL and step(lds=d - 1) == EINVAL and step(it=0) == EINVAL and seed(init=-1) == EINVAL
    for name in ('X', 'C', 'C_out', 'labels', 'd2', 'counts', 'sums', 'inertia', 'changed', 'reseeded', 'state', 'ws', 'status'):
        assert step(**{name: True}) == EINVAL, name
    for name in ('X', 'rows', 'Cs', 'ws', 'status'):
        assert seed(**{name: True}) == EINVAL, name
    for shape in ((50, 8, 0), (50, 8, 257), (50, 0, 5), (50, 129, 5), (-1, 8, 5)):
        assert L.dcahip_kmeans_workspace_bytes(*shape) == EINVAL
    assert L.dcahip_kmeans_workspace_bytes(0, 8, 5) >= 0 and L.dcahip_kmeans_workspace_bytes(50, 128, 256) > 0
    assert L.dcahip_kmeans_workspace_bytes(50, 8, 5) == L.dcahip_kmeans_workspace_bytes(50, 8, 5)
    assert step(n=0) == 0 and seed(n=0) == 0                     # nothing launched
    torch.cuda.synchronize()
    for name, t in out.items():
        assert torch.equal(t, keep[name]), name
    assert int(st.item()) == 0
    for call in (lambda: ops.kmeans_seed(X, 0), lambda: ops.kmeans_seed(X, 257), lambda: ops.kmeans_workspace_bytes(5, 129, 2),
                 lambda: ops.kmeans_seed(X.double(), 3)):
        with pytest.raises(ValueError, match='kmeans'):
            call()
    assert step() == 0 and seed() == 0                           # the same calls with lawful arguments run
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and (out['labels'] >= 0).all() and (out['rows'][:k] >= 0).all() and (out['rows'][k:] == -19).all()


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_coordinates_raise(ops, bad):
    from dca_amd import cluster
    n, d, k = 300, 5, 4
    X = np.random.RandomState(0).normal(size=(n, d)).astype(np.float32)
    Xb = X.copy()
    Xb[123, d - 1] = bad
    Xb[7, 0] = bad
    with pytest.raises(ValueError, match='2 coordinates are not finite'):
        ops.kmeans_seed(_dev(Xb), k)
    b = _buffers(n, d, k)
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='2 coordinates are not finite'):
        _step(ops, _dev(Xb), _dev(X[:k]), torch.empty(k, d, device='cuda'), b, 1, ws)
    Cb = X[:k].copy()
    Cb[2, 1] = bad
    b = _buffers(n, d, k)
    with pytest.raises(ValueError, match='1 coordinates are not finite'):
        _step(ops, _dev(X), _dev(Cb), torch.empty(k, d, device='cuda'), b, 1, ws)
    with pytest.raises(ValueError, match='not finite'):
        cluster.kmeans(Xb, k, ops=ops)
    assert cluster.kmeans(X, k, n_init=2, ops=ops).converged      # the clean operands pass


# ---------------------------------------------------------------------------------------------------- through the model
def test_autoencoder_cluster_dense_and_counts_resident(ops, monkeypatch):
    import scipy.sparse as sp
    from dca_amd import io, cluster
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G, k = 300, 200, 6
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
    assert net.cluster(dense, k, n_init=3, seed=2) is None
    assert torch.equal(net.engine.w, w)
    Z = dense.obsm['X_dca']
    lab = dense.obs['dca_kmeans']
    assert Z.shape == (n, 32) and Z.dtype == np.float32
    assert isinstance(lab.dtype, pd.CategoricalDtype) and list(lab.cat.categories) == [str(c) for c in range(k)]
    u = dense.uns['dca_kmeans']
    assert set(u) == {'centers', 'inertia', 'n_iter', 'converged', 'sizes', 'params'}
    assert u['params'] == {'n_clusters': k, 'n_init': 3, 'max_iter': 300, 'seed': 2}
    assert u['centers'].shape == (k, 32) and u['centers'].dtype == np.float32 and u['sizes'].dtype == np.int64
    codes = lab.astype(int).to_numpy()
    np.testing.assert_array_equal(np.bincount(codes, minlength=k), u['sizes'])
    assert (np.diff(u['sizes']) <= 0).all() and u['sizes'].sum() == n
    res = cluster.kmeans(Z, k, n_init=3, seed=2, ops=ops)          # the module's door on the stored latent: the same run
    np.testing.assert_array_equal(res.labels, codes)
    np.testing.assert_array_equal(res.centers.view(np.uint32), u['centers'].view(np.uint32))
    assert res.inertia == u['inertia'] and res.n_iter == u['n_iter'] and res.converged == u['converged']
    net.predict(dense, mode='latent')
    np.testing.assert_array_equal(dense.obsm['X_dca'].view(np.uint32), Z.view(np.uint32))
    counts = adata('counts')
    net.cluster(counts, k, n_init=3, seed=2)
    assert net.engine.csr is not None and int(net.engine.gather_status.item()) == 0
    np.testing.assert_array_equal(counts.obsm['X_dca'].view(np.uint32), Z.view(np.uint32))
    np.testing.assert_array_equal(counts.obs['dca_kmeans'].astype(int).to_numpy(), codes)
    np.testing.assert_array_equal(counts.uns['dca_kmeans']['centers'].view(np.uint32), u['centers'].view(np.uint32))
    net.group_stats(counts, 'dca_kmeans')
    g = counts.uns['dca_groups']
    assert g['groupby'] == 'dca_kmeans' and int(np.sum(g['counts'])) == n
