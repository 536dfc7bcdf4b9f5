"""K-NEIGHBOURS on the MI355X: dcahip_knn through HipOps.knn against the fp64 reference (tests/_knn_ref.py) -- bit for bit on
integer coordinates with many ties, to the float criterion on clusters far from the origin --, its independence of the
candidate split, queries that are not the candidates, leading dimensions, the refusals, and Autoencoder.neighbors on dense
and counts-resident data.

Bars: integer coordinates in [-4, 4] make every fp32 operation exact, so indices and squared distances equal the fp64
reference's bits (which pins the (d2, index) order).  Float data: tests/_knn_ref.float_tol, twice the first-order bound
(d + 3) 2^-24 of the fp32 direct form."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from _knn_ref import knn_ref, assert_knn_close, clustered

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(ops, Q, X, k, **kw):
    idx, d2 = ops.knn(_dev(Q), _dev(X), k, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- exact, with ties
# (n, d, k, splits): every d of {1, 2, 3, 31, 32, 33, 128} (below / at / above the unroll widths 8 and 32, the widest), every
# n of {1, 2, 63, 64, 65, 255, 256, 257, 1031} (one candidate; around a wave and around the 256-query workgroup; five
# workgroups, 128-query ones from k = 33 up), every k of {1, 15, 16, 17, 64} (the list sizes 16 / 32 / 64 and their edges),
# k > n - 1 (padding) in rows 1, 3, 5, and explicit splits where the ties are densest (d = 1: nine distinct values)
EXACT = [(1, 1, 1, 0), (2, 2, 1, 0), (2, 3, 15, 0), (63, 31, 16, 0), (64, 32, 64, 0), (65, 33, 17, 0), (255, 128, 15, 0),
         (256, 32, 15, 2), (257, 3, 64, 0), (257, 2, 1, 3), (1031, 1, 17, 7), (1031, 32, 16, 0), (1031, 128, 64, 5),
         (1031, 33, 15, 64), (255, 31, 64, 0)]


def _integer_points(n, d, seed):
    rs = np.random.RandomState(seed)
    X = rs.randint(-4, 5, size=(n, d)).astype(np.float32)
    for a, b in ((5, 2), (n - 1, 0), (n // 2, n // 3)):         # duplicated rows
        if n > 5:
            X[a] = X[b]
    return X


@pytest.mark.parametrize('n,d,k,splits', EXACT)
def test_integer_coordinates_equal_the_reference_bit_for_bit(ops, n, d, k, splits):
    X = _integer_points(n, d, 1000 * n + d)
    ridx, rd2 = knn_ref(X, X, k, self_offset=0)
    idx, d2 = _run(ops, X, X, k, self_offset=0, splits=splits)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (n, k)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2.view(np.uint32), rd2.astype(np.float32).view(np.uint32))
    if k > n - 1:
        assert (idx[:, n - 1:] == -1).all() and np.isposinf(d2[:, n - 1:]).all()


# ---------------------------------------------------------------------------------------------------- splits
def test_every_split_gives_the_same_bits(ops):
    n, d, k = 1031, 32, 15
    X = np.random.RandomState(5).normal(0.0, 1.0, (n, d)).astype(np.float32)
    X[40] = X[900]                                              # a tie across the split boundaries
    L = ops.L
    s0 = L.dcahip_knn_splits(n, n, d, k)
    assert s0 == L.dcahip_knn_splits(n, n, d, k) == ops.knn_splits(n, n, d, k) == 1        # 1 031 candidates: one split
    assert L.dcahip_knn_splits(100, 200000, d, k) == 64 and L.dcahip_knn_splits(68579, 68579, d, k) == 6
    r16 = lambda x: (x + 15) // 16 * 16
    for s in (0, 1, 2, 7, 64):
        assert L.dcahip_knn_workspace_bytes(n, n, d, k, s) == r16((s or s0) * n * k * 8) == \
            L.dcahip_knn_workspace_bytes(n, n, d, k, s)
    assert L.dcahip_knn_workspace_bytes(n, n, 33, k, 2) == r16(2 * n * k * 8) + n * 64 * 4
    base = _run(ops, X, X, k, self_offset=0, splits=1)
    assert_knn_close(base[0], base[1], X, X, k, self_offset=0, what='splits=1')
    for s in (2, 7, 64, 0):
        idx, d2 = _run(ops, X, X, k, self_offset=0, splits=s)
        np.testing.assert_array_equal(idx, base[0], err_msg='splits=%d' % s)
        np.testing.assert_array_equal(d2.view(np.uint32), base[1].view(np.uint32), err_msg='splits=%d' % s)


# ---------------------------------------------------------------------------------------------------- float accuracy
_clustered = {}


def _clustered_case(ops, d):
    """The clustered input at width d and its self-search on the device -- made once."""
    if d not in _clustered:
        X = clustered(1500, d)
        _clustered[d] = (X,) + _run(ops, X, X, 15, self_offset=0)
    return _clustered[d]


@pytest.mark.parametrize('d', [3, 32, 128])
def test_clusters_far_from_the_origin_meet_the_float_criterion(ops, d):
    X, idx, d2 = _clustered_case(ops, d)
    assert_knn_close(idx, d2, X, X, 15, self_offset=0, what='clustered d=%d' % d)
    assert (d2 >= 0).all()
    # d2(i, j) and d2(j, i) are the same bits wherever both were returned
    got = {}
    for i in range(len(X)):
        for j, v in zip(idx[i].tolist(), d2[i].view(np.uint32).tolist()):
            got[(i, j)] = v
    both = [(i, j) for (i, j) in got if (j, i) in got]
    assert len(both) > len(X) and all(got[(i, j)] == got[(j, i)] for i, j in both)
    # row 7 is a copy of row 3: at exactly 0, first in each other's list
    assert idx[7, 0] == 3 and d2[7, 0] == 0.0 and idx[3, 0] == 7 and d2[3, 0] == 0.0


# ---------------------------------------------------------------------------------------------------- queries != candidates
def test_a_query_block_equals_its_rows_of_the_self_search(ops):
    X, idx, d2 = _clustered_case(ops, 32)
    pidx, pd2 = _run(ops, X[100:200], X, 15, self_offset=100)
    np.testing.assert_array_equal(pidx, idx[100:200])
    np.testing.assert_array_equal(pd2.view(np.uint32), d2[100:200].view(np.uint32))
    sidx, sd2 = _run(ops, X[100:200], X, 15, self_offset=-1)   # nothing left out: the row itself first, at 0
    assert (sidx[:, 0] == np.arange(100, 200)).all() and (sd2[:, 0] == 0).all()
    np.testing.assert_array_equal(sidx[:, 1:], idx[100:200, :14])
    np.testing.assert_array_equal(sd2[:, 1:].view(np.uint32), d2[100:200, :14].view(np.uint32))


@pytest.mark.parametrize('d,ldq,ldx', [(32, 40, 36), (3, 5, 3), (33, 33, 47)])
def test_leading_dimensions_and_untouched_padding(ops, d, ldq, ldx):
    n, nq, k, ldo = 700, 100, 15, 20
    X = clustered(n, d, seed=3)
    Xb = torch.full((n, ldx), float('nan'), dtype=torch.float32)
    Xb[:, :d] = torch.from_numpy(X)
    Qb = torch.full((nq, ldq), float('nan'), dtype=torch.float32)
    Qb[:, :d] = torch.from_numpy(X[100:200])
    Xb, Qb = Xb.cuda(), Qb.cuda()
    ib = torch.full((nq, ldo), -7, dtype=torch.int32).cuda()
    db = torch.full((nq, ldo), -1.0, dtype=torch.float32).cuda()
    ops.knn(Qb[:, :d], Xb[:, :d], k, self_offset=100, out=(ib[:, :k], db[:, :k]))      # the NaN pad is not a coordinate
    torch.cuda.synchronize()
    ib, db = ib.cpu().numpy(), db.cpu().numpy()
    assert (ib[:, k:] == -7).all() and (db[:, k:] == -1.0).all()
    assert torch.isnan(Xb[:, d:]).all() and torch.isnan(Qb[:, d:]).all()
    idx, d2 = _run(ops, X[100:200], X, k, self_offset=100)
    np.testing.assert_array_equal(ib[:, :k], idx)
    np.testing.assert_array_equal(db[:, :k].view(np.uint32), d2.view(np.uint32))
    assert_knn_close(idx, d2, X[100:200], X, k, self_offset=100, what='ld d=%d' % d)


# ---------------------------------------------------------------------------------------------------- refusals
def test_limits_are_refused_before_any_launch(ops):
    X = _dev(np.zeros((50, 8), np.float32))
    for k in (0, 65):
        with pytest.raises(ValueError, match='1 .. 64'):
            ops.knn(X, X, k)
    W = _dev(np.zeros((50, 129), np.float32))
    with pytest.raises(ValueError, match='1 .. 128'):
        ops.knn(W, W, 5)
    with pytest.raises(ValueError, match='splits'):
        ops.knn(X, X, 5, splits=65)
    # the entry point itself: DCAHIP_EINVAL, outputs and status untouched
    from dca_amd import hip
    idx = torch.full((50, 64), -7, dtype=torch.int32).cuda()
    d2 = torch.full((50, 64), -1.0, dtype=torch.float32).cuda()
    ws = torch.zeros(1 << 20, dtype=torch.uint8).cuda()
    st = torch.zeros(1, dtype=torch.int32).cuda()
    p = hip.ptr

    def call(Xt, ld, n, d, k, splits=0, ldo=64, self_offset=-1):
        return ops.L.dcahip_knn(p(Xt), ld, n, p(Xt), ld, n, d, k, self_offset, splits, p(idx), p(d2), ldo, p(ws), p(st),
                                hip.stream())
    assert call(X, 8, 50, 8, 0) == EINVAL and call(X, 8, 50, 8, 65) == EINVAL
    assert call(W, 129, 50, 129, 5) == EINVAL and call(X, 8, 50, 0, 5) == EINVAL
    assert call(X, 8, 50, 8, 5, splits=65) == EINVAL and call(X, 8, 50, 8, 5, splits=-1) == EINVAL
    assert call(X, 7, 50, 8, 5) == EINVAL and call(X, 8, 50, 8, 5, ldo=4) == EINVAL
    assert call(X, 8, -1, 8, 5) == EINVAL and call(X, 8, 50, 8, 5, self_offset=-2) == EINVAL
    for bad in ((50, 50, 8, 0), (50, 50, 8, 65), (50, 50, 129, 5), (50, 50, 0, 5)):
        assert ops.L.dcahip_knn_splits(*bad) == EINVAL and ops.L.dcahip_knn_workspace_bytes(*bad, 0) == EINVAL
    torch.cuda.synchronize()
    assert (idx == -7).all() and (d2 == -1.0).all() and int(st.item()) == 0
    assert call(X, 8, 50, 8, 5) == 0                            # and the same call with lawful arguments runs
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and (idx[:, :5] >= 0).all() and (idx[:, 5:] == -7).all()


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
@pytest.mark.parametrize('d', [8, 5])                          # candidates read in place / through the padded copy
def test_non_finite_coordinates_raise(ops, bad, d):
    X = np.random.RandomState(0).normal(size=(300, d)).astype(np.float32)
    Q = X[:20].copy()
    Xb = X.copy()
    Xb[123, d - 1] = bad
    with pytest.raises(ValueError, match='1 coordinates are not finite'):
        ops.knn(_dev(Q), _dev(Xb), 5)
    Qb = Q.copy()
    Qb[7, 0] = bad
    with pytest.raises(ValueError, match='1 coordinates are not finite'):
        ops.knn(_dev(Qb), _dev(X), 5)
    idx, d2 = _run(ops, Q, X, 5)                               # the clean operands pass
    assert (idx[:, 0] == np.arange(20)).all()


# ---------------------------------------------------------------------------------------------------- through the model
def test_autoencoder_neighbors_dense_and_counts_resident(ops, monkeypatch):
    import scipy.sparse as sp
    from dca_amd import io
    from dca_amd._anndata import AnnData
    from dca_amd.network import AE_types
    from dca_amd.train import train
    n, G, k = 300, 200, 15
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
    assert net.neighbors(dense, n_neighbors=k) is None
    assert torch.equal(net.engine.w, w)
    Z = dense.obsm['X_dca']
    idx, dist = dense.obsm['dca_knn_indices'], dense.obsm['dca_knn_distances']
    assert Z.shape == (n, 32) and Z.dtype == np.float32 and idx.dtype == np.int32 and dist.dtype == np.float32
    assert dense.uns['dca_neighbors'] == {'n_neighbors': k, 'metric': 'euclidean', 'include_self': False}
    # the kernel's squared distances, through the engine, against the reference on the stored latent
    _, eidx, ed2 = net.engine.latent_knn(k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eidx.cpu().numpy(), idx)
    np.testing.assert_array_equal(np.sqrt(ed2.cpu().numpy()), dist)
    assert_knn_close(idx, ed2.cpu().numpy(), Z, Z, k, self_offset=0, what='model')
    net.predict(dense, mode='latent')                          # the same cells bound the same way: the same latent
    np.testing.assert_array_equal(dense.obsm['X_dca'].view(np.uint32), Z.view(np.uint32))
    counts = adata('counts')
    net.neighbors(counts, n_neighbors=k)
    assert net.engine.csr is not None and int(net.engine.gather_status.item()) == 0
    np.testing.assert_array_equal(counts.obsm['X_dca'].view(np.uint32), Z.view(np.uint32))
    np.testing.assert_array_equal(counts.obsm['dca_knn_indices'], idx)
    np.testing.assert_array_equal(counts.obsm['dca_knn_distances'].view(np.uint32), dist.view(np.uint32))
