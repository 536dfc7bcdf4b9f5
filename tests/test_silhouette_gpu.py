"""K-SILHOUETTE on the MI355X: dcahip_silhouette through the raw C entry and through HipOps against the host references
(tests/_silhouette_ref.py) -- bit for bit on integer coordinates, where every fp32 operation of the distance is exact and the
double sums of the fp32 square roots are exact in any order (the premise is asserted in tests/test_silhouette_cpu.py), for
every number of splits; to the float criterion on clusters far from the origin --, its determinism, the padding columns, the
refusals, choose_k, and Autoencoder.silhouette on dense and counts-resident data.

Bars on float data, tol = _knn_ref.float_tol(d) = 2 (d + 3) 2^-24: a and b within tol relative, s within 2 tol, the returned
nearest cluster within (1 + tol) of the reference's nearest, for every point (assert_silhouette_close).  The exact cases
compare with the fp32 restatement of the reference (silhouette_fp32: the same conventions on np.sqrt in float32 of the fp32
direct form) -- on these coordinates d2 is the fp64 reference's own value and the only rounding before the double sums is the
correctly rounded fp32 square root."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import synth_counts
from _kmeans_ref import int_data
from _silhouette_ref import (silhouette_ref, silhouette_fp32, assert_silhouette_close, edge_labels, float_labels, float_ref,
                             clustered, EXACT, EXACT_SPLITS, FLOAT_CASES, FLOAT_N)

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

    def untouched(self):
        b = self.buf.cpu().numpy()
        return (b[:self.PAD] == self.canary).all() and (b[self.PAD + self.count:] == self.canary).all()


def _raw(ops, X, codes, k, splits, pad=3, sentinel=99.0):
    """dcahip_silhouette through the C entry: a leading dimension of d + pad with the padding columns at a sentinel, canaries
    around every output and the workspace."""
    from dca_amd import hip
    n, d = X.shape
    ldx = d + pad
    Xp = torch.full((n, ldx), sentinel, device='cuda')
    Xp[:, :d] = _dev(X)
    lab = _dev(np.asarray(codes, np.int32))
    out = dict(s=Guarded(n, torch.float64, -5.0), a=Guarded(n, torch.float64, -7.0), b=Guarded(n, torch.float64, -9.0),
               nearest=Guarded(n, torch.int32, -11), counts=Guarded(k, torch.int32, -13),
               cluster_mean=Guarded(k, torch.float64, -15.0), mean=Guarded(1, torch.float64, -17.0),
               status=Guarded(1, torch.int32, 0))
    nbytes = ops.silhouette_workspace_bytes(n, d, k, splits)
    ws = Guarded(nbytes, torch.uint8, 0xA5)
    assert ws.ptr % 16 == 0
    o = out
    rc = ops.L.dcahip_silhouette(Xp.data_ptr(), ldx, n, d, lab.data_ptr(), k, splits, o['s'].ptr, o['a'].ptr, o['b'].ptr,
                                 o['nearest'].ptr, o['counts'].ptr, o['cluster_mean'].ptr, o['mean'].ptr, ws.ptr,
                                 o['status'].ptr, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for name, g in list(out.items()) + [('ws', ws)]:
        assert g.untouched(), name
    assert (Xp[:, d:] == sentinel).all() and torch.equal(lab.cpu(), torch.from_numpy(np.asarray(codes, np.int32)))
    return {name: g.get() for name, g in out.items()}


def _bits(r):
    return {name: r[name].tobytes() for name in ('s', 'a', 'b', 'nearest', 'counts', 'cluster_mean', 'mean')}


# ---------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize('n,d,k', EXACT)
def test_integer_coordinates_equal_the_reference_bit_for_bit_for_every_split(ops, n, d, k):
    X, _ = int_data(n, d, k)
    codes = edge_labels(n, k)
    ref = silhouette_fp32(X, codes, k)
    first = None
    for splits in EXACT_SPLITS:
        got = _raw(ops, X, codes, k, splits, pad=1 + (n + d) % 4)
        assert got['status'][0] == 0
        for name in ('s', 'a', 'b'):
            np.testing.assert_array_equal(got[name].view(np.uint64), ref[name].view(np.uint64), err_msg='%s splits %d' % (name, splits))
        np.testing.assert_array_equal(got['nearest'], ref['nearest'])
        np.testing.assert_array_equal(got['counts'], ref['counts'])
        bound = (n - 1) * 2.0 ** -53
        live = ref['counts'] > 0
        assert np.isnan(got['cluster_mean'][~live]).all()
        assert (np.abs(got['cluster_mean'][live] - ref['cluster_mean'][live]) <= bound).all()
        assert abs(got['mean'][0] - ref['mean']) <= bound
        if first is None:
            first = _bits(got)
        else:
            assert _bits(got) == first, splits                                 # the means too: one order for every split


def test_the_librarys_own_choice_of_more_than_one_split(ops):
    n, d, k = 2100, 5, 7
    assert ops.silhouette_splits(n, d, k) == 2 and ops.silhouette_splits(1031, 32, 16) == 1
    assert ops.silhouette_splits(1000000, 32, 16) == 1                         # no segment partials at 10^6 points
    assert ops.silhouette_workspace_bytes(n, d, k, 0) == ops.silhouette_workspace_bytes(n, d, k, 2) \
        > ops.silhouette_workspace_bytes(n, d, k, 1)
    X, _ = int_data(n, d, k)
    codes = edge_labels(n, k)
    ref = silhouette_fp32(X, codes, k)
    runs = [_raw(ops, X, codes, k, splits) for splits in (0, 1, 5)]
    for name in ('s', 'a', 'b'):
        np.testing.assert_array_equal(runs[0][name].view(np.uint64), ref[name].view(np.uint64))
    np.testing.assert_array_equal(runs[0]['nearest'], ref['nearest'])
    assert _bits(runs[0]) == _bits(runs[1]) == _bits(runs[2])


# ---------------------------------------------------------------------------------------------------- float data
@pytest.mark.parametrize('kind', ['random', 'kmeans'])
@pytest.mark.parametrize('d,k', FLOAT_CASES)
def test_float_data_every_point_meets_the_criterion(ops, d, k, kind):
    X = clustered(FLOAT_N, d)
    codes = float_labels(d, k, kind)
    ref = float_ref(d, k, kind)
    Xp = torch.full((FLOAT_N, d + 5), float('inf'), device='cuda')            # padding columns that would poison a sum
    Xp[:, :d] = _dev(X)
    runs = []
    for splits in (0, 3):
        got = {name: t.cpu().numpy() for name, t in ops.silhouette(Xp[:, :d], _dev(codes), k, splits=splits).items()}
        assert_silhouette_close(got, ref, d, codes, k, what='d %d k %d %s splits %d' % (d, k, kind, splits))
        live = ref['counts'] > 0
        assert (np.abs(got['cluster_mean'][live] - ref['cluster_mean'][live]) <= 2 * 2 * (d + 3) * 2.0 ** -24).all()
        assert abs(got['mean'][0] - ref['mean']) <= 2 * 2 * (d + 3) * 2.0 ** -24   # a mean of values each within 2 tol
        runs.append(got)
    again = {name: t.cpu().numpy() for name, t in ops.silhouette(Xp[:, :d], _dev(codes), k, splits=3).items()}
    assert _bits(again) == _bits(runs[1])                                      # two runs: the same bits


# ---------------------------------------------------------------------------------------------------- other behaviour
def test_a_non_finite_coordinate_raises_through_the_status_word(ops):
    n, d, k = 300, 5, 4
    X = np.random.RandomState(0).normal(size=(n, d)).astype(np.float32)
    codes = (np.arange(n) % k).astype(np.int32)
    codes[7] = -1
    for bad in (float('nan'), float('inf'), float('-inf')):
        Xb = X.copy()
        Xb[123, d - 1] = bad
        Xb[7, 0] = bad                                                         # an unlabelled row counts too
        with pytest.raises(ValueError, match='2 coordinates are not finite'):
            ops.silhouette(_dev(Xb), _dev(codes), k)
        got = _raw(ops, Xb, codes, k, 2)                                       # unspecified values, written in bounds
        assert got['status'][0] == 2
    assert np.isfinite(ops.silhouette(_dev(X), _dev(codes), k)['mean'].item())


def test_all_labels_in_one_cluster(ops):
    n, d, k = 257, 3, 5
    X, _ = int_data(n, d, k)
    codes = np.full(n, 3, np.int32)
    codes[[4, 200]] = -1
    ref = silhouette_fp32(X, codes, k)
    for splits in (1, 4):
        got = _raw(ops, X, codes, k, splits)
        lab = codes == 3
        assert np.isinf(got['b'][lab]).all() and (got['b'][lab] > 0).all() and (got['nearest'] == -1).all()
        assert np.isnan(got['s']).all() and np.isnan(got['a'][~lab]).all() and np.isnan(got['b'][~lab]).all()
        np.testing.assert_array_equal(got['a'][lab].view(np.uint64), ref['a'][lab].view(np.uint64))
        assert got['counts'].tolist() == [0, 0, 0, 255, 0] and np.isnan(got['cluster_mean']).all() and np.isnan(got['mean'][0])
    with pytest.raises(ValueError, match='1 cluster with points'):
        ops.silhouette(_dev(X), _dev(codes), k)
    with pytest.raises(ValueError, match='0 clusters with points'):
        ops.silhouette(_dev(X), _dev(np.full(n, -1, np.int32)), k)
    with pytest.raises(ValueError, match='0 clusters with points'):
        ops.silhouette(torch.empty(0, d, device='cuda'), torch.empty(0, dtype=torch.int32, device='cuda'), k)


def test_argument_errors_launch_nothing(ops):
    from dca_amd import hip
    n, d, k = 50, 8, 5
    X = _dev(np.random.RandomState(0).normal(size=(n, d)).astype(np.float32))
    lab = _dev((np.arange(n) % k).astype(np.int32))
    f = dict(device='cuda')
    out = dict(s=torch.full((n,), -5.0, dtype=torch.float64, **f), a=torch.full((n,), -7.0, dtype=torch.float64, **f),
               b=torch.full((n,), -9.0, dtype=torch.float64, **f), nearest=torch.full((n,), -11, dtype=torch.int32, **f),
               counts=torch.full((256,), -13, dtype=torch.int32, **f), cluster_mean=torch.full((256,), -15.0, dtype=torch.float64, **f),
               mean=torch.full((1,), -17.0, dtype=torch.float64, **f))
    keep = {name: t.clone() for name, t in out.items()}
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device='cuda')
    st = torch.zeros(1, dtype=torch.int32, device='cuda')
    L = ops.L

    def call(n=n, d=d, k=k, ldx=d, splits=0, **null):
        p = lambda name, t: None if name in null else t.data_ptr()
        return L.dcahip_silhouette(p('X', X), ldx, n, d, p('labels', lab), k, splits, p('s', out['s']), p('a', out['a']),
                                   p('b', out['b']), p('nearest', out['nearest']), p('counts', out['counts']),
                                   p('cluster_mean', out['cluster_mean']), p('mean', out['mean']), p('ws', ws), p('status', st),
                                   hip.stream())
    for bad in (dict(k=1), dict(k=0), dict(k=257), dict(d=0), dict(d=129), dict(n=-1), dict(ldx=d - 1), dict(splits=-1),
                dict(splits=65)):
        assert call(**bad) == EINVAL, bad
    for name in ('X', 'labels', 's', 'a', 'b', 'nearest', 'counts', 'cluster_mean', 'mean', 'ws', 'status'):
        assert call(**{name: True}) == EINVAL, name
    for shape in ((50, 8, 1), (50, 8, 257), (50, 0, 5), (50, 129, 5), (-1, 8, 5)):
        assert L.dcahip_silhouette_splits(*shape) == EINVAL
        assert L.dcahip_silhouette_workspace_bytes(*shape, 0) == EINVAL
    assert L.dcahip_silhouette_workspace_bytes(50, 8, 5, -1) == EINVAL and L.dcahip_silhouette_workspace_bytes(50, 8, 5, 65) == EINVAL
    assert L.dcahip_silhouette_workspace_bytes(0, 8, 5, 0) >= 0 and L.dcahip_silhouette_splits(0, 8, 5) == 1
    assert L.dcahip_silhouette_workspace_bytes(1031, 128, 256, 64) > L.dcahip_silhouette_workspace_bytes(1031, 128, 256, 1) > 0
    assert L.dcahip_silhouette_workspace_bytes(50, 8, 5, 7) == L.dcahip_silhouette_workspace_bytes(50, 8, 5, 7)
    assert call(n=0) == 0                                                      # nothing launched
    torch.cuda.synchronize()
    for name, t in out.items():
        assert torch.equal(t, keep[name]), name
    assert int(st.item()) == 0 and (ws == 0xA5).all()
    for bad in (lambda: ops.silhouette(X, lab, 1), lambda: ops.silhouette(X, lab, 257), lambda: ops.silhouette(X, lab, k, splits=65),
                lambda: ops.silhouette(X.double(), lab, k), lambda: ops.silhouette(X, lab.long(), k),
                lambda: ops.silhouette(X, lab[:49], k), lambda: ops.silhouette_workspace_bytes(5, 129, 2),
                lambda: ops.silhouette(X, lab, k, ws=torch.empty(16, dtype=torch.uint8, device='cuda'))):
        with pytest.raises(ValueError, match='silhouette'):
            bad()
    assert call() == 0                                                         # the same call with lawful arguments runs
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and (out['nearest'] >= 0).all() and out['counts'][:k].tolist() == [10] * k
    assert (out['counts'][k:] == -13).all() and (out['cluster_mean'][k:] == -15.0).all()


def test_the_module_on_host_and_device_input(ops):
    from dca_amd import silhouette as sil
    X = clustered(300, 5)
    names = np.asarray(['b', 'a', 'c'], dtype=object)[np.arange(300) % 3]
    names[[4, 40]] = None
    res = sil.silhouette(X, names, ops=ops)
    codes = np.asarray([{'a': 0, 'b': 1, 'c': 2}.get(v, -1) for v in names], np.int32)
    ref = silhouette_ref(X, codes, 3)
    assert res.names == ['a', 'b', 'c'] and isinstance(res.samples, np.ndarray) and res.sizes.dtype == np.int64
    got = dict(s=res.samples, a=res.intra, b=res.nearest_dist, nearest=res.nearest, counts=res.sizes)
    assert_silhouette_close(got, ref, 5, codes, 3, what='module')
    dev = sil.silhouette(_dev(X), _dev(codes), ops=ops)                        # device in: tensors out, the codes as they are
    assert dev.samples.is_cuda and dev.nearest.dtype == torch.int32 and dev.sizes.dtype == torch.int64 and dev.names == [0, 1, 2]
    assert dev.samples.cpu().numpy().tobytes() == res.samples.tobytes() and dev.mean == res.mean


def test_choose_k_on_three_well_separated_blobs(ops):
    from dca_amd import silhouette as sil
    rs = np.random.RandomState(0)
    centres = np.asarray([[0] * 4, [20] * 4, [-20, 20, 20, 20]], np.float64)
    X = np.concatenate([c + rs.normal(0, 1, (150, 4)) for c in centres]).astype(np.float32)
    res = sil.choose_k(X, range(2, 7), n_init=3, seed=1, ops=ops)
    assert res.best_k == 3 and res.table['k'].tolist() == [2, 3, 4, 5, 6]
    assert res.table['silhouette'][1] > 0.8 and (np.diff(res.table['inertia']) < 0).all()
    assert res.table['smallest_cluster'][1] == 150


# ---------------------------------------------------------------------------------------------------- through the model
def test_autoencoder_cluster_then_silhouette_dense_and_counts_resident(ops, monkeypatch):
    import scipy.sparse as sp
    from dca_amd import io
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
    net.cluster(dense, k, n_init=3, seed=2)
    assert net.silhouette(dense) is None
    assert torch.equal(net.engine.w, w)
    counts = adata('counts')
    net.cluster(counts, k, n_init=3, seed=2)
    net.silhouette(counts)
    assert net.engine.csr is not None and int(net.engine.gather_status.item()) == 0
    Z = dense.obsm['X_dca']
    np.testing.assert_array_equal(counts.obsm['X_dca'].view(np.uint32), Z.view(np.uint32))
    s = np.asarray(dense.obs['dca_silhouette'])
    assert s.dtype == np.float64 and s.tobytes() == np.asarray(counts.obs['dca_silhouette']).tobytes()
    assert np.asarray(dense.obs['dca_silhouette_nearest']).tolist() == np.asarray(counts.obs['dca_silhouette_nearest']).tolist()
    u, uc = dense.uns['dca_silhouette'], counts.uns['dca_silhouette']
    assert u['mean'] == uc['mean'] and u['cluster_mean'].tobytes() == uc['cluster_mean'].tobytes()
    names = [str(v) for v in u['names']]
    lab = np.asarray(dense.obs['dca_kmeans']).astype(str)
    codes = np.asarray([names.index(v) for v in lab], np.int32)
    ref = silhouette_ref(Z, codes, len(names))
    near = np.asarray([names.index(v) for v in np.asarray(dense.obs['dca_silhouette_nearest'])], np.int32)
    res = net.engine.latent_silhouette(codes, len(names))[1]
    assert res['s'].cpu().numpy().tobytes() == s.tobytes()
    got = dict(s=s, a=res['a'].cpu().numpy(), b=res['b'].cpu().numpy(), nearest=near, counts=u['sizes'])
    assert_silhouette_close(got, ref, 32, codes, len(names), what='model')
    assert abs(u['mean'] - ref['mean']) <= 2 * 2 * 35 * 2.0 ** -24
