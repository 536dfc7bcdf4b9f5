"""The host references of K-SILHOUETTE (dcahip_silhouette / HipOps.silhouette / dca_amd.silhouette / Engine.latent_silhouette /
Autoencoder.silhouette): the silhouette in fp64 from the direct-form distances of the neighbour search's reference with the
conventions of include/dcahip.h, its fp32 restatement (the kernel's arithmetic: fp32 direct-form d2, the correctly rounded
fp32 square root, double sums), the float criterion, and SilhouetteRefOps, the CPU oracle with the entries it lacks so that
the Python layers above the kernel run in the CPU suite."""
import numpy as np
import torch

from _knn_ref import d2_ref, direct_fp32, float_tol, clustered  # noqa: F401  (clustered: the float dataset of the tests)
from _kmeans_ref import KmeansRefOps, int_data  # noqa: F401


def delta_ref(X):
    """[n, n] Euclidean distances in fp64."""
    return np.sqrt(d2_ref(X, X))


def delta_fp32(X):
    """[n, n] the distances the kernel forms, as doubles: np.sqrt in float32 of the fp32 direct form."""
    d2 = direct_fp32(X, X)
    assert d2.dtype == np.float32
    return np.sqrt(d2).astype(np.float64)


def silhouette_from_delta(D, codes, k):
    """The silhouette of include/dcahip.h from a distance matrix D [n, n] (float64): dict of s, a, b float64 [n], nearest
    int32 [n], counts int64 [k], cluster_mean float64 [k], mean, S [n, k] (the per-cluster distance sums) and M [n, k] (the
    mean distance to every OTHER non-empty cluster; inf for the own cluster, an empty one and a point in no cluster).  Codes
    outside [0, k) are in no cluster: neither a query nor a candidate (s = a = b = NaN, nearest = -1).  n_own = 1: s = a = 0;
    max(a, b) = 0: s = 0; fewer than two non-empty clusters: b = inf, nearest = -1, s = NaN."""
    codes = np.asarray(codes).astype(np.int64)
    n = len(codes)
    lab = (codes >= 0) & (codes < k)
    counts = np.bincount(codes[lab], minlength=k).astype(np.int64)
    S = np.zeros((n, k))
    for c in np.flatnonzero(counts):
        S[:, c] = D[:, np.flatnonzero(lab & (codes == c))].sum(axis=1)         # the candidates of c, ascending
    own = np.where(lab, codes, 0)
    rows = np.arange(n)
    n_own = counts[own]
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.where(n_own > 1, S[rows, own] / (n_own - 1.0), 0.0)
        M = np.where(counts[None, :] > 0, S / np.maximum(counts, 1)[None, :].astype(np.float64), np.inf)
    M[rows, own] = np.inf
    M[~lab] = np.inf
    b = M.min(axis=1)
    nearest = np.where(np.isfinite(b), M.argmin(axis=1), -1).astype(np.int32)  # argmin: the lowest c of equal minima
    mx = np.maximum(a, b)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(mx > 0, (b - a) / np.where(mx > 0, mx, 1.0), 0.0)
    s = np.where(n_own > 1, s, 0.0)
    s = np.where(np.isfinite(b), s, np.nan)
    for v in (s, a, b):
        v[~lab] = np.nan
    nearest[~lab] = -1
    cluster_mean = np.full(k, np.nan)
    for c in np.flatnonzero(counts):
        cluster_mean[c] = s[lab & (codes == c)].sum() / counts[c]
    mean = s[lab].sum() / lab.sum() if lab.any() else np.nan
    return dict(s=s, a=a, b=b, nearest=nearest, counts=counts, cluster_mean=cluster_mean, mean=float(mean), S=S, M=M)


def silhouette_ref(X, codes, k):
    """The fp64 reference: silhouette_from_delta on the fp64 direct-form distances."""
    return silhouette_from_delta(delta_ref(np.asarray(X, np.float32)), codes, k)


def silhouette_fp32(X, codes, k):
    """The kernel's arithmetic restated on the host: fp32 direct-form d2, np.sqrt in float32, double sums.  Where every fp32
    operation of d2 is exact and the double sums are exact (int_data: asserted in tests/test_silhouette_cpu.py) these are the
    bits the kernel must give."""
    return silhouette_from_delta(delta_fp32(np.asarray(X, np.float32)), codes, k)


def assert_silhouette_close(got, ref, d, codes, k, what=''):
    """The float criterion, for EVERY point, tol = float_tol(d): a and b within tol relative of the reference, |s - s_ref| <=
    2 tol, the returned nearest cluster is another non-empty cluster whose reference mean distance is <= b_ref (1 + tol),
    counts equal, and a point in no cluster has NaN / NaN / NaN / -1.  (The fp32 direct form is within tol / 2 relative at
    first order, the square root halves that and adds 2^-24, the double sums add (n - 1) 2^-53; s = +-(1 - min / max) with
    min / max <= 1, so its absolute error is at most twice the relative error of the ratio.)  Returns the worst errors."""
    tol = float_tol(d)
    codes = np.asarray(codes).astype(np.int64)
    n = len(codes)
    lab = (codes >= 0) & (codes < k)
    s, a, b = (np.asarray(got[key], np.float64) for key in ('s', 'a', 'b'))
    nearest = np.asarray(got['nearest'])
    assert s.shape == a.shape == b.shape == nearest.shape == (n,), (what, s.shape)
    np.testing.assert_array_equal(np.asarray(got['counts']).astype(np.int64), ref['counts'])
    assert np.isnan(s[~lab]).all() and np.isnan(a[~lab]).all() and np.isnan(b[~lab]).all() and (nearest[~lab] == -1).all(), what
    i = np.flatnonzero(lab)
    assert np.isfinite(ref['b'][i]).all(), (what, 'the criterion needs two non-empty clusters')
    ea, eb = np.abs(a[i] - ref['a'][i]), np.abs(b[i] - ref['b'][i])
    es = np.abs(s[i] - ref['s'][i])
    wa = float((ea / np.maximum(ref['a'][i], 1e-300)).max()) if len(i) else 0.0
    wb = float((eb / np.maximum(ref['b'][i], 1e-300)).max()) if len(i) else 0.0
    ws = float(es.max()) if len(i) else 0.0
    print('%s worst relative error of a %.2e, of b %.2e (tol %.2e); worst error of s %.2e (bound %.2e)' % (what, wa, wb, tol, ws, 2 * tol))
    assert (ea <= tol * ref['a'][i]).all(), (what, 'a', wa)
    assert (eb <= tol * ref['b'][i]).all(), (what, 'b', wb)
    assert (es <= 2 * tol).all(), (what, 's', ws)
    near = nearest[i].astype(np.int64)
    assert ((near >= 0) & (near < k)).all() and (near != codes[i]).all() and (ref['counts'][near] > 0).all(), (what, 'nearest')
    assert (ref['M'][i, near] <= ref['b'][i] * (1 + tol)).all(), (what, 'the returned nearest cluster is too far')
    return wa, wb, ws


# ---------------------------------------------------------------------------------------------------- the cases of the tests
# (n, d, k) of the exact tests on int_data coordinates: every n of {2, 3, 63, 64, 65, 255, 256, 257, 1031} (around a wave and
# the 256-query block; five blocks), every d of {1, 2, 3, 31, 32, 33, 128} (around the pad widths), every k of {2, 3, 16, 17,
# 255, 256}; k > n in (2, 2, 3), (3, 3, 17), (63, 1, 255), (64, 31, 256), (255, 33, 256)
EXACT = [(2, 2, 3), (3, 3, 17), (63, 1, 255), (64, 31, 256), (65, 32, 2), (255, 33, 256), (256, 128, 16), (257, 3, 17),
         (257, 2, 255), (1031, 1, 3), (1031, 32, 16), (1031, 32, 256), (1031, 128, 255), (1031, 31, 2), (1031, 33, 17),
         (256, 32, 3)]
EXACT_SPLITS = (1, 2, 7, 64, 0)


def edge_labels(n, k):
    """int32 [n] labels with the edges of the contract: cluster 0 holds about 90 % of the points, cluster 1 is a singleton,
    the last cluster is empty (k > 2), two points carry -1 and two a value >= k (n >= 8).  Below 8 points: clusters 0 and 1
    alternate (k > n: every other cluster is empty)."""
    if n < 8:
        return (np.arange(n) % 2).astype(np.int32)
    rs = np.random.RandomState(131 * n + k)
    lab = np.where(rs.rand(n) < 0.9, 0, rs.randint(0, k, n)).astype(np.int32)
    lab[lab == 1] = 0
    if k > 2:
        lab[lab == k - 1] = k - 2 if k > 3 else 0
    else:
        lab[rs.choice(n, max(2, n // 10), replace=False)] = 1         # two clusters: the second keeps some points
    where = rs.choice(n, 5, replace=False)
    if k > 2:
        lab[where[0]] = 1                                              # the singleton
    lab[where[1]], lab[where[2]], lab[where[3]], lab[where[4]] = -1, k, -1, k + 5
    return lab


# (d, k) of the float tests on clustered(1031, d), each with the two labellings of float_labels
FLOAT_N = 1031
FLOAT_CASES = [(3, 2), (3, 12), (32, 12), (32, 40), (128, 2), (128, 40)]
_cache = {}


def float_labels(d, k, kind):
    """'random': RandomState(d + k).randint(0, k, n) -- s near 0, the nearest cluster nearly tied; 'kmeans': the labels of
    kmeans_ref (one k-means++ start)."""
    from _kmeans_ref import kmeans_ref
    key = ('labels', d, k, kind)
    if key not in _cache:
        if kind == 'random':
            _cache[key] = np.random.RandomState(d + k).randint(0, k, FLOAT_N).astype(np.int32)
        else:
            _cache[key] = kmeans_ref(clustered(FLOAT_N, d), k, n_init=1)['labels'].astype(np.int32)
    return _cache[key]


def float_ref(d, k, kind):
    """The fp64 reference of one float case, computed once (the distance matrix of a d is shared) and left unchanged."""
    if ('delta', d) not in _cache:
        _cache[('delta', d)] = delta_ref(clustered(FLOAT_N, d))
    key = ('ref', d, k, kind)
    if key not in _cache:
        _cache[key] = silhouette_from_delta(_cache[('delta', d)], float_labels(d, k, kind), k)
    return _cache[key]


class SilhouetteRefOps(KmeansRefOps):
    """KmeansRefOps + silhouette (dca_amd.ops.HipOps.silhouette) from the fp64 reference."""
    name = 'cpu-oracle-silhouette'

    def silhouette_splits(self, n, d, k):
        from dca_amd.silhouette import check_silhouette_args
        check_silhouette_args(int(n), int(d), int(k))
        return 1

    def silhouette_workspace_bytes(self, n, d, k, splits=0):
        from dca_amd.silhouette import check_silhouette_args
        check_silhouette_args(int(n), int(d), int(k), int(splits))
        return 0

    def silhouette(self, X, labels, k, splits=0, ws=None):
        from dca_amd.silhouette import check_silhouette_args
        n, d = X.shape
        if labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
            raise ValueError('dca_amd: silhouette: labels is a contiguous int32 tensor of shape (%d,)' % n)
        check_silhouette_args(n, d, int(k), int(splits))
        Xn = X.numpy()
        bad = int((~np.isfinite(Xn)).sum())
        if bad:
            raise ValueError('dca_amd: silhouette: %d coordinates are not finite (NaN or inf)' % bad)
        r = silhouette_ref(Xn, labels.numpy(), int(k))
        live = int((r['counts'] > 0).sum())
        if live < 2:
            raise ValueError('dca_amd: silhouette: %d cluster%s with points: a silhouette compares at least 2'
                             % (live, '' if live == 1 else 's'))
        return dict(s=torch.from_numpy(r['s']), a=torch.from_numpy(r['a']), b=torch.from_numpy(r['b']),
                    nearest=torch.from_numpy(r['nearest']), counts=torch.from_numpy(r['counts'].astype(np.int32)),
                    cluster_mean=torch.from_numpy(r['cluster_mean']), mean=torch.tensor([r['mean']], dtype=torch.float64))
