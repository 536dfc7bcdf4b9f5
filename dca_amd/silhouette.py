"""The silhouette coefficient of a clustering of a latent space, computed on the GPU (include/dcahip.h, dcahip_silhouette --
K-SILHOUETTE): the number that says whether a clustering is any good, which ``Autoencoder.cluster`` / ``cluster.kmeans`` do
not give (their inertia falls with every added cluster).  For a point i of cluster A, a_i is its mean Euclidean distance to the
other points of A, b_i its mean distance to the points of the nearest other cluster, s_i = (b_i - a_i) / max(a_i, b_i) in
[-1, 1]: near 1 the point sits well inside its cluster, near 0 between two, below 0 closer to another cluster than to its own.
Every pair of points is visited on the device (no sampling); scikit-learn's conventions where it has one.
``Autoencoder.silhouette`` is the door for a fitted model, this module the one for a stored ``X_dca``.

    res = silhouette(adata.obsm['X_dca'], adata.obs['dca_kmeans'])     # samples, intra, nearest_dist, nearest, cluster_mean, ..
    table, k = choose_k(adata.obsm['X_dca'], range(2, 21))             # k-means and its mean silhouette for every k
"""
from collections import namedtuple

import numpy as np

from ._device import as_points, default_ops, device_of

MAX_CLUSTERS = 256      # the limits of the kernel (include/dcahip.h)
MAX_D = 128
MAX_SPLITS = 64

SilhouetteResult = namedtuple('SilhouetteResult', 'samples intra nearest_dist nearest cluster_mean sizes mean names')
ChooseKResult = namedtuple('ChooseKResult', 'table best_k')


def check_silhouette_args(n, d, k, splits=0):
    """The argument limits of dcahip_silhouette as ValueErrors that name them (nothing is launched for such a call)."""
    if not 2 <= k <= MAX_CLUSTERS:
        raise ValueError('dca_amd: silhouette: the number of clusters must lie in 2 .. %d (got %d)' % (MAX_CLUSTERS, k))
    if not 1 <= d <= MAX_D:
        raise ValueError('dca_amd: silhouette: the points must have 1 .. %d coordinates (got %d)' % (MAX_D, d))
    if not 0 <= n < 1 << 31:
        raise ValueError('dca_amd: silhouette: at most 2^31 - 1 points (got %d)' % n)
    if not 0 <= splits <= MAX_SPLITS:
        raise ValueError('dca_amd: silhouette: splits is 0 (the library\'s choice) or 1 .. %d (got %d)' % (MAX_SPLITS, splits))


def check_label_count(k, what='silhouette'):
    """A silhouette needs two clusters to compare and the kernel takes at most 256."""
    if k < 2:
        raise ValueError('dca_amd: %s: %d distinct label%s: a silhouette compares at least 2 clusters'
                         % (what, k, '' if k == 1 else 's'))
    if k > MAX_CLUSTERS:
        raise ValueError('dca_amd: %s: %d distinct labels (at most %d)' % (what, k, MAX_CLUSTERS))


def silhouette(X, labels, ops=None):
    """The silhouette of every row of ``X`` [n, d] (host array or device tensor, taken as float32) under ``labels``.

    labels      any 1-d array of n labels (strings, integers, a pandas categorical); NaN / None: the point is in no cluster,
                neither scored nor counted in any mean distance.  The clusters are the sorted distinct labels
                (groups.label_codes).  An int32 tensor on the device is taken as codes 0 .. max as it is (any value outside:
                in no cluster).

    Returns SilhouetteResult(samples float64 [n] -- NaN for a point in no cluster --, intra = a float64 [n], nearest_dist = b
    float64 [n], nearest int32 [n] -- the index in ``names`` of the nearest other cluster, -1 for a point in no cluster --,
    cluster_mean float64 [k] -- NaN for a cluster without points --, sizes int64 [k], mean float -- over all labelled points,
    scikit-learn's silhouette_score --, names).  A cluster of one point scores 0.  Host input gives numpy arrays, a device
    tensor gives device tensors.  Runs on the GPU (there is no host fallback); 2 .. 256 clusters, at least two of them with
    points, d <= 128; non-finite input raises ValueError."""
    import torch
    ops = default_ops(ops)
    on_device = isinstance(X, torch.Tensor) and X.is_cuda
    dev = device_of(X, ops)
    Xt = as_points(X, dev, 'silhouette')
    n, d = Xt.shape
    if isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.device == dev and labels.dim() == 1:
        codes = labels.contiguous()
        k = int(codes.max().item()) + 1 if codes.numel() else 0
        names = list(range(max(k, 0)))
    else:
        from .groups import label_codes
        if isinstance(labels, torch.Tensor):
            labels = labels.cpu().numpy()
        if np.ndim(labels) != 1:
            raise ValueError('dca_amd: silhouette: labels are a 1-d array (got %d dimensions)' % np.ndim(labels))
        names, cnp = label_codes(labels)
        k = len(names)
        codes = torch.from_numpy(cnp).to(dev)
    if codes.shape[0] != n:
        raise ValueError('dca_amd: silhouette: %d labels for %d points' % (codes.shape[0], n))
    check_label_count(k)
    check_silhouette_args(n, d, k)
    r = ops.silhouette(Xt, codes, k)
    mean = float(r['mean'].item())
    out = (r['s'], r['a'], r['b'], r['nearest'], r['cluster_mean'], r['counts'].to(torch.int64))
    if not on_device:
        out = tuple(t.cpu().numpy() for t in out)
    return SilhouetteResult(*out, mean, names)


def choose_k(X, ks, n_init=10, max_iter=300, seed=0, ops=None):
    """K-means (cluster.kmeans) and the mean silhouette of its result for every k of ``ks`` (each 2 .. min(256, n)), all on
    the device: the points go up once and only the scalars of the table come back.

    Returns ChooseKResult(table, best_k): ``table`` a pandas DataFrame with one row per k in the order given -- k, inertia,
    silhouette (the mean over all points), n_iter, converged, smallest_cluster (its points) --, ``best_k`` the k of the
    highest mean silhouette, ties to the lowest k."""
    import pandas as pd
    from .cluster import kmeans
    ops = default_ops(ops)
    Xt = as_points(X, device_of(X, ops), 'choose_k')
    n, d = Xt.shape
    ks = [int(k) for k in ks]
    if not ks:
        raise ValueError('dca_amd: choose_k: no k to try')
    for k in ks:
        check_silhouette_args(n, d, k)
        if k > n:
            raise ValueError('dca_amd: choose_k: %d clusters of %d points' % (k, n))
    rows = []
    for k in ks:
        res = kmeans(Xt, k, n_init=n_init, max_iter=max_iter, seed=seed, ops=ops, on_device=True)
        sil = float(ops.silhouette(Xt, res.labels, k)['mean'].item())
        rows.append(dict(k=k, inertia=float(res.inertia), silhouette=sil, n_iter=int(res.n_iter),
                         converged=bool(res.converged), smallest_cluster=int(res.sizes.min().item())))
    table = pd.DataFrame(rows, columns=['k', 'inertia', 'silhouette', 'n_iter', 'converged', 'smallest_cluster'])
    best = max(rows, key=lambda r: (r['silhouette'], -r['k']))
    return ChooseKResult(table, best['k'])


def model_silhouette(net, adata, groupby='dca_kmeans', key_added='dca_silhouette', copy=False):
    """Autoencoder.silhouette (documented there)."""
    from .groups import label_codes, obs_labels
    eng = net.engine
    net._wanted('latent', False)                          # hidden_size=(): no centre layer
    n = adata.n_obs
    labels, key = obs_labels(adata, groupby, 'silhouette')
    names, codes = label_codes(labels)
    k = len(names)
    check_label_count(k)
    check_silhouette_args(n, eng.lay.hidden[eng.center], k)
    net._one_process('silhouette')
    adata = adata.copy() if copy else adata
    net._bind_inputs(adata)
    latent, r = eng.latent_silhouette(codes, k, chunk=net._chunk(n))
    nearest = r['nearest'].cpu().numpy()
    near = np.full(n, None, dtype=object)
    near[nearest >= 0] = np.array(names, dtype=object)[nearest[nearest >= 0]]
    adata.obsm['X_dca'] = latent.cpu().numpy()
    adata.obs[key_added] = r['s'].cpu().numpy().astype(np.float64)
    adata.obs[key_added + '_nearest'] = near
    adata.uns[key_added] = {'groupby': key, 'names': np.array(names, dtype=object),
                            'sizes': r['counts'].cpu().numpy().astype(np.int64),
                            'cluster_mean': r['cluster_mean'].cpu().numpy().astype(np.float64),
                            'mean': float(r['mean'].item()), 'params': {'metric': 'euclidean'}}
    return adata if copy else None
