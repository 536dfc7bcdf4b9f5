"""K-means clustering of a latent space, computed on the GPU (include/dcahip.h, dcahip_kmeans_seed / dcahip_kmeans_step --
K-MEANS): the step between ``dca(mode='latent')`` / ``Autoencoder.neighbors`` and ``Autoencoder.group_stats``, which the
reference leaves to the host.  Lloyd's algorithm from k-means++ seeds, deterministic: the seeding draws with integer
arithmetic, every sum is added in a fixed order, and the distance is the one of the neighbour search (dca_amd.neighbors).
``Autoencoder.cluster`` is the door for a fitted model, this module the one for a stored ``X_dca``.

    res = kmeans(adata.obsm['X_dca'], 12)                      # labels, centers, inertia, n_iter, converged, sizes
    labels, dist = kmeans_predict(new_latent, res.centers)     # new cells onto the fitted clustering
"""
from collections import namedtuple

import numpy as np

from ._device import as_points, default_ops, device_of

MAX_CLUSTERS = 256      # the limits of the kernels (include/dcahip.h)
MAX_D = 128
CHECK_EVERY = 8         # Lloyd iterations between two reads of the device's convergence state (the result does not depend on it)

KMeansResult = namedtuple('KMeansResult', 'labels centers inertia n_iter converged sizes')


def check_kmeans_args(n, d, k):
    """The argument limits of dcahip_kmeans_step / dcahip_kmeans_seed as ValueErrors that name them (nothing is launched for
    such a call)."""
    if not 1 <= k <= MAX_CLUSTERS:
        raise ValueError('dca_amd: kmeans: the number of clusters must lie in 1 .. %d (got %d)' % (MAX_CLUSTERS, k))
    if not 1 <= d <= MAX_D:
        raise ValueError('dca_amd: kmeans: the points must have 1 .. %d coordinates (got %d)' % (MAX_D, d))
    if not 0 <= n < 1 << 31:
        raise ValueError('dca_amd: kmeans: at most 2^31 - 1 points (got %d)' % n)


def renumber(sizes):
    """rank [k]: the number a run's cluster c gets in the result -- clusters by size descending, ties by their number in the
    run (as scanpy numbers Leiden clusters)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    order = np.lexsort((np.arange(len(sizes)), -sizes))
    rank = np.empty(len(sizes), dtype=np.int64)
    rank[order] = np.arange(len(sizes))
    return rank, order


def lloyd(ops, Xt, C, max_iter, ws, check_every=None):
    """Lloyd iterations on the device from the centres C [k, d] (updated in place) until the first converged iteration (no
    label changed, nothing re-seeded) or max_iter; the device's convergence state is read every ``check_every`` iterations
    only, the iterations past convergence being no-ops bit for bit.  If max_iter ends a run that has not converged, one more
    assignment gives the labels and the inertia of the centres returned.  Returns (labels int32 [n], C, inertia float, n_iter,
    converged, counts int32 [k]) -- device tensors where ops run on a device."""
    import torch
    check_every = int(check_every or CHECK_EVERY)
    n, d = Xt.shape
    k = C.shape[0]
    dev = Xt.device
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros(k, dtype=torch.int32, device=dev)
    sums = torch.zeros(k, d, dtype=torch.float64, device=dev)
    inertia = torch.zeros(1, dtype=torch.float64, device=dev)
    info = torch.zeros(3, dtype=torch.int32, device=dev)          # changed, reseeded, state
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    step = ops.kmeans_bind(Xt, C, C, labels, d2, counts, sums, inertia, info, ws, status)
    it, conv = 0, 0
    while it < max_iter:
        it += 1
        step(it)
        if it % check_every == 0 or it == max_iter:
            ops.kmeans_raise(status)
            conv = int(info[2].item())
            if conv:
                break
    if not conv:
        ops.kmeans_step(Xt, C, torch.empty_like(C), labels, d2, counts, sums, inertia, info, it + 1, ws, status, check=True)
    return labels, C, float(inertia.item()), conv or max_iter, bool(conv), counts


def kmeans(X, n_clusters, n_init=10, max_iter=300, seed=0, init=None, ops=None, on_device=None):
    """K-means of the rows of ``X`` [n, d] (host array or device tensor, taken as float32) into ``n_clusters`` clusters.

    init        None: k-means++ seeds drawn on the device, initialisation j of ``n_init`` from (seed, j); or an explicit
                [n_clusters, d] array of starting centres (n_init is then 1)
    n_init      runs; the one of the lowest inertia (compared as a double, ties to the lowest j) is returned
    max_iter    a run stops at the first converged iteration (no label changed and no cluster re-seeded) or here

    Returns KMeansResult(labels int32 [n], centers float32 [k, d], inertia float -- the sum of squared distances to the
    assigned centre --, n_iter, converged, sizes int64 [k]).  Clusters are numbered by size descending (ties by their number
    in the run), labels and centres permuted together.  An empty cluster takes the point farthest from its centre, one per
    iteration.  Host input gives numpy arrays, a device tensor gives device tensors.  Runs on the GPU (there is no host
    fallback); 1 <= n_clusters <= min(256, n), d <= 128; non-finite input raises ValueError."""
    import torch
    ops = default_ops(ops)
    if on_device is None:                                 # tensors out for a device tensor in (the engine asks for them)
        on_device = isinstance(X, torch.Tensor) and X.is_cuda
    dev = device_of(X, ops)
    Xt = as_points(X, dev, 'kmeans')
    n, d = Xt.shape
    k, n_init, max_iter, seed = int(n_clusters), int(n_init), int(max_iter), int(seed)
    check_kmeans_args(n, d, k)
    if k > n:
        raise ValueError('dca_amd: kmeans: %d clusters of %d points' % (k, n))
    if n_init < 1 or max_iter < 1:
        raise ValueError('dca_amd: kmeans: n_init and max_iter are at least 1 (got %d, %d)' % (n_init, max_iter))
    if not 0 <= seed < 1 << 64:
        raise ValueError('dca_amd: kmeans: seed is an unsigned 64-bit integer (got %d)' % seed)
    C0 = None
    if init is not None:
        C0 = as_points(init, dev, 'kmeans')
        if tuple(C0.shape) != (k, d):
            raise ValueError('dca_amd: kmeans: init must be [%d, %d] centres (got %s)' % (k, d, tuple(C0.shape)))
        n_init = 1
    ws = torch.empty(max(ops.kmeans_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=dev)
    best = None
    for j in range(n_init):
        C = C0.clone() if C0 is not None else ops.kmeans_seed(Xt, k, seed, j, ws=ws)[1]
        run = lloyd(ops, Xt, C, max_iter, ws)
        if best is None or run[2] < best[2]:
            best = run
    labels, C, inertia, n_iter, converged, counts = best
    sizes = counts.cpu().numpy().astype(np.int64)
    rank, order = renumber(sizes)
    labels = torch.as_tensor(rank.astype(np.int32)).to(dev)[labels.long()]
    centers = C[torch.as_tensor(order).to(dev)]
    sizes = sizes[order]
    if on_device:
        return KMeansResult(labels, centers, inertia, n_iter, converged, torch.as_tensor(sizes).to(dev))
    return KMeansResult(labels.cpu().numpy(), centers.cpu().numpy(), inertia, n_iter, converged, sizes)


def kmeans_predict(X, centers, ops=None):
    """``(labels int32 [n], distances float32 [n])``: the nearest of ``centers`` [k, d] to every row of ``X`` [n, d] (ties to
    the lowest number) and its Euclidean distance -- ``neighbors.knn(centers, 1, queries=X)`` reshaped, for mapping new cells
    onto a fitted clustering."""
    from .neighbors import knn
    idx, dist = knn(centers, 1, queries=X, ops=ops)
    return idx[:, 0], dist[:, 0]
