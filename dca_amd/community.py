"""Louvain clustering of the neighbour graph, computed on the GPU (include/dcahip.h, dcahip_graph_symmetrize /
dcahip_louvain_sweep -- K-LOUVAIN): community detection on the graph ``Autoencoder.neighbors`` writes, the step scanpy
users run as ``sc.tl.louvain`` on the host.  Modularity optimisation (Blondel et al. 2008) in integers throughout:
synchronous sweeps whose direction alternates, levels of aggregation until nothing merges.  Deterministic: the same labels on
every run, equal to the host restatement of the tests.  ``Autoencoder.louvain`` is the door for a fitted model, this module
the one for a stored neighbour graph.

    res = louvain(adata.obsm['dca_knn_indices'])               # labels, modularity, n_levels, sizes, ...
    q = modularity(indices, kmeans_labels)                     # the same number for any other labelling
    adata.obsp['connectivities'] = knn_adjacency(indices)      # W = A + A^T as a scipy CSR
"""
from collections import namedtuple

import numpy as np

from ._device import default_ops, device_of

R = 1024                # the denominator of the quantised resolution
MAX_G = 64 * R
CHECK_EVERY = 8         # sweeps between two reads of the device's state (the result does not depend on it)

LouvainResult = namedtuple('LouvainResult', 'labels modularity n_levels sizes level_sizes n_sweeps resolution')


def quantise(resolution):
    """g = round(resolution * 1024), the integer the scores use; ValueError outside 1 .. 65536."""
    g = int(round(float(resolution) * R))
    if not 1 <= g <= MAX_G:
        raise ValueError('dca_amd: louvain: the resolution must lie in 1/%d .. %d (got %r)' % (R, MAX_G // R, resolution))
    return g


def check_graph_args(n, k):
    """The limits of dcahip_graph_symmetrize as ValueErrors that name them (nothing is launched for such a call)."""
    if not 0 <= n < 1 << 31:
        raise ValueError('dca_amd: louvain: at most 2^31 - 1 vertices (got %d)' % n)
    if k < 1:
        raise ValueError('dca_amd: louvain: the index array has at least 1 column (got %d)' % k)
    if 2 * n * k >= 1 << 31:
        raise ValueError('dca_amd: louvain: the graph\'s total weight 2m must stay below 2^31; %d rows of %d neighbours can '
                         'reach %d' % (n, k, 2 * n * k))


def check_level_args(n, nnz, twom, g, max_sweeps):
    """The limits of dcahip_louvain_begin / dcahip_louvain_sweep as ValueErrors that name them."""
    if not 0 <= n < 1 << 31:
        raise ValueError('dca_amd: louvain: at most 2^31 - 1 vertices (got %d)' % n)
    if not 0 <= twom < 1 << 31 or not 0 <= nnz < 1 << 31:
        raise ValueError('dca_amd: louvain: the graph\'s total weight 2m and its entries must stay below 2^31 (got %d, %d)'
                         % (twom, nnz))
    if not 1 <= g <= MAX_G:
        raise ValueError('dca_amd: louvain: the quantised resolution must lie in 1 .. %d (got %d)' % (MAX_G, g))
    if max_sweeps < 1:
        raise ValueError('dca_amd: louvain: max_sweeps is at least 1 (got %d)' % max_sweeps)


def check_louvain_args(n, k, resolution=1.0, max_levels=32, max_sweeps=1000):
    """Every limit of ``louvain`` as a ValueError that names it (nothing is launched for such a call).  Returns g."""
    check_graph_args(int(n), int(k))
    g = quantise(resolution)
    if int(max_levels) < 1 or int(max_sweeps) < 1:
        raise ValueError('dca_amd: louvain: max_levels and max_sweeps are at least 1 (got %d, %d)' % (max_levels, max_sweeps))
    return g


def relabel(labels):
    """(cu int64 [n], nc): the communities of ``labels`` (a tensor of values in 0 .. n-1) renumbered 0 .. nc-1 by their lowest
    member vertex.  Device operations only."""
    import torch
    n = labels.numel()
    lab = labels.long()
    idx = torch.arange(n, dtype=torch.int64, device=labels.device)
    first = torch.full((n,), n, dtype=torch.int64, device=labels.device).scatter_reduce(0, lab, idx, 'amin')
    ids = torch.nonzero(first < n).flatten()
    order = torch.argsort(first[ids])                        # the lowest members are distinct: no ties
    new_id = torch.zeros(n, dtype=torch.int64, device=labels.device)
    new_id[ids[order]] = torch.arange(ids.numel(), dtype=torch.int64, device=labels.device)
    return new_id[lab], int(ids.numel())


def aggregate(rowptr, col, wt, cu, nc):
    """The coarse graph of a level: vertex = community cu[i] in 0 .. nc-1, the weight of (a, b) = the sum of the entries
    (i, j) with cu[i] = a, cu[j] = b, so a self-loop carries the weight inside a community in both directions.  Composed from
    device operations on 64-bit keys (unique / segment sums in integers); returns (rowptr int64 [nc + 1], col int32, wt
    int32), columns ascending in every row."""
    import torch
    dev = rowptr.device
    n = rowptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
    key = cu[rows] * nc + cu[col.long()]
    w = wt.long() if wt is not None else torch.ones_like(key)
    ukey, inv = torch.unique(key, return_inverse=True)
    wsum = torch.zeros(ukey.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, w)
    r = torch.div(ukey, nc, rounding_mode='floor')
    out = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    out[1:] = torch.cumsum(torch.bincount(r, minlength=nc), 0)
    return out, (ukey - r * nc).to(torch.int32), wsum.to(torch.int32)


def _indices(indices, dev):
    import torch
    if not isinstance(indices, torch.Tensor):
        indices = torch.from_numpy(np.ascontiguousarray(np.asarray(indices)))
    if indices.dim() != 2:
        raise ValueError('dca_amd: louvain: the neighbour indices are an [n, k] array (got %d dimensions)' % indices.dim())
    if indices.is_floating_point() or indices.dtype == torch.bool:
        raise ValueError('dca_amd: louvain: the neighbour indices are integers (got %s)' % indices.dtype)
    return indices.to(device=dev, dtype=torch.int32).contiguous()


def run_level(ops, rowptr, col, wt, twom, g, max_sweeps, check_every=None):
    """One level from singletons to its end; the device's state is read every ``check_every`` sweeps only, the sweeps past the
    end being no-ops.  Returns (labels int32 [n] -- the best state --, the integer Q, sweeps run)."""
    check_every = int(check_every or CHECK_EVERY)
    lev = ops.louvain_level(rowptr, col, wt, twom, g, max_sweeps)
    s = 0
    while True:
        lev.sweep(s)
        s += 1
        if s % check_every == 0:
            st = lev.read(s - 1)
            if st['done']:
                return lev.labels, st['q'], st['sweeps']


def louvain(indices, resolution=1.0, max_levels=32, max_sweeps=1000, ops=None, check_every=None, details=False,
            on_device=None):
    """Louvain communities of the graph W = A + A^T of a k-nearest-neighbour index array ``indices`` [n, k] (host array or
    device tensor of integers; -1 is padding, a row's own index is dropped, a mutual pair weighs 2).

    resolution  gamma of Q = sum_c [in_c / 2m - gamma (tot_c / 2m)^2], quantised to 1/1024 (1/1024 .. 64)
    max_levels  levels of aggregation at most; the run ends at the first level that merges nothing
    max_sweeps  sweeps per level at most; a level ends when a sweep fails to raise Q (it is discarded) or when two sweeps in a
                row, one of each direction, move nothing

    Returns LouvainResult(labels int32 [n], modularity float -- from the exact integers --, n_levels, sizes int64 -- the
    communities by size descending (ties by their lowest member), as the labels number them --, level_sizes -- the vertices
    left after each level --, n_sweeps -- per level run --, resolution -- the quantised value used).  Host input gives numpy
    arrays, a device tensor gives device tensors.  Runs on the GPU (there is no host fallback); n < 2^31 and 2 n k < 2^31.
    ``details=True`` returns (result, dict of q_int, twom, g) for tests and tools."""
    import torch
    from .cluster import renumber
    ops = default_ops(ops)
    if on_device is None:                                 # tensors out for a device tensor in (the engine asks for them)
        on_device = isinstance(indices, torch.Tensor) and indices.is_cuda
    dev = device_of(indices, ops)
    idx = _indices(indices, dev)
    n, k = idx.shape
    g = check_louvain_args(n, k, resolution, max_levels, max_sweeps)
    rowptr, col, _ = ops.graph_symmetrize(idx)
    twom = int(col.numel())
    wt = None
    members = torch.arange(n, dtype=torch.int64, device=dev)
    level_sizes, n_sweeps, q_int = [], [], 0
    while twom > 0 and len(level_sizes) < int(max_levels):
        labels, q_int, sweeps = run_level(ops, rowptr, col, wt, twom, g, int(max_sweeps), check_every)
        n_sweeps.append(int(sweeps))
        cu, nc = relabel(labels)
        if nc == rowptr.numel() - 1:
            break
        members = cu[members]
        level_sizes.append(nc)
        rowptr, col, wt = aggregate(rowptr, col, wt, cu, nc)
    nc = level_sizes[-1] if level_sizes else n
    sizes = torch.bincount(members, minlength=nc).cpu().numpy().astype(np.int64)
    rank, order = renumber(sizes)
    labels = torch.as_tensor(rank.astype(np.int32)).to(dev)[members]
    sizes = sizes[order]
    q = q_int / float(twom * twom * R) if twom else 0.0
    res = LouvainResult(labels if on_device else labels.cpu().numpy(), q, len(level_sizes),
                        torch.as_tensor(sizes).to(dev) if on_device else sizes, level_sizes, n_sweeps, g / float(R))
    return (res, dict(q_int=q_int, twom=twom, g=g)) if details else res


def modularity_int(rowptr, col, wt, labels, g):
    """(Q_int, 2m) of a labelling of a CSR graph, in integers on the graph's device: Q_int = M in - g tot2, M = 2m * 1024."""
    import torch
    dev = rowptr.device
    n = rowptr.numel() - 1
    lab = labels.to(device=dev).long()
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), rowptr[1:] - rowptr[:-1])
    w = wt.long() if wt is not None else torch.ones(col.numel(), dtype=torch.int64, device=dev)
    inside = int(w[lab[rows] == lab[col.long()]].sum().item())
    _, codes = torch.unique(lab, return_inverse=True)
    tot = torch.zeros(n + 1, dtype=torch.int64, device=dev).index_add_(0, codes[rows], w)
    twom = int(w.sum().item())
    tot2 = int((tot * tot).sum().item())                     # <= (2m)^2 < 2^62
    return twom * R * inside - g * tot2, twom


def modularity(indices, labels, resolution=1.0, ops=None):
    """The modularity of ANY labelling (k-means labels, annotations) of the graph ``louvain`` clusters: labels [n] integers,
    one community per distinct value.  The integers are formed on the device; the float is Q_int / ((2m)^2 1024), the number
    ``louvain`` reports for its own labels."""
    import torch
    ops = default_ops(ops)
    dev = device_of(indices, ops)
    g = quantise(resolution)
    idx = _indices(indices, dev)
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if labels.dim() != 1 or labels.numel() != idx.shape[0] or labels.is_floating_point():
        raise ValueError('dca_amd: modularity: labels are %d integers, one per row of the indices' % idx.shape[0])
    rowptr, col, _ = ops.graph_symmetrize(idx)
    q_int, twom = modularity_int(rowptr, col, None, labels, g)
    return q_int / float(twom * twom * R) if twom else 0.0


def knn_adjacency(indices):
    """``scipy.sparse.csr_matrix`` [n, n] of W = A + A^T for an index array [n, k] (host): integer weights, 2 for a mutual
    pair, no diagonal -- the graph ``louvain`` clusters, in the layout of ``obsp``."""
    import scipy.sparse as sp
    indices = np.asarray(indices)
    if indices.ndim != 2:
        raise ValueError('dca_amd: knn_adjacency: the neighbour indices are an [n, k] array')
    n, k = indices.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = indices.reshape(-1).astype(np.int64)
    keep = (cols != -1) & (cols != rows)
    if keep.any() and (cols[keep].min() < 0 or cols[keep].max() >= n):
        raise ValueError('dca_amd: knn_adjacency: an index lies outside 0 .. %d' % (n - 1))
    A = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int32), (rows[keep], cols[keep])), shape=(n, n))
    W = (A + A.T).tocsr()
    W.sort_indices()
    return W
