"""The k-nearest-neighbour graph of a latent space, computed on the GPU (include/dcahip.h, dcahip_knn -- K-NEIGHBOURS): what
follows ``dca(mode='latent')`` in every workflow (clustering, UMAP, diffusion pseudotime, label transfer) and what the
reference leaves to scanpy on the host.  Exact, Euclidean; ``Autoencoder.neighbors`` is the door for a fitted model, this
module the one for a stored ``X_dca`` and for mapping new cells onto a fitted atlas.

    idx, dist = knn(adata.obsm['X_dca'], 15)                   # every cell's 15 nearest OTHER cells
    idx, dist = knn(atlas_latent, 15, queries=new_latent)      # the atlas cells nearest to each new cell
    adata_obsp_distances = knn_graph(idx, dist)                # scipy CSR in the layout of scanpy's obsp['distances']
"""
import numpy as np

from ._device import as_points, default_ops, device_of

MAX_K = 64          # the limits of the kernel (include/dcahip.h)
MAX_D = 128
MAX_SPLITS = 64


def check_knn_args(nq, n, d, k, splits=0, self_offset=-1):
    """The argument limits of dcahip_knn as ValueErrors that name them (nothing is launched for such a call)."""
    if not 1 <= k <= MAX_K:
        raise ValueError('dca_amd: knn: k must lie in 1 .. %d (got %d)' % (MAX_K, k))
    if not 1 <= d <= MAX_D:
        raise ValueError('dca_amd: knn: the points must have 1 .. %d coordinates (got %d)' % (MAX_D, d))
    if not 0 <= n < 1 << 31 or not 0 <= nq < 1 << 31:
        raise ValueError('dca_amd: knn: at most 2^31 - 1 candidates and queries (got %d, %d)' % (n, nq))
    if not 0 <= splits <= MAX_SPLITS:
        raise ValueError('dca_amd: knn: splits must lie in 0 .. %d (got %d)' % (MAX_SPLITS, splits))
    if self_offset < -1:
        raise ValueError('dca_amd: knn: self_offset is -1 (none) or a row of the candidates (got %d)' % self_offset)


def knn(X, n_neighbors, queries=None, ops=None):
    """The ``n_neighbors`` nearest rows of ``X`` [n, d] to every row of ``queries`` [nq, d] -- or, with ``queries=None``, to
    every row of ``X`` itself, the row left out (by index: an identical copy of it elsewhere stays, at distance 0).
    ``X`` / ``queries``: host arrays or device tensors, taken as float32.  Returns ``(indices [nq, k] int32, distances
    [nq, k] float32)``, Euclidean distances, every row ascending in (distance, index); where ``X`` has fewer than k
    (other) rows the tail is -1 at inf.  Host inputs give numpy arrays, a device tensor ``X`` gives device tensors.
    Runs on the GPU (there is no host fallback); 1 <= n_neighbors <= 64, d <= 128."""
    import torch
    ops = default_ops(ops)
    on_device = isinstance(X, torch.Tensor) and X.is_cuda
    dev = device_of(X, ops)
    Xt = as_points(X, dev, 'knn')
    Qt = Xt if queries is None else as_points(queries, dev, 'knn')
    idx, d2 = ops.knn(Qt, Xt, int(n_neighbors), self_offset=0 if queries is None else -1)
    dist = torch.sqrt(d2)
    if on_device:
        return idx, dist
    return idx.cpu().numpy(), dist.cpu().numpy()


def knn_graph(indices, distances, n_cols=None):
    """``scipy.sparse.csr_matrix`` [n, n_cols] with distances[i, j] at (i, indices[i, j]) -- the layout of scanpy's
    ``obsp['distances']`` (a row's neighbours in the order given).  The -1 padding of short rows is dropped.  ``n_cols``
    defaults to the number of rows (a self-search); pass the number of candidates for a query search."""
    import scipy.sparse as sp
    indices = np.asarray(indices)
    distances = np.asarray(distances)
    if indices.ndim != 2 or indices.shape != distances.shape:
        raise ValueError('dca_amd: knn_graph: indices and distances are [n, k] arrays of one shape')
    n = indices.shape[0]
    n_cols = n if n_cols is None else int(n_cols)
    keep = indices >= 0
    if keep.any() and int(indices.max()) >= n_cols:
        raise ValueError('dca_amd: knn_graph: index %d is outside %d columns' % (int(indices.max()), n_cols))
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return sp.csr_matrix((distances[keep].astype(np.float32), indices[keep].astype(np.int32), indptr), shape=(n, n_cols))
