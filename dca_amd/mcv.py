"""Molecular cross-validation (Batson et al. 2019; count splitting, Neufeld et al. 2022) -- beyond the reference.

``val_loss``, ``net.score()`` on held-out cells and the ``--hyper`` objective all reconstruct a cell from its own noisy
counts, so an autoencoder that moves towards the identity lowers all of them.  Here every count is thinned binomially into
two independent parts, the model is fitted on one and scored on the molecules of the other.  Under the NB / ZINB model
thinning keeps theta and pi and scales the mean, so the held-out part is scored by the likelihood the engine already
computes (Autoencoder.score), with the fit part's size factors multiplied by (1 - f) / f.

The draw (include/dcahip.h, dcahip_csr_thin -- K-SPLIT): of the count y of cell i, gene j,

    a(i, j) = #{ t in [0, y) : word (t & 3) of philox4x32_10((i, j, t >> 2, THIN_TAG), key = seed) < threshold }

molecules go to the fit part and y - a to the held-out part: Binomial(y, threshold / 2^32) in integer arithmetic, a function
of (seed, i, j, y, threshold) only.  ``thin_counts_host`` is its numpy restatement, bit for bit the kernel's result, and the
path taken without a GPU.
"""
import numpy as np
import scipy.sparse as sp_sparse

THIN_TAG = 0x7468696E           # Philox counter word 3 of K-SPLIT; K-DROP puts its layer code (0 .. 255) there
MAX_COUNT = 1 << 24             # fp32 holds every integer up to it
_ONE_BY_ONE = 256               # counts above it are drawn one entry at a time, vectorised over their molecules

_M32 = np.uint64(0xffffffff)
_SH = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable uint32-valued arrays: the four output words as uint32 arrays.
    The generator of dca_amd/csrc/philox.hpp; tests/test_mcv_cpu.py pins it on the oracle's, which is pinned on the
    Random123 known-answer vectors."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(int(k0) & 0xffffffff), np.uint64(int(k1) & 0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ k0, p1 & _M32, (p0 >> _SH) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def threshold_of(fraction):
    """The integer threshold of a fraction f in (0, 1): int(f 2^32)."""
    f = float(fraction)
    if not 0.0 < f < 1.0:
        raise ValueError('dca_amd.mcv: fraction must lie strictly between 0 and 1 (got %r)' % (fraction,))
    return int(f * 4294967296.0)


def thin_counts_host(indptr, indices, values, row_ids, threshold, seed):
    """The numpy restatement of dcahip_csr_thin: the CSR (indptr [n + 1], indices, values; integer counts up to 2^24)
    thinned into (indptr_a, indices_a, values_a, indptr_b, indices_b, values_b) -- int64 / int32 / float32, rows and columns in
    the source order, A + B = the source, no stored zero in either part.  row_ids: the global cell id of every row (None: row r
    is cell r).  A negative, fractional or too large value raises ValueError."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices)
    n = len(indptr) - 1
    threshold = int(threshold)
    if not 0 <= threshold <= 1 << 32:
        raise ValueError('dca_amd.mcv: threshold must lie in [0, 2^32] (got %d)' % threshold)
    s, e = int(indptr[0]), int(indptr[-1])
    if n < 0 or s != 0 or e > len(indices) or (np.diff(indptr) < 0).any():
        raise ValueError('dca_amd.mcv: malformed CSR: indptr is not a non-decreasing row pointer from 0')
    v = np.asarray(values)[:e].astype(np.float32)
    bad = ~((v >= 0) & (v == np.floor(v)) & (v <= MAX_COUNT))
    if bad.any():
        raise ValueError('dca_amd.mcv: %d values are not counts (negative, not an integer or above 2^24)' % int(bad.sum()))
    y = v.astype(np.int64)
    j = indices[:e].astype(np.int64)
    per_row = np.diff(indptr)
    row = np.repeat(np.arange(n, dtype=np.int64), per_row)
    ids = np.arange(n, dtype=np.int64) if row_ids is None else np.asarray(row_ids, dtype=np.int64).reshape(-1)[:n]
    i = np.repeat(ids, per_row)
    seed = int(seed) & 0xffffffffffffffff
    k0, k1 = seed & 0xffffffff, seed >> 32
    thr = np.uint64(threshold)
    a = np.zeros(e, dtype=np.int64)
    # counts up to _ONE_BY_ONE: all entries that still have molecules left, one Philox block (four molecules) per pass
    sel = np.nonzero((y > 0) & (y <= _ONE_BY_ONE))[0]
    blk = 0
    while len(sel):
        words = philox4x32_10(i[sel], j[sel], blk, THIN_TAG, k0, k1)
        left = y[sel] - 4 * blk
        for w in range(4):
            a[sel] += (left > w) & (words[w].astype(np.uint64) < thr)
        blk += 1
        sel = sel[left > 4]
    # larger counts: one entry at a time, all of its blocks at once
    for q in np.nonzero(y > _ONE_BY_ONE)[0]:
        blocks = np.arange((int(y[q]) + 3) // 4, dtype=np.int64)
        words = np.stack(philox4x32_10(int(i[q]), int(j[q]), blocks, THIN_TAG, k0, k1), axis=1).reshape(-1)
        a[q] = int((words[:int(y[q])].astype(np.uint64) < thr).sum())
    out = []
    for part in (a, y - a):
        keep = part > 0
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(row[keep], minlength=n), out=ptr[1:])
        out += [ptr, j[keep].astype(np.int32), part[keep].astype(np.float32)]
    return tuple(out)


def _host_csr(X):
    """The canonical float32 CSR of a host matrix, as prep.upload_csr hands it to the device."""
    if not sp_sparse.issparse(X):
        X = sp_sparse.csr_matrix(np.asarray(X))
    elif X.format != 'csr':
        X = X.tocsr()
    if not X.has_canonical_format:
        X = X.copy()
        X.sum_duplicates()
    return X


def _device_ops(device):
    """HipOps when the split runs on the GPU (device=True, or 'auto' with a GPU and device preprocessing on), else None."""
    from . import io as _io
    if device is True or (device == 'auto' and _io._device_prep_available()):
        from .ops import HipOps
        ops = HipOps()
        if hasattr(ops, 'csr_thin'):
            return ops
    return None


def split_counts(adata, fraction=0.5, seed=0, device='auto'):
    """(fit, held): two AnnData objects with the obs / var of ``adata`` whose ``.X`` are the two parts of its counts -- of every
    count y, a ~ Binomial(y, fraction) molecules in ``fit`` and y - a in ``held``, independent of each other; scipy CSR
    (float32) for a sparse ``.X``, a dense array for a dense one.  Cell i is row i of ``adata``.  With a GPU the counts are
    uploaded as CSR and thinned there (dcahip_csr_thin); the host path (``device=False``, no GPU) gives the same bits.  The
    draw is a function of ``seed``: numpy's global stream is not touched.  Values that are not counts raise ValueError."""
    from ._anndata import AnnData
    threshold = threshold_of(fraction)
    X = adata.X
    n, G = X.shape
    ops = _device_ops(device)
    if ops is not None and n > 0 and G > 0:
        import torch
        from . import prep
        dev = torch.device('cuda', torch.cuda.current_device())
        A, B = ops.csr_thin(prep.upload_csr(X, dev, ops), None, threshold, seed)
        arrays = [t.cpu().numpy() for part in (A, B) for t in (part.indptr, part.indices, part.values)]
    else:
        C = _host_csr(X)
        arrays = thin_counts_host(C.indptr, C.indices, C.data, None, threshold, seed)
    parts = []
    for ptr, idx, val in (arrays[:3], arrays[3:]):
        P = sp_sparse.csr_matrix((val, idx, ptr), shape=(n, G))
        if not sp_sparse.issparse(X):
            P = P.toarray()
        parts.append(AnnData(P, obs=adata.obs.copy(), var=adata.var.copy()))
    return parts[0], parts[1]


def drop_empty(fit, held):
    """Drops the genes and then the cells whose FIT part holds no molecule from both parts (in place): they carry nothing to
    fit on.  Returns (genes dropped, cells dropped)."""
    from . import io as _io
    genes = np.asarray(fit.X.sum(axis=0)).reshape(-1) > 0
    if not genes.all():
        _io._subset(fit, cols=genes)
        _io._subset(held, cols=genes)
    cells = np.asarray(fit.X.sum(axis=1)).reshape(-1) > 0
    if not cells.all():
        _io._subset(fit, rows=cells)
        _io._subset(held, rows=cells)
    return int((~genes).sum()), int((~cells).sum())


def evaluation_set(fit, held, fraction):
    """What Autoencoder.score takes to evaluate the held-out molecules: ``.X`` the normalised fit input, ``.raw`` the held-out
    counts, ``obs['size_factors']`` the fit part's size factors x (1 - f) / f (thinning scales the mean and nothing else)."""
    from ._anndata import AnnData
    import pandas as pd
    f = float(fraction)
    ev = AnnData(fit.X, obs=pd.DataFrame(index=fit.obs_names), var=pd.DataFrame(index=fit.var_names))
    ev.raw = held
    ev.obs['size_factors'] = np.asarray(fit.obs['size_factors'].values, dtype=np.float64) * ((1.0 - f) / f)
    return ev


_DCA_ARGS = ('ae_type', 'normalize_per_cell', 'scale', 'log1p', 'hidden_size', 'hidden_dropout', 'batchnorm', 'activation',
             'init', 'network_kwds', 'epochs', 'reduce_lr', 'early_stop', 'batch_size', 'optimizer', 'learning_rate',
             'random_state', 'threads', 'verbose', 'training_kwds', 'check_counts')


def mcv(adata, fraction=0.5, seed=0, return_model=False, **dca_kwargs):
    """Molecular cross-validation of one configuration: splits the counts of ``adata`` (split_counts(fraction, seed)), fits
    on the fit part as ``dca()`` does -- ``dca_kwargs`` are the arguments of ``api.dca`` that concern normalisation, network
    and training, with its defaults -- and scores the held-out part of EVERY cell (its molecules are independent of the
    fit for each of them).  Genes and cells whose fit part is empty are dropped from both parts first.  Returns a dict:
    ``mcv_loss`` (the mean held-out NLL per cell and gene: compare configurations by it), ``gene_nll``, ``cell_nll``,
    ``history``, ``fraction``, ``seed``, ``n_cells`` / ``n_genes`` (after the drop), ``genes_dropped`` / ``cells_dropped``,
    and ``model`` with ``return_model=True``.  ``adata`` is not modified."""
    import inspect
    from . import api
    from .io import read_dataset, normalize
    from .train import train
    unknown = set(dca_kwargs) - set(_DCA_ARGS)
    if unknown:
        raise TypeError('dca_amd.mcv: mcv() takes the normalisation, network and training arguments of dca() (%s); got %s'
                        % (', '.join(_DCA_ARGS), ', '.join(sorted(unknown))))
    sig = inspect.signature(api.dca).parameters
    kw = {k: dca_kwargs.get(k, sig[k].default) for k in _DCA_ARGS}
    threshold_of(fraction)
    api._seed_host_generators(kw['random_state'])
    work = read_dataset(adata, transpose=False, test_split=False, copy=True, check_counts=kw['check_counts'])
    fit, held = split_counts(work, fraction, seed)
    genes_dropped, cells_dropped = drop_empty(fit, held)
    if genes_dropped or cells_dropped:
        print('dca: mcv: dropped %d genes and %d cells whose fit part is empty' % (genes_dropped, cells_dropped))
    fit = normalize(fit, filter_min_counts=False, size_factors=kw['normalize_per_cell'], normalize_input=kw['scale'],
                    logtrans_input=kw['log1p'])
    net = api._make_network(kw['ae_type'], fit.n_vars, kw['random_state'],
                            dict(kw['network_kwds'], hidden_size=kw['hidden_size'], hidden_dropout=kw['hidden_dropout'],
                                 batchnorm=kw['batchnorm'], activation=kw['activation'], init=kw['init']))
    fit_kwds = dict(kw['training_kwds'], epochs=kw['epochs'], reduce_lr=kw['reduce_lr'], early_stop=kw['early_stop'],
                    batch_size=kw['batch_size'], optimizer=kw['optimizer'], verbose=kw['verbose'], threads=kw['threads'],
                    learning_rate=kw['learning_rate'])
    history = train(fit[fit.obs.dca_split == 'train'], net, **fit_kwds)
    ev = evaluation_set(fit, held, fraction)
    net.score(ev)
    out = {'mcv_loss': float(ev.uns['dca_nll']),
           'gene_nll': np.asarray(ev.var['dca_nll'].values, dtype=np.float64),
           'cell_nll': np.asarray(ev.obs['dca_nll'].values, dtype=np.float64),
           'gene_names': np.asarray(ev.var_names), 'cell_names': np.asarray(ev.obs_names),
           'history': history.history, 'fraction': float(fraction), 'seed': int(seed),
           'n_cells': int(ev.n_obs), 'n_genes': int(ev.n_vars),
           'genes_dropped': genes_dropped, 'cells_dropped': cells_dropped}
    if return_model:
        out['model'] = net
    return out


def write_mcv(res, output_dir):
    """``--mcv``: mcv.json (every scalar of the result), gene_mcv_nll.tsv and cell_mcv_nll.tsv (index = name; nll)."""
    import json
    import os
    import pandas as pd
    os.makedirs(output_dir, exist_ok=True)
    scalars = {k: v for k, v in res.items() if isinstance(v, (int, float, str)) and not isinstance(v, bool)}
    with open(os.path.join(output_dir, 'mcv.json'), 'wt') as f:
        json.dump(scalars, f, sort_keys=True, indent=4)
    for name, key, idx in (('gene_mcv_nll.tsv', 'gene_nll', 'gene_names'), ('cell_mcv_nll.tsv', 'cell_nll', 'cell_names')):
        pd.DataFrame({'nll': res[key]}, index=pd.Index(res[idx])).to_csv(os.path.join(output_dir, name), sep='\t',
                                                                           float_format='%.6f')
