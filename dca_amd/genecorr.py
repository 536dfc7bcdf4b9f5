"""Gene-gene correlation of the denoised expression (one of the results the DCA paper shows: regulatory relationships that
dropout hides in the raw counts appear in the denoised matrix; the reference leaves it to numpy on the host after
``dca()``).

The only pass over cells x genes runs on the device (Engine.gene_gram -> dcahip_gram: the cross-products of the selected
genes' values, shifted by a constant near each gene's mean, in double); everything here is host arithmetic on [genes, genes]
float64 arrays.  ``Autoencoder.gene_correlation`` is the public entry; ``top_partners`` reads its result.
"""
import numpy as np

from .groups import VALUES, label_codes, obs_labels

MAX_GENES = 8192             # include/dcahip.h, dcahip_gram


def cov_from_moments(cross, dsum, n):
    """The unbiased covariance [g, g] in float64 from the shifted moments of n rows: cross = sum_r d d^T and dsum = sum_r d
    with d = x - shift (any constant shift): (cross - dsum dsum^T / n) / (n - 1); NaN everywhere for n < 2."""
    cross, dsum = np.asarray(cross, np.float64), np.asarray(dsum, np.float64)
    g = dsum.shape[0]
    if dsum.ndim != 1 or cross.shape != (g, g):
        raise ValueError('dca_amd: cov_from_moments: cross is %s, dsum %s' % (cross.shape, dsum.shape))
    if n < 2:
        return np.full((g, g), np.nan)
    return (cross - np.outer(dsum, dsum) / float(n)) / (n - 1.0)


def corr_from_moments(cross, dsum, n):
    """Pearson's r [g, g] in float64 from the shifted moments (cov_from_moments): r_ij = cov_ij / sqrt(cov_ii cov_jj),
    clipped to [-1, 1], the diagonal exactly 1.  A gene with cov_ii <= 0 (constant) has a NaN row and column, its own
    diagonal entry included -- np.corrcoef's convention; n < 2 gives NaN everywhere."""
    cov = cov_from_moments(cross, dsum, n)
    var = np.diagonal(cov)
    ok = var > 0                                                    # False for NaN
    sd = np.sqrt(np.where(ok, var, np.nan))
    with np.errstate(invalid='ignore'):
        corr = np.clip(cov / np.outer(sd, sd), -1.0, 1.0)           # NaN stays NaN
    corr[np.flatnonzero(ok), np.flatnonzero(ok)] = 1.0
    return corr


def gene_correlation(net, adata, genes=None, groupby=None, group=None, value='denoised', log1p=False,
                     key_added='dca_gene_corr', copy=False, output_subset=None):
    """Autoencoder.gene_correlation (documented there)."""
    eng = net.engine
    if value not in VALUES:
        raise ValueError('dca_amd: gene_correlation: value must be one of %s (got %r)' % (', '.join(VALUES), value))
    if log1p and eng.flags & 8:
        raise ValueError("dca_amd: gene_correlation: log1p does not apply to ae_type='normal': its mean is linear and may "
                         'be <= -1')
    n = adata.n_obs
    G_out = eng.lay.G_out
    var_names = np.asarray(adata.var_names)
    fitted = None                                       # var index of every output column of the network
    if output_subset:
        fitted = [int(np.where(var_names == x)[0][0]) for x in output_subset]
    if (len(fitted) if fitted is not None else adata.n_vars) != G_out:
        raise ValueError('dca_amd: gene_correlation: the network fits %d genes, the data has %d: name the fitted genes '
                         'with output_subset, in the order the network was trained with'
                         % (G_out, len(fitted) if fitted is not None else adata.n_vars))
    fitted = np.arange(adata.n_vars) if fitted is None else np.asarray(fitted)
    if genes is None:
        names = var_names[fitted]
        cols = np.arange(G_out)
    else:
        names = np.asarray(list(genes), dtype=object)
        if names.ndim != 1 or not len(names):
            raise ValueError('dca_amd: gene_correlation: genes is a list of at least one gene name')
        column = {v: c for c, v in enumerate(var_names[fitted].tolist())}
        unknown = [x for x in names.tolist() if x not in column]
        if unknown:
            raise ValueError('dca_amd: gene_correlation: %r is not a gene the network fits (%d of the %d names are not)'
                             % (unknown[0], len(unknown), len(names)))
        if len(set(names.tolist())) != len(names):
            raise ValueError('dca_amd: gene_correlation: genes names a gene more than once')
        cols = np.array([column[x] for x in names.tolist()], dtype=np.int64)
    if len(cols) > MAX_GENES:
        raise ValueError('dca_amd: gene_correlation: %d genes (at most %d: name fewer with genes=)' % (len(cols), MAX_GENES))
    keep, key = None, None
    if groupby is None:
        if group is not None:
            raise ValueError('dca_amd: gene_correlation: group=%r needs groupby' % (group,))
    else:
        if group is None:
            raise ValueError('dca_amd: gene_correlation: groupby needs group, the one label whose cells take part')
        labels, key = obs_labels(adata, groupby, 'gene_correlation')
        try:
            _, codes = label_codes(labels, [group])
        except ValueError as e:
            raise ValueError(str(e).replace('group_stats', 'gene_correlation')) from None
        keep = codes == 0
    adata = adata.copy() if copy else adata
    net._bind_inputs(adata)
    res = eng.gene_gram(cols, keep=keep, no_sf=(value == 'normalized'), log1p=log1p, chunk=net._chunk(n))
    count = int(res['count'])
    dsum, shift = res['dsum'].cpu().numpy(), res['shift'].cpu().numpy()
    cross = res['cross'].cpu().numpy()
    corr = corr_from_moments(cross, dsum, count)
    var = np.maximum(np.diagonal(cov_from_moments(cross, dsum, count)), 0.0)             # NaN for fewer than two cells
    adata.uns[key_added] = {'genes': np.array(names.tolist(), dtype=object), 'corr': corr,
                            'mean': shift + dsum / count if count else np.full(len(cols), np.nan), 'var': var,
                            'n_cells': count, 'value': value, 'log1p': bool(log1p), 'groupby': key, 'group': group}
    return adata if copy else None


def top_partners(adata, gene, n=20, key='dca_gene_corr'):
    """The n genes most correlated with `gene` in ``adata.uns[key]`` (Autoencoder.gene_correlation): (names, r), sorted by
    |r| descending (ties by position), the gene itself and the genes without a correlation (NaN: constant) left out."""
    d = adata.uns[key]
    names = np.asarray(d['genes'], dtype=object)
    at = np.flatnonzero(names == gene)
    if not len(at):
        raise ValueError('dca_amd: top_partners: %r is not one of the %d genes of uns[%r]' % (gene, len(names), key))
    r = np.asarray(d['corr'])[at[0]]
    cand = np.flatnonzero(np.isfinite(r) & (np.arange(len(r)) != at[0]))
    order = cand[np.argsort(-np.abs(r[cand]), kind='stable')][:max(int(n), 0)]
    return names[order], r[order]
