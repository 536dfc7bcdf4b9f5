"""Groups of cells compared on the denoised expression (beyond the reference, which leaves it to scanpy on the host after
``dca()``): per-group mean and variance, Welch's t against the rest or against one reference group, Benjamini-Hochberg
adjusted p-values and log fold changes.

The only pass over cells x genes runs on the device (Engine.group_moments -> dcahip_group_moments: per group the sums of
x and x^2 of every gene, in double); everything here is host arithmetic on [groups, genes] float64 arrays.
``method='wilcoxon'`` replaces Welch's t by the Wilcoxon rank-sum test, the test scanpy's tutorials recommend for this
step: Engine.rank_sums -> dcahip_ranksum sorts every gene on the device and returns exact integer rank sums and tie terms,
wilcoxon_from_ranks turns them into z scores and p-values here.
``Autoencoder.group_stats`` is the public entry; ``rank_genes_groups`` re-lays its result the way scanpy's function of
that name leaves its own.
"""
import numpy as np
import pandas as pd

MAX_GROUPS = 4096            # include/dcahip.h, dcahip_group_moments
VALUES = ('denoised', 'normalized')
METHODS = ('t-test', 'wilcoxon')
MAX_RANK_CELLS = 2097151     # include/dcahip.h, dcahip_ranksum: t^3 of a run of that many equal values fits 63 bits


def check_ranksum_args(g, n, m=0, K=1, ref=-1):
    """The limits of dcahip_ranksum (include/dcahip.h) as ValueErrors that name them."""
    if g < 1 or n < 1:
        raise ValueError('dca_amd: ranksum: %d genes of %d cells (at least one of each)' % (g, n))
    if n > MAX_RANK_CELLS:
        raise ValueError('dca_amd: ranksum: %d cells (at most %d)' % (n, MAX_RANK_CELLS))
    if not 0 <= m <= n:
        raise ValueError('dca_amd: ranksum: %d labelled cells of %d' % (m, n))
    if not 1 <= K <= MAX_GROUPS:
        raise ValueError('dca_amd: ranksum: %d groups (1 .. %d)' % (K, MAX_GROUPS))
    if not -1 <= ref < K:
        raise ValueError('dca_amd: ranksum: the reference group %d is not one of 0 .. %d (or -1: the rest)' % (ref, K - 1))


def label_codes(labels, groups=None, reference='rest'):
    """(names, codes): the sorted distinct labels and, per cell, the index of its label in names as int32 -- -1 for a
    NaN / None label and, with `groups`, for every label not listed (a named `reference` group always stays)."""
    lab = pd.Series(np.asarray(labels, dtype=object) if not isinstance(labels, (pd.Series, pd.Categorical)) else labels)
    lab = lab.astype(object).reset_index(drop=True)
    present = lab[lab.notna()]
    try:
        names = sorted(set(present.tolist()))
    except TypeError:
        raise ValueError('dca_amd: group_stats: the labels mix types that cannot be ordered (%s)'
                         % ', '.join(sorted({type(v).__name__ for v in present.tolist()}))) from None
    if groups is not None:
        keep = list(groups) + ([] if reference == 'rest' else [reference])
        unknown = [g for g in keep if g not in names]
        if unknown:
            raise ValueError('dca_amd: group_stats: no cell carries the label %r' % (unknown[0],))
        names = [g for g in names if g in keep]
    elif reference != 'rest' and reference not in names:
        raise ValueError('dca_amd: group_stats: no cell carries the reference label %r' % (reference,))
    index = {g: i for i, g in enumerate(names)}
    codes = np.array([-1 if na else index.get(v, -1) for v, na in zip(lab.tolist(), lab.isna().tolist())], dtype=np.int32)
    return names, codes


def obs_labels(adata, groupby, what):
    """(labels, key): the labels `groupby` names -- a column of adata.obs (key: its name) or an array of one label per cell
    (key: None)."""
    if isinstance(groupby, str):
        if groupby not in adata.obs.columns:
            raise ValueError('dca_amd: %s: adata.obs has no column %r' % (what, groupby))
        return adata.obs[groupby], groupby
    if np.ndim(groupby) != 1 or len(groupby) != adata.n_obs:
        raise ValueError('dca_amd: %s: %d labels for %d cells' % (what, np.size(groupby), adata.n_obs))
    return groupby, None


def moments_to_mean_var(s1, s2, n):
    """Mean and UNBIASED variance [K, G] from the sums of x and x^2 and the counts n [K]: (S2 - S1^2 / n) / (n - 1), clamped
    at 0; NaN for n < 2 (the mean: for n < 1)."""
    n = np.asarray(n, np.float64)[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(n >= 1, s1 / n, np.nan)
        var = np.where(n >= 2, np.maximum((s2 - s1 * s1 / n) / (n - 1.0), 0.0), np.nan)
    return mean, var


def welch_from_moments(m1, v1, n1, m2, v2, n2):
    """Welch's t and its two-sided p-value (Welch-Satterthwaite degrees of freedom) from means, unbiased variances and
    counts -- what scipy.stats.ttest_ind_from_stats(equal_var=False) computes.  A zero denominator gives t = 0, p = 1; a
    side with fewer than two cells gives NaN."""
    from scipy import stats
    n1 = np.broadcast_to(np.asarray(n1, np.float64).reshape(-1, 1), m1.shape)           # one count per group (row)
    n2 = np.broadcast_to(np.asarray(n2, np.float64).reshape(-1, 1), m1.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        vn1, vn2 = v1 / n1, v2 / n2
        den = np.sqrt(vn1 + vn2)
        t = (m1 - m2) / den
        df = (vn1 + vn2) ** 2 / (vn1 ** 2 / (n1 - 1.0) + vn2 ** 2 / (n2 - 1.0))
    zero = den == 0
    t = np.where(zero, 0.0, t)
    p = np.full(t.shape, np.nan)
    ok = np.isfinite(t) & np.isfinite(df) & ~zero
    p[ok] = 2.0 * stats.t.sf(np.abs(t[ok]), df[ok])
    p[zero] = 1.0
    return t, p


def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values of one vector; NaN entries stay NaN and do not count as tests."""
    p = np.asarray(p, np.float64)
    out = np.full(p.shape, np.nan)
    ok = np.flatnonzero(np.isfinite(p))
    m = len(ok)
    if m:
        order = ok[np.argsort(p[ok], kind='stable')]
        adj = p[order] * m / np.arange(1, m + 1)
        out[order] = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    return out


def wilcoxon_from_ranks(rank2, tie, counts, reference=None, tie_correct=False):
    """The Wilcoxon rank-sum test of every group [K, G] from the integers of dcahip_ranksum (Engine.rank_sums): dict with
    scores (z), pvals (two-sided, normal approximation, no continuity correction, as scanpy's 'wilcoxon'), pvals_adj
    (Benjamini-Hochberg per group), auroc = U / (n_c n_other) and U itself.

    reference None: rank2 / 2 is the rank sum R of group c among all N = sum(counts) cells: z = (R - n_c (N + 1) / 2) /
    sigma, sigma^2 = n_c (N - n_c) (N + 1) / 12, U = R - n_c (n_c + 1) / 2.  reference r: rank2 / 2 is U of c against r, N =
    n_c + n_r: z = (U - n_c n_r / 2) / sigma, sigma^2 = n_c n_r (N + 1) / 12.  tie_correct multiplies sigma^2 by
    1 - tie / (N^3 - N).  sigma = 0 gives z = 0, p = 1; an empty side, the reference's own row and a gene marked -1 (a NaN
    among its cells) give NaN."""
    from scipy import stats
    r2, tie = np.asarray(rank2, np.int64), np.asarray(tie, np.int64)
    n = np.asarray(counts, np.float64).reshape(-1, 1)
    half = r2.astype(np.float64) / 2.0                                  # rank2 < 2^44: exact
    if reference is None:
        N = np.full_like(n, n.sum())
        no = N - n
        U = half - n * (n + 1.0) / 2.0
    else:
        no = np.full_like(n, n[reference, 0])
        N = n + no
        U = half
    with np.errstate(divide='ignore', invalid='ignore'):
        var = n * no * (N + 1.0) / 12.0
        if tie_correct:
            var = var * (1.0 - tie.astype(np.float64) / (N ** 3 - N))
        var = np.broadcast_to(var, r2.shape)
        sigma = np.sqrt(np.maximum(var, 0.0))
        z = (U - n * no / 2.0) / sigma
        auroc = U / (n * no)
    zero = sigma == 0
    z = np.where(zero, 0.0, z)
    p = np.where(zero, 1.0, 2.0 * stats.norm.sf(np.abs(z)))
    bad = np.broadcast_to((n < 1) | (no < 1), r2.shape) | (r2 < 0)
    if reference is not None:
        bad = bad.copy()
        bad[reference] = True
    z, p, auroc, U = (np.where(bad, np.nan, a) for a in (z, p, auroc, np.broadcast_to(U, r2.shape)))
    return {'scores': z, 'pvals': p, 'pvals_adj': np.stack([benjamini_hochberg(row) for row in p]) if len(p) else p.copy(),
            'auroc': auroc, 'U': U}


def stats_from_moments(s1, s2, n, log1p=False, reference=None):
    """The statistics of every group [K, G] from the group moments: dict with mean, var, scores, pvals, pvals_adj,
    logfoldchanges.  reference: None = every group against all other cells of the K groups together (their moments are the
    totals minus the group's), or the index of the one group every other group is compared with (its own row: NaN)."""
    s1, s2, n = np.asarray(s1, np.float64), np.asarray(s2, np.float64), np.asarray(n, np.float64)
    mean, var = moments_to_mean_var(s1, s2, n)
    if reference is None:
        nr = n.sum() - n
        mr, vr = moments_to_mean_var(s1.sum(axis=0)[None] - s1, s2.sum(axis=0)[None] - s2, nr)
    else:
        nr = np.full_like(n, n[reference])
        mr, vr = np.broadcast_to(mean[reference], mean.shape), np.broadcast_to(var[reference], var.shape)
    t, p = welch_from_moments(mean, var, n, mr, vr, nr)
    back = np.expm1 if log1p else (lambda a: a)
    with np.errstate(divide='ignore', invalid='ignore'):
        lfc = np.log2((back(mean) + 1e-9) / (back(mr) + 1e-9))
    if reference is not None:
        t[reference], p[reference], lfc[reference] = np.nan, np.nan, np.nan
    return {'mean': mean, 'var': var, 'scores': t, 'pvals': p,
            'pvals_adj': np.stack([benjamini_hochberg(row) for row in p]) if len(p) else p.copy(), 'logfoldchanges': lfc}


def group_stats(net, adata, groupby, groups=None, value='denoised', log1p=False, reference='rest', copy=False,
                output_subset=None, method='t-test', tie_correct=False):
    """Autoencoder.group_stats (documented there)."""
    eng = net.engine
    if value not in VALUES:
        raise ValueError('dca_amd: group_stats: value must be one of %s (got %r)' % (', '.join(VALUES), value))
    if method not in METHODS:
        raise ValueError('dca_amd: group_stats: method must be one of %s (got %r)' % (', '.join(METHODS), method))
    if tie_correct and method != 'wilcoxon':
        raise ValueError("dca_amd: group_stats: tie_correct belongs to method='wilcoxon'")
    if method == 'wilcoxon' and not hasattr(eng.ops, 'ranksum'):
        raise NotImplementedError('dca_amd: group_stats: method=\'wilcoxon\' needs ops with ranksum (ops %s has none)'
                                  % eng.ops.name)
    if method == 'wilcoxon' and adata.n_obs > MAX_RANK_CELLS:
        raise ValueError("dca_amd: group_stats: method='wilcoxon' ranks at most %d cells (got %d)"
                         % (MAX_RANK_CELLS, adata.n_obs))
    if log1p and eng.flags & 8:
        raise ValueError("dca_amd: group_stats: log1p does not apply to ae_type='normal': its mean is linear and may be "
                         '<= -1')
    n = adata.n_obs
    labels, key = obs_labels(adata, groupby, 'group_stats')
    names, codes = label_codes(labels, groups, reference)
    if not names:
        raise ValueError('dca_amd: group_stats: no cell carries a label: there is no group')
    if len(names) > MAX_GROUPS:
        raise ValueError('dca_amd: group_stats: %d groups (at most %d)' % (len(names), MAX_GROUPS))
    G_out = eng.lay.G_out
    cols = None
    if output_subset:
        cols = [int(np.where(adata.var_names == x)[0][0]) for x in output_subset]
    if (len(cols) if cols is not None else adata.n_vars) != G_out:
        raise ValueError('dca_amd: group_stats: the network fits %d genes, the data has %d: name the fitted genes with '
                         'output_subset, in the order the network was trained with'
                         % (G_out, len(cols) if cols is not None else adata.n_vars))
    adata = adata.copy() if copy else adata
    net._bind_inputs(adata)
    chunk = net._chunk(n)
    res = eng.group_moments(codes, len(names), no_sf=(value == 'normalized'), log1p=log1p, chunk=chunk)
    counts = res['count'].cpu().numpy()
    ref = None if reference == 'rest' else names.index(reference)
    st = stats_from_moments(res['sum'].cpu().numpy(), res['sumsq'].cpu().numpy(), counts, log1p, ref)
    if method == 'wilcoxon':                            # mean, var and the fold change stay; the test is the rank-sum one
        rk = eng.rank_sums(codes, len(names), reference=ref, no_sf=(value == 'normalized'), log1p=log1p, chunk=chunk)
        wt = wilcoxon_from_ranks(rk['rank2'].cpu().numpy(), rk['tie'].cpu().numpy(), counts, ref, tie_correct)
        for k in ('scores', 'pvals', 'pvals_adj', 'auroc'):
            st[k] = wt[k]
    if len(names) < 2:                                  # one group: its moments alone; nothing to compare it with
        for k in ('scores', 'pvals', 'pvals_adj', 'logfoldchanges') + (('auroc',) if method == 'wilcoxon' else ()):
            st[k] = np.full_like(st['mean'], np.nan)
    if cols is not None:                                # genes the network does not fit: NaN
        for k, v in st.items():
            full = np.full((len(names), adata.n_vars), np.nan)
            full[:, cols] = v
            st[k] = full
    out = {'groupby': key, 'names': np.array(names, dtype=object), 'counts': counts.astype(np.int64), 'value': value,
           'log1p': bool(log1p), 'reference': reference}
    out.update(st)
    if method == 'wilcoxon':
        out['method'], out['tie_correct'] = method, bool(tie_correct)
    adata.uns['dca_groups'] = out
    return adata if copy else None


def rank_genes_groups(adata, n_genes=100, key_added='rank_genes_groups'):
    """Re-lays ``adata.uns['dca_groups']`` (Autoencoder.group_stats) into the structure scanpy's
    ``tl.rank_genes_groups`` leaves in ``adata.uns[key_added]``: ``params`` plus ``names``, ``scores``, ``pvals``,
    ``pvals_adj`` and ``logfoldchanges`` as numpy record arrays with one field per group, n_genes rows, the genes of every
    group sorted by score descending (ties by gene index).  The genes a gene-subset network does not fit (no mean in any
    group) are left out; a group without statistics (a single cell: its scores are NaN) keeps its field, the fitted genes in
    index order with NaN entries.
    The group compared against (``reference`` other than 'rest') has no field, as in scanpy.  scanpy is not a dependency of
    this package and this layout is taken from its documentation, not verified against an installed scanpy: the tests
    check the structure only.  Returns the stored dict."""
    d = adata.uns['dca_groups']
    var_names = np.asarray(adata.var_names)
    groups = [(i, str(g)) for i, g in enumerate(d['names']) if d['reference'] == 'rest' or g != d['reference']]
    fitted = np.flatnonzero(np.isfinite(d['mean']).any(axis=0))
    rows = min(int(n_genes), len(fitted))
    order = {}
    for i, g in groups:
        o = fitted[np.argsort(-d['scores'][i, fitted], kind='stable')]         # NaN sorts last, in index order
        order[g] = o[:rows]
    out = {'params': {'groupby': d['groupby'], 'reference': d['reference'], 'method': d.get('method', 't-test'), 'use_raw': False,
                      'layer': None, 'corr_method': 'benjamini-hochberg'}}
    width = max([len(str(v)) for v in var_names] + [1])
    out['names'] = np.rec.fromarrays([var_names[order[g]].astype('U%d' % width) for _, g in groups],
                                     names=[g for _, g in groups]) if groups else np.recarray((0,), dtype=[])
    for key, dt in (('scores', np.float32), ('pvals', np.float64), ('pvals_adj', np.float64), ('logfoldchanges', np.float32)):
        out[key] = np.rec.fromarrays([d[key][i, order[g]].astype(dt) for i, g in groups],
                                     names=[g for _, g in groups]) if groups else np.recarray((0,), dtype=[])
    adata.uns[key_added] = out
    return out
