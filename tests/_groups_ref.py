"""The fp64 reference of the group statistics (Engine.group_moments / Autoencoder.group_stats / dcahip_group_moments):
the element value from the fp32 operands, the moments of every group code by a plain loop, the statistics by scipy's
two-pass ttest_ind on the element matrix itself (not from moments).  GroupRefOps is the CPU oracle with the one entry it
lacks, so that the Python layers above the kernel run in the CPU suite."""
import numpy as np
from scipy import stats

from oracle.cpu_ops import CpuRefOps, _mat, _vec

MSE, NO_SF, LOG1P = 8, 16, 32


def elements(flags, a_mean, sf):
    """x [B, G] in fp64 from the fp32 pre-activations of the mean head and the fp32 size factors (include/dcahip.h,
    dcahip_group_moments): clip(exp(a), 1e-5, 1e6) (a itself with MSE), times sf without NO_SF, log1p with LOG1P."""
    a = np.asarray(a_mean, np.float32).astype(np.float64)
    x = a if flags & MSE else np.clip(np.exp(a), 1e-5, 1e6)
    if not flags & NO_SF:
        x = x * np.asarray(sf, np.float32).astype(np.float64)[:, None]
    return np.log1p(x) if flags & LOG1P else x


def moments(x, codes, K):
    """(S1 [K, G], S2 [K, G], n [K]) of the rows of x per code, by a plain loop; a code outside [0, K) leaves the row out."""
    x = np.asarray(x, np.float64)
    s1, s2, n = np.zeros((K, x.shape[1])), np.zeros((K, x.shape[1])), np.zeros(K, np.int64)
    for r, c in enumerate(np.asarray(codes).tolist()):
        if 0 <= c < K:
            s1[c] += x[r]
            s2[c] += x[r] * x[r]
            n[c] += 1
    return s1, s2, n


def abs_moments(x, codes, K):
    """(sum |x|, sum x^2) per code: what the error bars of the sums scale with."""
    s1, s2, _ = moments(np.abs(x), codes, K)
    return s1, s2


def two_pass_stats(x, codes, K, reference=None):
    """mean, unbiased variance, Welch t and two-sided p-value [K, G] straight from the element matrix:
    scipy.stats.ttest_ind(equal_var=False) of every group against the other rows with a code in [0, K) (reference None) or
    against the rows of group `reference`."""
    x, codes = np.asarray(x, np.float64), np.asarray(codes)
    inside = (codes >= 0) & (codes < K)
    out = {k: np.full((K, x.shape[1]), np.nan) for k in ('mean', 'var', 'scores', 'pvals')}
    for k in range(K):
        a = x[codes == k]
        b = x[inside & (codes != k)] if reference is None else x[codes == reference]
        if len(a):
            out['mean'][k] = a.mean(axis=0)
        if len(a) > 1:
            out['var'][k] = a.var(axis=0, ddof=1)
        if len(a) > 1 and len(b) > 1 and k != reference:
            t, p = stats.ttest_ind(a, b, axis=0, equal_var=False)
            out['scores'][k], out['pvals'][k] = t, p
    return out


def bh(p):
    """Benjamini-Hochberg, restated directly: adj_(i) = min over j >= i of p_(j) m / j, at most 1."""
    p = np.asarray(p, np.float64)
    m = len(p)
    order = np.argsort(p, kind='stable')
    out = np.empty(m)
    for rank, i in enumerate(order, 1):
        out[i] = min(min(p[j] * m / r for r, j in enumerate(order, 1) if r >= rank), 1.0)
    return out


class GroupRefOps(CpuRefOps):
    """CpuRefOps + group_moments (include/dcahip.h) in numpy fp64."""
    name = 'cpu-oracle-groups'

    def group_moments_workspace_doubles(self, B, G, K):
        return 1

    def group_moments(self, a_mean, lda, sf, codes, B, G, K, flags, sum_acc, sumsq_acc, ldg, ws):
        assert not (flags & MSE and flags & LOG1P) and 1 <= K <= 4096
        x = elements(flags, _mat(a_mean, B, G, lda), _vec(sf, B))
        s1, s2, _ = moments(x, _vec(codes, B), K)
        _mat(sum_acc, K, G, ldg)[:] += s1
        _mat(sumsq_acc, K, G, ldg)[:] += s2
