"""The fp64 reference of the scoring pass (Engine.score / Autoencoder.score / dcahip_nll_marginals): the element-wise NLL
of a fitted model from the oracle -- OracleAE.predict (mean * sf, theta, pi) into oracle.zinb_np.zinb_nll / nb_nll /
poisson_nll, (mean - y)^2 for 'normal' -- and its row and column sums.  ScoreRefOps is the CPU oracle with the one entry
it lacks, so that the Python layers above the kernel run in the CPU suite."""
import numpy as np

from oracle import zinb_np as Z
from oracle.cpu_ops import CpuRefOps, _mat, _vec

TOTAL_RTOL = 1e-5            # the bar of every single-step loss test
RTOL, ATOL_SCALE = 2e-5, 2e-5  # per value: rtol |ref| + atol_scale max|ref| (helpers.assert_grads_close's atol_scale)


def elements(flags, mu, theta, pi, y, ridge):
    """Element-wise NLL [n, G] (fp64) from the head activations; flags as dcahip_zinb_nll (1 pi, 2 const. dispersion,
    4 Poisson, 8 squared error).  mu = mean * sf; theta [n, G], [n, 1] or [G]."""
    mu, y = np.asarray(mu, np.float64), np.asarray(y, np.float64)
    if flags & 8:
        return np.square(mu - y)
    if flags & 4:
        return Z.poisson_nll(y, mu)
    theta = np.broadcast_to(np.asarray(theta, np.float64), mu.shape)
    if flags & 1:
        return Z.zinb_nll(y, mu, theta, np.broadcast_to(np.asarray(pi, np.float64), mu.shape), ridge)
    return Z.nb_nll(y, mu, theta)


def kernel_elements(flags, am, ad, ap, tw, y, sf, ridge, dtype=np.float64):
    """The same from head PRE-activations (the kernel's operands), evaluated in `dtype`."""
    c = lambda a: None if a is None else np.asarray(a, dtype)
    am, ad, ap, tw, y, sf = c(am), c(ad), c(ap), c(tw), c(y), c(sf)
    if flags & 8:
        return np.square(am * sf[:, None] - y)
    mu, theta, pi = Z.heads_forward(am, None if flags & 2 else ad, ap if flags & 1 else None, sf)
    if flags & 4:
        return Z.poisson_nll(y, mu)
    if flags & 2:
        theta = np.broadcast_to(Z.const_disp(tw).reshape(1, -1), mu.shape)
    if flags & 1:
        return Z.zinb_nll(y, mu, theta, pi, dtype(ridge))
    return Z.nb_nll(y, mu, theta)


AE_FLAGS = {'normal': 8, 'poisson': 4, 'nb': 2, 'nb-conddisp': 0, 'nb-shared': 0, 'nb-fork': 0, 'zinb': 3,
            'zinb-conddisp': 1, 'zinb-shared': 1, 'zinb-fork': 1, 'zinb-elempi': 1}


def oracle_score(net, X, Y, sf):
    """(cell [n], gene [G]) sums of the element-wise NLL of the fp64 oracle network `net` (OracleAE) on these cells."""
    out = net.predict(np.asarray(X, np.float64), np.asarray(sf, np.float64))
    el = elements(AE_FLAGS[net.ae_type], out['mean'], out['dispersion'], out['dropout'], Y, net.ridge)
    return el.sum(axis=1), el.sum(axis=0)


def assert_marginals_close(cell, gene, cell_ref, gene_ref, what='', total_rtol=TOTAL_RTOL):
    cell, gene = np.asarray(cell, np.float64), np.asarray(gene, np.float64)
    tot = cell_ref.sum()
    print('%s total rel %.2e / %.2e' % (what, abs(cell.sum() / tot - 1), abs(gene.sum() / tot - 1)))
    for name, got, ref in (('cell', cell, cell_ref), ('gene', gene, gene_ref)):
        tol = RTOL * np.abs(ref) + ATOL_SCALE * np.abs(ref).max()
        err = np.abs(got - ref)
        print('%s %s worst error / tolerance %.3f' % (what, name, float((err / tol).max())))
        assert (err <= tol).all(), (what, name, float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())
    assert abs(cell.sum() - tot) <= total_rtol * abs(tot), (what, cell.sum(), tot)
    assert abs(gene.sum() - tot) <= total_rtol * abs(tot), (what, gene.sum(), tot)


class ScoreRefOps(CpuRefOps):
    """CpuRefOps + nll_marginals (include/dcahip.h) in numpy fp64 from the oracle's likelihood functions."""
    name = 'cpu-oracle-score'

    def nll_marginals_workspace_doubles(self, B, G):
        return 1

    def nll_marginals(self, a_mean, a_disp, a_pi, lda, theta_w, Y, ldy, sf, B, G, ridge, flags, cell_out, gene_acc, ws):
        el = kernel_elements(flags, _mat(a_mean, B, G, lda), _mat(a_disp, B, G, lda), _mat(a_pi, B, G, lda),
                             _vec(theta_w, G), _mat(Y, B, G, ldy), _vec(sf, B), ridge)
        _vec(cell_out, B)[:] = el.sum(axis=1)
        _vec(gene_acc, G)[:] += el.sum(axis=0)
