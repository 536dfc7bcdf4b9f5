"""The adversarial grid of the likelihood's inputs on which the range bound of the fp16 x 2 gradient planes is checked
(include/dcahip.h, dcahip_zinb_nll_planes_h2: |g| <= max(1e4, 2 y_max + 50) + ridge / 2, from which Engine._data_scales
takes d_exp).  Every combination of the edge values is one gene; the size factors are the rows."""
import itertools

import numpy as np

from oracle import zinb_np as Z

A_MEAN = (-120., -14., 0., 5., 8., 13.8, 15., 30., 95.)
A_DISP = (-100., -12., -3., 0., 9.21, 9.3, 20., 9500.)      # as theta_w: exp() spans the 1e-3 and the 1e4 clip
A_PI = (-30., -5., 0., 5., 30.)
Y = (0., 0.5, 1., 2.52, 254., 255., 5000., 8000.)
SF = (0.05, 1., 20.)
RIDGES = (0.0, 0.05, 1e3)


def grid(y_values=Y):
    """am, ad, ap, y [3, G], sf [3], tw [G] (fp32-representable float64), G = 9 x 8 x 5 x len(y_values)."""
    cols = np.array(list(itertools.product(A_MEAN, A_DISP, A_PI, y_values)), np.float32).astype(np.float64)
    B = len(SF)
    am, ad, ap, y = (np.ascontiguousarray(np.broadcast_to(cols[:, k], (B, cols.shape[0]))) for k in range(4))
    sf = np.array(SF, np.float32).astype(np.float64)
    return am, ad, ap, y, sf, cols[:, 1].copy()


def bound(y, ridge):
    return np.maximum(1e4, 2.0 * y + 50.0) + 0.5 * ridge


def d_exp_of(y_max, ridge):
    """Engine._data_scales."""
    return int(np.floor(np.log2(65000.0 / (max(1e4, 2.0 * y_max + 50.0) + 0.5 * float(ridge)))))


def oracle_grads(flags, am, ad, ap, y, sf, tw, ridge, n_total=1.0):
    """(loss_mean, {head: d loss / d pre-activation scaled by 1 / n_total}) of the heads that go to fp16 planes."""
    has_pi, cdisp = bool(flags & 1), bool(flags & 2)
    with np.errstate(all='ignore'):
        if has_pi:
            _, lm, dm, dd, dp = Z.zinb_loss_and_grads(am, None if cdisp else ad, ap, y, sf, ridge, n_total,
                                                      theta_w=tw if cdisp else None)
        else:
            _, lm, dm, dd = Z.nb_loss_and_grads(am, None if cdisp else ad, y, sf, n_total, theta_w=tw if cdisp else None)
            dp = None
    out = {'mean': dm}
    if not cdisp:
        out['disp'] = dd
    if has_pi:
        out['pi'] = dp
    return lm, out


def worst_bound_ratio(flags, ridge, y_values=Y):
    """max |g| / bound(y, ridge) of the fp64 oracle over the grid, element-wise in y; asserts every gradient finite."""
    am, ad, ap, y, sf, tw = grid(y_values)
    _, g = oracle_grads(flags, am, ad, ap, y, sf, tw, ridge)
    worst = 0.0
    for name, v in g.items():
        assert np.isfinite(v).all(), (flags, ridge, name)
        worst = max(worst, float((np.abs(v) / bound(y, ridge)).max()))
    return worst
