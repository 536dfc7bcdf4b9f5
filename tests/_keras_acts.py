"""hard_sigmoid, exponential, swish and gelu (keras.activations of TF 2.4, the names Activation(self.activation) accepts,
dca/network.py:132-135) in fp64, and the test oracles extended with them.

    hard_sigmoid  clip(0.2 x + 0.5, 0, 1)          slope 0.2 inside the clip, 0 outside
    exponential   exp(x)                            slope exp(x) = h
    swish         x s(x), s = sigmoid               slope s(x) (1 + x (1 - s(x)))
    gelu          0.5 x (1 + erf(x / sqrt 2))       slope Phi(x) + x phi(x)   (Keras' default approximate=False)

swish and gelu are not monotonic (minima near x = -1.28 and x = -0.75): their slope is a function of the pre-activation,
not of the output -- the kernels read xhat + beta (batch norm) or Z (include/dcahip.h, conventions)."""
import numpy as np
from scipy.special import erf, expit

from oracle import net_np as N
from oracle.cpu_ops import CpuRefOps, _chunks, _mat, _vec

NEW = {'hard_sigmoid': 10, 'exponential': 11, 'swish': 12, 'gelu': 13}
PRE = 12                      # codes from here up: slope from the pre-activation


def fwd(code, x):
    if code == 10:
        return np.clip(0.2 * x + 0.5, 0.0, 1.0)
    if code == 11:
        return np.exp(x)
    if code == 12:
        return x * expit(x)
    if code == 13:
        return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
    raise ValueError(code)


def grad(code, x):
    """d act / dx at the pre-activation x."""
    if code == 10:
        return np.where((x > -2.5) & (x < 2.5), 0.2, 0.0)
    if code == 11:
        return np.exp(x)
    if code == 12:
        s = expit(x)
        return s * (1.0 + x * (1.0 - s))
    if code == 13:
        return 0.5 * (1.0 + erf(x / np.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)
    raise ValueError(code)


def grad_from_out(code, h):
    """The slope through the output h: defined for the monotonic codes 10 and 11 only."""
    if code == 10:
        return np.where((h > 0.0) & (h < 1.0), 0.2, 0.0)
    if code == 11:
        return h
    raise ValueError('code %d: the slope is not a function of the output' % code)


def _bisect(f, lo, hi, it=80):
    lo, hi = np.broadcast_arrays(np.asarray(lo, np.float64), np.asarray(hi, np.float64))
    lo, hi = lo.copy(), hi.copy()
    for _ in range(it):
        mid = 0.5 * (lo + hi)
        up = f(mid) > 0
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    return 0.5 * (lo + hi)


def minimum(code):
    """x of the minimum of swish / gelu (slope 0)."""
    return float(_bisect(lambda x: grad(code, x), -3.0, 0.0))


def slope_from_out_upper_branch(code, h):
    """The slope a backward that reads only h would produce for swish / gelu: h inverted on the increasing branch
    x >= minimum(code), the slope taken there.  Wrong for every element whose pre-activation lies below the minimum."""
    xm = minimum(code)
    h = np.maximum(h, fwd(code, xm))
    x = _bisect(lambda x: fwd(code, x) - h, np.full_like(h, xm), np.abs(h) + 2.0)
    return grad(code, x)


def extend_oracle(monkeypatch):
    """oracle.net_np with the four names: its backward works from the pre-activation (act_grad)."""
    codes = dict(N.ACT_CODES)
    codes.update(NEW)
    f0, g0, o0 = N.act_fwd, N.act_grad, N.act_grad_from_out
    monkeypatch.setattr(N, 'ACT_CODES', codes)
    monkeypatch.setattr(N, 'act_fwd', lambda c, x: fwd(c, x) if c in NEW.values() else f0(c, x))
    monkeypatch.setattr(N, 'act_grad', lambda c, x: grad(c, x) if c in NEW.values() else g0(c, x))
    monkeypatch.setattr(N, 'act_grad_from_out', lambda c, h: grad_from_out(c, h) if c in NEW.values() else o0(c, h))


class KerasActOps(CpuRefOps):
    """The CPU oracle with the pre-activation operands of codes 12 and 13 (include/dcahip.h, conventions): the `beta`
    argument of the batch-norm backward (pre-activation xhat + beta) and, without batch norm, Z in the Hact slot.
    Needs extend_oracle for the forward and for codes 10, 11."""

    def _dy(self, dH, ldd, Hact, ldh, xhat, ldx, B, H, act, beta):
        d = _mat(dH, B, H, ldd).astype(np.float64)
        if act >= PRE:
            assert beta is not None, 'codes 12, 13 need the pre-activation offset beta'
            x = _mat(xhat, B, H, ldx).astype(np.float64) + _vec(beta, H).astype(np.float64)
            return d * grad(act, x)
        assert beta is None
        return d * N.act_grad_from_out(act, _mat(Hact, B, H, ldh).astype(np.float64))

    def bn_bwd_sums(self, dH, ldd, Hact, ldh, xhat, ldx, B, H, part, act=1, beta=None):
        R = _chunks(B)
        cr = -(-B // R)
        dy = self._dy(dH, ldd, Hact, ldh, xhat, ldx, B, H, act, beta)
        xh = _mat(xhat, B, H, ldx).astype(np.float64)
        p = _vec(part, R * 2 * H).reshape(R, 2, H)
        for r in range(R):
            s = slice(r * cr, min(B, (r + 1) * cr))
            p[r, 0] = dy[s].sum(0)
            p[r, 1] = (dy[s] * xh[s]).sum(0)

    def bn_bwd_apply(self, dH, ldd, Hact, ldh, xhat, ldx, inv_std, sums, E, n_total, B, H, dZ, ldz,
                     dbeta, act=1, beta=None):
        s = _vec(sums, E * 2 * H).reshape(E, 2, H).astype(np.float64).sum(0)
        dy = self._dy(dH, ldd, Hact, ldh, xhat, ldx, B, H, act, beta)
        xh = _mat(xhat, B, H, ldx).astype(np.float64)
        inv = _vec(inv_std, H).astype(np.float64)
        _mat(dZ, B, H, ldz)[:] = inv * (dy - s[0] / n_total - xh * s[1] / n_total)
        if dbeta is not None:
            _vec(dbeta, H)[:] = s[0]

    def relu_bwd(self, dH, ldd, Hact, ldh, B, H, dZ, ldz, act=1):
        v = _mat(Hact, B, H, ldh).astype(np.float64)          # codes 12, 13: the pre-activation Z
        slope = grad(act, v) if act >= PRE else N.act_grad_from_out(act, v)
        _mat(dZ, B, H, ldz)[:] = _mat(dH, B, H, ldd).astype(np.float64) * slope


def shift_biases(p, hs, batchnorm, by=-0.8):
    """Moves the pre-activations of every hidden layer down (beta with batch norm, the Dense bias without) so that a
    share of them lies below swish's and gelu's minimum, where the slope differs from the one on the increasing branch
    with the same output."""
    p = dict(p)
    for i in range(len(hs)):
        k = ('beta%d' if batchnorm else 'b%d') % i
        if k in p:
            p[k] = (p[k] + np.float32(by)).astype(p[k].dtype)
    return p
