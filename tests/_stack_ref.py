"""fp64 reference of the fused hidden stack (K-STACK, include/dcahip.h), numpy only, one STEP at a time.

Every layer is Dense -> BatchNormalization(center, no scale, eps 1e-3, momentum 0.99, biased variance) -> activation
(dca/network.py:124-135).  The steps are the ones of dcahip_hidden_stack_fwd / _bwd:

    forward   0       (mean, M2) of row ranges of the first layer's pre-activation
              1 + i   layer i: merge the (count, mean, M2) entries, normalise + activate, next layer's pre-activation
                      and ITS (mean, M2) over row ranges
    backward  0       dy = dH act'(x) of the last layer and (sum dy, sum dy xhat) over row ranges
              1 + j   layer i = n - 1 - j: dZ = inv (dy - S1 / n - xhat S2 / n), d beta, gW (bias gradient in row K),
                      dHprev, and the sums of the layer below over row ranges

The slope is ALWAYS taken at the pre-activation x = xhat + beta (the mathematical truth); the forms through the output
h that the kernels use for codes 0-11 are here only to be checked against it (tests/test_stack_ref_cpu.py).

Tolerances.  Beside every reduction or product X a step returns
    X_mag   sum |terms| of the expression that makes the element, expanded down to the step's inputs, and
    X_in    the first-order allowance for what enters the expression already rounded (see slope_tolerance and the
            `*_tol` arguments),
so that a caller judges |got - X| against rel * X_mag + X_in (error_and_bound)."""
import math

import numpy as np

BN_MOMENTUM = 0.99
BN_EPS = 1e-3
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772
CODES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13)
ACT_PRE = 12                  # codes from here up: the kernels, too, take the slope from the pre-activation
REL = 1e-6                    # |err| <= REL * sum |terms| (tests/test_sparse_gpu.py)

_erf = np.frompyfunc(math.erf, 1, 1)


def erf(x):
    return _erf(np.asarray(x, np.float64)).astype(np.float64)


def sigmoid(x):
    e = np.exp(-np.abs(x))
    s = 1.0 / (1.0 + e)
    return np.where(x >= 0, s, e * s)


def _phi(x):
    return np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _Phi(x):
    return 0.5 * (1.0 + erf(x / math.sqrt(2.0)))


# ------------------------------------------------------------------ activations
def act_fwd(code, x):
    x = np.asarray(x, np.float64)
    if code == 0: return x.copy()
    if code == 1: return np.maximum(x, 0.0)
    if code == 2: return np.tanh(x)
    if code == 3: return sigmoid(x)
    if code == 4: return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if code == 5: return SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))
    if code == 6: return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    if code == 7: return x / (1.0 + np.abs(x))
    if code == 8: return np.where(x > 0, x, 0.3 * x)
    if code == 10: return np.clip(0.2 * x + 0.5, 0.0, 1.0)
    if code == 11: return np.exp(x)
    if code == 12: return x * sigmoid(x)
    if code == 13: return x * _Phi(x)
    raise ValueError(code)


def act_slope(code, x):
    """d act / dx at the pre-activation x."""
    x = np.asarray(x, np.float64)
    if code == 0: return np.ones_like(x)
    if code == 1: return (x > 0).astype(np.float64)
    if code == 2: return 1.0 / np.cosh(x) ** 2
    if code == 3: return sigmoid(x) * sigmoid(-x)
    if code == 4: return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))
    if code == 5: return SELU_SCALE * np.where(x > 0, 1.0, SELU_ALPHA * np.exp(np.minimum(x, 0.0)))
    if code == 6: return sigmoid(x)
    if code == 7: return 1.0 / (1.0 + np.abs(x)) ** 2
    if code == 8: return np.where(x > 0, 1.0, 0.3)
    if code == 10: return np.where(np.abs(x) < 2.5, 0.2, 0.0)
    if code == 11: return np.exp(x)
    if code == 12:
        s = sigmoid(x)
        return s * (1.0 + x * sigmoid(-x))
    if code == 13: return _Phi(x) + x * _phi(x)
    raise ValueError(code)


def act_slope_from_out(code, h):
    """The slope through the output h = act(x), as the kernels form it for codes 0-11 (act_grad_other)."""
    h = np.asarray(h, np.float64)
    if code == 0: return np.ones_like(h)
    if code == 1: return (h > 0).astype(np.float64)
    if code == 2: return 1.0 - h * h
    if code == 3: return h * (1.0 - h)
    if code == 4: return np.where(h > 0, 1.0, h + 1.0)
    if code == 5: return np.where(h > 0, SELU_SCALE, h + SELU_SCALE * SELU_ALPHA)
    if code == 6: return -np.expm1(-h)
    if code == 7: return (1.0 - np.abs(h)) ** 2
    if code == 8: return np.where(h > 0, 1.0, 0.3)
    if code == 10: return np.where((h > 0) & (h < 1), 0.2, 0.0)
    if code == 11: return h.copy()
    raise ValueError('code %d: the slope is not a function of the output' % code)


def ulp32(v):
    """Spacing of the fp32 numbers at |v|."""
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def slope_tolerance(code, x, h):
    """Allowance for the slope an fp32 kernel forms from an operand that enters the step already ROUNDED, against
    act_slope(code, x):
        REL * (sum |terms| of the slope expression)  +  ONE ulp32(v) times the coefficient |d slope / d v|,
    v = the stored output h for codes 0-11 and v = x = xhat + beta (the kernel's fp32 sum) for codes 12, 13."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    z = np.zeros_like(x)
    if code in (0, 1, 8, 10):
        return z                                     # piecewise constant: exact on either side of the kink
    if code == 2: mag, sens, v = 1.0 + h * h, 2.0 * np.abs(h), h
    elif code == 3: mag, sens, v = np.abs(h * (1.0 - h)), np.abs(1.0 - 2.0 * h), h
    elif code == 4: mag, sens, v = np.where(h > 0, 1.0, np.abs(h) + 1.0), np.where(h > 0, 0.0, 1.0), h
    elif code == 5: mag, sens, v = np.where(h > 0, SELU_SCALE, np.abs(h) + SELU_SCALE * SELU_ALPHA), np.where(h > 0, 0.0, 1.0), h
    elif code == 6: mag, sens, v = -np.expm1(-h), np.exp(-h), h
    elif code == 7: mag, sens, v = (1.0 - np.abs(h)) ** 2, 2.0 * (1.0 - np.abs(h)), h
    elif code == 11: mag, sens, v = np.abs(h), np.ones_like(h), h
    elif code == 12:
        s = sigmoid(x)
        mag, sens, v = s * (1.0 + np.abs(x) * sigmoid(-x)), np.ones_like(x), x       # |swish''| <= 0.5
    elif code == 13:
        mag, sens, v = _Phi(x) + np.abs(x) * _phi(x), np.ones_like(x), x            # |gelu''| <= 0.8
    else:
        raise ValueError(code)
    return REL * mag + ulp32(v) * sens


# ------------------------------------------------------------------ statistics
def block_ranges(B, rows_per_wg):
    """Row blocks of a K-STACK launch: ceil(B / rows_per_wg) workgroups, the rows spread evenly (chunk_rows)."""
    nwg = max(1, -(-B // rows_per_wg))
    cr = -(-B // nwg)
    return [(min(B, w * cr), min(B, (w + 1) * cr)) for w in range(nwg)]


MAX_CHUNKS = 256              # kMaxChunks of dcahip_layers.hip


def chunk_ranges(B, R=None):
    """Row chunks of col_moments / bn_bwd_sums (n_chunks, chunk_rows): R = ceil(B / 64) chunks, at most MAX_CHUNKS, of
    ceil(B / R) rows each.  Below the cap this is block_ranges(B, 64); under it the trailing chunks can be empty."""
    if R is None:
        R = min(MAX_CHUNKS, max(1, -(-B // 64)))
    cr = -(-B // R)
    return [(min(B, r * cr), min(B, (r + 1) * cr)) for r in range(R)]


def entries_tolerance(counts, mean, m2):
    """t_mean, t_M2 (moments_tolerance) of a merge whose INPUTS are the entries (count, mean, M2) themselves, exact as
    handed in: mean_mag = sum n_e |mean_e| / N, the terms of M2 are M2_e and n_e (mean_e - mean)^2 (the result is rounded
    to fp32, so every term counts), and an error REL |mean_e| of a difference mean_e - mean moves M2 by
    2 n_e |mean_e - mean| REL |mean_e|.  Entries with count 0 do not enter."""
    n, gm, gq = merge_stats(counts, mean, m2)
    c = np.asarray(counts, np.float64)[:, None]
    am, d = np.abs(np.asarray(mean, np.float64)), np.abs(np.asarray(mean, np.float64) - gm)
    t_mean = REL * (c * am).sum(0) / n + ulp32(gm)
    t_m2 = REL * gq + (2.0 * c * d * REL * am).sum(0)
    return t_mean, t_m2


def moments_tolerance(st, g):
    """What the statistics of a batch may be off by when an fp32 kernel forms them from (mean, M2) of row chunks:
    st = range_stats over the chunks, g = range_stats over the one range of all rows.  Everything is a function of the
    reference; on a column whose mean is far larger than its spread the terms exceed the flat classes (an fp32 mean
    carries ulp32(mean), however it is added up), elsewhere they are negligible beside them.
        t_mean = REL * mean_mag + ulp32(mean)
        t_M2   = sum over chunks (REL * m2_mag + m2_in)  +  sum over chunks 2 count |mean_chunk - mean| REL mean_mag_chunk
    Returns t_mean [H], t_M2 [H]."""
    mean = g['mean'][0]
    t_mean = REL * g['mean_mag'][0] + ulp32(mean)
    t_m2 = (REL * st['m2_mag'] + st['m2_in']).sum(0)
    t_m2 = t_m2 + (2.0 * st['count'][:, None] * np.abs(st['mean'] - mean) * REL * st['mean_mag']).sum(0)
    return t_mean, t_m2


def fwd_bounds(o, code, beta, t_mean, t_m2, n, EL, momentum=BN_MOMENTUM):
    """Bounds of xhat, H, inv_std, mm, mv of fwd_step's result o: the flat classes EL (rtol, atol) plus the first-order
    effect of t_mean / t_M2 (moments_tolerance) on each."""
    flat = lambda k, ref: EL[k][1] + EL[k][0] * np.abs(ref)
    inv = o['inv_std']
    x = o['xhat'] + (0.0 if beta is None else np.asarray(beta, np.float64))
    b = {'xhat': flat('xhat', o['xhat']) + inv * t_mean,
         'H': flat('H', o['H']) + np.abs(act_slope(code, x)) * inv * t_mean,
         'inv_std': 1e-5 * inv + 0.5 * inv ** 3 * t_m2 / n}
    if 'mm' in o:
        b['mm'] = flat('mm', o['mm']) + (1.0 - momentum) * t_mean
        b['mv'] = flat('mv', o['mv']) + (1.0 - momentum) * t_m2 / n
    return b


def split_ranges(counts):
    r, out = 0, []
    for c in counts:
        out.append((r, r + int(c)))
        r += int(c)
    return out


def range_stats(Z, ranges):
    """(mean, M2) of every row range (an empty range: 0, 0) with the magnitudes they are judged against."""
    Z = np.asarray(Z, np.float64)
    R, H = len(ranges), Z.shape[1]
    o = {k: np.zeros((R, H)) for k in ('mean', 'm2', 'mean_mag', 'm2_mag', 'm2_in')}
    o['count'] = np.zeros(R)
    for r, (a, b) in enumerate(ranges):
        if b <= a:
            continue
        z = Z[a:b]
        m = z.mean(0)
        o['count'][r] = b - a
        o['mean'][r] = m
        o['m2'][r] = np.square(z - m).sum(0)
        o['mean_mag'][r] = np.abs(z).sum(0) / (b - a)
        o['m2_mag'][r] = o['m2'][r]
        # the rounding of each z - m (both operands of size mean_mag) carried through the square: not a shift of the mean,
        # which would cancel to second order
        o['m2_in'][r] = 2.0 * np.abs(z - m).sum(0) * REL * o['mean_mag'][r]
    return o


def merge_stats(counts, mean, m2):
    """Chan et al. merge of (count, mean, M2) entries [E], [E, H], [E, H]; an entry with count 0 is ignored."""
    counts = np.asarray(counts, np.float64)
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    keep = counts > 0
    c, m, q = counts[keep][:, None], mean[keep], m2[keep]
    n = c.sum()
    if n <= 0:
        return 0.0, np.zeros(mean.shape[1]), np.zeros(mean.shape[1])
    gm = (c * m).sum(0) / n
    return float(n), gm, (q + c * np.square(m - gm)).sum(0)


# ------------------------------------------------------------------ forward
def fwd_step(step, Z, counts=None, mean=None, m2=None, beta=None, W=None, bias=None, mm=None, mv=None, act=1,
             ranges=None, momentum=BN_MOMENTUM, eps=BN_EPS):
    """Step `step` of the forward pass from what it reads: Z [B, H] of the step's layer, the entries it is handed
    (counts [E], mean [E, H], m2 [E, H]), beta [H], the NEXT layer's W [H, H'] / bias [H'] (None behind the last
    layer), the moving statistics.  ranges: row ranges whose (mean, M2) of the layer made are returned."""
    Z = np.asarray(Z, np.float64)
    ranges = [(0, Z.shape[0])] if ranges is None else ranges
    if step == 0:
        return {'stats': range_stats(Z, ranges)}
    n, gm, gq = merge_stats(counts, mean, m2)
    var = gq / n if n > 0 else np.zeros_like(gq)
    inv = 1.0 / np.sqrt(var + eps)
    xh = (Z - gm) * inv
    x = xh + (0.0 if beta is None else np.asarray(beta, np.float64))
    H = act_fwd(act, x)
    o = {'n': n, 'mean': gm, 'var': var, 'inv_std': inv, 'xhat': xh, 'H': H}
    if mm is not None:
        o['mm'] = mm - (mm - gm) * (1.0 - momentum)
        o['mv'] = mv - (mv - var) * (1.0 - momentum)
    if W is not None:
        W = np.asarray(W, np.float64)
        o['Z'] = H @ W + (0.0 if bias is None else np.asarray(bias, np.float64))
        o['stats'] = range_stats(o['Z'], ranges)
    return o


def fwd_pass(Z0, layers, act=1, momentum=BN_MOMENTUM, eps=BN_EPS):
    """The whole forward pass composed from the steps.  layers[i]: dict(beta, mm, mv) and, for i > 0, W, bias.
    Returns one dict per layer (Z, xhat, inv_std, H, mm, mv)."""
    Z = np.asarray(Z0, np.float64)
    st = fwd_step(0, Z)['stats']
    out = []
    for i, L in enumerate(layers):
        N = layers[i + 1] if i + 1 < len(layers) else {}
        o = fwd_step(i + 1, Z, st['count'], st['mean'], st['m2'], L.get('beta'), N.get('W'), N.get('bias'),
                     L['mm'], L['mv'], act, None, momentum, eps)
        out.append({'Z': Z, 'xhat': o['xhat'], 'inv_std': o['inv_std'], 'H': o['H'], 'mm': o['mm'], 'mv': o['mv']})
        if 'Z' in o:
            Z, st = o['Z'], o['stats']
    return out


# ------------------------------------------------------------------ backward
def _dy(dH, Hact, xhat, beta, act, dH_tol):
    xhat = np.asarray(xhat, np.float64)
    x = xhat + (0.0 if beta is None else np.asarray(beta, np.float64))
    s = act_slope(act, x)
    dH = np.asarray(dH, np.float64)
    t = np.abs(dH) * slope_tolerance(act, x, Hact) + np.abs(s) * dH_tol
    return dH * s, t


def _range_sums(dy, t_dy, xhat, ranges):
    R, H = len(ranges), dy.shape[1]
    o = {k: np.zeros((R, 2, H)) for k in ('sums', 'sums_mag', 'sums_in')}
    for r, (a, b) in enumerate(ranges):
        d, x, t = dy[a:b], xhat[a:b], t_dy[a:b]
        o['sums'][r, 0], o['sums'][r, 1] = d.sum(0), (d * x).sum(0)
        o['sums_mag'][r, 0], o['sums_mag'][r, 1] = np.abs(d).sum(0), np.abs(d * x).sum(0)
        o['sums_in'][r, 0], o['sums_in'][r, 1] = t.sum(0), (t * np.abs(x)).sum(0)
    return o


def bwd_step(step, dH, Hact, xhat, inv_std=None, beta=None, S1=None, S2=None, n_total=None, Hprev=None, W=None,
             low=None, act=1, ranges=None, dH_tol=0.0, S_tol=(0.0, 0.0)):
    """Step `step` of the backward pass from what it reads: dH / Hact / xhat [B, H] of the step's layer, inv_std, beta,
    the GLOBAL sums S1 = sum dy, S2 = sum dy xhat and n_total, the layer's input Hprev [B, K] and kernel W [K, H];
    low = dict(Hact, xhat, beta) of the layer below (None for the first layer).  dH_tol / S_tol: allowances for inputs
    that are themselves results (the whole-pass composition; sums added up in fp32 by the kernel).
    Returns dy; step 0: the sums over `ranges`; step >= 1: dZ, dbeta (the local share, sum dy over these rows),
    gW [K + 1, H] (row K = bias gradient), dHprev, low_dy and the sums of the layer below over `ranges` -- each
    reduction with its _mag and _in (module docstring)."""
    xhat = np.asarray(xhat, np.float64)
    ranges = [(0, xhat.shape[0])] if ranges is None else ranges
    dy, t_dy = _dy(dH, Hact, xhat, beta, act, dH_tol)
    o = {'dy': dy, 'dy_in': t_dy}
    if step == 0:
        o.update(_range_sums(dy, t_dy, xhat, ranges))
        return o
    inv = np.asarray(inv_std, np.float64)
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    m1, m2 = S1 / n_total, S2 / n_total
    o['dbeta'], o['dbeta_mag'], o['dbeta_in'] = dy.sum(0), np.abs(dy).sum(0), t_dy.sum(0)
    dZ = inv * (dy - m1 - xhat * m2)
    o['dZ'] = dZ
    o['dZ_mag'] = inv * (np.abs(dy) + np.abs(m1) + np.abs(xhat * m2))
    o['dZ_in'] = inv * (t_dy + S_tol[0] / n_total + np.abs(xhat) * S_tol[1] / n_total)
    if Hprev is None:
        return o
    T = REL * o['dZ_mag'] + o['dZ_in']                   # what dZ may be off by where it enters the products below
    Hp, W = np.asarray(Hprev, np.float64), np.asarray(W, np.float64)
    o['gW'] = np.vstack([Hp.T @ dZ, dZ.sum(0)[None]])
    o['gW_mag'] = np.vstack([np.abs(Hp).T @ np.abs(dZ), np.abs(dZ).sum(0)[None]])
    o['gW_in'] = np.vstack([np.abs(Hp).T @ T, T.sum(0)[None]])
    o['dHprev'] = dZ @ W.T
    o['dHprev_mag'] = np.abs(dZ) @ np.abs(W).T
    o['dHprev_in'] = T @ np.abs(W).T
    if low is not None:
        Tp = REL * o['dHprev_mag'] + o['dHprev_in']
        lx = np.asarray(low['xhat'], np.float64)
        ldy, lt = _dy(o['dHprev'], low['Hact'], lx, low.get('beta'), act, Tp)
        o['low_dy'], o['low_dy_in'] = ldy, lt
        for k, v in _range_sums(ldy, lt, lx, ranges).items():
            o['low_' + k] = v
    return o


def bwd_pass(dH, layers, n_total, act=1):
    """The whole backward pass composed from the steps.  layers[i]: dict(Hact, xhat, inv_std, beta) and, for i > 0, W
    (its input is layers[i - 1]['Hact']).  Results that feed the next step carry their allowance along, so every _mag /
    _in is that of the chain from the stored forward outputs.  Returns one dict per layer (bwd_step's, plus dZ0 in [0])."""
    n = len(layers)
    out = [None] * n
    T = layers[n - 1]
    o0 = bwd_step(0, dH, T['Hact'], T['xhat'], beta=T.get('beta'), act=act)
    sums, tol, dH_tol = o0['sums'][0], REL * o0['sums_mag'][0] + o0['sums_in'][0], 0.0
    for i in reversed(range(n)):
        L = layers[i]
        P = layers[i - 1] if i > 0 else None
        o = bwd_step(n - i, dH, L['Hact'], L['xhat'], L['inv_std'], L.get('beta'), sums[0], sums[1], n_total,
                     P['Hact'] if P else None, L.get('W') if P else None,
                     dict(Hact=P['Hact'], xhat=P['xhat'], beta=P.get('beta')) if P else None, act, None, dH_tol,
                     (tol[0], tol[1]))
        out[i] = o
        if P:
            dH, dH_tol = o['dHprev'], REL * o['dHprev_mag'] + o['dHprev_in']
            sums, tol = o['low_sums'][0], REL * o['low_sums_mag'][0] + o['low_sums_in'][0]
    return out


def error_and_bound(o, name, got, rel=REL):
    """(|got - o[name]|, rel * o[name + '_mag'] + o[name + '_in']): the error of a reduction or product and the bound it is
    judged against."""
    err = np.abs(np.asarray(got, np.float64) - o[name])
    return err, rel * o[name + '_mag'] + o.get(name + '_in', 0.0)
