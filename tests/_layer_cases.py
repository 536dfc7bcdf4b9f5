"""Inputs of the per-layer kernel tests (tests/test_layer_kernels_gpu.py) that the CPU test of their bounds
(tests/test_stack_ref_cpu.py) needs as well: numpy only.  Every array is fp32 -- what a kernel reads -- and is widened to
fp64 by the reference."""
import numpy as np

import _stack_ref as SR

# B x H of the large-batch kernels (col_moments + bn_relu_apply, bn_bwd_sums + bn_bwd_apply), from their branch points:
#   65 x 20      two chunks of 33 / 32 rows, one ragged strip
#   1 x 5        one row: M2 = 0, inv_std = eps^-1/2, xhat = 0 (forward only)
#   130 x 64     three chunks of 44 / 44 / 42 rows, exactly one full strip
#   2800 x 130   175 row blocks of the apply kernels: grid.y = 2 for 3 strips, the blocks with y = 0 walk strips 0 and 2
#   16450 x 70   the chunk cap: 256 chunks of 65 rows, chunk 253 holds 5, chunks 254 and 255 none; 1029 row blocks of the
#                apply kernels: grid.y = 1, every block walks both strips
LARGE_SHAPES = [(65, 20), (1, 5), (130, 64), (2800, 130), (16450, 70)]
COND_SHAPES = [(65, 20), (2800, 130)]

# (mean, std) of the conditioned columns; then a constant column and a zero column.  Column indices: one list per width,
# at H = 130 in all three strips.
COND_STATS = [(300.0, 0.3), (3000.0, 0.3), (-300.0, 3.0), (1e-3, 1e-4)]
COND_COLS = {20: [1, 7, 19, 10, 3, 18], 130: [1, 66, 129, 64, 3, 128]}
CONST_VALUE = 2.5
WORST_COL = 1                  # index into COND_COLS[H] of the (3000, 0.3) column


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def large_fwd_problem(B, H, conditioned=False, seed=None):
    """Z [B, H], beta, moving mean / variance [H].  conditioned: six columns are replaced (COND_STATS, constant, zero).
    A conditioned column's standardised values keep 0.4 away from zero and its beta is 0, so that no pre-activation lies
    within the column's allowance for xhat of the kink of relu; the constant and the zero column (xhat = 0) get a beta of
    +0.5 / -0.5 for the same reason (checked by fwd_conditions, never filtered)."""
    rng = np.random.RandomState(4000 + B + 3 * H if seed is None else seed)
    p = dict(B=B, H=H, Z=f32(rng.normal(size=(B, H)) * 1.5 + rng.normal(size=H)), beta=f32(rng.normal(size=H) * 0.3),
             mm0=f32(rng.normal(size=H) * 0.1), mv0=f32(rng.uniform(0.5, 1.5, size=H)), cond=[])
    if conditioned:
        cols = COND_COLS[H]
        for c, (m, s) in zip(cols, COND_STATS):
            u = rng.choice([-1.0, 1.0], size=B) * (0.4 + 0.8 * np.abs(rng.normal(size=B)))
            p['Z'][:, c] = f32(m + s * u)
            p['beta'][c] = 0.0
        p['Z'][:, cols[4]], p['beta'][cols[4]] = CONST_VALUE, 0.5
        p['Z'][:, cols[5]], p['beta'][cols[5]] = 0.0, -0.5
        p['cond'] = cols
    return p


def fwd_conditions(code, x, dx=None):
    """What the forward tests require of the reference pre-activation x = xhat + beta (asserted on the host before any
    launch).  dx: the allowance for xhat where it exceeds the flat class (conditioned columns): relu's kink must be
    further away than that, or kernel and reference could take different sides of it."""
    if code == 10:
        assert np.abs(np.abs(x) - 2.5).min() > 1e-4, 'hard_sigmoid: a pre-activation within 1e-4 of the kink at 2.5'
    if code == 11:
        assert np.abs(x).max() < 40.0, 'exponential: |x| >= 40'
    if dx is not None and code in (1, 8):
        wide = np.broadcast_to(dx > 1e-5, x.shape)
        assert (np.abs(x)[wide] > 2.0 * np.broadcast_to(dx, x.shape)[wide]).all(), 'a pre-activation within its allowance of 0'


def bwd_conditions(code, x, Hact):
    """Backward tests: the hard_sigmoid kink as above; codes 1 and 8 take their mask from the stored h, so no stored h may
    have underflowed (0 < |h| < 1e-30) or have lost the sign of x."""
    fwd_conditions(code, x)
    if code in (1, 8):
        a = np.abs(Hact)
        assert not ((a > 0) & (a < 1e-30)).any(), 'a stored activation of magnitude below 1e-30'
        assert np.array_equal(np.asarray(x) > 0, np.asarray(Hact) > 0), 'a stored activation lost the sign of x'


def bwd_problem(B, H, code, K=0, seed=None):
    """The fp32 operands of one layer's backward, as tests/test_bn_bwd_beta_gpu.py builds them: dH, xhat, beta, inv_std
    and Hact = fp32(act(xhat + beta)); with K the layer's input Hp [B, K] and kernel W [K, H]."""
    rng = np.random.RandomState(1000 * B + 10 * H + K + 77 * code if seed is None else seed)
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    p = dict(B=B, H=H, K=K, code=code, dH=f(rng.normal(0, 1, (B, H))), xhat=f(rng.normal(0, 1, (B, H))),
             beta=f(rng.normal(0, .5, H) - (0.8 if code >= SR.ACT_PRE else 0.0)), inv_std=f(rng.uniform(.5, 2., H)))
    p['x'] = p['xhat'] + p['beta']
    p['Hact'] = f(SR.act_fwd(code, p['x']))
    if K:
        p['Hp'], p['W'] = f(rng.normal(0, 1, (B, K))), f(rng.normal(0, .3, (K, H)))
    bwd_conditions(code, p['x'], p['Hact'])
    return p
