"""Inputs of the four-wave K-HEADS edge tests (tests/test_heads_small_edges_gpu.py) that the CPU test of their reach
conditions (tests/test_heads_small_edges_cpu.py) needs as well.  A case is the keyword arguments of
test_heads_fused_gpu.run_case: the GPU half passes them to run_case, the CPU half to oracle_case(), which draws the same
inputs (test_heads_fused_gpu.draw_inputs) and stops at the fp64 reference.

Shapes: G = 300 (nine full gene tiles and one of 12 genes), hL = 64, and
    B = 32    NT = 1   the four-wave kernel's direct output form; the default batch size
    B = 33    NT = 2   the second row tile holds a single row; partials + the reduce kernels
    B = 96    NT = 3   (constant-dispersion clip only: the reduce chain from four-wave partials)
    B = 128   NT = 4   the largest four-wave batch, every tile full
    B = 160   NT = 5   the smallest 8-wave batch (clip and weight-scale cases only)
    B = 512   NT = 16  8-wave with two batch splits (clip case only)
and B = 5, G = 6, hL = 16: one partial tile in every dimension (Gp = 8: g_theta has two padding slots).
"""
import numpy as np

from conftest import synth_counts
from test_heads_edges_gpu import repeat_counts, tile_scales           # noqa: F401  (tile_scales: for both halves)
from test_heads_fused_gpu import draw_inputs, reference

G, HL = 300, 64
TINY = (5, 6, 16)                                  # B, G, hL
FLAGS = [1, 0, 3, 2]
LAST_TILE = 32 * ((G - 1) // 32)                   # first gene of the last, partial gene tile

ORACLE_KEYS = ('flags', 'B', 'G', 'hL', 'seed', 'ridge', 'odd_counts', 'counts', 'hscale', 'tw', 'wscale')


def ridge_of(flags):
    return 0.05 if flags & 1 else 0.0


def oracle_case(**kw):
    """The fp64 half of run_case on a case: out['_ref'] as run_case leaves it (what tile_scales reads), the inputs, and the
    reference's loss and gradients."""
    kw = {k: v for k, v in kw.items() if k in ORACLE_KEYS}
    flags, B, g, ridge = kw['flags'], kw['B'], kw['G'], kw.pop('ridge', 0.0)
    heads, Hm, W, b, tw, y, sf, _ = draw_inputs(**kw)
    n_total = float(B * g)
    _, lm, gW, gb, dH, dth, mag, D = reference(Hm, W, b, tw, y, sf, flags, ridge, n_total)
    return {'_ref': {'H': Hm, 'D': [D[h] for h in heads], 'W': np.stack([W[h] for h in heads]), 'n_total': n_total},
            'heads': heads, 'y': y, 'tw': tw, 'b': b, 'loss': lm, 'gW': gW, 'gb': gb, 'dH': dH, 'g_theta': dth}


# ------------------------------------------------------------------------------------------------- (a) tile rescale
RESCALE_B = [32, 33, 128]
RESCALE_KINDS = ['around4000', 'outliers']
RESCALE_D_EXP = [0, -3]                            # (the GPU half adds the engine's pick for the counts)


def rescale_counts(kind, B, seed):
    """'outliers': test_heads_edges_gpu.repeat_counts -- sparse counts up to 70 000 beside the lowest-expressed genes.
    'around4000' stands in for repeat_counts' 'around400', which reaches the branch of neither assertion at 32 rows: its
    gradients stay below 1 300, under the 937.5 = kDLim 2^-5 of d_exp = -3 for most flags, and the counts of its last
    gene tile still carry every tile beyond the 117 of d_exp = 0.  Here: counts around 4 000 throughout (gradients in the
    thousands), the last gene tile capped at 40: its gradients stay below 117, on the fast path at either exponent."""
    if kind == 'outliers':
        return repeat_counts(kind, B, G, seed)
    assert kind == 'around4000'
    rng = np.random.RandomState(seed)
    y = rng.poisson(4000.0 * rng.lognormal(0, 0.25, G)[None, :] * rng.lognormal(0, 0.2, B)[:, None]).astype(np.float64)
    y *= rng.uniform(size=(B, G)) >= 0.05
    y[:, LAST_TILE:] = np.minimum(synth_counts(B, G - LAST_TILE, seed), 40.0)
    return y


def rescale_case(flags, B, kind):
    return dict(flags=flags, B=B, G=G, hL=HL, seed=B + G + flags, ridge=ridge_of(flags),
                counts=rescale_counts(kind, B, B + flags))


# ------------------------------------------------------------------------------------------------- (b), (c) escapes
ESCAPE_B = [32, 33]


def escaped_fp32(y):
    """The counts the fp32 path cannot put into a 16-bit queue slot: non-integers and 65 535 and more."""
    return (y != np.floor(y)) | (y >= 65535.0)


def escaped_byte(y):
    """The counts the byte store keeps as 255 and resolves through the overflow list."""
    return y >= 255.0


def escape_case(flags, B):
    """fp32 escapes at element (0, 0), at (B - 1, G - 1) -- the last row of the last, partial gene tile; for B = 33 that is
    row 32, the lone row of the second row tile -- and in between."""
    y = synth_counts(B, G, 17)
    y[0, :6] = [2.52, 0.5, 17.0, 70000.0, 200.0, 5000.0]
    y[1, 1:4] = [16.0, 16.5, 65535.0]
    y[B - 1, 40:44] = [65534.0, 65535.0, 65536.0, 0.25]
    y[B - 1, LAST_TILE] = 16.5
    y[B - 1, G - 1] = 1e5
    return dict(flags=flags, B=B, G=G, hL=HL, seed=23 + flags + B, ridge=ridge_of(flags), counts=y)


def compact_case(flags, B):
    """The byte store: 254 (stored), 255 and 256 (escapes), 65 535 and 70 000 through the overflow list, at the positions
    of escape_case."""
    y = synth_counts(B, G, 19)
    y[0, :5] = [255, 254, 256, 65535, 70000]
    y[3, 31:34] = [255, 254, 256]
    y[10, 150] = 1000
    y[B - 1, 0] = 65535
    y[B - 1, 40:43] = [254, 255, 256]
    y[B - 1, LAST_TILE] = 70000
    y[B - 1, G - 1] = 255
    return dict(flags=flags, B=B, G=G, hL=HL, seed=29 + flags + B, counts=y, compact=True)


# ------------------------------------------------------------------------------------------------- (d) row-tile scale
HSCALES = {
    128: {'zero_tile': [0.0, 1.0, 1.0, 1.0],
          'spread': [1.0, 2.0 ** -40, 2.0 ** 20, 2.0 ** -7],
          'all_2^-23': [2.0 ** -23] * 4},
    32: {'all_zero': [0.0],
         '2^15': [2.0 ** 15]},
}
HSCALE_CASES = [(B, name) for B in (128, 32) for name in HSCALES[B]]


def hscale_case(flags, B, name):
    """As test_heads_row_scale_spread: counts capped at 40, so that no tile rescales and product_tol holds for every
    element."""
    y = np.minimum(synth_counts(B, G, B + G), 40.0)
    return dict(flags=flags, B=B, G=G, hL=HL, seed=31 + flags, ridge=0.02 if flags & 1 else 0.0, counts=y,
                hscale=HSCALES[B][name])


# ------------------------------------------------------------------------------------------------- (e) gene-tile weight scale
WSCALE = [1.0, 0.0, 2.0 ** -30, 2.0 ** -10, 4.0, 1.0, 2.0 ** -10, 4.0, 2.0 ** -30, 0.0]
WSCALE_B = [32, 128, 160]


def wscale_case(flags, B):
    """Gene tiles 1 and 9 (the partial one) all zero in every head, the others between 2^-30 and 4 times the usual weights.
    Counts capped at 40 as in hscale_case."""
    y = np.minimum(synth_counts(B, G, B + G + 1), 40.0)
    return dict(flags=flags, B=B, G=G, hL=HL, seed=37 + flags + B, ridge=ridge_of(flags), counts=y, wscale=WSCALE)


# ------------------------------------------------------------------------------------------------- (f) constant-dispersion clip
CLIP_LO, CLIP_HI = np.log(1e-3), np.log(1e4)       # exp(theta_w) in [1e-3, 1e4]: theta_w in [-6.908, 9.210]
CLIP_VALUES = [-100.0, -12.0, -7.5, -6.5, 9.0, 9.3, 20.0, 9500.0]
CLIP_TILES = [0, 4, 9]                             # the first, an inner and the last gene tile
CLIP_B = [32, 96, 160, 512]
CLIP_FLAGS = [3, 2]


def clip_tw(g=G):
    """N(0, 1.5) with CLIP_VALUES written into the first four and the last four genes of each tile of CLIP_TILES, rotated
    from tile to tile so that the first and the last gene of a tile see different values.  (g = 6, the tiny shape: six of
    the values, both sides of both bounds.)"""
    tw = np.random.RandomState(101).normal(0, 1.5, g)
    if g == TINY[1]:
        tw[:] = [-100.0, -6.5, 9.0, 9.3, 9500.0, -7.5]
        return tw
    for n, t in enumerate(CLIP_TILES):
        lo, hi = 32 * t, min(g, 32 * t + 32)
        pos = [lo, lo + 1, lo + 2, lo + 3, hi - 4, hi - 3, hi - 2, hi - 1]
        tw[pos] = np.roll(CLIP_VALUES, 3 * n)
    return tw


def clip_outside(tw):
    """Genes whose exp(theta_w) lies outside the clip (fp32-rounded theta_w, fp64 exp: the values nearest a bound are 0.089
    away from it, fp32 expf is good to 1e-6 relative)."""
    t = np.asarray(tw, np.float32).astype(np.float64)
    return (t < CLIP_LO) | (t > CLIP_HI)


def clip_case(flags, B, shape=None):
    g, hl = (G, HL) if shape is None else shape[1:]
    return dict(flags=flags, B=B, G=g, hL=hl, seed=41 + flags + B, ridge=ridge_of(flags), tw=clip_tw(g))


# ------------------------------------------------------------------------------- terms beside product_tol, from the inputs alone
def _oracle_inputs(kw):
    kw = {k: v for k, v in kw.items() if k in ORACLE_KEYS}
    flags, B, g, ridge = kw['flags'], kw['B'], kw['G'], kw.pop('ridge', 0.0)
    return (flags, ridge, float(B * g)) + draw_inputs(**kw)[:7]


def disp_floor_terms(**kw):
    """Conditional dispersion: what the fp32 evaluation of the dispersion head's gradient of a y > 0 element may lose to
    cancellation beyond product_tol's per-element allowance (oracle/x3_np.py::disp_grad_floor; the CPU proof is
    tests/test_x3_arith_cpu.py::test_heads_disp_gradient_floor), carried to the outputs it enters, in loss units:
    {gW_disp: |H|^T f, gb_disp: column sums of f, dH: f |W_disp|^T}.  Zero for all but the elements that lost about three
    digits; {} with a constant dispersion."""
    from oracle import x3_np as X
    from oracle import zinb_np as Z
    flags, ridge, n_total, heads, H, W, b, tw, y, sf = _oracle_inputs(kw)
    if flags & 2:
        return {}
    am, ad = H @ W['mean'] + b['mean'], H @ W['disp'] + b['disp']
    mu, theta = Z.mean_act(am) * sf[:, None], Z.disp_act(ad)
    gd = Z._act_grads(am, ad)[1]
    dpsi, l1p, last = X.dth_terms(mu, theta, y)
    f = X.disp_grad_floor(mu, theta, gd, y, (-dpsi + l1p + last) * gd) / n_total
    return {'gW_disp': np.abs(H).T @ f, 'gb_disp': f.sum(0), 'dH': f @ np.abs(W['disp']).T}


def add_terms(*terms):
    out = {}
    for t in terms:
        for k, v in t.items():
            out[k] = out.get(k, 0.0) + v
    return out


# ------------------------------------------------------------------------------------------------- (d) a row tile at 2^15 and more
# H at 2^15 .. 2^20 puts the pre-activations a = H W + b at 1e5 .. 1e7: every head saturates but for the few elements
# whose sum cancels to within the heads' live windows (MeanAct exp(a) in [1e-5, 1e6], DispAct softplus(a) in [1e-4, 1e4],
# sigmoid(a) (1 - sigmoid(a)) != 0).  The forward product is an fp32 dot product (oracle/x3_np.py, contract of
# dcahip_x3_product_32x32: |a' - a| <= 5e-7 sum|h w|, then one fp32 rounding of a' + b), so at this scale a' is off by
# 0.1 .. 10 -- as wide as the windows.  What ANY fp32 forward leaves of such an element's gradient is the likelihood's own
# modulus of continuity over that error box, not a property of the backward products product_tol speaks of.
BIG_H = 2.0 ** 10                                  # row tiles whose largest |H| reaches this get the term; every other row none
FWD_TOL = 5e-7                                     # tests/test_heads_fused_gpu.py::test_x3_products_are_fp32_accurate
MOD_STEPS = 8                                      # grid steps per half box
# outside these (by a margin of 1) a head's activation and its derivative are constant: the clips of MeanAct and DispAct
# are exact; sigmoid beyond |a| = 100 is within 4e-44 of 0 or 1, which the likelihood multiplies by 1 / eps = 1e10 at most
LIVE = {'mean': (np.log(1e-5), np.log(1e6)), 'disp': (np.log(np.expm1(1e-4)), 1e4), 'pi': (-100.0, 100.0)}


def _planes(A, heads, tw, y, sf, flags, ridge, n_total):
    """The oracle's per-element gradient planes, one per head in loss units; constant dispersion adds 'theta': the
    per-element chained d / d theta_w (the oracle returns its column sums: it is asked row by row)."""
    from oracle import zinb_np as Z
    has_pi, cdisp = bool(flags & 1), bool(flags & 2)

    def one(r):
        if has_pi:
            _, _, dm, dd, dp = Z.zinb_loss_and_grads(A['mean'][r], None if cdisp else A['disp'][r], A['pi'][r], y[r], sf[r],
                                                     ridge, n_total, tw if cdisp else None)
        else:
            _, _, dm, dd = Z.nb_loss_and_grads(A['mean'][r], None if cdisp else A['disp'][r], y[r], sf[r], n_total,
                                               tw if cdisp else None)
            dp = None
        return dm, dd, dp
    if cdisp:
        parts = [one(slice(r, r + 1)) for r in range(len(sf))]
        dm = np.concatenate([p[0] for p in parts]); dd = np.stack([p[1] for p in parts])
        dp = np.concatenate([p[2] for p in parts]) if has_pi else None
    else:
        dm, dd, dp = one(slice(None))
    P = {'mean': dm, ('theta' if cdisp else 'disp'): dd}
    if has_pi:
        P['pi'] = dp
    return P


def forward_error_terms(A_of=None, **kw):
    """For a case with row tiles at BIG_H and more: omega[plane] [B, G] >= 0, a bound on the change of the oracle's gradient
    plane when every head's pre-activation moves inside its forward error box
        delta_h = FWD_TOL sum|h w| + 2^-24 |a|.
    Zero in every row of an ordinary tile, and for every element none of whose boxes reaches its head's LIVE window (all
    it depends on is constant there).  For the others: over the grid of 2 MOD_STEPS + 1 points per live head, the largest
    |f - f(a)| plus, per axis, the largest step between neighbouring grid points (what f can do inside a cell if it is
    monotone there; the jumps at the clips are steps of the grid like any other).
    Returns (omega, add): add[key] is what omega allows the output `key` of run_case --  gW_h: |H|^T omega_h,
    dH: sum_h omega_h |W_h|^T,  gb_h and g_theta: column sums.
    A_of(heads, H, W, b) -> {head: A'}: another forward product for the rows of the big tiles (the CPU proof passes the
    fp16-piece model of oracle/x3_np.py); then also returned: the change of every gradient plane from A to A', and
    (heads, H, W)."""
    flags, ridge, n_total, heads, H, W, b, tw, y, sf = _oracle_inputs(kw)
    B, g = y.shape
    tile_max = np.abs(np.pad(H, ((0, -B % 32), (0, 0)))).reshape(-1, 32 * H.shape[1]).max(1)
    rows = np.flatnonzero(np.repeat(tile_max >= BIG_H, 32)[:B])
    assert rows.size
    Hb = H[rows]
    A = {h: Hb @ W[h] + b[h] for h in heads}
    delta = {h: FWD_TOL * (np.abs(Hb) @ np.abs(W[h])) + 2.0 ** -24 * np.abs(A[h]) for h in heads}
    live = {h: (A[h] + delta[h] >= LIVE[h][0] - 1.0) & (A[h] - delta[h] <= LIVE[h][1] + 1.0) for h in heads}
    planes = ['mean', 'theta' if flags & 2 else 'disp'] + (['pi'] if flags & 1 else [])
    om = {k: np.zeros((B, g)) for k in planes}
    steps = np.linspace(-1.0, 1.0, 2 * MOD_STEPS + 1)
    for i, c in zip(*np.nonzero(np.any([live[h] for h in heads], axis=0))):
        axes = [h for h in heads if live[h][i, c]]
        mesh = np.meshgrid(*[A[h][i, c] + steps * delta[h][i, c] for h in axes], indexing='ij')
        shape = mesh[0].shape
        Ag = {h: np.full((1, mesh[0].size), A[h][i, c]) for h in heads}
        for h, m in zip(axes, mesh):
            Ag[h] = m.reshape(1, -1)
        n = mesh[0].size
        P = _planes(Ag, heads, np.full(n, tw[c]), np.full((1, n), y[rows[i], c]), sf[rows[i]:rows[i] + 1], flags, ridge, n_total)
        for k in planes:
            f = P[k].reshape(shape)
            v = np.abs(f - f[(MOD_STEPS,) * len(axes)]).max()
            v += sum(np.abs(np.diff(f, axis=ax)).max() for ax in range(len(axes)))
            om[k][rows[i], c] = v
    add = {'dH': sum(om[h] @ np.abs(W[h]).T for h in heads)}
    for h in heads:
        add['gW_' + h] = np.abs(H).T @ om[h]
        add['gb_' + h] = om[h].sum(0)
    if 'theta' in om:
        add['g_theta'] = om['theta'].sum(0)
    if A_of is None:
        return om, add
    Am = A_of(heads, Hb, W, b)
    assert all((np.abs(Am[h] - A[h]) <= delta[h]).all() for h in heads)         # the model's forward stays inside the box
    args = (heads, tw, y[rows], sf[rows], flags, ridge, n_total)
    base, moved = _planes(A, *args), _planes(Am, *args)
    diff = {k: np.zeros((B, g)) for k in planes}
    for k in planes:
        diff[k][rows] = moved[k] - base[k]
    return om, add, diff, (heads, H, W)

