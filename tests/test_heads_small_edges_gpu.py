"""K-HEADS' four-wave kernel (heads_fused_small_kernel: every batch of at most 128 rows, so every batch of the reference's
default size 32) at its edges against the fp64 oracle, at the strict per-element bounds of tests/test_heads_fused_gpu.py: the
tile rescale, the count escapes of the fp32 and the byte store, d_exp != 0, the row tile's and the gene tile's scale, both
output forms (NT == 1 writes the gradients itself, NT = 2 .. 4 leaves partials to the reduce kernels) and determinism; and,
on both kernels, the clip of the constant dispersion and gene tiles of very different weight magnitude.  The inputs come from
tests/_heads_small_cases.py; tests/test_heads_small_edges_cpu.py proves from the oracle alone that they reach the branches.

check_repeat (tests/test_heads_edges_gpu.py) applies to the four-wave kernel as it stands: a tile that rescales ends at
kD0 - shift = 13 - floor(log2 max|g|), the exponent the 8-wave kernel's repeat step lands at, and a tile that does not stays at
exactly kD0, which is inside the kD0 - K_DSLACK that tile_scales allows for.

Three terms stand beside product_tol, all computed from the inputs alone (held() below; the row-scale cases without a big
tile and the clip cases pass check() as it is):

  * D's fp16 floor for EVERY element, not only behind a tile that rescaled: D = g 2^kD is two fp16 pieces, good to 2^-25
    absolute at that scale (oracle/x3_np.py::split2; the last assertion of test_x3_arith_cpu.py::test_heads_repeat_path_bound),
    so an output element carries up to 2^-(kD + 25) sum|b| beside product_tol sum|a b| -- the contract product_tol's docstring
    states and check_repeat's floor_keys applies.  A 32-row sum over a column of saturated heads (weights x 4) or of a
    lowly expressed gene at d_exp = -3 leaves sum|a b| as small as that floor: the first run missed product_tol alone by
    1.6 times there (rescale, outliers, B = 33, d_exp = -3: gW_disp of a gene whose gradients are 1e-6 .. 1e-5, floor 2^-30).
    For a typical element the floor is 1e-4 of its bound.

  * conditional dispersion: d nll / d theta of a y > 0 element is the sum -dpsi + log1p(mu / theta) + (y theta - theta mu) /
    (theta (theta + mu)); where mu << theta it cancels to ~ -mu / theta^2 and keeps the ABSOLUTE fp32 error of its terms, a
    few 1e-8.  product_tol speaks of sum|a b|, and a column of D in which only such elements meet non-zero rows of H (weights
    x 4 saturate most of a tile; 32 rows) makes that sum as small as they are: the first run of these cases missed
    their bound on gW_disp alone, by 2.4 (byte store, B = 32) to 320 times (weights x 4, B = 32; 12 times at B = 160, the
    8-wave kernel), every miss traced to such an element.  oracle/x3_np.py::disp_grad_floor states what the element may lose beyond product_tol's own
    3e-6 of it (tests/test_x3_arith_cpu.py::test_heads_disp_gradient_floor: the fp32 sum, op by op, stays inside and does
    exceed 3e-6), tests/_heads_small_cases.py::disp_floor_terms carries it to gW_disp, gb_disp and dH.

  * a row tile of H at 2^15 and more (two of the row-scale cases): see test_small_row_tile_scale.

The workspace is NaN-filled by run_case: a read of a slot nobody wrote shows in every case.
"""
import numpy as np
import pytest

import _heads_small_cases as C
from oracle import x3_np as X
from test_heads_edges_gpu import check_repeat, engine_d_exp, tile_scales
from test_heads_fused_gpu import check, ops, run_case      # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def four_wave(B):
    return (B + 31) // 32 < 5                                   # make_heads_plan: p.small = NT < kWr8MinNT


def held(out, d_exp, kw):
    """check_repeat with D's fp16 floor for every element (floor_keys) and the dispersion term: see the module docstring."""
    return check_repeat(out, d_exp, floor_keys=tuple(out['_mag']), extra=C.disp_floor_terms(**kw))


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.RESCALE_B)
@pytest.mark.parametrize('kind', C.RESCALE_KINDS)
def test_small_tile_rescale(ops, flags, B, kind):
    """A tile whose largest gradient 2^(8 + d_exp) is beyond the fp16 range is scaled down as a whole -- at d_exp 0, -3 and the
    engine's pick for the counts, on the direct output form (B = 32) and through the reduce kernels (33: a row tile of one
    row; 128).  Some tile rescales (d_exp 0 and -3) and some tile does not (every d_exp): proven by the CPU half."""
    assert four_wave(B)
    kw = C.rescale_case(flags, B, kind)
    for d_exp in sorted(set(C.RESCALE_D_EXP) | {engine_d_exp(kw['counts'], C.G)}, reverse=True):
        out = run_case(ops, d_exp=d_exp, **kw)
        m, over = held(out, d_exp, kw)
        assert not over.all(), (kind, d_exp)
        if d_exp in C.RESCALE_D_EXP:
            assert over.any(), (kind, d_exp, float(m.max()))


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.ESCAPE_B)
def test_small_escapes_fp32_counts(ops, flags, B):
    """fp32 counts that do not fit the queue's 16-bit slot -- 2.52, 0.5, 0.25, 16.5 (non-integers), 65 535, 65 536, 70 000 and
    1e5 -- are re-read from memory; 65 534 is the largest that fits.  At element (0, 0), at (B - 1, G - 1) and, for B = 33, in
    the lone row of the second row tile."""
    assert four_wave(B)
    kw = C.escape_case(flags, B)
    m, over = held(run_case(ops, **kw), 0, kw)
    assert over.any() and not over.all()


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.ESCAPE_B)
def test_small_escapes_compact(ops, flags, B):
    """The byte store against the ORACLE (tests/test_sparse_gpu.py compares it with the fp32-count path of the same kernel):
    254 is stored, 255, 256, 65 535 and 70 000 are escapes resolved through the overflow list."""
    assert four_wave(B)
    kw = C.compact_case(flags, B)
    m, over = held(run_case(ops, **kw), 0, kw)
    assert over.any() and not over.all()


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B,name', C.HSCALE_CASES)
def test_small_row_tile_scale(ops, flags, B, name):
    """The row tile's scale eHt, which the four-wave kernel takes from the decoder rows its product waves hold: an all-zero
    tile beside three ordinary ones, tiles 2^-40 .. 2^20 apart in one launch, every tile at 2^-23, and on the direct form all
    of H zero (gW exactly 0; gb, dH and the loss as the oracle has them) and H at 2^15.  Counts capped at 40: no tile
    rescales, and check() holds as in test_heads_row_scale_spread -- but for the two launches with a tile at 2^15 / 2^20.
    There the pre-activations are 1e5 .. 1e7, an fp32 forward product is off by 0.1 .. 10, and the few elements of the tile
    that are not saturated move with it: a correctly rounded fp32 forward in front of the fp64 likelihood misses product_tol
    by up to seven orders of magnitude (test_heads_row_scale_spread leaves such a tile out for that reason).  They are held to
        |err| <= product_tol sum|a b| + 2^-(kD0 + 25) sum|b| + add
    per element: D's fp16 floor beside a large H, which product_tol's docstring states as the kernel's contract
    (check_repeat's floor_keys), and add: what the gradient of the oracle itself can change by inside the forward product's
    error box (tests/_heads_small_cases.py::forward_error_terms; proven on the arithmetic model by
    tests/test_x3_arith_cpu.py::test_heads_big_row_tile_forward_bound) -- zero for every output element that sums over no
    unsaturated element of the big tile, which keeps the bound of the other cases."""
    assert four_wave(B)
    kw = C.hscale_case(flags, B, name)
    out = run_case(ops, **kw)
    m, over, _ = tile_scales(out, 0)
    assert (m * 2.0 ** (X.K_DEXP0 - X.K_DSLACK) < X.K_DLIM).all() and not over.any()
    floor = C.disp_floor_terms(**kw)
    if max(kw['hscale']) >= C.BIG_H:
        add = C.forward_error_terms(**kw)[1]
        for k in out['_mag']:
            print('%s: output elements without a forward term: %d of %d' % (k, int((add[k] == 0).sum()), add[k].size))
        # (1.00001: product_tol of the term itself, the gradient the kernel evaluated being up to add away from the oracle's)
        check_repeat(out, 0, floor_keys=tuple(out['_mag']), extra=C.add_terms(floor, {k: 1.00001 * v for k, v in add.items()}))
    else:
        check(out)
    if name == 'all_zero':
        for k in out:
            if k.startswith('gW_'):
                assert (out[k][0] == 0.0).all(), k


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.WSCALE_B)
def test_gene_tile_weight_scale(ops, flags, B):
    """The gene tile's scale eW on both kernels (B = 160: the 8-wave one): two all-zero weight tiles (block_exp(0) = 0: their
    pre-activations are the biases alone, their dH contribution is 0, their gW is not) among tiles 2^-30, 2^-10, 1 and 4 times
    the usual weights."""
    assert four_wave(B) == (B < 160)
    kw = C.wscale_case(flags, B)
    m, over = held(run_case(ops, **kw), 0, kw)
    assert not over.any()


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize('flags', C.CLIP_FLAGS)
@pytest.mark.parametrize('B', C.CLIP_B + [C.TINY[0]])
def test_constant_dispersion_clip(ops, flags, B):
    """ConstantDispersionLayer's clip: g_theta is EXACTLY 0 where exp(theta_w) lies outside [1e-3, 1e4] and the chained sum
    elsewhere, in each of the three places the chain is written (make_heads_plan in dcahip_heads.hip decides):
        B = 32    p.small, NT == 1            the four-wave kernel's own store
        B = 96    p.small, NT == 3 (S = NT)   reduce_dw_body over the four-wave kernel's partials
        B = 160   !p.small, S == 1 (NT = 5)   the 8-wave kernel's direct store
        B = 512   !p.small, S == 2 (NT = 16)  reduce_dw_body over the 8-wave kernel's partials
    and B = 5, G = 6 (Gp = 8): the four-wave store must leave g_theta[G:Gp] alone."""
    kw = C.clip_case(flags, B, C.TINY if B == C.TINY[0] else None)
    out = run_case(ops, **kw)
    check(out)
    got, ref = out['g_theta']
    outside = C.clip_outside(kw['tw'])
    assert outside.any() and (ref[outside] == 0.0).all()
    assert (got[outside] == 0.0).all(), np.flatnonzero(got[outside] != 0.0)[:8].tolist()
    assert (got[~outside] != 0.0).all()
    pad = out['_ref']['theta_pad']
    assert pad.size == (-kw['G']) % 4 and (pad == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize('flags', [1, 3])
@pytest.mark.parametrize('B', [32, 128])
@pytest.mark.parametrize('kind', C.RESCALE_KINDS)
def test_small_kernel_is_deterministic(ops, flags, B, kind):
    """Two launches of case (a), on the direct form and through the reduce kernels: every output bit-equal."""
    kw = C.rescale_case(flags, B, kind)
    a, b = run_case(ops, **kw), run_case(ops, **kw)
    for k in a:
        if k in ('_mag', '_ref'):
            continue
        assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k
