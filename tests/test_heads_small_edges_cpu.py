"""The reach conditions of the four-wave K-HEADS edge tests (tests/test_heads_small_edges_gpu.py), from the fp64 oracle alone:
for every case of tests/_heads_small_cases.py the inputs reach the branch the GPU half means to test, so that half cannot
pass by missing it.  Conditions on the inputs -- nothing here is measured on a kernel.
"""
import numpy as np
import pytest

import _heads_small_cases as C
from oracle import x3_np as X

tile_scales = C.tile_scales


def finite(o):
    return (np.isfinite(o['loss']) and np.isfinite(o['dH']).all() and all(np.isfinite(v).all() for v in o['gW'].values())
            and all(np.isfinite(v).all() for v in o['gb'].values())
            and (o['g_theta'] is None or np.isfinite(o['g_theta']).all()))


@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.RESCALE_B)
@pytest.mark.parametrize('kind', C.RESCALE_KINDS)
def test_rescale_cases_reach_the_branch_and_the_fast_path(flags, B, kind):
    """(a): at d_exp 0 and -3 some (row tile, gene tile) holds a gradient beyond kDLim 2^-(8 + d_exp) -- with the margin of
    tile_scales, which counts a tile from 0.999 kDLim on, so also one beyond 1.002 kDLim is asked for: the kernel's fp32
    maximum cannot stay below -- and some tile holds none."""
    o = C.oracle_case(**C.rescale_case(flags, B, kind))
    assert finite(o)
    for d_exp in C.RESCALE_D_EXP:
        m, over, _ = tile_scales(o, d_exp)
        assert over.shape == ((B + 31) // 32, 10)
        assert (m * 2.0 ** (X.K_DEXP0 + d_exp) > X.K_DLIM * 1.002).any(), (kind, d_exp, float(m.max()))
        assert over.any() and not over.all(), (kind, d_exp, int(over.sum()))


@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.ESCAPE_B)
@pytest.mark.parametrize('case,escaped', [(C.escape_case, C.escaped_fp32), (C.compact_case, C.escaped_byte)])
def test_escape_cases_place_their_escapes(flags, B, case, escaped):
    """(b), (c): escapes at element (0, 0) and (B - 1, G - 1), in the last, partial gene tile, and for B = 33 in row 32, the
    lone row of the second row tile; every count of the issue's list is there; the largest of them send their tiles through
    the rescale while other tiles stay on the fast path."""
    kw = case(flags, B)
    o = C.oracle_case(**kw)
    y = o['y']
    esc = escaped(y)
    assert esc[0, 0] and esc[B - 1, C.G - 1] and esc[:, C.LAST_TILE:].any()
    assert esc[32 * ((B - 1) // 32):].any()
    if B == 33:
        assert esc[32].sum() >= 3
    want = (254, 255, 256, 65535, 70000) if kw.get('compact') else (2.52, 0.5, 0.25, 16.5, 65534, 65535, 65536, 70000, 1e5)
    assert all((y == float(np.float32(c))).any() for c in want)
    if kw.get('compact'):
        assert (y == np.floor(y)).all() and (y >= 0).all()
    assert finite(o)
    m, over, _ = tile_scales(o, 0)
    assert over.any() and not over.all()


@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B,name', C.HSCALE_CASES)
def test_row_scale_cases(flags, B, name):
    """(d): the fp32-rounded H holds the all-zero tile (and no other zero tile, nor an underflow: every other tile keeps its
    non-zero pattern); no tile rescales; every gradient of the oracle is finite.  With all of H zero the oracle's gW is
    exactly zero while gb, dH and the loss are not."""
    kw = C.hscale_case(flags, B, name)
    o = C.oracle_case(**kw)
    H = o['_ref']['H']
    assert np.array_equal(H, H.astype(np.float32).astype(np.float64))
    H1 = C.oracle_case(**dict(kw, hscale=None))['_ref']['H']
    for t, s in enumerate(kw['hscale']):
        rows = slice(32 * t, 32 * t + 32)
        if s == 0.0:
            assert not H[rows].any()
        else:
            assert np.array_equal(H[rows] != 0, H1[rows] != 0) and np.array_equal(H[rows], H1[rows] * s)
            assert -60 < X.block_exp(H[rows]) < 60                  # inside block_exp's clamp
    assert finite(o)
    m, over, _ = tile_scales(o, 0)
    assert (m * 2.0 ** (X.K_DEXP0 - X.K_DSLACK) < X.K_DLIM).all() and not over.any()
    if name == 'all_zero':
        assert all(not v.any() for v in o['gW'].values())
        assert all(v.any() for v in o['gb'].values()) and o['dH'].any() and o['loss'] > 0


@pytest.mark.parametrize('flags', C.FLAGS)
@pytest.mark.parametrize('B', C.WSCALE_B)
def test_weight_scale_case(flags, B):
    """(e): the fp32-rounded weights hold the two all-zero gene tiles in every head (tile 1 and the partial tile 9), every
    other tile is non-zero and the scales 2^-30, 2^-10, 1 and 4 are all there; the zero tiles' pre-activations are the biases
    alone, so their gW is not zero; no tile rescales; everything finite."""
    kw = C.wscale_case(flags, B)
    assert set(C.WSCALE) == {0.0, 2.0 ** -30, 2.0 ** -10, 1.0, 4.0} and len(C.WSCALE) == 10 and C.WSCALE[9] == 0.0
    o = C.oracle_case(**kw)
    W = o['_ref']['W']
    assert np.array_equal(W, W.astype(np.float32).astype(np.float64))
    W1 = C.oracle_case(**dict(kw, wscale=None))['_ref']['W']
    exps = set()
    for t, s in enumerate(C.WSCALE):
        cols = slice(32 * t, min(C.G, 32 * t + 32))
        if s == 0.0:
            assert not W[:, :, cols].any()
            assert all(o['gW'][h][:, cols].any() and o['gb'][h][cols].any() for h in o['heads'])
        else:
            assert np.array_equal(W[:, :, cols], W1[:, :, cols] * s) and (W[:, :, cols] != 0).all()
            exps.add(X.block_exp(W[:, :, cols]))
    assert max(exps) - min(exps) >= 30                               # tiles of very different magnitude in one launch
    assert finite(o)
    m, over, _ = tile_scales(o, 0)
    assert not over.any()


def test_clip_vector():
    """(f): in the first, an inner and the last gene tile a gene on each side of each clip bound, the first and the last gene
    of the tile among them; nothing nearer than 0.08 to a bound (the whole vector: the N(0, 1.5) draw as well), where fp32
    expf (relative error ~1e-6) and fp64 exp agree on the side."""
    tw = C.clip_tw().astype(np.float32).astype(np.float64)
    out = C.clip_outside(tw)
    assert np.minimum(np.abs(tw - C.CLIP_LO), np.abs(tw - C.CLIP_HI)).min() > 0.08
    for t in C.CLIP_TILES:
        lo, hi = 32 * t, min(C.G, 32 * t + 32)
        seg = tw[lo:hi]
        vals = set(np.float32(C.CLIP_VALUES).astype(np.float64).tolist())
        assert vals <= set(seg.tolist())
        assert (seg < C.CLIP_LO).any() and ((seg > C.CLIP_LO) & (seg < 0)).any()
        assert (seg > C.CLIP_HI).any() and ((seg < C.CLIP_HI) & (seg > 8)).any()
        assert tw[lo] in vals and tw[hi - 1] in vals
    assert out.sum() >= 15 and (~out).sum() >= 250
    tiny = C.clip_tw(C.TINY[1])
    o6 = C.clip_outside(tiny)
    assert o6.tolist() == [True, False, False, True, True, True]


@pytest.mark.parametrize('flags', C.CLIP_FLAGS)
@pytest.mark.parametrize('B', C.CLIP_B + [C.TINY[0]])
def test_clip_case_oracle_gradient(flags, B):
    """(f): the oracle's g_theta is exactly 0 on every gene outside the clip and non-zero on every gene inside it."""
    kw = C.clip_case(flags, B, C.TINY if B == C.TINY[0] else None)
    o = C.oracle_case(**kw)
    out = C.clip_outside(o['tw'])
    assert finite(o)
    assert (o['g_theta'][out] == 0.0).all() and (o['g_theta'][~out] != 0.0).all()
    assert out.any() and (~out).any()
