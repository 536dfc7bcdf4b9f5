"""K-HEADS phase order (F -> Z -> dW -> dH, the dH partial requested right after Z): the path that differs from a
first work item is the one where a workgroup's SECOND and later work items start their dH accumulators from the partial
the earlier items left.  That needs more work items than the 256 persistent workgroups (more than 256 gene tiles) and
at least 5 row tiles, so that the 8-wave kernel runs (kWr8MinNT in dcahip_heads.hip).  The smallest such shapes, against
the fp64 reference() and the product_tol of tests/test_heads_fused_gpu.py (imported, not restated).
"""
import numpy as np
import pytest

from conftest import synth_counts
from test_heads_fused_gpu import reference, product_tol, run_case, check

# B, G, hL
SHAPES = [(160, 9632, 64),      # 301 full gene tiles: 45 workgroups read back a partial
          (200, 9620, 64),      # ragged last row tile and ragged last gene tile
          (288, 12000, 32)]     # fewer hidden units than the K tile
FIRST_ROUND_GENES = 256 * 32    # gene tiles the 256 workgroups take as their FIRST work item (identity order)

_runs = {}


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def case(ops, flags, shape):
    """One launch per (flags, shape), shared by the tests that only read it."""
    key = (flags, shape)
    if key not in _runs:
        B, G, hL = shape
        _runs[key] = run_case(ops, flags, B, G, hL, seed=B + G, ridge=0.05 if flags & 1 else 0.0)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize('flags', [1, 0, 3, 2])
@pytest.mark.parametrize('shape', SHAPES)
def test_partial_read_back_vs_oracle(ops, flags, shape):
    check(case(ops, flags, shape))


@pytest.mark.gpu
def test_partial_read_back_with_repeat_path_and_escape(ops):
    """Counts of 200, 5 000, 65 535 and 70 000 in the first row tile: the tile repeats F + Z at a lower scale (nothing of
    dW or dH has started when it decides) and two counts leave the queue's 16 bits.  A repeated tile carries the contract
    product_tol sum|ab| + 2^-(kDe + 25) sum|b| (see product_tol), which check() applies as its edge form."""
    B, G, hL = SHAPES[0]
    check(run_case(ops, 1, B, G, hL, seed=B + G, ridge=0.05, odd_counts=True), edge=True)


@pytest.mark.gpu
def test_two_launches_are_bit_equal(ops):
    B, G, hL = SHAPES[0]
    a = case(ops, 1, SHAPES[0])
    b = run_case(ops, 1, B, G, hL, seed=B + G, ridge=0.05)
    for k in a:
        if k in ('_mag', '_ref'):
            continue
        assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k


@pytest.mark.gpu
def test_permuted_tile_order_gives_bit_equal_weight_gradients(ops):
    """Which workgroup reads back which partial follows the order of the gene tiles; a tile's weight / bias gradients
    do not (each is per gene tile)."""
    B, G, hL = SHAPES[0]
    ntg = (G + 31) // 32
    n_ord = ops.heads_tile_order_len(G)
    a = case(ops, 1, SHAPES[0])
    order = np.r_[np.random.RandomState(4).permutation(ntg), np.arange(ntg, n_ord)]
    b = run_case(ops, 1, B, G, hL, seed=B + G, ridge=0.05, tile_order=order)
    check(b)
    for k in a:
        if k.startswith(('gW_', 'gb_')):
            assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k


@pytest.mark.parametrize('flags', [1, 2])           # (three heads with a conditional dispersion, one head with a constant one)
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_rejects_a_dropped_partial(flags, shape):
    """Negative control (no GPU): a kernel whose later work items did not start from the partial would lose what the
    gene tiles of its earlier items gave to dH.  Against the fp64 reference at these shapes that loss is far beyond
    product_tol in either direction -- the first round's contribution dropped or the later rounds' -- so such a kernel
    cannot pass test_partial_read_back_vs_oracle."""
    B, G, hL = shape
    has_pi, cdisp = bool(flags & 1), bool(flags & 2)
    rng = np.random.RandomState(B + G)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    heads = ['mean'] + ([] if cdisp else ['disp']) + (['pi'] if has_pi else [])
    Hm = f(np.maximum(rng.normal(0.3, 1.0, (B, hL)), 0))
    W = {h: f(rng.normal(0, 0.25, (hL, G))) for h in heads}
    b = {h: f(rng.normal(0, 0.3, G)) for h in heads}
    tw = f(rng.normal(0, 1.5, G))
    y = f(synth_counts(B, G, B + G))
    sf = f(rng.lognormal(0, 0.3, B))
    _, _, _, _, dH, _, mag, D = reference(Hm, W, b, tw, y, sf, flags, 0.05 if has_pi else 0.0, float(B * G))
    assert G > FIRST_ROUND_GENES
    later = sum(D[h][:, FIRST_ROUND_GENES:] @ W[h][:, FIRST_ROUND_GENES:].T for h in heads)
    tol = product_tol('dH', B, G)
    for dropped in (later, dH - later):
        ratio = (np.abs(dropped) / np.maximum(mag['dH'], 1e-300)).max()
        assert ratio > 100 * tol, (float(ratio), tol)
