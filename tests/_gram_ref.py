"""The fp64 reference of the gene cross-products (dcahip_gram / Engine.gene_gram / Autoencoder.gene_correlation): the contract
of include/dcahip.h evaluated by numpy, the derived error bound, the launch plan restated from the comment above
gram_kernel (dca_amd/csrc/dcahip_gram.hip), the operands of the kernel tests (shared by the CPU and the GPU file), and
GramRefOps, the CPU oracle with the one entry it lacks, so that the Python layers above the kernel run in the CPU suite.

The bound.  d = fl(x - shift) carries one rounding (x is fp32, exact in double), a product of two of them a third, and an
m-term sum in ANY order at most m - 1 more per term: |sum - exact| <= gamma_(m+2) sum |d_i| |d_j|, held here at
    E_ij = (m + 4) 2^-53 sum_r |d_ri| |d_rj|,       m = the number of kept rows
(the standard bound of a double dot product, a little to spare; a fused multiply-add only removes roundings).  dsum is the
same with the second operand 1.  The accumulators are ADDED to: one more rounding at the accumulator's own magnitude, half
an ulp of the stored double (acc_half_ulp), as tests/test_groups_gpu.py counts it."""
import numpy as np
import torch

from oracle.cpu_ops import CpuRefOps, _mat, _vec

U = 2.0 ** -53
MAX_G = 8192
# (B, G) at the edges of the 64-gene tile, of the instruction's depth of 4 rows and of the staging depth of 32 rows
SHAPES = [(1, 1), (3, 5), (4, 16), (5, 17), (33, 63), (37, 65), (70, 130), (300, 200)]


# ---------------------------------------------------------------------------------------------------- the launch plan
def _up32(v):
    return -(-v // 32) * 32


def plan(B, G, cols=True):
    """The launch plan as the comment above gram_kernel states it, for B >= 1 rows: dict(T, NT, capmax, rows_max, blocks --
    the rows of every row block --, slices -- (cap, rows_per, S) of every row block --, S -- of the first row block --,
    part -- the doubles of the partial tiles the largest row block needs --, ws -- the workspace query)."""
    T = -(-G // 64)
    Gp, NT = 64 * T, T * (T + 1) // 2
    capmax = 1 if NT >= 1024 else min(64, (1024 + NT // 2) // NT)

    def part(c):
        return c * (NT * 4096 + T * 64) if c > 1 else 0
    rows_max = ((64 << 20) - 8 * part(capmax)) // (4 * Gp) // 32 * 32
    n = -(-B // rows_max) if cols else 1
    rows_blk = _up32(-(-B // n)) if cols else B
    blocks = [min(rows_blk, B - r0) for r0 in range(0, B, rows_blk)]
    slices = []
    for b in blocks:
        cap = min(capmax, -(-b // 32))
        rows_per = _up32(-(-b // cap))
        slices.append((cap, rows_per, -(-b // rows_per)))
    bq = min(_up32(B), rows_max)
    return dict(T=T, NT=NT, capmax=capmax, rows_max=rows_max, blocks=blocks, slices=slices, S=slices[0][2],
                part=part(slices[0][0]), ws=part(min(capmax, bq // 32)) + bq * Gp // 2)


def boundary_shapes(B=70):
    """One shape on each side of the single-slice / multi-slice boundary of the plan: the widest G whose triangle has fewer
    tiles than the chip takes workgroups (more than one slice for B > 32) and the next gene (one slice)."""
    T = 1
    while plan(B, 64 * (T + 1))['capmax'] > 1:
        T += 1
    multi, single = (B, 64 * T), (B, 64 * T + 1)
    assert plan(*multi)['S'] > 1 and plan(*single)['S'] == 1
    return multi, single


# ---------------------------------------------------------------------------------------------------- the contract
def gram_ref(x, cols, keep, shift):
    """(cross [G, G], dsum [G], absprod [G, G], absd [G], m) in float64: the contract over the kept rows of x (fp32 [B, W]),
    rows added in ascending order; absprod = sum |d_i| |d_j| and absd = sum |d| scale the bounds."""
    x = np.asarray(x, np.float32)
    cols = np.arange(len(shift)) if cols is None else np.asarray(cols)
    rows = np.arange(x.shape[0]) if keep is None else np.flatnonzero(np.asarray(keep) != 0)
    g = len(cols)
    cross, dsum, absprod, absd = np.zeros((g, g)), np.zeros(g), np.zeros((g, g)), np.zeros(g)
    for r in rows:
        d = x[r, cols].astype(np.float64) - np.asarray(shift, np.float64)
        cross += np.outer(d, d)
        dsum += d
        absprod += np.outer(np.abs(d), np.abs(d))
        absd += np.abs(d)
    return cross, dsum, absprod, absd, len(rows)


def gram_ref_fast(x, cols, keep, shift):
    """gram_ref by matrix products (another order of the same sums: for the wide shapes, where a row loop is slow)."""
    x = np.asarray(x, np.float32)
    cols = np.arange(len(shift)) if cols is None else np.asarray(cols)
    rows = np.arange(x.shape[0]) if keep is None else np.flatnonzero(np.asarray(keep) != 0)
    d = x[np.ix_(rows, cols)].astype(np.float64) - np.asarray(shift, np.float64)[None, :]
    a = np.abs(d)
    return d.T @ d, d.sum(axis=0), a.T @ a, a.sum(axis=0), len(rows)


def bound(absprod, m):
    return (m + 4) * U * absprod


def acc_half_ulp(acc):
    """Half an ulp of every stored double (0 for 0)."""
    a = np.abs(np.asarray(acc, np.float64))
    out = np.zeros_like(a)
    nz = a > 0
    out[nz] = U * 2.0 ** np.floor(np.log2(a[nz]))
    return out


# ---------------------------------------------------------------------------------------------------- operands
VARIANTS = ('plain', 'cols', 'keep10', 'keepnone')
_cases = {}


def case(shape, variant='plain'):
    """Operands of one call and their reference, made once per (shape, variant): uniform fp32 in [0.5, 2], gene 0 constant,
    gene 1 with a coefficient of variation of 1e-4, the shift = the fp64 column mean.
      plain     ldx = G + 3, every row, every column
      cols      the G genes are a shuffled subset of a matrix 37 columns wider
      keep10    a tenth of the rows out (rows 3, 13, ..), their values NaN
      keepnone  every row out, all values NaN"""
    key = (shape, variant)
    if key in _cases:
        return _cases[key]
    B, G = shape
    rng = np.random.default_rng(100003 * B + G)
    W = G + 37 if variant == 'cols' else G
    x = rng.uniform(0.5, 2.0, size=(B, W)).astype(np.float32)
    cols = rng.permutation(W)[:G].astype(np.int32) if variant == 'cols' else None
    at = cols if cols is not None else np.arange(G)
    x[:, at[0]] = np.float32(1.25)
    if G > 1:
        x[:, at[1]] = (1.5 * (1.0 + 1e-4 * rng.standard_normal(B))).astype(np.float32)
    keep = None
    if variant == 'keep10':
        keep = np.ones(B, np.int32)
        keep[3::10] = 0
    elif variant == 'keepnone':
        keep = np.zeros(B, np.int32)
    shift = x[:, at].astype(np.float64).mean(axis=0)
    ref = (gram_ref if B * G * G <= 4e6 else gram_ref_fast)(x, cols, keep, shift)
    if keep is not None:
        x[keep == 0] = np.nan                           # after the reference: a row that is out is never used
    _cases[key] = dict(x=x, ldx=W + 3, cols=cols, keep=keep, shift=shift, cross=ref[0], dsum=ref[1], absprod=ref[2],
                       absd=ref[3], m=ref[4])
    return _cases[key]


def int_case(shape):
    """Integer-valued operands: fp32 integers in [-64, 64] in a matrix 5 columns wider, shuffled cols, integer shifts in
    [-8, 8], rows 2, 9, .. out.  |d| <= 72 and every sum stays far below 2^53: the int64 result is exact in double."""
    B, G = shape
    rng = np.random.default_rng(7 * B + 13 * G)
    W = G + 5
    x = rng.integers(-64, 65, size=(B, W)).astype(np.float32)
    cols = rng.permutation(W)[:G].astype(np.int32)
    shift = rng.integers(-8, 9, size=G).astype(np.float64)
    keep = np.ones(B, np.int32)
    keep[2::7] = 0
    d = (x[:, cols].astype(np.int64) - shift.astype(np.int64)[None, :])[keep != 0]
    if B * G * G <= 1e8:
        cross = d.T @ d                                 # int64
    else:                                               # integers below 2^53: a float64 product is exact in any order
        cross = d.astype(np.float64).T @ d.astype(np.float64)
        assert B * 72 * 72 < 2 ** 53
    return dict(x=x, ldx=W, cols=cols, keep=keep, shift=shift, cross=cross, dsum=d.sum(axis=0))


def row_block_shape():
    """The narrowest shape that the plan cuts into more than one row block: the widest G with two slices (the partial tiles
    leave the least room for the gathered image) and one row more than fits."""
    G = boundary_shapes()[0][1]
    shape = (plan(1, G)['rows_max'] + 1, G)
    assert len(plan(*shape)['blocks']) == 2
    return shape


# ---------------------------------------------------------------------------------------------------- CPU oracle
class GramRefOps(CpuRefOps):
    """CpuRefOps + gram (include/dcahip.h) in numpy fp64."""
    name = 'cpu-oracle-gram'

    def gram_workspace_doubles(self, B, G):
        assert 1 <= G <= MAX_G
        return plan(B, G)['ws'] if B > 0 else 0

    def gram(self, x, ldx, cols, keep, shift, B, G, cross, ldc, dsum, ws):
        assert 1 <= G <= MAX_G and ldc >= G and ldx >= 1
        if B == 0:
            return
        c = np.arange(G) if cols is None else _vec(cols, G).astype(np.int64)
        xm = _mat(x, B, int(c.max()) + 1, ldx)
        k = None if keep is None else _vec(keep, B)
        cr, ds, _, _, _ = gram_ref_fast(xm, c, k, _vec(shift, G))
        _mat(cross, G, G, ldc)[:] += cr
        _vec(dsum, G)[:] += ds


def to_int_tensor(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
