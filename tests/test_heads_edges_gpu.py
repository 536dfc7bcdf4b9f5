"""K-HEADS' rare branches against the fp64 oracle at the strict per-element bounds of tests/test_heads_fused_gpu.py: the
repeat path of the 8-wave persistent kernel (a tile whose scaled gradient would leave the fp16 range is re-run at a lower
exponent kDe), the count escapes (fp32 counts that do not fit the 16-bit queue slot, compact bytes 255 through the overflow
list), row tiles of different magnitude inside one wave, and the argument checks of d_exp and ridge.

The repeat path scales a whole 32 x 32 tile by what its largest gradient needs, so an output element that sums over such a
tile is held to product_tol plus the floor of D's second fp16 piece at 2^kDe (oracle/x3_np.py::repeat_floor,
tests/test_x3_arith_cpu.py::test_heads_repeat_path_bound); every other element to product_tol alone.
"""
import types

import numpy as np
import pytest
import torch

from conftest import synth_counts
from oracle import x3_np as X
from test_heads_fused_gpu import check, ops, product_tol, run_case      # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def heads_plan(B, G):
    """make_heads_plan (dcahip_heads.hip) restated for the 8-wave kernel: batch splits S and, with a tail launch, S2."""
    NT, ngb, WR, cus, kmax = (B + 31) // 32, (G + 31) // 32, 8, 256, 2048
    assert NT >= 5
    smax = (NT + WR - 1) // WR
    best, S = 1e300, 1
    for s in range(1, smax + 1):
        if s * ngb > kmax:
            break
        cost = ((s * ngb + cus - 1) // cus) * ((NT + s * WR - 1) // (s * WR) + 0.75)
        if cost < best - 1e-9:
            best, S = cost, s
    npart = min(S * ngb, cus // S * S) // S
    return NT, S, npart


def tiles_per_wave(B, G):
    NT, S, _ = heads_plan(B, G)
    return NT // (S * 8)


def tile_scales(out, d_exp):
    """From the oracle's gradient: the largest |g| (unscaled: D n_total) of every (row tile, gene tile) over the product
    planes, which tiles may take the repeat path (max |g| 2^(8 + d_exp) > kDLim, within the fp32 / fp64 margin), and the
    lowest exponent kDe each may end at (the repeat step lands at 13 - floor(log2 max|g|); otherwise kD0 - K_DSLACK)."""
    r = out['_ref']
    g = np.abs(np.stack(r['D'])) * r['n_total']
    B, G = g.shape[1], g.shape[2]
    NT, ntg = (B + 31) // 32, (G + 31) // 32
    gp = np.zeros((g.shape[0], NT * 32, ntg * 32)); gp[:, :B, :G] = g
    m = gp.reshape(g.shape[0], NT, 32, ntg, 32).max(axis=(0, 2, 4))
    kd0 = X.K_DEXP0 + d_exp
    over = m * 2.0 ** kd0 > X.K_DLIM * 0.999
    with np.errstate(divide='ignore'):
        kde_rep = 13 - np.floor(np.log2(np.maximum(m * 1.001, 1e-300))).astype(int)
    kde = np.where(over, np.minimum(kd0 - X.K_DSLACK, kde_rep), kd0 - X.K_DSLACK)
    return m, over, kde


def check_repeat(out, d_exp, floor_keys=(), extra=None):
    """check() without the product bound, then per element: product_tol where no tile of its sum may have repeated, the
    repeat path's derived bound (product_tol sum|ab| + 2^-(kDe + 25) sum|b|, in loss units: / n_total) where one may.  Below
    d_exp = -3 (kD0 < 5) and for floor_keys the derived bound holds for every element: D's fp16 floor 2^-(kD0 + 25) is then
    beyond what product_tol leaves for the smallest gradients.  extra: as in check() (an absolute term beside either bound)."""
    if d_exp < -3:
        floor_keys = tuple(out['_mag'])
    mag = out['_mag']
    extra = extra or {}
    check({k: v for k, v in out.items() if k != '_mag'}, extra=extra)
    m, over, kde = tile_scales(out, d_exp)
    r = out['_ref']
    rows, genes = out['dH'][0].shape[0], out['gW_mean'][0].shape[1]
    fw, fh = X.repeat_floor(kde, np.pad(r['H'], ((0, kde.shape[0] * 32 - rows), (0, 0))), r['W'])
    fw, fh = fw / r['n_total'], fh[:rows] / r['n_total']
    col_over = np.repeat(over.any(0), 32)[:genes]              # dW[:, gene]: a sum over every row tile of the gene's tile
    row_over = np.repeat(over.any(1), 32)[:rows]               # dH[row, :]: a sum over every gene tile of the row's tile
    worst = {}
    for k in mag:
        g, ref = out[k]
        err = np.abs(g - ref)
        x = extra.get(k, 0.0)
        tol = product_tol(k, rows, genes)
        strict_mask = ~row_over[:, None] if k == 'dH' else ~col_over[None, :]
        if k in floor_keys:
            strict_mask = np.zeros_like(strict_mask)
        strict = np.where(strict_mask, np.maximum(err - x, 0.0) / np.maximum(mag[k], 1e-300), 0.0).max()
        assert strict <= tol, (k, 'no repeated tile in the sum', float(strict), tol)
        floor = fh if k == 'dH' else fw
        derived = np.where(strict_mask, 0.0, err / (tol * mag[k] + floor + x)).max()
        assert derived <= 1.0, (k, 'repeat path: err / derived bound', float(derived))
        worst[k] = (float(strict), float(derived))
    print('repeat check: tiles over %d of %d; per key (strict err/sum|ab|, repeated err/derived bound): %s'
          % (int(over.sum()), over.size, worst))
    return m, over


def engine_d_exp(y, G):
    """Engine._heads_d_exp on these counts (its rule: the count one element in 20 000 exceeds)."""
    from dca_amd.engine import Engine
    fake = types.SimpleNamespace(Y=torch.as_tensor(y, dtype=torch.float32).cuda(), lay=types.SimpleNamespace(G_out=G))
    return Engine._heads_d_exp(fake)


def repeat_counts(kind, B, G, seed):
    rng = np.random.RandomState(seed)
    if kind == 'around400':
        # counts around 400 throughout, the last gene tile lowly expressed
        y = rng.poisson(400.0 * rng.lognormal(0, 0.25, G)[None, :] * rng.lognormal(0, 0.2, B)[:, None]).astype(np.float64)
        y[:, G - 32:] = synth_counts(B, 32, seed)
        y *= rng.uniform(size=(B, G)) >= 0.05
        return y
    y = synth_counts(B, G, seed)
    low = np.argsort(y.mean(0))[:8]                             # sparse outliers beside the lowest-expressed genes
    for i, c in enumerate((200, 5000, 65534, 65535, 70000)):
        y[(37 * i + 5) % B, low[i]] = c
    y[B - 1, low[5]] = 70000
    return y


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
@pytest.mark.parametrize('B', [160, 512])
@pytest.mark.parametrize('kind', ['around400', 'outliers'])
def test_heads_repeat_path_8wave(ops, flags, B, kind):
    """The repeat path on the persistent kernel (B >= 160), at d_exp 0, -3 and the engine's pick for the counts.  The host
    proves from the oracle's gradient that the path is reached (some tile's max |g| 2^(8 + d_exp) beyond kDLim) and that
    some tile stays on the fast path."""
    G = 300
    y = repeat_counts(kind, B, G, B + flags)
    d_eng = engine_d_exp(y, G)
    assert d_eng < 0                                            # both count sets reach the engine's lower start
    for d_exp in sorted({0, -3, d_eng}, reverse=True):
        out = run_case(ops, flags, B, G, 64, seed=B + G + flags, ridge=0.05 if flags & 1 else 0.0, counts=y, d_exp=d_exp)
        m, over = check_repeat(out, d_exp)
        assert not over.all(), (kind, d_exp)
        if d_exp in (0, -3):                                    # (the engine's pick is there to keep tiles off the path)
            assert over.any(), (kind, d_exp, float(m.max()))


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
def test_heads_escapes_8wave_fp32_counts(ops, flags):
    """fp32 counts on the persistent kernel: non-integer values (libm lgamma route) and counts >= 65 535, which do not fit
    the queue's 16-bit slot and are re-read from memory -- against the oracle at the strict bounds."""
    B, G = 192, 300
    y = synth_counts(B, G, 17)
    y[0, :6] = [2.52, 0.5, 17.0, 70000.0, 200.0, 5000.0]
    y[1, 1:4] = [16.0, 16.5, 65535.0]
    y[100, 40:44] = [65534.0, 65535.0, 65536.0, 0.25]
    y[191, 299] = 1e5
    out = run_case(ops, flags, B, G, 64, seed=23 + flags, ridge=0.05 if flags & 1 else 0.0, counts=y)
    m, over = check_repeat(out, 0)
    assert over.any() and not over.all()


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
def test_heads_escapes_8wave_compact(ops, flags):
    """The byte store on the persistent kernel: 254 (stored), 255 and 256 (escapes), counts >= 65 535 through the overflow
    list -- against the oracle (tests/test_sparse_gpu.py compares the two count paths with each other)."""
    B, G = 224, 300
    y = synth_counts(B, G, 19)
    y[0, :5] = [254, 255, 256, 65535, 70000]
    y[3, 31:34] = [255, 254, 256]
    y[200, 0] = 65534; y[223, 299] = 255; y[100, 150] = 1000
    out = run_case(ops, flags, B, G, 64, seed=29 + flags, counts=y, compact=True)
    m, over = check_repeat(out, 0)
    assert over.any() and not over.all()


SPREADS = {
    'mod23': lambda NT: [2.0 ** -((5 * t) % 23) for t in range(NT)],
    'zero_tile': lambda NT: [0.0 if t == 0 else 1.0 for t in range(NT)],
    'tile_2^-20': lambda NT: [2.0 ** -20 if t == 1 else 1.0 for t in range(NT)],
}


@pytest.mark.parametrize('spread', list(SPREADS))
@pytest.mark.parametrize('B,G', [(2048, 2000), (4096, 2000), (2048, 16500)])
def test_heads_row_scale_spread(ops, B, G, spread):
    """Row tiles of different magnitude inside one wave (every wave holds at least two: B = 2 048 / 4 096 at G = 2 000 give
    S = 4, two / four tiles per wave; 2 048 x 16 500 has a tail launch): an all-zero tile, a tile 2^-20 below its siblings,
    and a spread of up to 22 bits in every wave.  Counts stay below the repeat path, so product_tol holds for every element.
    (Not here: a tile at 2^16, whose exponent would be negative.  Its pre-activations saturate the heads, its gradients fall
    under D's fp16 floor 2^-(kD0 + 25), and 2^16 H multiplies what they lose: dW misses even check()'s 2e-4.)"""
    import os
    assert tiles_per_wave(B, G) >= 2
    NT = B // 32
    y = np.minimum(synth_counts(B, G, B + G), 40.0)
    flags = 1
    out = run_case(ops, flags, B, G, 64, seed=31, ridge=0.02, counts=y, hscale=SPREADS[spread](NT),
                   threads=max(1, min(16, os.cpu_count() or 1)))
    m, over, _ = tile_scales(out, 0)
    assert (m * 2.0 ** (X.K_DEXP0 - X.K_DSLACK) < X.K_DLIM).all() and not over.any()
    check(out)


@pytest.mark.parametrize('d_exp,ridge', [(1, 0.0), (-25, 0.0), (0, -1.0), (0, 2e3), (0, float('nan'))])
def test_heads_fused_rejects_d_exp_and_ridge_out_of_range(ops, d_exp, ridge):
    """dcahip_heads_fused: d_exp in [-24, 0], ridge in [0, 1e3] (EINVAL otherwise: nothing is launched)."""
    with pytest.raises(RuntimeError, match='heads_fused'):
        run_case(ops, 1, 192, 40, 64, seed=1, ridge=ridge, d_exp=d_exp)
