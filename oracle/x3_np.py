"""TEST INFRASTRUCTURE ONLY (see oracle/__init__.py): numpy restatement of the arithmetic the HIP kernels use for an
fp32-accurate matrix product on the 16-bit matrix pipe.  Two forms:

  bf16 x 3 (the first-layer kernels and the plane GEMMs; K-HEADS until round 5): every fp32 operand as three bf16 pieces
  (round-to-nearest-even residuals, `split_pair` in dca_amd/csrc/dcahip_sparse.hip / dcahip_gemm.hip), SIX piece products
  a1b1 a1b2 a2b1 a1b3 a2b2 a3b1 (`MFMA_X3`), each exact in fp32 (8 x 8 mantissa bits), accumulated in fp32;

  fp16 x 2 (K-HEADS from round 6, dca_amd/csrc/dcahip_heads.hip): every operand BLOCK scaled by the power of two that brings
  its largest magnitude into [2^13, 2^14), then two fp16 pieces x 2^e = h1 + h2 (round to nearest; 2^-22 relative, or 2^-25
  absolute where h2 is an fp16 denormal, which the matrix pipe preserves), THREE piece products a1b1 + a1b2 + a2b1 (`MFMA_H3`;
  the dropped a2b2 is 2^-22 of a product), accumulated in fp32, the scales taken out at the end (exact).

Replaces nothing of the reference: it states what "matrix products: fp32 results as split 16-bit products" (DESIGN.md
section 7) means, so that the bounds the GPU parity tests hold the kernels to (tests/test_heads_fused_gpu.py::product_tol,
tests/test_sparse_gpu.py) can be checked on the CPU against fp64, together with the reason narrower builds must fail them.
"""
import numpy as np


def bf16_round(x):
    """fp32 -> nearest bf16 (ties to even), returned as fp32 (v_cvt_pk_bf16_f32)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def split3(x):
    """x = p0 + p1 + p2 up to 2^-24 |x|: three bf16 pieces of an fp32 array."""
    x = np.asarray(x, np.float32)
    p0 = bf16_round(x)
    r = (x - p0).astype(np.float32)
    p1 = bf16_round(r)
    p2 = bf16_round((r - p1).astype(np.float32))
    return p0, p1, p2


def matmul_x3(a, b, products=6):
    """a [M, K] @ b [K, N] as the kernels compute it: piece products accumulated in fp32, small terms first."""
    A, B = split3(a), split3(b)
    terms = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]          # (piece of a, piece of b): MFMA_X3's order
    if products == 3:
        terms = [(1, 0), (0, 1), (0, 0)]
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for i, j in terms:
        # a bf16 x bf16 product is exact in fp32; the sum over K runs in fp32 (the MFMA's accumulator)
        acc = (acc + (A[i].astype(np.float32) @ B[j].astype(np.float32)).astype(np.float32)).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------------------- fp16 x 2
def block_exp(x, top=13):
    """The exponent e with max|x| 2^e in [2^top, 2^(top + 1)); 0 for an all-zero block (block_exp in dcahip_heads.hip)."""
    m = float(np.abs(np.asarray(x, np.float32)).max()) if np.size(x) else 0.0
    if not (m > 0.0) or not np.isfinite(m):
        return 0
    return int(np.clip(top + 1 - np.frexp(m)[1], -60, 60))


def split2(x, e=0):
    """x 2^e = h1 + h2: two fp16 pieces (round to nearest even, denormals kept), returned as fp32 arrays."""
    xs = np.ldexp(np.asarray(x, np.float32), e).astype(np.float32)
    h1 = xs.astype(np.float16)
    r = (xs - h1.astype(np.float32)).astype(np.float32)           # exact: |xs - h1| <= 2^-11 |xs|
    h2 = r.astype(np.float16)
    return h1.astype(np.float32), h2.astype(np.float32)


def matmul_h2(a, b, products=3, ea=None, eb=None):
    """a [M, K] @ b [K, N] as K-HEADS computes it: block scales, two fp16 pieces per operand, the piece products accumulated
    in fp32 (small terms first), the scales taken out.  products = 2 drops a2 b1 (what a narrower build would do)."""
    ea = block_exp(a) if ea is None else ea
    eb = block_exp(b) if eb is None else eb
    A, B = split2(a, ea), split2(b, eb)
    terms = [(1, 0), (0, 1), (0, 0)][3 - products:]
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for i, j in terms:
        acc = (acc + (A[i] @ B[j]).astype(np.float32)).astype(np.float32)
    return np.ldexp(acc.astype(np.float64), -(ea + eb))


# ---------------------------------------------------------------------------------------- K-HEADS' scale rule, one wave
K_DEXP0 = 8             # kDExp0: D = g 2^(8 + d_exp)
K_DLIM = 30000.0        # kDLim: a scaled |D| beyond this repeats the tile at a lower exponent
K_DSLACK = 2            # kDSlack: D's scale may sit this many bits below kD0 to spare the dW accumulators a move


def _h3(a, b):
    """sum of the three piece products a2 b1 + a1 b2 + a1 b1 (MFMA_H3's order) accumulated in fp32."""
    acc = np.zeros((a[0].shape[0], b[0].shape[1]), np.float32)
    for i, j in ((1, 0), (0, 1), (0, 0)):
        acc = (acc + (a[i] @ b[j]).astype(np.float32)).astype(np.float32)
    return acc


def repeat_exponent(dmax, kd):
    """The exponent a tile's D ends at from the start kd: the repeat step of heads_fused_h2_kernel (dmax = max |g| of the tile,
    over the matrix-product planes)."""
    kde = kd
    while float(np.float32(dmax) * np.float32(2.0 ** kde)) > K_DLIM and kde >= kd - 200:
        need = np.frexp(float(np.float32(dmax) * np.float32(2.0 ** kde)))[1] - 1 - 13
        if need <= 0:
            break
        kde -= min(need, 100)
    return kde


def heads_wave(Ht, g, W, d_exp=0, rule='fixed'):
    """What ONE wave of the persistent K-HEADS kernel computes for its row tiles over every gene tile: dW = H^T g and the rows
    of dH = g W^T that belong to it, in g units (the unscaled gradient: no 1 / n).
      Ht [T, 32, K]: the wave's row tiles (H), in the order the wave takes them;  g [NH, 32 T, G]: the unscaled gradient of
      each matrix-product head;  W [NH, K, G]: the head weights.
    rule 'fixed': D's scale kD in [kD0 - K_DSLACK, kD0] (kD = accE - eH where that lies in the window, else kD0), the dW
      accumulators moved to 2^(eH + kDe) where a tile needs it, an all-zero tile moving nothing;
    rule 'parent': kD = kD0 - (eH - min eH), the accumulators at 2^(min eH + kD0), an all-zero tile counted with eH = 0.
    Returns eH [T], kD and kDe [T, gene tiles] (kDe < kD: the tile took the repeat path), dW [NH, K, G], dH [32 T, K]."""
    Ht = np.asarray(Ht, np.float32); g = np.asarray(g, np.float32); W = np.asarray(W, np.float32)
    T, NH, K, G = Ht.shape[0], g.shape[0], W.shape[1], W.shape[2]
    ntg = (G + 31) // 32
    kd0 = K_DEXP0 + d_exp
    zero = [not np.any(Ht[t]) for t in range(T)]
    eH = [block_exp(Ht[t]) for t in range(T)]
    nz = [e for e, z in zip(eH, zero) if not z] if rule == 'fixed' else eH
    ehmin = min(nz) if nz else 0
    Hp = [split2(Ht[t].T.copy(), eH[t]) for t in range(T)]
    kD = np.zeros((T, ntg), int); kDe = np.zeros((T, ntg), int)
    dW = np.zeros((NH, K, G)); dH = np.zeros((32 * T, K))
    for j in range(ntg):
        gs = slice(32 * j, min(G, 32 * j + 32))
        eW = block_exp(W[:, :, gs])
        Wp = [split2(W[h][:, gs].T.copy(), eW) for h in range(NH)]          # [genes, K]: the B operand of dH
        acc = np.zeros((NH, K, gs.stop - gs.start), np.float32)
        accE = ehmin + kd0
        for t in range(T):
            gt = g[:, 32 * t:32 * t + 32, gs]
            if rule == 'fixed':
                kda = accE - eH[t]
                kdt = kda if (not zero[t] and kd0 - K_DSLACK <= kda <= kd0) else kd0
            else:
                kdt = kd0 - (eH[t] - ehmin)
            kde = repeat_exponent(np.abs(gt).max(), kdt)
            kD[t, j], kDe[t, j] = kdt, kde
            Dp = [split2(gt[h], kde) for h in range(NH)]
            dH[32 * t:32 * t + 32] += np.ldexp(sum(_h3(Dp[h], Wp[h]).astype(np.float64) for h in range(NH)), -(kde + eW))
            if rule == 'fixed':
                if not zero[t] and accE != eH[t] + kde:
                    acc = np.ldexp(acc, eH[t] + kde - accE).astype(np.float32)
                    accE = eH[t] + kde
            elif kde != kdt:
                acc = np.ldexp(acc, kde - kdt).astype(np.float32)
            for h in range(NH):
                acc[h] = (acc[h] + _h3(Hp[t], Dp[h])).astype(np.float32)
            if rule == 'parent' and kde != kdt:
                acc = np.ldexp(acc, kdt - kde).astype(np.float32)
        dW[:, :, gs] = np.ldexp(acc.astype(np.float64), -accE)
    return dict(eH=np.array(eH), kD=kD, kDe=kDe, dW=dW, dH=dH)


def repeat_floor(kDe, H, W):
    """The absolute term of the repeat path's bound, in g units: D's second fp16 piece rounds to 2^-25 at D's scale 2^kDe,
    so an element of a product that sums over tiles carried at 2^kDe gains at most 2^-(kDe + 25) sum |b| from them beyond the
    fp32 dot-product term (b: the other operand).  kDe [row tiles, gene tiles]; H [32 T, K]; W [NH, K, G].
    Returns (dW floor [K, G] -- the same for every head, dH floor [32 T, K])."""
    T, ntg = kDe.shape
    G = W.shape[2]
    f = np.ldexp(1.0, -(np.asarray(kDe) + 25))                                        # [T, ntg]
    Ha = np.abs(np.asarray(H, np.float64)).reshape(T, 32, -1).sum(1)                  # [T, K]: sum over a tile's rows
    col = np.minimum(np.arange(G) // 32, ntg - 1)
    fw = Ha.T @ f                                                                     # [K, ntg]
    Wa = np.abs(np.asarray(W, np.float64)).sum(0)                                     # [K, G] over heads
    Wt = np.stack([Wa[:, 32 * j:32 * j + 32].sum(1) for j in range(ntg)], 1)         # [K, ntg]
    fh = f @ Wt.T                                                                     # [T, K]
    return fw[:, col], np.repeat(fh, 32, axis=0)


# ------------------------------------------------------------------ K-HEADS' dispersion gradient of a y > 0 element in fp32
# d nll / d theta of the NB case (dca/loss.py:87-88) as the kernels sum it (zinb_nz_elem / nll_elem in zinb_math.hpp):
#     dth = -dpsi + l1p + (y tp - theta mu) / (tp (tp + mu)),   dpsi = psi(y + tp) - psi(tp),  l1p = log1p(mu / tp).
# Each term is good to a few ulp of ITSELF; where mu << theta the first and the last cancel (dth ~ -mu / theta^2 for y = 1),
# and what is left carries the terms' absolute error.  Roundings, in units of 2^-23 of the term: dpsi 1.5 (reciprocals of
# 1 ulp, their sum), l1p 3 (v_log_f32, the ln 2 product, the compensation), the last 3.5 (two products, their difference,
# two reciprocals of 1 ulp, two products) -- 4 each bounds them all, the two additions included.
DTH_ULPS = 4.0
D_ELEM_REL = 3e-6       # what tests/test_heads_fused_gpu.py::product_tol carries for the fp32 likelihood arithmetic of one element

EPS_NB = 1e-10          # dca/loss.py:65


def dth_terms(mu, theta, y):
    """(dpsi, l1p, last) of dth in fp64, element-wise."""
    from scipy.special import digamma
    tp = theta + EPS_NB
    return digamma(y + tp) - digamma(tp), np.log1p(mu / tp), (y * tp - theta * mu) / (tp * (tp + mu))


def disp_grad_floor(mu, theta, gd, y, d_disp):
    """What the fp32 evaluation of g_disp = dth gd (the unscaled gradient of the dispersion head's pre-activation) may be off
    by BEYOND the D_ELEM_REL |g_disp| that product_tol carries: max(0, DTH_ULPS 2^-23 (dpsi + |l1p| + (y tp + theta mu) /
    (tp (tp + mu))) gd - D_ELEM_REL |g_disp|), for y > 0; zero for y = 0 (its own formula, a series where it would cancel).
    Non-zero only where the sum has lost about three decimal digits to cancellation."""
    tp = theta + EPS_NB
    dpsi, l1p, _ = dth_terms(mu, theta, y)
    terms = dpsi + np.abs(l1p) + (y * tp + theta * mu) / (tp * (tp + mu))
    eps = DTH_ULPS * 2.0 ** -23 * terms * np.abs(gd)
    return np.where(y > 0, np.maximum(eps - D_ELEM_REL * np.abs(d_disp), 0.0), 0.0)


def dth_fp32(mu, theta, y):
    """dth of an integer count 1 <= y <= 16 summed as zinb_nz_elem does, every operation rounded to fp32 (correctly rounded:
    the kernel's reciprocal and logarithm are good to 1 ulp, so this is the favourable end of what the kernel may return)."""
    f = np.float32
    mu, theta, y = f(mu), f(theta), f(y)
    tp = (theta + f(EPS_NB)).astype(f)
    rtp, rtm = (f(1) / tp).astype(f), (f(1) / (tp + mu).astype(f)).astype(f)
    x = (mu * rtp).astype(f)
    u = (f(1) + x).astype(f)
    l1p = ((x - (u - f(1)).astype(f)).astype(f) * (tp * rtm).astype(f) + np.log(u.astype(np.float64)).astype(f)).astype(f)
    dpsi = np.zeros_like(tp)
    for i in range(16):
        dpsi = np.where(i < y, (dpsi + (f(1) / (tp + f(i)).astype(f)).astype(f)).astype(f), dpsi)
    num = ((y * tp).astype(f) - (theta * mu).astype(f)).astype(f)
    last = ((num * rtp).astype(f) * rtm).astype(f)
    return (((-dpsi + l1p).astype(f)) + last).astype(f)
