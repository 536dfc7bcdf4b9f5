"""The split-bf16 arithmetic of the matrix-pipe kernels, restated in numpy (oracle/x3_np.py), against fp64: the bound the
GPU tests hold the kernels to, and why three products instead of six cannot meet it."""
import numpy as np
import pytest

from oracle import x3_np as X


def test_three_pieces_carry_an_fp32_value():
    rng = np.random.RandomState(0)
    x = (rng.standard_normal(20000) * np.exp(rng.uniform(-20, 20, 20000))).astype(np.float32)
    p0, p1, p2 = X.split3(x)
    for p in (p0, p1, p2):
        assert (p.view(np.uint32) & 0xFFFF == 0).all()                 # bf16 values
    err = np.abs(x.astype(np.float64) - (p0.astype(np.float64) + p1 + p2))
    assert (err <= 2.0 ** -24 * np.abs(x)).all()
    assert np.array_equal(X.bf16_round(np.float32([1.0, 1.00390625, 1.01171875])), np.float32([1.0, 1.0, 1.015625]))  # ties to even


def test_six_products_are_fp32_accurate_and_three_are_not():
    rng = np.random.RandomState(1)
    for M, K, N in ((64, 4096, 64), (32, 20000, 64), (96, 512, 32)):
        a = rng.standard_normal((M, K)).astype(np.float32)
        b = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        ref = a.astype(np.float64) @ b.astype(np.float64)
        mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        e6 = (np.abs(X.matmul_x3(a, b, 6) - ref) / mag).max()
        e3 = (np.abs(X.matmul_x3(a, b, 3) - ref) / mag).max()
        assert e6 <= 5e-7, (M, K, N, e6)                                # DESIGN section 4.1's contract (dcahip_x3_product_32x32)
        assert e3 >= 8 * e6, (M, K, N, e3, e6)                          # random signs: the dropped terms average out, and still show
    # operands whose second pieces line up: the dropped a2 b2 term is 2^-18 of every product -- systematic, whatever K
    a = np.full((32, 256), 1.0 + 2.0 ** -9, np.float32); b = np.full((256, 32), 1.0 + 2.0 ** -9, np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    e6 = (np.abs(X.matmul_x3(a, b, 6) - ref) / ref).max()
    e3 = (np.abs(X.matmul_x3(a, b, 3) - ref) / ref).max()
    assert e6 <= 1.2e-7 and 3e-6 <= e3 <= 5e-6, (e6, e3)                # 2^-18 = 3.8e-6: beyond every bound the GPU tests use


def test_first_layer_forward_from_count_tables():
    """dcahip_enc0_fwd_lut's algebra: Z = L (W / std) + (b - sum_g (mean / std) W[g, :]) with L looked up per count from
    the cell's table equals the dense X W + b of dca/network.py:124-126 on the input of dca/io.py:88-111."""
    rng = np.random.RandomState(2)
    n, G, H = 48, 700, 64
    y = rng.poisson(0.3, (n, G)).astype(np.float64) * (rng.uniform(size=(n, G)) < 0.5)
    y[3, 5] = 40.0; y[7, 9] = 300.0
    fac = rng.lognormal(0, 0.4, n).astype(np.float32).astype(np.float64)
    L = np.log1p(y / fac[:, None])
    mean = L.mean(0); std = np.maximum(L.std(0, ddof=1), 1e-3)
    W = (rng.standard_normal((G, H)) * 0.1).astype(np.float32); b = (rng.standard_normal(H) * 0.3).astype(np.float32)
    ref = ((L - mean) / std) @ W.astype(np.float64) + b
    table = np.log1p(np.arange(64)[None, :] / fac[:, None]).astype(np.float32)          # dcahip_enc0_lut
    codes = np.minimum(y, 255).astype(np.int64)
    Lk = np.where(codes < 64, np.take_along_axis(table, np.minimum(codes, 63), axis=1),
                  np.log1p(y / fac[:, None]).astype(np.float32)).astype(np.float32)       # beyond the table: the formula
    Wp = (W / std[:, None].astype(np.float32)).astype(np.float32)
    c0 = -((mean / std)[:, None] * W.astype(np.float64)).sum(0)
    Z = X.matmul_x3(Lk, Wp).astype(np.float64) + c0.astype(np.float32) + b
    mag = np.abs(L / std) @ np.abs(W).astype(np.float64) + np.abs(mean / std) @ np.abs(W).astype(np.float64) + np.abs(b)
    assert (np.abs(Z - ref) <= 1e-6 * mag).all(), float((np.abs(Z - ref) / mag).max())


def test_two_fp16_pieces_carry_an_fp32_value_after_block_scaling():
    """x 2^e = h1 + h2 to 2^-22 |x 2^e| where h2 is a normal fp16 (|x 2^e| >= 2^-3), to 2^-25 absolute below (h2 an fp16
    denormal: the matrix pipe of gfx950 preserves them, tools/microbench/mfma_f16_denorm.hip)."""
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(20000) * np.exp(rng.uniform(-12, 0, 20000))).astype(np.float32)
    e = X.block_exp(x)
    assert 2.0 ** 13 <= np.abs(x).max() * 2.0 ** e < 2.0 ** 14
    h1, h2 = X.split2(x, e)
    xs = np.ldexp(x.astype(np.float64), e)
    err = np.abs(xs - (h1.astype(np.float64) + h2))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25)).all()
    assert np.isfinite(h1).all() and np.abs(h1).max() < 65504
    assert X.block_exp(np.zeros(5, np.float32)) == 0


def test_three_fp16_products_are_fp32_accurate_and_two_are_not():
    """K-HEADS' arithmetic from round 6 against fp64: random operands, operands with a wide dynamic range (gradients), and the
    systematic case; a build that drops one cross term is off by 2^-12 of every product."""
    rng = np.random.RandomState(1)
    for M, K, N in ((64, 4096, 64), (32, 20000, 64), (96, 512, 32)):
        a = rng.standard_normal((M, K)).astype(np.float32)
        b = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
        ref = a.astype(np.float64) @ b.astype(np.float64)
        mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        e3 = (np.abs(X.matmul_h2(a, b, 3) - ref) / mag).max()
        e2 = (np.abs(X.matmul_h2(a, b, 2) - ref) / mag).max()
        e6 = (np.abs(X.matmul_x3(a, b, 6) - ref) / mag).max()
        assert e3 <= 5e-7 and e3 <= 4 * e6 + 1e-8, (M, K, N, e3, e6)   # the contract of dcahip_x3_product_32x32; within 4x of bf16 x 3 / six
        assert e2 >= 20 * e3, (M, K, N, e2, e3)
    # gradients: a log-normal spread of three decades around the typical value, the block scale fixed by the largest
    a = (rng.standard_normal((64, 4096)) * np.exp(rng.normal(0, 1.5, (64, 4096)))).astype(np.float32)
    b = (rng.standard_normal((4096, 64)) * 0.05).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    assert (np.abs(X.matmul_h2(a, b, 3) - ref) / mag).max() <= 5e-7
    # operands whose second pieces line up: the dropped a2 b2 is 2^-22 of every product -- systematic, whatever K
    a = np.full((32, 256), 1.0 + 2.0 ** -11, np.float32); b = np.full((256, 32), 1.0 + 2.0 ** -11, np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    e3 = (np.abs(X.matmul_h2(a, b, 3) - ref) / ref).max()
    e2 = (np.abs(X.matmul_h2(a, b, 2) - ref) / ref).max()
    assert e3 <= 3e-7 and 2e-4 <= e2 <= 6e-4, (e3, e2)


def test_fp16_pieces_on_the_operands_of_a_training_step():
    """The three products of K-HEADS on the operands of an actual step (decoder output after ReLU, glorot head weights, the
    ZINB gradient planes of the oracle: a median |g| of 0.16, a largest of several hundred) with the kernel's scales -- H and W
    by their largest magnitude, D = g 2^8 (kDExp0) -- against fp64: inside the bounds of product_tol."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import make_problem, oracle_net
    from oracle import zinb_np as Z
    n, G, hs = 256, 1500, (64, 32, 64)
    Xd, Y, sf, p = make_problem(n, G, hs, 'zinb-conddisp', True, seed=3)
    net = oracle_net('zinb-conddisp', p, hs, True)
    net.loss_and_grads(Xd.astype(np.float64), Y.astype(np.float64), sf.astype(np.float64))
    c = net.cache
    _, _, dm, dd, dpi = Z.zinb_loss_and_grads(c['a_mean'], c['a_disp'], c['a_pi'], Y.astype(np.float64), c['sf'], 0.0, None, None)
    g = (np.concatenate([dm, dd, dpi], axis=1) * (n * G)).astype(np.float32)          # unscaled gradients
    H = np.maximum(c['H'][-1], 0).astype(np.float32)
    W = np.concatenate([p['W_mean'], p['W_disp'], p['W_pi']], axis=1).astype(np.float32)
    # D = g 2^8 where that fits the fp16 range; a tile holding a larger gradient (here: several hundred, at a large count) is
    # scaled down as a whole by the kernel's slow path -- emulated on the whole matrix (the less favourable case)
    ed = min(8, X.block_exp(g))
    assert ed < 8 and np.abs(g).max() * 2.0 ** ed < 2.0 ** 14

    def err(a, b, **kw):
        ref = a.astype(np.float64) @ b.astype(np.float64)
        mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
        return (np.abs(X.matmul_h2(a, b, 3, **kw) - ref) / np.maximum(mag, 1e-300)).max()
    assert err(H, W) <= 5e-7                                                           # F
    assert err(g, W.T.copy(), ea=ed) <= 1e-6                                           # dH
    assert err(H.T.copy(), g, eb=ed) <= 1.5e-6                                         # dW


# ---------------------------------------------------------------------------------------- K-HEADS' scale rule (one wave)
def _wave_problem(T, G, seed, scale=None, counts=None, K=64):
    """A wave's row tiles and the unscaled ZINB gradient (conditional dispersion) of the oracle on synth_counts."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import synth_counts
    from oracle import zinb_np as Z
    rng = np.random.RandomState(seed)
    B = 32 * T
    f = lambda a: a.astype(np.float32).astype(np.float64)
    H = f(np.maximum(rng.normal(0.3, 1.0, (B, K)), 0))
    if scale is not None:
        H = f(H * np.repeat(np.asarray(scale, np.float64), 32)[:, None])
    W = np.stack([f(rng.normal(0, 0.25, (K, G))) for _ in range(3)])
    b = [f(rng.normal(0, 0.3, G)) for _ in range(3)]
    y = synth_counts(B, G, seed) if counts is None else counts
    sf = f(rng.lognormal(0, 0.3, B))
    A = [H @ W[h] + b[h] for h in range(3)]
    n = float(B * G)
    _, _, dm, dd, dp = Z.zinb_loss_and_grads(A[0], A[1], A[2], y, sf, 0.0, n, None)
    g = (np.stack([dm, dd, dp]) * n).astype(np.float32)
    return H, g, W


def _wave_errors(H, g, W, rule, d_exp=0):
    """max |err| / sum|ab| of dW and dH of X.heads_wave against fp64, the model's output, and both absolute errors."""
    T = H.shape[0] // 32
    o = X.heads_wave(H.reshape(T, 32, -1), g, W, d_exp, rule)
    g64 = g.astype(np.float64)
    rW = np.einsum('rk,hrg->hkg', H, g64); mW = np.einsum('rk,hrg->hkg', np.abs(H), np.abs(g64))
    rH = np.einsum('hrg,hkg->rk', g64, W); mH = np.einsum('hrg,hkg->rk', np.abs(g64), np.abs(W))
    eW, eH = np.abs(o['dW'] - rW), np.abs(o['dH'] - rH)
    return (eW / np.maximum(mW, 1e-300)).max(), (eH / np.maximum(mH, 1e-300)).max(), o, (eW, mW, eH, mH)


def _product_tol(key, rows):
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_heads_fused_gpu import product_tol
    return product_tol(key, rows)


# (case, wave's row tiles, H scale per tile, the parent rule fails dW, the parent rule fails dH)
SPREAD_CASES = [
    ('normal tiles', 2, None, False, False),
    ('one all-zero row tile of 2', 2, [0.0, 1.0], True, False),
    ('one all-zero row tile of 4', 4, [1.0, 0.0, 1.0, 1.0], True, False),
    ('sibling tile at 2^-12', 2, [1.0, 2.0 ** -12], False, False),
    ('sibling tile at 2^-20', 2, [1.0, 2.0 ** -20], False, True),
]


@pytest.mark.parametrize('case,T,scale,parent_fails_dw,parent_fails_dh', SPREAD_CASES)
def test_heads_scale_rule_against_row_scale_spread(case, T, scale, parent_fails_dw, parent_fails_dh):
    """K-HEADS' scale rule for one wave of the persistent kernel (X.heads_wave: G = 1 000, synth_counts, ZINB with a per-cell
    dispersion) against fp64.  The round-6 rule kD = kD0 - (eH - min eH) scaled D down by the H-magnitude spread of the wave's
    tiles: an all-zero tile (eH = 0 against ~11) cost the OTHER tiles' D 11 bits, which dW reads, and a tile 2^-20 below its
    sibling lost 20 bits of D, which dH (= D W^T, no H in it) reads.  The rule the kernel has now keeps kD within
    K_DSLACK of kD0 and moves the dW accumulators instead: product_tol on every case."""
    H, g, W = _wave_problem(T, 1000, 3, scale)
    rows = 32 * T
    tw, th = _product_tol('gW_mean', rows), _product_tol('dH', rows)
    pw, ph, po, _ = _wave_errors(H, g, W, 'parent')
    fw, fh, fo, _ = _wave_errors(H, g, W, 'fixed')
    print('%s: parent dW %.2e dH %.2e | fixed dW %.2e dH %.2e (bounds %.1e / %.1e)' % (case, pw, ph, fw, fh, tw, th))
    assert (pw > tw) == parent_fails_dw and (ph > th) == parent_fails_dh, (case, pw, ph)
    assert fw <= tw and fh <= th, (case, fw, fh)
    assert ((fo['kD'] <= X.K_DEXP0) & (fo['kD'] >= X.K_DEXP0 - X.K_DSLACK)).all()
    if parent_fails_dw or parent_fails_dh:
        assert po['kD'].min() < X.K_DEXP0 - X.K_DSLACK


def test_heads_scale_rule_keeps_the_parent_scales_on_like_tiles():
    """Row tiles of like magnitude (the scale exponents of a training step's decoder output): the fixed rule takes the
    scales the round-6 rule took wherever no tile repeats -- the same arithmetic, bit for bit."""
    H, g, W = _wave_problem(2, 300, 5)
    g = np.clip(g, -100, 100)                                  # no tile beyond the fp16 range: no repeat
    po = X.heads_wave(H.reshape(2, 32, -1), g, W, 0, 'parent')
    fo = X.heads_wave(H.reshape(2, 32, -1), g, W, 0, 'fixed')
    assert abs(int(po['eH'][0]) - int(po['eH'][1])) <= X.K_DSLACK
    assert (po['kDe'] == po['kD']).all()
    assert np.array_equal(po['kD'], fo['kD']) and np.array_equal(po['dW'], fo['dW']) and np.array_equal(po['dH'], fo['dH'])


@pytest.mark.parametrize('count,d_exp', [(5000, 0), (65535, 0), (70000, 0), (65535, -3), (70000, -3)])
def test_heads_repeat_path_bound(count, d_exp):
    """The repeat path rescales a whole 32 x 32 tile by what its largest gradient needs, so the tile's other genes are carried
    at 2^kDe < 2^kD: D's second fp16 piece rounds to 2^-25 at that scale.  The bound the GPU tests hold such elements to:
        |err| <= product_tol sum|ab| + 2^-(kDe + 25) sum|b|           (X.repeat_floor; b = the other operand)
    -- the model meets it with room (< 0.5 of it), and product_tol alone as well at these shapes: the floor is what the
    repeat path guarantees, not what it typically loses."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import synth_counts
    y = synth_counts(64, 1000, 4)
    gl = int(np.argsort(y.mean(0))[0])                        # the outlier beside the lowest-expressed gene
    y[5, gl] = count
    H, g, W = _wave_problem(2, 1000, 4, counts=y)
    fw, fh, o, (eW, mW, eH, mH) = _wave_errors(H, g, W, 'fixed', d_exp)
    assert o['kDe'][0, gl // 32] < o['kD'][0, gl // 32]             # the outlier's tile took the repeat path ...
    assert (o['kDe'] >= o['kD']).any() and (o['kDe'] < o['kD']).any()   # ... and not every tile did
    floor_w, floor_h = X.repeat_floor(o['kDe'], H, W)
    rw = (eW / (_product_tol('gW_mean', 64) * mW + floor_w[None])).max()
    rh = (eH / (_product_tol('dH', 64) * mH + floor_h)).max()
    print('count %d d_exp %d: dW %.2e dH %.2e of sum|ab|; against the derived bound %.2f / %.2f' % (count, d_exp, fw, fh, rw, rh))
    assert rw <= 0.5 and rh <= 0.5, (rw, rh)
    assert fw <= _product_tol('gW_mean', 64) and fh <= _product_tol('dH', 64), (fw, fh)
    # the floor is exact arithmetic: a single D element at 2^kDe is within 2^-(kDe + 25) of its g
    Dt = g[:, 0:32, 32 * (gl // 32):32 * (gl // 32) + 32]
    h1, h2 = X.split2(Dt, int(o['kDe'][0, gl // 32]))
    err = np.abs(np.ldexp(h1.astype(np.float64) + h2, -int(o['kDe'][0, gl // 32])) - Dt)
    assert (err <= np.maximum(2.0 ** -22 * np.abs(Dt), 2.0 ** -(o['kDe'][0, gl // 32] + 25))).all()


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
@pytest.mark.parametrize('B,name', [(128, 'spread'), (32, '2^15')])
def test_heads_big_row_tile_forward_bound(flags, B, name):
    """A row tile of H at 2^15 and more (tests/test_heads_small_edges_gpu.py, case (d)): the pre-activations are 1e5 .. 1e7, an
    fp32 forward product is off by 0.1 .. 10 there, and the few elements of the tile that are NOT saturated move with it.
    The bound the GPU test holds such a launch to adds, per output element, what the likelihood's gradient can change by
    when each pre-activation of the big tile moves inside the forward product's error box
        delta = 5e-7 sum|h w| + 2^-24 |a|        (the contract of dcahip_x3_product_32x32, then one fp32 rounding of a' + b)
    -- tests/_heads_small_cases.py::forward_error_terms; nothing for the rows of ordinary tiles.  Shown here on the model of
    the kernel's forward (X.matmul_h2 per 32 x 32 tile pair with the kernel's block scales, fp64 everywhere else):
      - the model's forward stays inside the box (asserted by forward_error_terms),
      - the model's gradients, with EXACT backward products, meet the added term alone, and
      - they miss product_tol (for some flags by five orders of magnitude): that bound speaks of the backward products, it
        cannot hold the conditioning of the likelihood on a forward product of this size."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _heads_small_cases as C

    def model_forward(heads, Hb, W, b):
        G = W[heads[0]].shape[1]
        A = {h: np.zeros((Hb.shape[0], G)) for h in heads}
        for r0 in range(0, Hb.shape[0], 32):
            Ht = Hb[r0:r0 + 32].astype(np.float32)
            eH = X.block_exp(Ht)
            for g0 in range(0, G, 32):
                eW = X.block_exp(np.stack([W[h][:, g0:g0 + 32] for h in heads]))
                for h in heads:
                    acc = X.matmul_h2(Ht, W[h][:, g0:g0 + 32].astype(np.float32), 3, ea=eH, eb=eW)
                    A[h][r0:r0 + 32, g0:g0 + 32] = (acc.astype(np.float32) + b[h][g0:g0 + 32].astype(np.float32)).astype(np.float64)
        return A

    om, add, diff, (heads, H, W) = C.forward_error_terms(A_of=model_forward, **C.hscale_case(flags, B, name))
    o = C.oracle_case(**C.hscale_case(flags, B, name))
    # (1e-18, in loss units: the rounding of the oracle's own fp64 sums; a sigmoid beyond |a| = 100, see LIVE, is far below)
    assert all((np.abs(diff[k]) <= om[k] + 1e-18).all() for k in om)
    missed = 0.0
    for h in heads:
        err = np.abs(H.T @ diff[h])
        assert (err <= add['gW_' + h] * (1 + 1e-12) + 1e-9).all()
        assert (np.abs(diff[h].sum(0)) <= add['gb_' + h] * (1 + 1e-12) + 1e-9).all()
        mag = np.abs(H).T @ np.abs(o['_ref']['D'][heads.index(h)])
        missed = max(missed, float((err / np.maximum(_product_tol('gW_' + h, B) * mag, 1e-300)).max()))
    errh = np.abs(sum(diff[h] @ W[h].T for h in heads))
    assert (errh <= add['dH'] * (1 + 1e-12) + 1e-9).all()
    if 'theta' in om:
        assert (np.abs(diff['theta'].sum(0)) <= add['g_theta'] * (1 + 1e-12) + 1e-9).all()
    print('%s flags %d: the model misses product_tol on gW by a factor %.3g' % (name, flags, missed))
    if not flags & 2:                                # (DispAct's window is 1e4 wide: every launch has elements inside it)
        assert missed > 1.0


@pytest.mark.parametrize('flags', [1, 0])
@pytest.mark.parametrize('case,B', [('wscale', 32), ('wscale', 128), ('compact', 32), ('rescale', 33)])
def test_heads_disp_gradient_floor(flags, case, B):
    """The dispersion head's gradient of a y > 0 element, g_disp = dth gd with
        dth = -dpsi + log1p(mu / tp) + (y tp - theta mu) / (tp (tp + mu)),
    summed in fp32 as zinb_nz_elem does (X.dth_fp32, every operation correctly rounded), against fp64 on the inputs of the
    four-wave edge cases: the sum stays inside DTH_ULPS 2^-23 of its terms, the bound X.disp_grad_floor is built on; where
    mu << theta it cancels, and the fp32 sum is then off by MORE than the 3e-6 of the element that product_tol carries (up to
    1e-3 of it) -- so the floor is needed.  (It is non-zero for about a quarter of the elements and adds a tenth to a third to
    product_tol's bound of a typical gW_disp element: the cancellation is mild nearly everywhere.)"""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _heads_small_cases as C
    from oracle import zinb_np as Z
    kw = {'wscale': lambda: C.wscale_case(flags, B), 'compact': lambda: C.compact_case(flags, B),
          'rescale': lambda: C.rescale_case(flags, B, 'outliers')}[case]()
    o = C.oracle_case(**kw)
    _, _, n_total, heads, H, W, b, tw, y, sf = C._oracle_inputs(kw)
    am, ad = H @ W['mean'] + b['mean'], H @ W['disp'] + b['disp']
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    mu, theta, gd = f32(Z.mean_act(am) * sf[:, None]), f32(Z.disp_act(ad)), Z._act_grads(am, ad)[1]
    dpsi, l1p, last = X.dth_terms(mu, theta, y)
    dth = -dpsi + l1p + last
    nz = y > 0
    # the terms are the oracle's gradient (mu and theta rounded to fp32 move it by 1e-7 of its terms at most)
    D = o['_ref']['D'][heads.index('disp')] * n_total
    terms = dpsi + np.abs(l1p) + (y * (theta + X.EPS_NB) + theta * mu) / ((theta + X.EPS_NB) * (theta + X.EPS_NB + mu))
    assert (np.abs(dth * gd - D)[nz] <= 2.0 ** -22 * (terms * gd)[nz] + 1e-300).all()
    small = nz & (y <= 16) & (y == np.floor(y))
    err = np.abs(X.dth_fp32(mu, theta, y).astype(np.float64) - dth) * gd
    assert (err[small] <= X.DTH_ULPS * 2.0 ** -23 * (terms * gd)[small]).all()
    beyond = small & (err > X.D_ELEM_REL * np.abs(dth * gd)) & (gd > 0)
    floor = X.disp_grad_floor(mu, theta, gd, y, dth * gd)
    print('%s B %d flags %d: fp32 sum beyond 3e-6 of the element: %d of %d (worst %.1e of it); floor non-zero for %d'
          % (case, B, flags, int(beyond.sum()), int(small.sum()), float((err[beyond] / np.abs(dth * gd)[beyond]).max(initial=0)),
             int((floor > 0).sum())))
    assert beyond.any()
    assert (err[small] <= floor[small] + X.D_ELEM_REL * np.abs(dth * gd)[small]).all()
    assert (floor[~nz] == 0).all()
