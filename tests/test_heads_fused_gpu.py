"""K-HEADS parity: dcahip_heads_fused (heads forward + NLL + weight / bias / input gradients in
one kernel) against the fp64 oracle -- numpy matmuls around oracle.zinb_np -- on seeded inputs,
through the C ABI.  Tolerances against fp64; the kernel computes in fp32 (MFMA, exact fp32).
"""
import numpy as np
import pytest
import torch

from conftest import synth_counts
from oracle import zinb_np as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from dca_amd.ops import HipOps
    return HipOps()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def reference(Hm, W, b, tw, y, sf, flags, ridge, n_total, threads=1):
    """fp64: A = H W + b per head -> loss / grads -> gW, gb, dH, (g_theta).  threads > 1: the element-wise
    likelihood over row chunks on host threads (benchmark-size cases)."""
    has_pi, cdisp = bool(flags & 1), bool(flags & 2)
    heads = ['mean'] + ([] if cdisp else ['disp']) + (['pi'] if has_pi else [])
    A = {h: Hm @ W[h] + b[h] for h in heads}
    if threads > 1:
        if has_pi:
            ls, lm, dm, dd, dp = Z.rows_in_parallel(Z.zinb_loss_and_grads, (A['mean'], A.get('disp'), A['pi'], y, sf),
                                                    threads, ridge=ridge, n_total=n_total, theta_w=tw if cdisp else None)
        else:
            ls, lm, dm, dd = Z.rows_in_parallel(Z.nb_loss_and_grads, (A['mean'], A.get('disp'), y, sf), threads,
                                                n_total=n_total, theta_w=tw if cdisp else None)
            dp = None
    elif has_pi:
        ls, lm, dm, dd, dp = Z.zinb_loss_and_grads(A['mean'], A.get('disp'), A['pi'], y, sf, ridge,
                                                   n_total, tw if cdisp else None)
    else:
        ls, lm, dm, dd = Z.nb_loss_and_grads(A['mean'], A.get('disp'), y, sf, n_total,
                                             tw if cdisp else None)
        dp = None
    D = {'mean': dm}
    if not cdisp:
        D['disp'] = dd
    if has_pi:
        D['pi'] = dp
    gW = {h: Hm.T @ D[h] for h in heads}
    gb = {h: D[h].sum(0) for h in heads}
    dH = sum(D[h] @ W[h].T for h in heads)
    # sum |a b| of the two backward products: the scale their fp32-dot-product accuracy is stated against
    mag = {'gW_' + h: np.abs(Hm).T @ np.abs(D[h]) for h in heads}
    mag['dH'] = sum(np.abs(D[h]) @ np.abs(W[h]).T for h in heads)
    return heads, ls / n_total, gW, gb, dH, (dd if cdisp else None), mag, D


def draw_inputs(flags, B, G, hL, seed, odd_counts=False, counts=None, hscale=None, tw=None, wscale=None):
    """The host inputs of run_case (numpy only: the CPU half of the four-wave edge tests draws the same ones): every array
    fp32-rounded and widened to fp64.  Returns them and the generator, which run_case goes on drawing the row permutation
    from.  hscale: a factor per 32-row tile of H; wscale: a factor per 32-gene tile, on the weights of every head of the
    tile; tw: the [G] log-dispersion vector in place of the N(0, 1.5) draw (which is still taken: the later draws keep
    their values)."""
    cdisp, has_pi = bool(flags & 2), bool(flags & 1)
    rng = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    heads = ['mean'] + ([] if cdisp else ['disp']) + (['pi'] if has_pi else [])
    Hm = f(np.maximum(rng.normal(0.3, 1.0, (B, hL)), 0))          # post-ReLU activations
    if hscale is not None:
        Hm = f(Hm * np.repeat(np.asarray(hscale, np.float64), 32)[:B, None])
    W = {h: rng.normal(0, 0.25, (hL, G)) for h in heads}
    if wscale is not None:
        assert len(wscale) == (G + 31) // 32
        W = {h: W[h] * np.repeat(np.asarray(wscale, np.float64), 32)[None, :G] for h in heads}
    W = {h: f(W[h]) for h in heads}
    b = {h: f(rng.normal(0, 0.3, G)) for h in heads}
    tw_drawn = f(rng.normal(0, 1.5, G))
    if tw is None:
        tw = tw_drawn
    else:
        tw = f(np.asarray(tw, np.float64))
        assert tw.shape == (G,)
    y = f(synth_counts(B, G, seed)) if counts is None else f(counts)
    if odd_counts:        # non-integer 'counts' (check_counts=False), large and > 65535 counts
        y[0, :6] = [2.52, 0.5, 17.0, 70000.0, 200.0, 5000.0]
        y[1, 1:4] = [16.0, 16.5, 65535.0]
    sf = f(rng.lognormal(0, 0.3, B))
    return heads, Hm, W, b, tw, y, sf, rng


def run_case(ops, flags, B, G, hL, seed, ridge=0.0, use_perm=True, odd_counts=False, tile_order=None, counts=None,
             threads=1, d_exp=0, hscale=None, compact=False, tw=None, wscale=None):
    """d_exp: the kernel's starting gradient exponent (dcahip_heads_fused); hscale: a factor per 32-row tile of H;
    wscale: a factor per 32-gene tile of the weights of every head; tw: an explicit [G] log-dispersion vector;
    compact: the counts from the byte store (dca_amd.compact, escapes >= 255 through the overflow list).  out['_ref'] keeps
    what the scale-rule checks of tests/test_heads_edges_gpu.py need: H, the gradient planes of the products, the weights
    (and 'theta_pad': what the launch left in g_theta[G:Gp], which it must not write)."""
    cdisp = bool(flags & 2)
    heads, Hm, W, b, tw, y, sf, rng = draw_inputs(flags, B, G, hL, seed, odd_counts, counts, hscale, tw, wscale)
    nh = len(heads)
    n_total = float(B * G)
    _, lm, gW, gb, dH, dth, mag, Dref = reference(Hm, W, b, tw, y, sf, flags, ridge, n_total, threads)

    Gp = (G + 3) // 4 * 4
    NH = nh * Gp
    ldh = (hL + 3) // 4 * 4
    Wh = np.zeros((hL + 1, NH))
    for k, h in enumerate(heads):
        Wh[:hL, k * Gp:k * Gp + G] = W[h]
        Wh[hL, k * Gp:k * Gp + G] = b[h]
    Hp = np.zeros((B, ldh)); Hp[:, :hL] = Hm
    n_store = B + 5
    if use_perm:
        perm = rng.permutation(n_store)[:B + 2].astype(np.int32); cur = 2
        rows = perm[cur:cur + B]
    else:
        perm = None; cur = 1
        rows = np.arange(cur, cur + B)
    Yst = np.zeros((n_store, Gp)); Yst[rows, :G] = y
    sfst = np.ones(n_store); sfst[rows] = sf

    dWh = dev(Wh)
    dHp, dY, dsf = dev(Hp), dev(Yst), dev(sfst)
    cc = None
    if compact:
        from dca_amd import compact as C
        cc = C.build(ops, dY, n_store, G)
        assert cc is not None and (cc.ovf_col is not None) == bool((Yst >= 255).any())
    dperm = torch.as_tensor(perm).cuda() if perm is not None else None
    dcur = torch.tensor([cur], dtype=torch.int64, device='cuda')
    dtw = dev(np.concatenate([tw, np.zeros(Gp - G)]))
    gWd = torch.full((hL + 1, NH), 7.0, device='cuda')
    gth = torch.full((Gp,), 7.0, device='cuda')
    dHd = torch.full((B, ldh), 7.0, device='cuda')
    part = torch.zeros(ops.max_partials, dtype=torch.float64, device='cuda')
    nb = ops.heads_fused_workspace_bytes(B, hL, G, Gp, flags)
    assert nb > 0
    ws = torch.full((nb // 4,), float('nan'), device='cuda')      # every slot read must be written
    n = ops.heads_fused(dHp, ldh, dWh, NH, dWh[hL], Gp, dtw if cdisp else None, dY, Gp, dsf, dperm,
                        dcur, B, hL, G, ridge, 1.0 / n_total, flags, gWd, NH,
                        gth if cdisp else None, dHd, ldh, part, ws,
                        tile_order=None if tile_order is None else torch.as_tensor(tile_order, dtype=torch.int32).cuda(),
                        compact=cc, d_exp=d_exp)
    loss = torch.zeros(1, device='cuda')
    ops.loss_finalize(part, n, 1.0 / n_total, loss)
    torch.cuda.synchronize()
    out = {'loss': (loss.item(), lm)}
    gWn = gWd.cpu().numpy().astype(np.float64)
    for k, h in enumerate(heads):
        out['gW_' + h] = (gWn[:hL, k * Gp:k * Gp + G], gW[h])
        out['gb_' + h] = (gWn[hL, k * Gp:k * Gp + G], gb[h])
        if Gp > G:
            out['pad_' + h] = (gWn[:, k * Gp + G:(k + 1) * Gp], np.zeros((hL + 1, Gp - G)))
    out['dH'] = (dHd.cpu().numpy().astype(np.float64)[:, :hL], dH)
    out['_mag'] = mag
    out['_ref'] = {'H': Hm, 'D': [Dref[h] for h in heads], 'W': np.stack([W[h] for h in heads]), 'n_total': n_total}
    if cdisp:
        # oracle returns d loss / d theta_w already chained when theta_w is given
        out['g_theta'] = (gth.cpu().numpy().astype(np.float64)[:G], dth)
        out['_ref']['theta_pad'] = gth.cpu().numpy()[G:]
    return out


def product_tol(key, rows, genes=None):
    """Bound on |C - A B| / sum|a b| for the two backward matrix products of K-HEADS (dW = H^T D: keys gW_*, dH = D W^T), by
    the number of batch rows of the case.  What the bound carries: the products themselves (arithmetic contract
    dcahip_x3_product_32x32: two fp16 pieces of block-scaled operands, three products = an fp32 dot product, <= 5e-7) and the
    fp32 likelihood arithmetic behind D (fast exp / log / rcp: up to ~3e-6 relative on single elements, 1e-7 typical -- it
    dominates where a sum has few terms).  The bounds are the ones the six-product bf16 kernel of rounds 2 - 5 was held to
    (measured then, six | three bf16 products, profiles/r04g_heads_product_ratios.txt:
        dH, up to 260 rows   <= 4.0e-7 | >= 3.2e-6        gW, fewer than 96 rows  <= 4.0e-6 | >= 6.3e-6
        dH, 4 096 rows       <= 7.2e-8 | >= 3.9e-7        gW, 96 rows and more    <= 9.9e-7 | >= 2.5e-6).
    Round 6's kernel passes them with three fp16 products; a build with TWO (-DDCA_EXP_H2_TWO: one operand's second piece
    dropped, 2^-11 instead of 2^-22) fails every case of this file and the golden-vector cases that go through the kernel --
    39 of 39 (tools/gpu_heads_narrow_check.sh, profiles/r06n_heads_two_product_rejection.txt) -- which the 2e-4 relative
    tolerance of check() alone would not notice.
    The bounds assume D = g 2^kD carried at kD >= 5 (d_exp >= -3, kD within K_DSLACK of 8 + d_exp whatever the spread of
    the row tiles' magnitudes).  Where a tile takes K-HEADS' repeat path (its largest |g| 2^kD beyond the fp16 range: kDe < kD
    for the whole 32 x 32 tile), below d_exp = -3, and for gradients that fall under D's fp16 floor beside a large H, the
    kernel's contract is product_tol sum|ab| + 2^-(kDe + 25) sum|b| (b: the other operand; oracle/x3_np.py::repeat_floor,
    tests/test_heads_edges_gpu.py)."""
    if key == 'dH':
        # (dH sums over heads x genes: the 2e-7 of the benchmark shape is what 60 000 terms average the element errors to;
        #  a launch over fewer genes keeps the bound of the small cases)
        return 2e-7 if (rows >= 4096 and (genes is None or genes >= 20000)) else 1e-6
    return 1.5e-6 if rows >= 96 else 5e-6


def check(out, edge=False, extra=None):
    """extra: {key: array}, an absolute term per output element beside the bounds below, for inputs whose fp64 reference is
    itself ill-conditioned in fp32 (derived from the inputs alone: tests/_heads_small_cases.py).  None: the bounds alone."""
    extra = extra or {}
    got, ref = out['loss']
    assert abs(got - ref) <= (3e-5 if edge else 3e-6) * abs(ref), ('loss', got, ref)
    mag = out.get('_mag', {})
    worst = 0.0
    for k, v in out.items():
        if k in ('loss', '_mag', '_ref'):
            continue
        g, r = v
        if k in mag and not edge:
            rows = out['dH'][0].shape[0]
            genes = out['gW_mean'][0].shape[1]
            ratio = (np.maximum(np.abs(g - r) - extra.get(k, 0.0), 0.0) / np.maximum(mag[k], 1e-300)).max()
            worst = max(worst, ratio)
            assert ratio <= product_tol(k, rows, genes), (k, rows, genes, float(ratio))
        scale = max(np.abs(r).max(), 1e-30)
        err = np.abs(g - r)
        if k.startswith('pad_'):
            assert (g == 0).all(), k
            continue
        # sums of B (or 3G) fp32 terms: 2e-4 relative + 2e-5 of the tensor's scale
        bad = err > 2e-4 * np.abs(r) + 2e-5 * scale + extra.get(k, 0.0)
        assert not bad.any(), (k, int(bad.sum()), float(err.max()), float(scale), np.argwhere(bad)[:4].tolist())
    if mag and not edge:
        print('backward products: max |err| / sum|ab| = %.2e' % worst)


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
@pytest.mark.parametrize('B,G,hL', [(8, 40, 64), (33, 1000, 64), (5, 6, 16), (150, 203, 50), (260, 333, 64)])
def test_heads_fused_vs_oracle(ops, flags, B, G, hL):
    out = run_case(ops, flags, B, G, hL, seed=B + G, ridge=0.05 if flags & 1 else 0.0)
    check(out)


@pytest.mark.parametrize('flags', [1, 3])
def test_heads_fused_benchmark_shape_vs_oracle(ops, flags):
    """The launch bench.py's roofline line is quoted on (BASELINE configs[2] at the bench batch): B = 4 096 cells x
    G = 20 000 genes, hL = 64, ZINB with conditional (flags 1) / constant (flags 3) dispersion, counts from the
    bench's own generator (dca_amd/synth.py: ~93 % zeros) -- against the fp64 oracle (numpy matmuls around
    oracle.zinb_np, dca/loss.py:122-156), same tolerances as every other case here."""
    import os
    from dca_amd import synth
    B, G = 4096, 20000
    y = synth.generate_counts(B, G, device='cuda', seed=11 + flags)[:, :G].cpu().numpy()
    assert 0.90 < (y == 0).mean() < 0.96
    out = run_case(ops, flags, B, G, 64, seed=7, ridge=0.02, counts=y, threads=max(1, min(64, os.cpu_count() or 1)))
    check(out)


@pytest.mark.parametrize('flags,B,G', [(1, 2048, 16500), (3, 4096, 8500)])
def test_heads_fused_tail_launch_vs_oracle(ops, flags, B, G):
    """Shapes whose uniform plan would end in a poorly filled round of workgroups (make_heads_plan in dcahip_heads.hip):
    2 048 rows x 16 500 genes = 516 gene tiles x 2 batch splits on 256 workgroups = 4 full rounds + 4 tiles, 4 096 x 8 500 = 266
    tiles x 4 = 4 rounds + 10 tiles.  The left-over tiles go to a SECOND launch of the kernel with 8 / 16 batch splits, whose
    partial sums the reduce kernels add per gene tile: every tolerance of the other cases, on both dispersion forms."""
    import os
    out = run_case(ops, flags, B, G, 64, seed=B + G, ridge=0.03, threads=max(1, min(64, os.cpu_count() or 1)))
    check(out)


@pytest.mark.parametrize('flags', [1, 0, 3, 2])
def test_heads_fused_odd_counts(ops, flags):
    """Non-integer counts (libm lgamma route), counts above 16 (Stirling route), counts that do
    not fit the 16-bit queue slot (re-read from memory)."""
    out = run_case(ops, flags, 40, 70, 64, seed=5, odd_counts=True)
    check(out, edge=True)


def test_heads_fused_no_perm_and_determinism(ops):
    a = run_case(ops, 1, 200, 500, 64, seed=3, use_perm=False)
    check(a)
    b = run_case(ops, 1, 200, 500, 64, seed=3, use_perm=False)
    for k in a:
        if k in ('_mag', '_ref'):
            continue
        assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k


def test_heads_fused_ragged_shapes(ops):
    """Batch and gene counts that end inside a tile (192 = 6 row tiles, 777 genes = 24.3 gene tiles)."""
    out = run_case(ops, 1, 192, 777, 64, seed=9)
    check(out)


@pytest.mark.parametrize('flags,B,G', [(1, 200, 777), (3, 96, 333), (0, 260, 1000), (1, 2048, 16500)])     # (the last: a tail launch)
def test_heads_fused_tile_order_changes_nothing(ops, flags, B, G):
    """dcahip_heads_fused with a tile_order: any order of the 32-gene tiles gives the results of the identity order -- bitwise
    for the weight / bias / dispersion gradients (each is per gene tile) unless the launch's plan has a tail launch (the
    last case: see below); the input gradient dH and the loss are sums over gene tiles whose association follows the
    order (a workgroup accumulates the tiles it is handed), so they agree to fp32 / fp64 re-association."""
    ntg = (G + 31) // 32
    n_ord = ops.heads_tile_order_len(G)
    assert n_ord == (ntg + 1) // 2 * 2
    a = run_case(ops, flags, B, G, 64, seed=11)
    check(a)
    rng = np.random.RandomState(4)
    for order in (np.r_[np.arange(ntg)[::-1], np.arange(ntg, n_ord)], np.r_[rng.permutation(ntg), np.arange(ntg, n_ord)]):
        b = run_case(ops, flags, B, G, 64, seed=11, tile_order=order)
        check(b)
        for k in a:
            if k in ('_mag', '_ref'):
                continue
            if k == 'loss':
                assert abs(a[k][0] - b[k][0]) <= 1e-6 * abs(a[k][0])
            elif k == 'dH':
                scale = np.abs(a[k][0]).max()
                assert np.abs(np.asarray(a[k][0]) - np.asarray(b[k][0])).max() <= 2e-6 * scale
            elif G >= 16500:
                # a plan with a TAIL launch: the tiles the order puts last are summed over more batch splits than the others
                # (8 partial sums instead of 2), so a tile's gradient moves by fp32 re-association when the order moves it there
                scale = np.abs(a[k][0]).max()
                assert np.abs(np.asarray(a[k][0]) - np.asarray(b[k][0])).max() <= 2e-6 * scale, k
            else:
                assert np.array_equal(np.asarray(a[k][0]), np.asarray(b[k][0])), k


@pytest.mark.parametrize('K', [64, 4096])
@pytest.mark.parametrize('dist', ['uniform', 'lognormal'])
def test_x3_products_are_fp32_accurate(ops, K, dist):
    """The arithmetic contract of K-HEADS' matrix products (include/dcahip.h, dcahip_x3_product_32x32): three bf16
    pieces per operand, six products, fp32 accumulation == the accuracy of an fp32 dot product.  Per element
    |C - A B| <= 5e-7 sum|a b| against fp64 (4 ulp of fp32 at the scale of the sum: what the MFMA's fp32 accumulation
    leaves; the operand split itself loses < 2^-26) -- on K = 64 (the contraction length of the forward product) and
    K = 4 096 (the weight gradient over a bench batch), for uniform operands and for operands spread over +-4 e-folds.
    Printed beside it: the exact-fp32 GEMM of this library (v_mfma_f32_32x32x2_f32, dcahip_sgemm with split_k < 0) on the
    same operands; as ONE k-ordered chain it measures 1.6e-7 / 3.7e-7 at K = 64 and 1.2e-7 / 4.6e-7 at K = 4 096.  (Three products would give 2e-6, plain bf16 1e-3: tools/microbench/bf16x3_mfma.hip.)"""
    rng = np.random.RandomState(K + len(dist))
    shape = lambda *s: rng.uniform(-1, 1, s) * (np.exp(4 * rng.uniform(-1, 1, s)) if dist == 'lognormal' else 1.0)
    A = shape(32, K).astype(np.float32)
    Bm = shape(K, 32).astype(np.float32)
    dA, dB = dev(A), dev(Bm)
    C = torch.zeros(32, 32, device='cuda')
    ops.x3_product_32x32(dA, dB, C, K)
    C32 = torch.zeros(32, 32, device='cuda')
    ws = torch.zeros(max(ops.sgemm_workspace_bytes(0, 0, 32, 32, K, False, -1) // 4, 4), device='cuda')
    ops.sgemm(0, 0, 32, 32, K, dA, K, dB, 32, C32, 32, ws=ws, split_k=-1)       # split_k < 0: the exact-fp32 MFMA kernel
    torch.cuda.synchronize()
    ref = A.astype(np.float64) @ Bm.astype(np.float64)
    mag = np.abs(A.astype(np.float64)) @ np.abs(Bm.astype(np.float64))
    err = (np.abs(C.cpu().numpy().astype(np.float64) - ref) / mag).max()
    err32 = (np.abs(C32.cpu().numpy().astype(np.float64) - ref) / mag).max()
    print('x3 products K=%d %s: max err / sum|ab| = %.2e (exact-fp32 MFMA GEMM: %.2e)' % (K, dist, err, err32))
    assert err <= 5e-7, (err, err32)
