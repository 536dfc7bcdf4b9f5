"""HipOps: tensor-level view of the C ABI (one method per entry point of include/dcahip.h).

The training engine (engine.py) is written against this small interface.  The product always
instantiates HipOps -- construction fails loudly without the HIP library or without a GPU.
(Tests exercise the engine's host logic on CPU by injecting an oracle-backed object with the
same methods; that object lives under oracle/ and is never imported from this package.)
"""
import ctypes

import torch

from . import hip


class HipOps:
    name = 'hip'
    device_type = 'cuda'

    def __init__(self):
        hip.require_gpu()
        self.L = hip.lib()
        self.max_partials = self.L.dcahip_zinb_max_partials()

    # ------------------------------------------------------------------ loss
    def zinb_nll(self, a_mean, a_disp, a_pi, lda, theta_w, Y, ldy, sf, perm, cursor, B, G, ridge,
                 inv_n, flags, d_mean, d_disp, d_pi, ldd, partials):
        n = ctypes.c_int(0)
        p = hip.ptr
        hip.check(self.L.dcahip_zinb_nll(p(a_mean), p(a_disp), p(a_pi), lda, p(theta_w), p(Y), ldy,
                                         p(sf), p(perm), p(cursor), B, G, ridge, inv_n, flags,
                                         p(d_mean), p(d_disp), p(d_pi), ldd, p(partials),
                                         ctypes.byref(n), hip.stream()), 'zinb_nll')
        return n.value

    def zinb_nll_planes(self, a_mean, a_disp, a_pi, lda, theta_w, Y, ldy, sf, perm, cursor, B, G, ridge, inv_n, flags,
                        planes, col_mean, col_disp, col_pi, d_theta, ldd_theta, partials):
        """zinb_nll with the gradient planes written as pre-split bf16 pieces into planes [3, rows, ld] at the given
        columns (the operand of gemm_p3); the per-gene dispersion gradient (const. dispersion) stays fp32 in d_theta."""
        n = ctypes.c_int(0)
        p = hip.ptr
        hip.check(self.L.dcahip_zinb_nll_planes(p(a_mean), p(a_disp), p(a_pi), lda, p(theta_w), p(Y), ldy, p(sf), p(perm),
                                                p(cursor), B, G, ridge, inv_n, flags, p(planes), planes.stride(1),
                                                planes.stride(0), col_mean, col_disp, col_pi, p(d_theta), ldd_theta,
                                                p(partials), ctypes.byref(n), hip.stream()), 'zinb_nll_planes')
        return n.value

    def zinb_nll_planes_h2(self, a_mean, a_disp, a_pi, lda, theta_w, Y, ldy, sf, perm, cursor, B, G, ridge, inv_n, flags, d_exp,
                           planes, col_mean, col_disp, col_pi, d_theta, ldd_theta, partials):
        """zinb_nll_planes with the head planes as TWO fp16 pieces of the unscaled gradient g 2^d_exp (the operand of gemm_h2)."""
        n = ctypes.c_int(0)
        p = hip.ptr
        hip.check(self.L.dcahip_zinb_nll_planes_h2(p(a_mean), p(a_disp), p(a_pi), lda, p(theta_w), p(Y), ldy, p(sf), p(perm),
                                                   p(cursor), B, G, ridge, inv_n, flags, int(d_exp), p(planes), planes.stride(1),
                                                   planes.stride(0), col_mean, col_disp, col_pi, p(d_theta), ldd_theta,
                                                   p(partials), ctypes.byref(n), hip.stream()), 'zinb_nll_planes_h2')
        return n.value

    def nll_marginals_workspace_doubles(self, B, G):
        n = int(self.L.dcahip_nll_marginals_workspace_doubles(B, G))
        hip.check(min(n, 0), 'nll_marginals_workspace_doubles')
        return n

    def nll_marginals(self, a_mean, a_disp, a_pi, lda, theta_w, Y, ldy, sf, B, G, ridge, flags, cell_out, gene_acc, ws):
        """Row sums (cell_out [B], overwritten) and column sums (gene_acc [G], added to) of the element-wise NLL of B
        consecutive rows, in double; Y / sf start at the first row."""
        p = hip.ptr
        hip.check(self.L.dcahip_nll_marginals(p(a_mean), p(a_disp), p(a_pi), lda, p(theta_w), p(Y), ldy, p(sf), B, G,
                                              ridge, flags, p(cell_out), p(gene_acc), p(ws), hip.stream()), 'nll_marginals')

    def group_moments_workspace_doubles(self, B, G, K):
        n = int(self.L.dcahip_group_moments_workspace_doubles(B, G, K))
        hip.check(min(n, 0), 'group_moments_workspace_doubles')
        return n

    def group_moments(self, a_mean, lda, sf, codes, B, G, K, flags, sum_acc, sumsq_acc, ldg, ws):
        """Per group code (codes [B] int32; outside [0, K): left out) the column sums of the denoised mean and of its
        square over B consecutive rows, in double, ADDED to sum_acc / sumsq_acc [K, ldg]; flags: 8 linear mean, 16 without
        the size factor, 32 log1p.  sf / codes start at the first row."""
        p = hip.ptr
        hip.check(self.L.dcahip_group_moments(p(a_mean), lda, p(sf), p(codes), B, G, K, flags, p(sum_acc), p(sumsq_acc),
                                              ldg, p(ws), hip.stream()), 'group_moments')

    def gram_workspace_doubles(self, B, G):
        n = int(self.L.dcahip_gram_workspace_doubles(B, G))
        hip.check(min(n, 0), 'gram_workspace_doubles')
        return n

    def gram(self, x, ldx, cols, keep, shift, B, G, cross, ldc, dsum, ws):
        """Centred cross-products of G columns of B consecutive rows of the fp32 plane x, in double: with d[r][j] =
        x[r][cols[j]] - shift[j] over the rows whose keep word is not 0 (cols int32 [G], None: column j; keep int32 [B],
        None: every row), sum_r d[r][i] d[r][j] is ADDED to cross [G, ldc] (the full square, symmetric bit for bit) and
        sum_r d[r][j] to dsum [G].  keep starts at the first row; ws: gram_workspace_doubles(B, G) doubles (None is
        allowed without cols when the rows make a single slice)."""
        p = hip.ptr
        hip.check(self.L.dcahip_gram(p(x), ldx, p(cols), p(keep), p(shift), B, G, p(cross), ldc, p(dsum), p(ws),
                                     hip.stream()), 'gram')

    def ranksum_workspace_bytes(self, g, n):
        """The workspace of ranksum for g genes of n cells, in bytes (per workgroup of its grid, not per gene)."""
        from .groups import check_ranksum_args
        check_ranksum_args(int(g), int(n))
        nbytes = int(self.L.dcahip_ranksum_workspace_bytes(g, n))
        hip.check(min(nbytes, 0), 'ranksum_workspace_bytes')
        return nbytes

    def ranksum(self, x, ldx, g, n, order, m, gstart, K, ref, rank2, tie, ldr, ws):
        """K-RANKS (include/dcahip.h, dcahip_ranksum): per row of the gene-major fp32 plane x [g, ldx] the m cells order
        lists (int32 columns, group after group; gstart int32 [K + 1] the group boundaries) are sorted and every group's
        doubled rank sum (ref = -1) or doubled Mann-Whitney U against group ref, and the tie term sum t^3 - t, are WRITTEN
        to columns [0, g) of rank2 / tie (int64 [K, ldr]); a row with a NaN among the m cells gets -1.  ws:
        ranksum_workspace_bytes(g, n) bytes.  A limit of the kernel (K 1 .. 4096, n <= 2 097 151) raises ValueError."""
        from .groups import check_ranksum_args
        g, n, m, K, ref = int(g), int(n), int(m), int(K), int(ref)
        check_ranksum_args(g, n, m, K, ref)
        if ldx < n or ldr < g:
            raise ValueError('dca_amd: ranksum: ldx = %d for %d cells, ldr = %d for %d genes' % (ldx, n, ldr, g))
        if x.dtype != torch.float32 or rank2.dtype != torch.int64 or tie.dtype != torch.int64:
            raise ValueError('dca_amd: ranksum: x is float32, rank2 and tie are int64')
        if gstart.dtype != torch.int32 or gstart.numel() < K + 1 or (m and (order.dtype != torch.int32 or order.numel() < m)):
            raise ValueError('dca_amd: ranksum: order is int32 [%d], gstart int32 [%d]' % (m, K + 1))
        need = self.ranksum_workspace_bytes(g, n)
        if ws.numel() * ws.element_size() < need:
            raise ValueError('dca_amd: ranksum: the workspace holds %d bytes, %d are needed'
                             % (ws.numel() * ws.element_size(), need))
        p = hip.ptr
        hip.check(self.L.dcahip_ranksum(p(x), ldx, g, n, p(order) if m else None, m, p(gstart), K, ref, p(rank2), p(tie), ldr,
                                        p(ws), hip.stream()), 'ranksum')

    def loss_finalize(self, partials, n, scale, loss_out):
        hip.check(self.L.dcahip_loss_finalize(hip.ptr(partials), n, scale, hip.ptr(loss_out),
                                              hip.stream()), 'loss_finalize')

    def step_end(self, loss, weight, hist, rows_per_slot, acc, cursor, advance):
        p = hip.ptr
        hip.check(self.L.dcahip_step_end(p(loss), weight, p(hist), rows_per_slot, p(acc), p(cursor),
                                         advance, hip.stream()), 'step_end')

    def heads_infer(self, a_mean, a_disp, a_pi, lda, sf, B, G, mean_sf, theta, pi, ldo, flags=0):
        p = hip.ptr
        hip.check(self.L.dcahip_zinb_heads_infer(p(a_mean), p(a_disp), p(a_pi), lda, p(sf), B, G,
                                                 p(mean_sf), p(theta), p(pi), ldo, flags, hip.stream()),
                  'heads_infer')

    # ------------------------------------------------------------------ fused heads
    def heads_fused_workspace_bytes(self, B, hL, G, plane, flags):
        return self.L.dcahip_heads_fused_workspace_bytes(B, hL, G, plane, flags)

    def x3_product_32x32(self, A, B, C, K):
        hip.check(self.L.dcahip_x3_product_32x32(hip.ptr(A), hip.ptr(B), hip.ptr(C), K, hip.stream()), "x3_product_32x32")

    def has(self, entry):
        """Whether the loaded library exports `entry`."""
        return hasattr(self.L, entry)

    def heads_tile_order_len(self, G):
        return int(self.L.dcahip_heads_tile_order_len(G))

    def heads_fused(self, H, ldh, Wh, ldw, bh, plane, theta_w, Y, ldy, sf, perm, cursor, B, hL, G,
                    ridge, inv_n, flags, gW, ldg, g_theta, dH, lddh, partials, ws, tile_order=None, loss_out=None,
                    compact=None, d_exp=0):
        """loss_out (a device float): the call also finishes the batch loss there (no loss_finalize launch needed).
        compact (dca_amd.compact.CompactCounts): the counts are read from the byte store instead of Y.
        d_exp (<= 0): scale exponent of the gradient planes for datasets with very large counts (include/dcahip.h)."""
        n = ctypes.c_int(0)
        p = hip.ptr
        c = compact
        hip.check(self.L.dcahip_heads_fused(p(H), ldh, p(Wh), ldw, p(bh), plane, p(theta_w), p(Y), ldy,
                                            p(c.Yc) if c is not None else None, c.ldc if c is not None else 0,
                                            p(c.ovf_ptr) if c is not None else None,
                                            p(c.ovf_col) if c is not None else None,
                                            p(c.ovf_val) if c is not None else None,
                                            p(sf), p(perm), p(cursor), B, hL, G, ridge, inv_n, flags,
                                            p(gW), ldg, p(g_theta), p(dH), lddh, p(partials),
                                            ctypes.byref(n), p(ws), ws.numel() * ws.element_size(),
                                            p(tile_order), p(loss_out), int(d_exp), hip.stream()), 'heads_fused')
        return n.value

    # ------------------------------------------------------------------ compact counts, sparse first layer
    def counts_compact_ld(self, G):
        return int(self.L.dcahip_counts_compact_ld(G))

    def counts_compact(self, Y, ldy, n, G, Yc, ldc, status):
        hip.check(self.L.dcahip_counts_compact(hip.ptr(Y), ldy, n, G, hip.ptr(Yc), ldc, hip.ptr(status), hip.stream()),
                  'counts_compact')

    def enc0_lut_entries(self):
        """Entries per cell of the table enc0_lut writes."""
        return int(self.L.dcahip_enc0_lut_entries())

    def enc0_lut(self, fac, do_log, n, lutp):
        hip.check(self.L.dcahip_enc0_lut(hip.ptr(fac), int(do_log), n, hip.ptr(lutp), hip.stream()), 'enc0_lut')

    def enc0_sparse_supported(self, H1):
        return bool(self.L.dcahip_enc0_sparse_supported(int(H1)))

    def enc0_dw_sparse_workspace_bytes(self, B, G, H1):
        return int(self.L.dcahip_enc0_dw_sparse_workspace_bytes(B, G, H1))

    def enc0_dw_sparse(self, c, perm, cursor, row_base, B, G, H1, dZ, ldz, gW, ldg, ws, form=0):
        """gW [G + 1, ldg] = [X^T dZ ; colsum dZ] with X described by the compact counts c (its normalisation fields).
        form: which of the two 64-unit kernels (0: by the shape, 1: the first, 2: the ring kernel; include/dcahip.h)."""
        p = hip.ptr
        c.ensure_lut(self)                   # the per-cell table of the common counts: made on the first call for this store
        hip.check(self.L.dcahip_enc0_dw_sparse(p(c.Yc), c.ldc, p(c.ovf_ptr), p(c.ovf_col), p(c.ovf_val), p(c.fac),
                                               int(c.do_log), p(c.lutp), p(c.mean), p(c.std), p(perm), p(cursor), int(row_base),
                                               B, G, H1, p(dZ), ldz, p(gW), ldg, p(ws), ws.numel() * ws.element_size(),
                                               int(form), hip.stream()), 'enc0_dw_sparse')

    def enc0_fwd_lut_workspace_bytes(self, B, G, H1):
        """0: this first-layer width is not taken by the matrix-pipe forward."""
        return int(self.L.dcahip_enc0_fwd_lut_workspace_bytes(B, G, H1))

    def enc0_fwd_lut(self, c, perm, cursor, row_base, B, G, H1, W, ldw, bias, Z, ldz, ws):
        """Z [B, ldz] = X W + bias on the matrix pipe, X looked up from the byte store; ws zero-initialised once."""
        p = hip.ptr
        c.ensure_lut(self)
        hip.check(self.L.dcahip_enc0_fwd_lut(p(c.Yc), c.ldc, p(c.ovf_ptr), p(c.ovf_col), p(c.ovf_val), p(c.fac),
                                             int(c.do_log), p(c.lutp), p(c.mean), p(c.std), p(perm), p(cursor), int(row_base),
                                             B, G, H1, p(W), ldw, p(bias), p(Z), ldz, p(ws),
                                             ws.numel() * ws.element_size(), hip.stream()), 'enc0_fwd_lut')

    # ------------------------------------------------------------------ gemm
    def sgemm_workspace_bytes(self, ta, tb, M, N, K, colsum_row=False, split_k=0):
        return self.L.dcahip_sgemm_workspace_bytes(int(ta), int(tb), M, N, K, int(colsum_row), split_k)

    def sgemm(self, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, perm=None, cursor=None,
              colsum_row=False, split_k=0, ws=None):
        p = hip.ptr
        wsb = ws.numel() * ws.element_size() if ws is not None else 0
        hip.check(self.L.dcahip_sgemm(int(ta), int(tb), M, N, K, p(A), lda, p(B), ldb, p(C), ldc,
                                      p(bias), p(perm), p(cursor), int(colsum_row), split_k, p(ws),
                                      wsb, hip.stream()), 'sgemm')

    def sgemm_plan(self, ta, tb, M, N, K, A, lda, B, ldb, colsum_row=False, split_k=0):
        """What sgemm would launch for these arguments (nothing is launched; A and B give their alignment only): the tuple
        (tile rows, tile columns, m tiles, n tiles, split, k slab, arithmetic 0 exact / 1 three bf16 pieces, loader width 4 / 1)."""
        out = (ctypes.c_int * 8)()
        hip.check(self.L.dcahip_sgemm_plan(int(ta), int(tb), M, N, K, int(colsum_row), split_k, hip.ptr(A), lda,
                                           hip.ptr(B), ldb, ctypes.addressof(out)), 'sgemm_plan')
        return tuple(out)

    @staticmethod
    def sgemm_reduce_lanes(split, outputs):
        """Lanes per output of the reduce behind a split product of `outputs` = (M + colsum_row) * N elements, as
        include/dcahip.h states the rule under dcahip_sgemm_plan: 0 (no reduce launch), 1 or 16."""
        if split <= 1:
            return 0
        return 16 if split >= 16 and outputs <= 65536 else 1

    # ------------------------------------------------------------------ products from pre-split operands
    def planes_alloc(self, rows, cols, device):
        """Three bf16 planes [3, rows, r8(cols)] (zeros)."""
        return torch.zeros(3, rows, (cols + 7) // 8 * 8, dtype=torch.bfloat16, device=device)

    def split_planes(self, src, ld, R, C, planes, perm=None, cursor=None):
        """planes [3, >= R, ldp] <- the three bf16 pieces of src [R, C] (rows gathered through perm / cursor)."""
        hip.check(self.L.dcahip_split_planes(hip.ptr(src), ld, hip.ptr(perm), hip.ptr(cursor), R, C, hip.ptr(planes),
                                             planes.shape[2], planes.stride(0), hip.stream()), 'split_planes')

    def gemm_p3_workspace_bytes(self, M, N, K, colsum_row=False, split_k=0):
        return self.L.dcahip_gemm_p3_workspace_bytes(M, N, K, int(colsum_row), split_k)

    def gemm_p3(self, ta, tb, M, N, K, A, B, C, ldc, bias=None, perm=None, cursor=None, colsum_row=False, split_k=0,
                ws=None):
        """C = op(A) op(B) from planes A, B ([3, rows, ld] bf16 tensors or views of them)."""
        p = hip.ptr
        wsb = ws.numel() * ws.element_size() if ws is not None else 0
        hip.check(self.L.dcahip_gemm_p3(int(ta), int(tb), M, N, K, p(A), A.stride(1), A.stride(0), p(B), B.stride(1),
                                        B.stride(0), p(C), ldc, p(bias), p(perm), p(cursor), int(colsum_row), split_k,
                                        p(ws), wsb, hip.stream()), 'gemm_p3')

    def gemm_planes_plan(self, pieces, ta, tb, M, N, K, gather=False, colsum_row=False, split_k=0):
        """What gemm_p3 (pieces 3) / gemm_h2 (pieces 2) would launch for this shape (nothing is launched): the tuple (kernel 0
        gemm_p3_kernel / 1 the 256 x 256 eight-wave kernel / 2 gemm_h2m_kernel, tile rows, tile columns, m tiles, n tiles,
        split, k slab, first tail tile, tail slices, k per tail slice, column-sum instantiation, workspace bytes)."""
        out = (ctypes.c_int * 12)()
        hip.check(self.L.dcahip_gemm_planes_plan(int(pieces), int(ta), int(tb), M, N, K, int(bool(gather)), int(colsum_row),
                                                 split_k, ctypes.addressof(out)), 'gemm_planes_plan')
        return tuple(out)

    # ---- fp16 x 2 planes (include/dcahip.h: dcahip_gemm_h2).  exp: an int32 device tensor [2] = (block exponent, scratch)
    def absmax_exp(self, src, ld, R, C, exp):
        """exp[0] <- the exponent that brings max |src [R, C]| into [2^13, 2^14) (stays on the device: capturable)."""
        hip.check(self.L.dcahip_absmax_exp(hip.ptr(src), ld, R, C, hip.ptr(exp), hip.ptr(exp[1:]), hip.stream()), 'absmax_exp')

    def split_planes_h2(self, src, ld, R, C, planes, exp=None, perm=None, cursor=None):
        """planes [>= 2, >= R, ldp] <- the two fp16 pieces of src [R, C] 2^exp[0] (rows gathered through perm / cursor)."""
        hip.check(self.L.dcahip_split_planes_h2(hip.ptr(src), ld, hip.ptr(perm), hip.ptr(cursor), R, C, hip.ptr(planes),
                                                planes.shape[2], planes.stride(0), hip.ptr(exp), hip.stream()), 'split_planes_h2')

    def gemm_h2_supported(self, M, N, K):
        return bool(self.L.dcahip_gemm_h2_supported(M, N, K))

    def gemm_h2_workspace_bytes(self, M, N, K, colsum_row=False, split_k=0):
        return self.L.dcahip_gemm_h2_workspace_bytes(M, N, K, int(colsum_row), split_k)

    def gemm_h2(self, ta, tb, M, N, K, A, B, C, ldc, exp_a=None, exp_b=None, exp_a_add=0, exp_b_add=0, alpha=1.0, bias=None,
                colsum_row=False, split_k=0, ws=None):
        """C = alpha 2^-(ea + eb) op(A) op(B) from fp16 x 2 planes A, B ([>= 2, rows, ld] tensors or views of them)."""
        p = hip.ptr
        wsb = ws.numel() * ws.element_size() if ws is not None else 0
        hip.check(self.L.dcahip_gemm_h2(int(ta), int(tb), M, N, K, p(A), A.stride(1), A.stride(0), p(exp_a), int(exp_a_add),
                                        p(B), B.stride(1), B.stride(0), p(exp_b), int(exp_b_add), float(alpha), p(C), ldc, p(bias),
                                        int(colsum_row), split_k, p(ws), wsb, hip.stream()), 'gemm_h2')

    def transpose(self, src, ld_src, R, C, dst, ld_dst, perm=None, cursor=None):
        """dst [C, R] = src[rows]^T; rows = perm[cursor : cursor + R] when perm is given."""
        hip.check(self.L.dcahip_transpose_rows(hip.ptr(src), ld_src, hip.ptr(perm), hip.ptr(cursor), R, C,
                                               hip.ptr(dst), ld_dst, hip.stream()), 'transpose')

    # ------------------------------------------------------------------ batch norm
    def col_moments_chunks(self, B):
        return self.L.dcahip_col_moments_chunks(B)

    def col_moments(self, Z, ldz, B, H, part):
        hip.check(self.L.dcahip_col_moments(hip.ptr(Z), ldz, B, H, hip.ptr(part), hip.stream()),
                  'col_moments')

    def moments_combine(self, entries, counts, E, H, out):
        hip.check(self.L.dcahip_moments_combine(hip.ptr(entries), hip.ptr(counts), E, H, hip.ptr(out),
                                                hip.stream()), 'moments_combine')

    def bn_relu_apply(self, Z, ldz, B, H, entries, counts, E, beta, mm, mv, momentum, eps, relu,
                      Hout, ldh, xhat, ldx, inv_std):
        p = hip.ptr
        hip.check(self.L.dcahip_bn_relu_apply(p(Z), ldz, B, H, p(entries), p(counts), E, p(beta),
                                              p(mm), p(mv), momentum, eps, int(relu), p(Hout), ldh,
                                              p(xhat), ldx, p(inv_std), hip.stream()), 'bn_relu_apply')

    # beta (the batch-norm backward entries below): the layer's batch-norm offset, which codes >= hip.ACT_PRE need for their
    # pre-activation xhat + beta; the other codes do not read it (None: NULL)
    def bn_bwd_sums(self, dH, ldd, Hact, ldh, xhat, ldx, B, H, part, act=1, beta=None):
        p = hip.ptr
        hip.check(self.L.dcahip_bn_bwd_sums(p(dH), ldd, p(Hact), ldh, p(xhat), ldx, B, H, p(part),
                                            act, p(beta), hip.stream()), 'bn_bwd_sums')

    def bn_bwd_apply(self, dH, ldd, Hact, ldh, xhat, ldx, inv_std, sums, E, n_total, B, H, dZ, ldz,
                     dbeta, act=1, beta=None):
        p = hip.ptr
        hip.check(self.L.dcahip_bn_bwd_apply(p(dH), ldd, p(Hact), ldh, p(xhat), ldx, p(inv_std),
                                             p(sums), E, float(n_total), B, H, p(dZ), ldz, p(dbeta),
                                             act, p(beta), hip.stream()), 'bn_bwd_apply')

    @property
    def bn_fused_max_rows(self):
        return int(self.L.dcahip_bn_fused_max_rows())

    def bn_relu_train_small(self, Z, ldz, B, H, beta, mm, mv, momentum, eps, act, Hout, ldh, xhat, ldx, inv_std):
        p = hip.ptr
        hip.check(self.L.dcahip_bn_relu_train_small(p(Z), ldz, B, H, p(beta), p(mm), p(mv), momentum, eps, int(act),
                                                    p(Hout), ldh, p(xhat), ldx, p(inv_std), hip.stream()),
                  'bn_relu_train_small')

    def bn_bwd_small(self, dH, ldd, Hact, ldh, xhat, ldx, inv_std, n_total, B, H, dZ, ldz, dbeta, act=1, beta=None):
        p = hip.ptr
        hip.check(self.L.dcahip_bn_bwd_small(p(dH), ldd, p(Hact), ldh, p(xhat), ldx, p(inv_std), float(n_total), B, H,
                                             p(dZ), ldz, p(dbeta), act, p(beta), hip.stream()), 'bn_bwd_small')

    @property
    def dense_small_max_k(self):
        return int(self.L.dcahip_dense_small_max_k())

    def dense_bn_small(self, Hp, ldp, W, ldw, bias, B, K, H, batchnorm, beta, mm, mv, momentum, eps, act, Z, ldz,
                       xhat, ldx, Hout, ldh, inv_std):
        p = hip.ptr
        hip.check(self.L.dcahip_dense_bn_small(p(Hp), ldp, p(W), ldw, p(bias), B, K, H, int(batchnorm), p(beta), p(mm), p(mv),
                                               momentum, eps, int(act), p(Z), ldz, p(xhat), ldx, p(Hout), ldh, p(inv_std),
                                               hip.stream()), 'dense_bn_small')

    def hidden_small_chain(self, layers, Hin, ldin, B, batchnorm, momentum, eps, act):
        """layers: dicts with the fields of dcahip_small_layer (tensors or None); one launch for the whole list."""
        arr = self._small_layers(layers)
        hip.check(self.L.dcahip_hidden_small_chain(arr, len(layers), hip.ptr(Hin), ldin, B, int(batchnorm), momentum, eps,
                                                   int(act), hip.stream()), 'hidden_small_chain')

    # ------------------------------------------------------------------ K-STACK (throughput batches, one launch per direction)
    @property
    def hidden_stack_max_rows(self):
        return int(self.L.dcahip_hidden_stack_max_rows())

    def hidden_stack_workspace_bytes(self, n_layers, B):
        return int(self.L.dcahip_hidden_stack_workspace_bytes(n_layers, B))

    def hidden_stack_fwd(self, layers, B, momentum, eps, act, ws, rows_per_wg=64, steps=None):
        """layers: dicts with the fields of dcahip_small_layer; entry 0 without a kernel (its Z comes from the first GEMM).
        steps = (first, last) of the pass's n + 1 steps in ONE launch (default: all of them, cooperative)."""
        arr = self._small_layers(layers)
        first, last = steps if steps is not None else (0, len(layers))
        hip.check(self.L.dcahip_hidden_stack_fwd(arr, len(layers), B, momentum, eps, int(act), int(rows_per_wg), first, last,
                                                 hip.ptr(ws), ws.numel() * ws.element_size(), hip.stream()), 'hidden_stack_fwd')

    def hidden_stack_bwd(self, layers, B, n_total, act, dZ0, ldz0, ws, rows_per_wg=64, steps=None):
        """layers: dicts with the fields of dcahip_stack_bwd_layer; steps = (first, last) of the pass's n + 2 steps.
        A whole pass over a batch of at most 64 rows is one workgroup's work and needs no workspace (ws=None)."""
        arr = self._bwd_layers(layers)
        first, last = steps if steps is not None else (0, len(layers) + 1)
        hip.check(self.L.dcahip_hidden_stack_bwd(arr, len(layers), B, float(n_total), int(act), hip.ptr(dZ0), ldz0,
                                                 int(rows_per_wg), first, last, hip.ptr(ws),
                                                 0 if ws is None else ws.numel() * ws.element_size(),
                                                 hip.stream()), 'hidden_stack_bwd')

    # ---- the two layer structs of include/dcahip.h, filled from dicts with their fields (tensors or None; absent: NULL / 0)
    def _small_layers(self, layers):
        arr = (hip.SmallLayer * len(layers))()
        for q, d in zip(arr, layers):
            for k in ('W', 'bias', 'beta', 'moving_mean', 'moving_var', 'Z', 'xhat', 'Hout', 'inv_std'):
                setattr(q, k, hip.ptr(d.get(k)))
            for k in ('ldw', 'K', 'H', 'ldz', 'ldx', 'ldh'):
                setattr(q, k, int(d.get(k, 0)))
        return arr

    def _bwd_layers(self, layers):
        arr = (hip.StackBwdLayer * len(layers))()
        for q, d in zip(arr, layers):
            for k in ('W', 'Hact', 'xhat', 'inv_std', 'Hprev', 'gW', 'dbeta', 'dH', 'beta'):
                setattr(q, k, hip.ptr(d.get(k)))
            for k in ('ldw', 'K', 'H', 'ldh', 'ldx', 'ldp', 'ldg', 'lddh'):
                setattr(q, k, int(d.get(k, 0)))
        return arr

    # ---- K-STACK between the exchanges of a data-parallel step (SyncBN): one step per call
    def hidden_stack_fwd_sync(self, layers, B, momentum, eps, act, step, ext_entries, ext_counts, ext_E, stat_out, ws):
        """Step `step` of the forward pass with the input layer's statistics from every rank (ext_entries [E, 2, H],
        ext_counts [E]); stat_out [2, H'] <- this rank's (mean, M2) of the layer made."""
        arr = self._small_layers(layers)
        hip.check(self.L.dcahip_hidden_stack_fwd_sync(arr, len(layers), B, momentum, eps, int(act), int(step),
                                                      hip.ptr(ext_entries), hip.ptr(ext_counts), int(ext_E), hip.ptr(stat_out),
                                                      hip.ptr(ws), ws.numel() * ws.element_size(), hip.stream()),
                  'hidden_stack_fwd_sync')

    def hidden_stack_bwd_sync(self, layers, B, n_total, act, dZ0, ldz0, step, ext_sums, sums_out, ws):
        arr = self._bwd_layers(layers)
        hip.check(self.L.dcahip_hidden_stack_bwd_sync(arr, len(layers), B, float(n_total), int(act), hip.ptr(dZ0), ldz0,
                                                      int(step), hip.ptr(ext_sums), hip.ptr(sums_out), hip.ptr(ws),
                                                      ws.numel() * ws.element_size(), hip.stream()), 'hidden_stack_bwd_sync')

    def dense_bn_bwd_small(self, dH, ldd, Hact, ldh, xhat, ldx, inv_std, Hp, ldp, W, ldw, B, K, H, batchnorm, n_total, act,
                           gW, ldg, dbeta, dHp, lddp, beta=None):
        p = hip.ptr
        hip.check(self.L.dcahip_dense_bn_bwd_small(p(dH), ldd, p(Hact), ldh, p(xhat), ldx, p(inv_std), p(Hp), ldp, p(W), ldw,
                                                   B, K, H, int(batchnorm), float(n_total), int(act), p(gW), ldg, p(dbeta),
                                                   p(dHp), lddp, p(beta), hip.stream()), 'dense_bn_bwd_small')

    def relu_bwd(self, dH, ldd, Hact, ldh, B, H, dZ, ldz, act=1):
        p = hip.ptr
        hip.check(self.L.dcahip_relu_bwd(p(dH), ldd, p(Hact), ldh, B, H, p(dZ), ldz, act, hip.stream()),
                  'relu_bwd')

    def relu_fwd(self, Z, ldz, B, H, Hout, ldh, act=1):
        hip.check(self.L.dcahip_relu_fwd(hip.ptr(Z), ldz, B, H, hip.ptr(Hout), ldh, act, hip.stream()),
                  'relu_fwd')

    def colsum_chain(self, x, ldx, B, N, theta_w, out):
        p = hip.ptr
        hip.check(self.L.dcahip_colsum_chain(p(x), ldx, B, N, p(theta_w), p(out), hip.stream()),
                  'colsum_chain')

    # ------------------------------------------------------------------ other optimizers, regularisers
    def optimizer_step(self, kind, w, g, slot1, slot2, n, lr, it, clip):
        p = hip.ptr
        hip.check(self.L.dcahip_optimizer_step(hip.OPT_KINDS[kind], p(w), p(g), p(slot1), p(slot2), n, p(lr),
                                               p(it), clip, hip.stream()), 'optimizer_step')

    def prelu_workspace_doubles(self, h):
        return int(self.L.dcahip_prelu_workspace_doubles(h))

    def prelu_fwd(self, x, ldx, alpha, B, h, out, ldo):
        p = hip.ptr
        hip.check(self.L.dcahip_prelu_fwd(p(x), ldx, p(alpha), B, h, p(out), ldo, hip.stream()), 'prelu_fwd')

    def prelu_bwd(self, d, ldd, x, ldx, alpha, B, h, galpha, ws):
        p = hip.ptr
        hip.check(self.L.dcahip_prelu_bwd(p(d), ldd, p(x), ldx, p(alpha), B, h, p(galpha), p(ws), hip.stream()),
                  'prelu_bwd')

    def elempi_workspace_doubles(self, G):
        return int(self.L.dcahip_elempi_workspace_doubles(G))

    def elempi_fwd(self, a_mean, lda, k, c, B, G, a_pi, ldp):
        p = hip.ptr
        hip.check(self.L.dcahip_elempi_fwd(p(a_mean), lda, p(k), p(c), B, G, p(a_pi), ldp, hip.stream()), 'elempi_fwd')

    def elempi_bwd(self, m, lda, d_mean, d_pi, ldd, k, B, G, gk, gc, ws):
        p = hip.ptr
        hip.check(self.L.dcahip_elempi_bwd(p(m), lda, p(d_mean), p(d_pi), ldd, p(k), B, G, p(gk), p(gc), p(ws),
                                           hip.stream()), 'elempi_bwd')

    def bcast_cols(self, s, lds, B, G, out, ldo):
        hip.check(self.L.dcahip_bcast_cols(hip.ptr(s), lds, B, G, hip.ptr(out), ldo, hip.stream()), 'bcast_cols')

    def row_sums_strided(self, x, ldx, B, G, out, ldo):
        hip.check(self.L.dcahip_row_sums_strided(hip.ptr(x), ldx, B, G, hip.ptr(out), ldo, hip.stream()),
                  'row_sums_strided')

    def nadam_step(self, w, g, m, v, n, lr, it, m_schedule, clip):
        p = hip.ptr
        hip.check(self.L.dcahip_nadam_step(p(w), p(g), p(m), p(v), n, p(lr), p(it), p(m_schedule), clip, hip.stream()),
                  'nadam_step')

    def dropout_apply(self, x, ldx, perm, cursor, B, h, rate, seed, step, layer, row0, out, ldo):
        p = hip.ptr
        hip.check(self.L.dcahip_dropout_apply(p(x), ldx, p(perm), p(cursor), B, h, float(rate), int(seed),
                                              p(step), int(layer), int(row0), p(out), ldo, hip.stream()),
                  'dropout_apply')

    def counter_add(self, counter, v):
        hip.check(self.L.dcahip_counter_add(hip.ptr(counter), v, hip.stream()), 'counter_add')

    def reg_desc(self, segs):
        """segs: list of (start, end, l1, l2) over the flat parameter buffer."""
        d = hip.RegDesc()
        d.nseg = len(segs)
        for k, (a, b, l1, l2) in enumerate(segs):
            d.start[k], d.end[k], d.l1[k], d.l2[k] = int(a), int(b), float(l1), float(l2)
        return d

    def l1l2_workspace_doubles(self):
        return self.L.dcahip_l1l2_workspace_doubles()

    def l1l2_apply(self, desc, w, g, loss_inout, ws):
        p = hip.ptr
        hip.check(self.L.dcahip_l1l2_apply(ctypes.byref(desc), p(w), p(g), p(loss_inout), p(ws),
                                           hip.stream()), 'l1l2_apply')

    # ------------------------------------------------------------------ preprocessing
    def prep_chunks(self, n):
        return self.L.dcahip_prep_chunks(n)

    def prep_row_sums(self, Y, ldy, n, G, out):
        hip.check(self.L.dcahip_prep_row_sums(hip.ptr(Y), ldy, n, G, hip.ptr(out), hip.stream()),
                  'prep_row_sums')

    def prep_col_pass(self, Y, ldy, n, G, fac, do_log, X, ldx, col_part):
        p = hip.ptr
        hip.check(self.L.dcahip_prep_col_pass(p(Y), ldy, n, G, p(fac), int(do_log), p(X), ldx,
                                              p(col_part), hip.stream()), 'prep_col_pass')

    def prep_col_finish(self, col_part, R, G, n_total, sums, mean, stdv):
        p = hip.ptr
        hip.check(self.L.dcahip_prep_col_finish(p(col_part), R, G, float(n_total), p(sums), p(mean),
                                                p(stdv), hip.stream()), 'prep_col_finish')

    def prep_scale(self, X, ldx, n, G, mean, stdv):
        p = hip.ptr
        hip.check(self.L.dcahip_prep_scale(p(X), ldx, n, G, p(mean), p(stdv), hip.stream()), 'prep_scale')

    def csr_expand(self, indptr, indices, values, nnz, rows, G, Y, ldy, status):
        """Rows of a CSR chunk (int32 indptr / indices, fp32 values, device tensors) -> every element of Y[:rows, :ldy];
        status (int32 device word) += what had to be ignored (include/dcahip.h)."""
        p = hip.ptr
        hip.check(self.L.dcahip_csr_expand(p(indptr), p(indices), p(values), nnz, rows, G, p(Y), ldy, p(status),
                                           hip.stream()), 'csr_expand')

    def csr_compress(self, X, ld, rows, G, base, indptr, indices, values, status):
        """Dense fp32 rows X[:rows, :G] (row stride ld) -> their CSR: indptr[:rows + 1] (int64, from `base` on), the entries
        from position 0 of indices (int32) / values (fp32), whose common length is the capacity; status (int32 device word)
        += the entries that did not fit (include/dcahip.h)."""
        p = hip.ptr
        cap = min(int(indices.numel()), int(values.numel()))
        hip.check(self.L.dcahip_csr_compress(p(X), ld, rows, G, int(base), p(indptr), p(indices), p(values), cap, p(status),
                                             hip.stream()), 'csr_compress')

    def csr_subset(self, csr, row_keep, col_keep, n_out, out_indptr, out_indices, out_values, ws, status):
        """A resident CSR (prep.CsrCounts) without the rows / columns whose byte in row_keep [n] / col_keep [G] (uint8 or
        bool device tensors, None: keep all) is 0 -> out_indptr[:n_out + 1] (int64, from 0), the kept entries in out_indices /
        out_values (their common length is the capacity), columns renumbered; ws: n + G int32 of scratch; status (int32
        device word) += what had to be ignored or did not fit, or that row_keep does not keep n_out rows (include/dcahip.h)."""
        p = hip.ptr
        cap = min(int(out_indices.numel()), int(out_values.numel()))
        hip.check(self.L.dcahip_csr_subset(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G, p(row_keep),
                                           p(col_keep), int(n_out), p(out_indptr), p(out_indices), p(out_values), cap, p(ws),
                                           p(status), hip.stream()), 'csr_subset')

    def csr_thin(self, csr, row_ids, threshold, seed):
        """K-SPLIT (include/dcahip.h, dcahip_csr_thin): the resident CSR (prep.CsrCounts) thinned binomially into two parts,
        (A, B) as new CsrCounts with A + B = csr: of every count y, a ~ Binomial(y, threshold / 2^32) molecules go to A and
        y - a to B, drawn from Philox4x32-10 with key `seed` and the counter (cell, gene, molecule block).  row_ids: int64
        [n] device tensor of the rows' global cell ids (None: row r is cell r).  The outputs are allocated at csr.nnz and cut
        to their own size.  A value that is not a count (negative, fractional, above 2^24) or a malformed CSR raises
        ValueError."""
        from .prep import CsrCounts
        p = hip.ptr
        threshold, seed = int(threshold), int(seed) & 0xffffffffffffffff
        if not 0 <= threshold <= 1 << 32:
            raise ValueError('dca_amd: csr_thin: threshold must lie in [0, 2^32] (got %d)' % threshold)
        dev, n, nnz = csr.device, csr.n, csr.nnz
        if row_ids is not None:
            assert row_ids.dtype == torch.int64 and row_ids.numel() >= n
        parts = [(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev),
                  torch.empty(nnz, dtype=torch.float32, device=dev)) for _ in range(2)]
        ws = torch.empty(int(self.L.dcahip_csr_thin_workspace_bytes(n, nnz)), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        (pa, ia, va), (pb, ib, vb) = parts
        hip.check(self.L.dcahip_csr_thin(p(csr.indptr), p(csr.indices) if nnz else None, p(csr.values) if nnz else None, nnz,
                                         n, csr.G, p(row_ids), threshold, seed, p(pa), p(ia) if nnz else None,
                                         p(va) if nnz else None, p(pb), p(ib) if nnz else None, p(vb) if nnz else None, nnz,
                                         p(ws) if nnz else None, p(status), hip.stream()), 'csr_thin')
        ends = torch.stack([pa[n], pb[n]]).cpu()
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: csr_thin: %d values are not counts (negative, not an integer or above 2^24), or '
                             'entries / rows lie outside the matrix' % bad)
        out = []
        for (ptr, idx, val), total in zip(parts, ends.tolist()):
            if total < nnz:
                idx, val = idx[:total].clone(), val[:total].clone()
            out.append(CsrCounts(ptr, idx, val, n, csr.G))
        return out[0], out[1]

    def knn_splits(self, nq, n, d, k):
        """The number of candidate splits dcahip_knn takes for this shape when it is asked for 0."""
        s = int(self.L.dcahip_knn_splits(nq, n, d, k))
        hip.check(min(s, 0), 'knn_splits')
        return s

    def knn(self, Q, X, k, self_offset=-1, splits=0, out=None):
        """K-NEIGHBOURS (include/dcahip.h, dcahip_knn): the k nearest rows of X [n, d] to every row of Q [nq, d] (fp32 device
        tensors, unit column stride, any row stride), exact, Euclidean.  Returns (idx [nq, k] int32, d2 [nq, k] float32):
        per query the k smallest under (squared distance, index), in that order; -1 / +inf where X has fewer than k rows.
        self_offset >= 0: query q is row self_offset + q of X and is left out by index.  splits: 0 = the library's choice,
        1 .. 64 = that many candidate ranges (same bits).  out: (idx, d2) tensors to write into (row stride >= k, the same
        for both).  A limit of the kernel (k 1 .. 64, d 1 .. 128) or a non-finite coordinate raises ValueError."""
        from .neighbors import check_knn_args
        p = hip.ptr
        for t in (Q, X):
            if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError('dca_amd: knn: operands are 2-d float32 tensors with unit column stride')
        (nq, d), n = Q.shape, X.shape[0]
        if X.shape[1] != d:
            raise ValueError('dca_amd: knn: queries have %d columns, candidates %d' % (d, X.shape[1]))
        k, splits, self_offset = int(k), int(splits), int(self_offset)
        check_knn_args(nq, n, d, k, splits, self_offset)
        dev = X.device
        if out is None:
            idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
            d2 = torch.empty(nq, k, dtype=torch.float32, device=dev)
        else:
            idx, d2 = out
            if idx.dtype != torch.int32 or d2.dtype != torch.float32 or idx.shape != (nq, k) or d2.shape != (nq, k) or \
                    (nq > 1 and idx.stride(0) != d2.stride(0)) or (k > 1 and (idx.stride(1) != 1 or d2.stride(1) != 1)):
                raise ValueError('dca_amd: knn: out = (int32 [nq, k], float32 [nq, k]) with one row stride')
        if nq == 0:
            return idx, d2
        ldq = Q.stride(0) if nq > 1 else d
        ldx = X.stride(0) if n > 1 else d
        ldo = idx.stride(0) if nq > 1 else k
        nbytes = int(self.L.dcahip_knn_workspace_bytes(nq, n, d, k, splits))
        hip.check(min(nbytes, 0), 'knn_workspace_bytes')
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.check(self.L.dcahip_knn(p(Q), ldq, nq, p(X) if n else None, ldx, n, d, k, self_offset, splits, p(idx), p(d2), ldo,
                                    p(ws), p(status), hip.stream()), 'knn')
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: knn: %d coordinates are not finite (NaN or inf)' % bad)
        return idx, d2

    def kmeans_workspace_bytes(self, n, d, k):
        """The workspace of kmeans_seed and kmeans_step for this shape, in bytes."""
        from .cluster import check_kmeans_args
        check_kmeans_args(int(n), int(d), int(k))
        nbytes = int(self.L.dcahip_kmeans_workspace_bytes(n, d, k))
        hip.check(min(nbytes, 0), 'kmeans_workspace_bytes')
        return nbytes

    @staticmethod
    def _kmeans_points(X, what='points'):
        if X.dtype != torch.float32 or X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1):
            raise ValueError('dca_amd: kmeans: the %s are a 2-d float32 tensor with unit column stride' % what)
        return X.stride(0) if X.shape[0] > 1 else X.shape[1]

    def kmeans_raise(self, status):
        """Reads the status word of kmeans_seed / kmeans_step (a synchronisation) and raises on non-finite coordinates."""
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: kmeans: %d coordinates are not finite (NaN or inf)' % bad)

    def kmeans_seed(self, X, k, seed=0, init=0, ws=None):
        """K-MEANS (include/dcahip.h, dcahip_kmeans_seed): k-means++ seeds of the rows of X [n, d] (fp32 device tensor, unit
        column stride), drawn on the device with the integer arithmetic tests/_kmeans_ref.seed_ref restates.  Returns
        (rows int32 [k], C float32 [k, d] = those rows of X).  (seed, init) name the draw.  A limit of the kernel or a
        non-finite coordinate raises ValueError."""
        from .cluster import check_kmeans_args
        p = hip.ptr
        ldx = self._kmeans_points(X)
        n, d = X.shape
        k, seed, init = int(k), int(seed), int(init)
        check_kmeans_args(n, d, k)
        if n < 1:
            raise ValueError('dca_amd: kmeans: no points to draw seeds from')
        if not 0 <= seed < 1 << 64 or not 0 <= init < 1 << 31:
            raise ValueError('dca_amd: kmeans: seed is an unsigned 64-bit, init a non-negative 32-bit integer (got %d, %d)'
                             % (seed, init))
        dev = X.device
        need = self.kmeans_workspace_bytes(n, d, k)
        if ws is None:
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        if ws.numel() * ws.element_size() < need:
            raise ValueError('dca_amd: kmeans: the workspace holds %d bytes, %d are needed' % (ws.numel() * ws.element_size(), need))
        rows = torch.empty(k, dtype=torch.int32, device=dev)
        C = torch.empty(k, d, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.check(self.L.dcahip_kmeans_seed(p(X), ldx, n, d, k, seed, init, p(rows), p(C), d, p(ws), p(status), hip.stream()),
                  'kmeans_seed')
        self.kmeans_raise(status)
        return rows, C

    def kmeans_bind(self, X, C_in, C_out, labels, d2, counts, sums, inertia, info, ws, status):
        """The arguments of kmeans_step checked once: returns ``step(it)``, which enqueues iteration ``it`` >= 1 on these
        tensors and nothing else (a Lloyd loop is launch-bound: the checks are not repeated per iteration)."""
        from .cluster import check_kmeans_args
        p = hip.ptr
        ldx = self._kmeans_points(X)
        ldc = self._kmeans_points(C_in, 'centres')
        ldco = self._kmeans_points(C_out, 'centres')
        n, d = X.shape
        k = C_in.shape[0]
        check_kmeans_args(n, d, k)
        if C_in.shape[1] != d or tuple(C_out.shape) != (k, d):
            raise ValueError('dca_amd: kmeans: points have %d columns, the centres are %s and %s'
                             % (d, tuple(C_in.shape), tuple(C_out.shape)))
        for t, dt, shape, name in ((labels, torch.int32, (n,), 'labels'), (d2, torch.float32, (n,), 'd2'),
                                   (counts, torch.int32, (k,), 'counts'), (sums, torch.float64, (k, d), 'sums'),
                                   (inertia, torch.float64, (1,), 'inertia'), (info, torch.int32, (3,), 'info'),
                                   (status, torch.int32, (1,), 'status')):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError('dca_amd: kmeans: %s is a contiguous %s tensor of shape %s' % (name, dt, shape))
        need = self.kmeans_workspace_bytes(n, d, k)
        if ws.numel() * ws.element_size() < need:
            raise ValueError('dca_amd: kmeans: the workspace holds %d bytes, %d are needed' % (ws.numel() * ws.element_size(), need))
        fn = self.L.dcahip_kmeans_step
        head = (p(X), ldx, n, d, k, p(C_in), ldc, p(C_out), ldco, p(labels), p(d2), p(counts), p(sums), d, p(inertia),
                p(info), p(info) + 4, p(info) + 8) if n else None
        tail = (p(ws), p(status)) if n else None
        keep = (X, C_in, C_out, labels, d2, counts, sums, inertia, info, ws, status)      # alive as long as the closure

        def step(it):
            if int(it) < 1:
                raise ValueError('dca_amd: kmeans: iterations are numbered from 1 (got %d)' % it)
            if keep[0].shape[0]:
                hip.check(fn(*head, int(it), *tail, hip.stream()), 'kmeans_step')
        return step

    def kmeans_step(self, X, C_in, C_out, labels, d2, counts, sums, inertia, info, it, ws, status, check=True):
        """K-MEANS (include/dcahip.h, dcahip_kmeans_step): one Lloyd iteration, number ``it`` >= 1, of the points X [n, d]
        from the centres C_in [k, d] -> C_out [k, d] (may be C_in); labels int32 [n] in / out (-1 before the first
        iteration), d2 float32 [n], counts int32 [k], sums float64 [k, d], inertia float64 [1], info int32 [3] = (changed,
        reseeded, state: zeroed before the first iteration, the first converged iteration afterwards).  status: int32 [1],
        zeroed by the caller; check=True reads it (a synchronisation) and raises on non-finite coordinates, check=False
        leaves that to a later kmeans_raise(status)."""
        self.kmeans_bind(X, C_in, C_out, labels, d2, counts, sums, inertia, info, ws, status)(it)
        if check:
            self.kmeans_raise(status)

    def silhouette_splits(self, n, d, k):
        """The number of candidate splits dcahip_silhouette takes for this shape when it is asked for 0."""
        from .silhouette import check_silhouette_args
        check_silhouette_args(int(n), int(d), int(k))
        s = int(self.L.dcahip_silhouette_splits(n, d, k))
        hip.check(min(s, 0), 'silhouette_splits')
        return s

    def silhouette_workspace_bytes(self, n, d, k, splits=0):
        """The workspace of silhouette for this shape and this many splits (0: the library's choice), in bytes."""
        from .silhouette import check_silhouette_args
        check_silhouette_args(int(n), int(d), int(k), int(splits))
        nbytes = int(self.L.dcahip_silhouette_workspace_bytes(n, d, k, splits))
        hip.check(min(nbytes, 0), 'silhouette_workspace_bytes')
        return nbytes

    def silhouette_raise(self, status, counts):
        """Reads the status word and the cluster sizes of silhouette (a synchronisation) and raises on non-finite coordinates
        and on fewer than two clusters with points."""
        bad, live = torch.stack([status[0].to(torch.int64), (counts > 0).sum()]).tolist()
        if bad:
            raise ValueError('dca_amd: silhouette: %d coordinates are not finite (NaN or inf)' % bad)
        if live < 2:
            raise ValueError('dca_amd: silhouette: %d cluster%s with points: a silhouette compares at least 2'
                             % (live, '' if live == 1 else 's'))

    def silhouette(self, X, labels, k, splits=0, ws=None):
        """K-SILHOUETTE (include/dcahip.h, dcahip_silhouette): the silhouette coefficient of every row of X [n, d] (fp32
        device tensor, unit column stride, any row stride) under labels [n] (int32 codes in [0, k); any other value: in no
        cluster), Euclidean, every pair visited.  Returns a dict of device tensors: s, a, b float64 [n] (NaN for a point in no
        cluster), nearest int32 [n] (-1), counts int32 [k], cluster_mean float64 [k], mean float64 [1].  splits: 0 = the
        library's choice, 1 .. 64 = that many candidate ranges.  A limit of the kernel (k 2 .. 256, d 1 .. 128), a non-finite
        coordinate or fewer than two clusters with points raises ValueError."""
        from .silhouette import check_silhouette_args
        p = hip.ptr
        if X.dtype != torch.float32 or X.dim() != 2 or (X.shape[1] > 1 and X.stride(1) != 1):
            raise ValueError('dca_amd: silhouette: the points are a 2-d float32 tensor with unit column stride')
        n, d = X.shape
        if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
            raise ValueError('dca_amd: silhouette: labels is a contiguous int32 tensor of shape (%d,)' % n)
        k, splits = int(k), int(splits)
        check_silhouette_args(n, d, k, splits)
        ldx = X.stride(0) if n > 1 else d
        dev = X.device
        need = self.silhouette_workspace_bytes(n, d, k, splits)
        if ws is None:
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        if ws.numel() * ws.element_size() < need:
            raise ValueError('dca_amd: silhouette: the workspace holds %d bytes, %d are needed'
                             % (ws.numel() * ws.element_size(), need))
        nan = float('nan')
        r = dict(s=torch.full((n,), nan, dtype=torch.float64, device=dev), a=torch.full((n,), nan, dtype=torch.float64, device=dev),
                 b=torch.full((n,), nan, dtype=torch.float64, device=dev), nearest=torch.full((n,), -1, dtype=torch.int32, device=dev),
                 counts=torch.zeros(k, dtype=torch.int32, device=dev),
                 cluster_mean=torch.full((k,), nan, dtype=torch.float64, device=dev),
                 mean=torch.full((1,), nan, dtype=torch.float64, device=dev))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.check(self.L.dcahip_silhouette(p(X) if n else None, ldx, n, d, p(labels) if n else None, k, splits, p(r['s']), p(r['a']),
                                           p(r['b']), p(r['nearest']), p(r['counts']), p(r['cluster_mean']), p(r['mean']),
                                           p(ws), p(status), hip.stream()), 'silhouette')
        self.silhouette_raise(status, r['counts'])
        return r

    def graph_symmetrize_workspace_bytes(self, n, k):
        """The workspace of graph_symmetrize for an [n, k] index array, in bytes."""
        from .community import check_graph_args
        check_graph_args(int(n), int(k))
        nbytes = int(self.L.dcahip_graph_symmetrize_workspace_bytes(n, k))
        hip.check(min(nbytes, 0), 'graph_symmetrize_workspace_bytes')
        return nbytes

    def graph_symmetrize(self, idx):
        """K-LOUVAIN (include/dcahip.h, dcahip_graph_symmetrize): W = A + A^T of the index array idx [n, k] (int32 device
        tensor, unit column stride; -1 is padding, an entry equal to its row is dropped) as a CSR of unit entries.  Returns
        (rowptr int64 [n + 1], col int32 [2m], deg int32 [n]); the order inside a row is not fixed.  Reads 2m (a
        synchronisation).  An entry outside 0 .. n-1 other than -1, or a limit of the kernel (2 n k < 2^31), raises
        ValueError."""
        from .community import check_graph_args
        p = hip.ptr
        if idx.dtype != torch.int32 or idx.dim() != 2 or (idx.shape[1] > 1 and idx.stride(1) != 1):
            raise ValueError('dca_amd: louvain: the neighbour indices are a 2-d int32 tensor with unit column stride')
        n, k = idx.shape
        check_graph_args(n, k)
        dev = idx.device
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        deg = torch.zeros(n, dtype=torch.int32, device=dev)
        cap = 2 * n * k
        col = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        if n == 0:
            return rowptr, col[:0], deg
        ws = torch.empty(max(self.graph_symmetrize_workspace_bytes(n, k), 16), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.check(self.L.dcahip_graph_symmetrize(p(idx), idx.stride(0) if n > 1 else k, n, k, p(rowptr), p(col), cap, p(deg),
                                                 p(ws), p(status), hip.stream()), 'graph_symmetrize')
        bad = int(status.item())
        if bad:
            raise ValueError('dca_amd: louvain: %d neighbour indices lie outside 0 .. %d (and are not the padding -1)' % (bad, n - 1))
        return rowptr, col[:int(rowptr[n].item())], deg

    def louvain_level(self, rowptr, col, wt, twom, g, max_sweeps, labels=None, best_q=None):
        """K-LOUVAIN (include/dcahip.h, dcahip_louvain_begin / dcahip_louvain_sweep): one level on the CSR graph (rowptr int64
        [n + 1], col int32 [nnz], wt int32 [nnz] or None for unit weights), the arguments checked once.  It starts from
        singletons, or from ``labels`` (int32 [n]) with ``best_q`` the integer Q the first sweep has to exceed.  Returns a
        LouvainLevel: ``sweep(s)`` enqueues sweep s = 0, 1, .., ``read(s)`` the state after it (a synchronisation)."""
        return LouvainLevel(self, rowptr, col, wt, twom, g, max_sweeps, labels, best_q)

    def csr_gather(self, csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, Y, ldy, X, ldx, sf_out, status):
        """The minibatch tile of a resident CSR (prep.CsrCounts): storage rows perm[*cursor + r] (perm given) or row0 + r ->
        every element of Y[:B, :ldy], X[:B, :ldx] (X = the normalised input, None: not written), sf_out[:B] = sf[row];
        status (int32 device word) += what had to be ignored (include/dcahip.h)."""
        p = hip.ptr
        hip.check(self.L.dcahip_csr_gather(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G, p(perm),
                                           p(cursor), int(row0), B, p(sf), p(fac), int(bool(do_log)), p(mean), p(std),
                                           p(Y), ldy, p(X), ldx if X is not None else 0, p(sf_out), p(status),
                                           hip.stream()), 'csr_gather')

    def csr_gather_cols(self, csr, col_out, G_out, perm, cursor, row0, B, sf, fac, do_log, mean, std, Y, ldy, X, ldx, sf_out,
                        status):
        """csr_gather for a network that fits G_out of the G input genes: X[:B, :ldx] over all input genes as csr_gather
        writes it, Y[:B, :ldy] over the output columns, Y[r, col_out[g]] = the count of gene g (col_out: int32 [G] device
        tensor, -1 = not fitted), zero elsewhere (include/dcahip.h)."""
        p = hip.ptr
        assert col_out.dtype == torch.int32 and col_out.numel() >= csr.G
        hip.check(self.L.dcahip_csr_gather_cols(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G, p(perm),
                                                p(cursor), int(row0), B, p(sf), p(fac), int(bool(do_log)), p(mean), p(std),
                                                p(Y), ldy, p(X), ldx if X is not None else 0, p(sf_out), p(status),
                                                p(col_out), int(G_out), hip.stream()), 'csr_gather_cols')

    def csr_gather_compact(self, csr, perm, cursor, row0, B, sf, fac, do_log, mean, std, Yc, ldc, ovf_ptr, ovf_col, ovf_val,
                           X, ldx, sf_out, fac_out, status):
        """The minibatch tile of a resident CSR in the byte-store format (compact.CompactCounts of the tile's B rows): every
        byte of Yc[:B, :ldc], the tile's overflow list (ovf_ptr [B + 1], ovf_col / ovf_val with the list's capacity as their
        length; all None when the dataset holds no count >= 255), sf_out[:B], fac_out[:B] and, when X is given, csr_gather's
        X[:B, :ldx].  status (int32 device word) += what had to be ignored or did not fit the list (include/dcahip.h)."""
        p = hip.ptr
        cap = int(ovf_col.numel()) if ovf_col is not None else 0
        hip.check(self.L.dcahip_csr_gather_compact(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G,
                                                   p(perm), p(cursor), int(row0), B, p(sf), p(fac), int(bool(do_log)), p(mean),
                                                   p(std), p(Yc), ldc, p(ovf_ptr), p(ovf_col), p(ovf_val), cap, p(X),
                                                   ldx if X is not None else 0, p(sf_out), p(fac_out), p(status),
                                                   hip.stream()), 'csr_gather_compact')

    def csr_col_pass(self, csr, fac, do_log, col_part, status):
        """prep_col_pass's per-gene partials [R][2][Gp] (R = prep_chunks(n)) from a resident CSR, bit for bit."""
        p = hip.ptr
        hip.check(self.L.dcahip_csr_col_pass(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G, p(fac),
                                             int(bool(do_log)), p(col_part), p(status), hip.stream()), 'csr_col_pass')

    def csr_row_sums(self, csr, out, status):
        """prep_row_sums of a resident CSR (exact for counts)."""
        p = hip.ptr
        hip.check(self.L.dcahip_csr_row_sums(p(csr.indptr), p(csr.indices), p(csr.values), csr.nnz, csr.n, csr.G, p(out),
                                             p(status), hip.stream()), 'csr_row_sums')

    # ------------------------------------------------------------------ optimizer
    def rmsprop_clip_end(self, w, g, ms, n, lr, rho, eps, clip, loss, weight, hist, rows_per_slot, acc, cursor, advance):
        """The update followed by step_end's bookkeeping in the same launch (include/dcahip.h: dcahip_rmsprop_clip)."""
        p = hip.ptr
        hip.check(self.L.dcahip_rmsprop_clip(p(w), p(g), p(ms), n, p(lr), rho, eps, clip, p(loss), weight, p(hist),
                                             rows_per_slot, p(acc), p(cursor), advance, hip.stream()), 'rmsprop_clip')

    def rmsprop_clip(self, w, g, ms, n, lr, rho, eps, clip):
        self.rmsprop_clip_end(w, g, ms, n, lr, rho, eps, clip, None, 0.0, None, 0, None, None, 0)


class LouvainLevel:
    """One level of K-LOUVAIN on the device (HipOps.louvain_level).  ``labels`` / ``tot``: the current (best) state;
    ``labels_new``: what the last sweep decided, kept or not; ``ki``: the weighted degrees."""

    def __init__(self, ops, rowptr, col, wt, twom, g, max_sweeps, labels=None, best_q=None):
        from .community import check_level_args
        n = rowptr.numel() - 1
        nnz = col.numel()
        twom, g, max_sweeps = int(twom), int(g), int(max_sweeps)
        check_level_args(n, nnz, twom, g, max_sweeps)
        if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or not rowptr.is_contiguous() or not col.is_contiguous() or \
                (wt is not None and (wt.dtype != torch.int32 or wt.numel() != nnz or not wt.is_contiguous())):
            raise ValueError('dca_amd: louvain: the graph is rowptr int64 [n + 1], col int32 [nnz], wt int32 [nnz] or None')
        dev = rowptr.device
        p = hip.ptr
        self.n, self.g, self.twom = n, g, twom
        self.ki = torch.zeros(n, dtype=torch.int32, device=dev)
        self.labels = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tot = torch.zeros(n, dtype=torch.int32, device=dev)
        self.labels_new = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tot_new = torch.zeros(n, dtype=torch.int32, device=dev)
        self.state = torch.zeros(24, dtype=torch.int64, device=dev)
        self._keep = (rowptr, col, wt)
        graph = (n, nnz, p(rowptr), p(col) if nnz else None, p(wt) if wt is not None and nnz else None)
        L = ops.L
        hip.check(L.dcahip_louvain_begin(*graph, p(self.ki) if n else None, p(self.labels) if n else None,
                                         p(self.tot) if n else None, twom, g, p(self.state), hip.stream()), 'louvain_begin')
        if labels is not None:
            if labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
                raise ValueError('dca_amd: louvain: labels is an int32 tensor of shape (%d,)' % n)
            if n and (int(labels.min()) < 0 or int(labels.max()) >= n):
                raise ValueError('dca_amd: louvain: labels lie in 0 .. %d' % (n - 1))
            self.labels.copy_(labels)
            self.tot.zero_().index_add_(0, labels.long(), self.ki)
            q = int(best_q)
            if not -(1 << 127) <= q < 1 << 127:
                raise ValueError('dca_amd: louvain: best_q is a 128-bit integer')
            self.state[2] = self.state[10] = (q & ((1 << 64) - 1)) - ((1 << 64) if q & (1 << 63) else 0)
            self.state[3] = self.state[11] = q >> 64
        tail = (p(self.ki), p(self.labels), p(self.tot), p(self.labels_new), p(self.tot_new)) if n else (None,) * 5
        fn, st = L.dcahip_louvain_sweep, p(self.state)

        def sweep(s):
            hip.check(fn(*graph, *tail, twom, g, int(s), max_sweeps, st, hip.stream()), 'louvain_sweep')
        self.sweep = sweep

    def read(self, s):
        """The state after sweep s: dict of done (0 running, 1 Q did not rise, 2 two idle sweeps, 3 max_sweeps), sweeps, q
        (the best integer Q), idle, kept (whether sweep s was), and the sums of sweep s: moved, inside, tot2."""
        w = [int(v) for v in self.state.cpu().tolist()]
        st = w[8 * ((s + 1) & 1):][:8]
        sm = w[16 + 4 * (s & 1):][:4]
        u = lambda v: v & ((1 << 64) - 1)
        return dict(done=st[0], sweeps=st[1], q=(st[3] << 64) | u(st[2]), idle=st[4], kept=bool(st[5]), moved=u(sm[0]),
                    inside=u(sm[1]), tot2=u(sm[2]))
