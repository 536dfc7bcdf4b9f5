/*
 * dcahip.h -- C ABI of libdcahip.so: the MI355X (gfx950) kernels behind the DCA
 * ZINB-autoencoder training path.
 *
 * The reference (theislab/dca v0.3.3) has NO native / FFI interface on this path: every
 * FLOP is a stock TensorFlow CPU kernel reached through Keras.  Each entry
 * point below therefore cites the reference Python call site(s) whose TensorFlow ops it
 * replaces; a maintainer binds them with ctypes exactly as dca_amd/hip.py does (see
 * INTEGRATION.md for the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to row-major fp32 unless stated; the caller
 *     (host code / PyTorch as allocator) owns every buffer, the library allocates nothing
 *     and keeps no global state (no environment variables, no setters: every choice of kernel is a pure function of the
 *     arguments of the call; kernels that were measured and lost -- the pipelined one-wave-per-SIMD K-HEADS, the
 *     non-zero-only first-layer forward, the small-batch byte-store weight gradient, the four-wave matrix-pipe forward --
 *     were removed from the sources; the version control history keeps them);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant
 *     across streams and capturable into a hipGraph (no host synchronisation inside);
 *   - return value: 0 on success, otherwise the hipError_t of the failed launch or
 *     DCAHIP_EINVAL for an argument the kernels cannot take (never throws, never aborts);
 *   - "gather": kernels that consume a minibatch read row r of the batch from storage row
 *     perm[*cursor + r] of the resident matrix, so the shuffled batch is never materialised
 *     (reference: Keras slices index_array[batch_start:batch_end] on the host and feeds
 *     copies, dca/train.py:91-98).  perm == NULL means identity (row r); cursor == NULL
 *     means offset 0.  `cursor` lives in device memory so a captured step graph can be
 *     replayed for every batch of an epoch.
 *   - activation slopes: the backward entries of the hidden layers derive the slope of codes 0-11 from the
 *     layer's OUTPUT h, and of the non-monotonic codes 12 (swish) and 13 (gelu) from its PRE-activation:
 *     xhat + beta with batch norm (the `beta` argument of the batch-norm backward entries, the `beta` field of
 *     dcahip_stack_bwd_layer; NULL allowed for codes 0-11), Z in the `Hact` slot without (see
 *     dcahip_bn_relu_apply for the code list).
 */
#ifndef DCAHIP_H
#define DCAHIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DCAHIP_VERSION 2
#define DCAHIP_EINVAL (-22)

/* flags for dcahip_zinb_nll */
#define DCAHIP_NLL_HAS_PI      1   /* ZINB (pi head present); otherwise plain NB          */
#define DCAHIP_NLL_CONST_DISP  2   /* theta = clip(exp(theta_w[g]),1e-3,1e4) per gene      */
#define DCAHIP_NLL_POISSON     4   /* mean head only: poisson_loss, dca/loss.py:36-55     */
#define DCAHIP_NLL_MSE         8   /* linear mean head only: mse_loss, dca/loss.py:24-27  */

int dcahip_version(void);

/* Upper bound of `double` slots dcahip_zinb_nll writes to loss_partials. */
int dcahip_zinb_max_partials(void);

/*
 * NB / ZINB negative log-likelihood of one minibatch and its gradient with respect to the
 * head PRE-activations, one pass over the B x G tile (28 B/element: reads 3 pre-activation
 * planes + y, writes 3 gradient planes).
 * Replaces: MeanAct/DispAct/sigmoid (dca/network.py:38-39,369-380), ColwiseMultLayer
 * (dca/layers.py:85), NB.loss (dca/loss.py:72-114), ZINB.loss (dca/loss.py:122-156),
 * ConstantDispersionLayer.theta_exp (dca/layers.py:21) and TensorFlow's autodiff of them.
 * With DCAHIP_NLL_POISSON / DCAHIP_NLL_MSE (ae_type 'poisson' / 'normal', dca/network.py:143-156,
 * 233-246) only a_mean / d_mean are used: poisson_loss on clip(exp(a)) * sf, mse_loss on a * sf.
 *
 *   a_mean, a_disp, a_pi : [B, lda] pre-activations (a_disp NULL with CONST_DISP, a_pi NULL
 *                          without HAS_PI)
 *   theta_w              : [G] log-dispersion (CONST_DISP only)
 *   y, ldy               : resident raw-count matrix (gathered by perm/cursor), sf: [n] size
 *                          factors indexed by the same storage row
 *   inv_n                : 1 / (B_global * G): the reduce_mean divisor folded into the grads
 *   d_mean, d_disp, d_pi : [B, ldd] gradients out (all NULL => loss only, e.g. validation).
 *                          With CONST_DISP d_disp receives d nll/d theta * inv_n per element
 *                          (column-reduce it with dcahip_colsum_chain).
 *                          Columns g in [G, ldd-plane width) are not touched; columns in the
 *                          last partial quad (g >= G, < roundup4(G)) are written as 0.
 *   loss_partials        : [>= dcahip_zinb_max_partials()] doubles; *n_partials_out (host
 *                          int, may be NULL) = slots written = grid size (deterministic).
 */
int dcahip_zinb_nll(const float* a_mean, const float* a_disp, const float* a_pi, long lda,
                    const float* theta_w,
                    const float* y, long ldy, const float* sf,
                    const int* perm, const long long* cursor,
                    int B, int G, float ridge, float inv_n, int flags,
                    float* d_mean, float* d_disp, float* d_pi, long ldd,
                    double* loss_partials, int* n_partials_out, void* stream);

/*
 * dcahip_zinb_nll with the gradient planes leaving as PRE-SPLIT bf16 pieces (see dcahip_gemm_p3): the operand of the
 * heads' weight- and input-gradient products is written once in the form both read, instead of fp32 planes that each
 * product splits again.  d_planes [3][>= B][ldp] bf16 (plane_stride elements between pieces); the head planes start at
 * columns col_mean / col_disp / col_pi of a row (multiples of 4; columns nobody writes must be zero: the products read
 * whole rows).  Constant dispersion: d nll / d theta still goes to the fp32 plane d_theta (ld ldd_theta) that
 * dcahip_colsum_chain reduces, col_disp is ignored.  NB / ZINB only, gradient always, 16-byte aligned vector operands
 * (lda, ldy multiples of 4).  Same loss partials as dcahip_zinb_nll.
 */
int dcahip_zinb_nll_planes(const float* a_mean, const float* a_disp, const float* a_pi, long lda,
                           const float* theta_w, const float* y, long ldy, const float* sf,
                           const int* perm, const long long* cursor, int B, int G, float ridge,
                           float inv_n, int flags, void* d_planes, long ldp, long plane_stride,
                           long col_mean, long col_disp, long col_pi, float* d_theta, long ldd_theta,
                           double* loss_partials, int* n_partials_out, void* stream);

/* The same with the head planes as TWO fp16 pieces of the UNSCALED gradient g 2^d_exp (g = d nll / d pre-activation without the
 * 1 / n factor; dcahip_gemm_h2 takes the factor and the exponent out): d_planes [2][>= B][ldp] fp16.  The caller picks d_exp
 * from the bound |g| <= max(1e4, 2 y_max + 50) (+ ridge / 2) of the likelihood's formulas, so that nothing leaves the fp16
 * range: d_exp = 2 for counts up to 8 000.  A per-gene dispersion's fp32 plane d_theta keeps inv_n. */
int dcahip_zinb_nll_planes_h2(const float* a_mean, const float* a_disp, const float* a_pi, long lda,
                              const float* theta_w, const float* y, long ldy, const float* sf,
                              const int* perm, const long long* cursor, int B, int G, float ridge,
                              float inv_n, int flags, int d_exp, void* d_planes, long ldp, long plane_stride,
                              long col_mean, long col_disp, long col_pi, float* d_theta, long ldd_theta,
                              double* loss_partials, int* n_partials_out, void* stream);

/*
 * K-SCORE: the two marginals of the element-wise negative log-likelihood of B consecutive rows -- what a fitted model is
 * scored by (held-out cells, NB against ZINB, badly fitted genes / cells).  The element value is the one dcahip_zinb_nll
 * sums (dca/loss.py:72-156: NB.loss / ZINB.loss before the reduce_mean, the ridge term ridge * pi^2 included; poisson_loss /
 * mse_loss with the flags below), evaluated by the same device functions, WITHOUT an inv_n factor.
 *
 *   a_mean, a_disp, a_pi, lda, theta_w, ridge, flags : as dcahip_zinb_nll (DCAHIP_NLL_HAS_PI / CONST_DISP / POISSON / MSE)
 *   y, ldy, sf      : targets and size factors of the B rows, already offset to the first row (row r of the planes
 *                     belongs to y + r * ldy and sf[r]: no perm / cursor)
 *   cell_out        : [B]  doubles, OVERWRITTEN with sum over g of nll(row, g)
 *   gene_acc        : [G]  doubles, ADDED to: += sum over the rows of nll(row, g), so that chunks of cells accumulate
 *   workspace       : [>= dcahip_nll_marginals_workspace_doubles(B, G)] doubles (0 for B <= 0 or G <= 0, DCAHIP_EINVAL
 *                     when the count does not fit an int); needs no initialisation
 *
 * Every element value is converted to double before it is added.  Fixed summation order, no atomics: two calls on the same
 * inputs give bit-identical outputs.  Any B >= 1, G >= 1; 16-byte aligned operands with lda, ldy multiples of 4 (and
 * >= roundup4(G)) take 16-byte loads, anything else the scalar path; columns >= G of the planes never reach an output.
 * DCAHIP_EINVAL (nothing launched): the argument errors of dcahip_zinb_nll, lda or ldy < G, NULL cell_out / gene_acc /
 * workspace.
 */
int dcahip_nll_marginals_workspace_doubles(int B, int G);
int dcahip_nll_marginals(const float* a_mean, const float* a_disp, const float* a_pi, long lda,
                         const float* theta_w, const float* y, long ldy, const float* sf,
                         int B, int G, float ridge, int flags,
                         double* cell_out, double* gene_acc, double* workspace, void* stream);

/*
 * K-GROUPS: first and second moments of the denoised expression per group of cells -- what a comparison of groups
 * (clusters, conditions, batches) on the denoised data starts from (mean, variance, Welch's t), without the cells x genes
 * matrix leaving the device.
 *
 *   a_mean, lda     : B consecutive rows of the mean head's PRE-activation plane (as dcahip_nll_marginals reads it)
 *   sf, codes       : size factor and group code of the B rows, already offset to the first row
 *   flags           : DCAHIP_NLL_MSE (linear mean head), DCAHIP_GROUP_NO_SF, DCAHIP_GROUP_LOG1P
 *   sum_acc, sumsq_acc : [K][ldg] doubles, ADDED to, so that chunks of cells accumulate
 *   workspace       : [>= dcahip_group_moments_workspace_doubles(B, G, K)] doubles (0 for B, G or K <= 0, DCAHIP_EINVAL
 *                     when the count does not fit an int or K > 4096); non-decreasing in B, so a workspace sized for a
 *                     chunk of rows serves every shorter chunk of the same G and K; needs no initialisation
 *
 * Element value, in fp32 and by the device function dcahip_zinb_heads_infer stores its mean with (the same bits):
 * x = clip(expf(a), 1e-5f, 1e6f) * sf[row] (the clip by comparisons: a NaN stays a NaN), or a * sf[row] with
 * DCAHIP_NLL_MSE; DCAHIP_GROUP_NO_SF drops the factor, DCAHIP_GROUP_LOG1P takes log1pf of the result.
 * For every row with 0 <= codes[row] < K:
 *   sum_acc[code * ldg + g] += (double)x,  sumsq_acc[code * ldg + g] += (double)x * (double)x.
 * Any other code leaves the row out (-1 is "in no group"; no code is ever used as an index without the range check).
 *
 * Fixed summation order (ascending row within a group), no atomics: two calls on the same inputs give bit-identical
 * outputs.  Any B >= 1, G >= 1, 1 <= K <= 4096, ldg >= G; a 16-byte aligned plane with lda a multiple of 4 takes 16-byte
 * loads, anything else the scalar path; columns >= G of the plane never reach an output.
 * DCAHIP_EINVAL (nothing launched): NULL a_mean / codes / sum_acc / sumsq_acc / workspace, NULL sf without
 * DCAHIP_GROUP_NO_SF, lda < G, ldg < G, K outside 1 .. 4096, B or G <= 0, DCAHIP_NLL_MSE together with DCAHIP_GROUP_LOG1P
 * (a linear mean may be <= -1).
 */
#define DCAHIP_GROUP_NO_SF   16  /* x = mean, not mean * sf[row]                     */
#define DCAHIP_GROUP_LOG1P   32  /* x = log1pf(...) of the above                     */
int dcahip_group_moments_workspace_doubles(int B, int G, int K);
int dcahip_group_moments(const float* a_mean, long lda, const float* sf, const int* codes,
                         int B, int G, int K, int flags,
                         double* sum_acc, double* sumsq_acc, long ldg,
                         double* workspace, void* stream);

/*
 * K-RANKS (dca_amd/csrc/dcahip_ranksum.hip): the Wilcoxon rank-sum (Mann-Whitney) statistics of groups of cells, gene by
 * gene, as exact integers -- what scanpy's rank_genes_groups(method='wilcoxon') sorts every gene on the host for, without the
 * cells x genes matrix leaving the device.  The sort is this library's own (a stable LSD radix sort per gene).
 *
 *   x, ldx          : GENE-MAJOR fp32: g rows (genes) of n cell values, row stride ldx >= n (dcahip_transpose_rows writes it)
 *   order           : [m] int32, the labelled cells as DISTINCT column numbers of x, group after group; a cell that is
 *                     not listed takes no part (whatever it holds, NaN included)
 *   gstart          : [K + 1] int32, starts at 0, does not decrease, ends at m: positions gstart[c] .. gstart[c + 1] of
 *                     order are group c (the caller's responsibility; a group code is clamped before it is an index)
 *   ref             : -1 = every group against the pooled labelled cells; 0 <= ref < K = every group against group ref
 *   rank2, tie, ldr : [K][ldr] 64-bit integers, WRITTEN (not added to) in columns [0, g); columns >= g are not touched
 *   workspace       : >= dcahip_ranksum_workspace_bytes(g, n) bytes, 16-byte aligned, any content: a status word, the
 *                     group code of every position of order, and per WORKGROUP of the persistent grid (min(g, 512), 256
 *                     for n > 262 144) two uint32 [n] and two uint16 [n] arrays -- it does not grow with g beyond the grid.
 *                     The query returns DCAHIP_EINVAL for g <= 0, n <= 0 or n > 2 097 151
 *
 * Per row the m values are ordered as real numbers: -0.0f ties with +0.0f, denormals and +-inf take their natural place;
 * inside a run [a, b) (0-based sorted positions) of equal values ties keep group order.  With P(p) the number of cells of
 * group ref at sorted positions below p, every cell i of group c of row j adds to rank2[c * ldr + j]
 *   ref < 0 :  a_i + b_i + 1    twice the cell's mid-rank: rank2 is twice the rank sum of group c
 *   ref >= 0:  P(a_i) + P(b_i)  twice the Mann-Whitney U of c against ref (a ref cell below counts 2, a tied one 1)
 * and tie[c * ldr + j] is the sum of t^3 - t over the runs of the pooled sample of that comparison: all m cells with ref < 0
 * (the same number for every c), the cells of c and ref together with ref >= 0, t counting only those (row ref: ref alone).
 * A group without cells gets rank2 = 0; m == 0 writes zeros.
 * A row whose m values hold a NaN gets -1 in every rank2 and tie entry of that row, the other rows are not affected.  An
 * order entry outside [0, n) is never used as an index: every row gets -1 instead.
 *
 * Integers throughout (64-bit accumulators; n <= 2 097 151 keeps t^3 below 2^63), no floating-point atomics: the results
 * are exact and identical from run to run.  The time of a row does not depend on its ties (no thread walks along a run).
 * 1 <= K <= 4096, 0 <= m <= n <= 2 097 151.
 * DCAHIP_EINVAL (nothing launched): NULL x / gstart / rank2 / tie / workspace, NULL order with m > 0, ldx < n, ldr < g,
 * g <= 0, n <= 0 or above the limit, m outside 0 .. n, K outside 1 .. 4096, ref outside -1 .. K - 1.
 */
long dcahip_ranksum_workspace_bytes(int g, int n);
int dcahip_ranksum(const float* x, long ldx, int g, int n,
                   const int* order, int m, const int* gstart, int K, int ref,
                   long long* rank2, long long* tie, long ldr,
                   void* workspace, void* stream);

/*
 * K-GRAM: centred cross-products of selected columns of an fp32 plane, in double -- what a gene-gene correlation of the
 * denoised expression starts from (covariance = (cross - dsum dsum^T / n) / (n - 1)), without the cells x genes matrix
 * leaving the device.
 *
 *   x, ldx          : B consecutive rows of an fp32 plane (the values dcahip_zinb_heads_infer wrote, or their log1p)
 *   cols            : [G] int32 column of x per selected gene, NULL = column j; the entries are the CALLER's
 *                     responsibility (no range check: x[r * ldx + cols[j]] is read as it stands)
 *   keep            : [B] int32, a row with keep[r] == 0 is left out (whatever it holds, NaN included); NULL = every row
 *   shift           : [G] doubles, any constant near the gene's mean (it only has to be the same in every call that
 *                     adds to the same accumulators)
 *   cross, ldc      : [G][ldc] doubles, ADDED to over the full G x G square;  dsum : [G] doubles, ADDED to
 *   ws              : [>= dcahip_gram_workspace_doubles(B, G)] doubles: the selected columns of a row block as a compact
 *                     fp32 image (gathered once, not once per tile column) and the row slices' partial tiles;
 *                     non-decreasing in B, so a workspace sized for a chunk of rows serves every shorter chunk of the
 *                     same G; at most 64 MiB; needs no initialisation; may be NULL for cols == NULL with a single row
 *                     slice.  The query returns 0 for B <= 0, DCAHIP_EINVAL for G outside 1 .. 8192
 *
 * For the kept rows r < B and i, j < G, with d[r][j] = (double)x[r * ldx + cols[j]] - shift[j] (one rounding):
 *   cross[i * ldc + j] += sum_r d[r][i] d[r][j],   dsum[j] += sum_r d[r][j].
 * Products and sums in double on the fp64 matrix pipe; only the 64 x 64 tiles with tile_i <= tile_j are computed and the
 * SAME double is added at [i][j] and at [j][i]: accumulators that were symmetric stay symmetric bit for bit.  Fixed
 * summation order (rows ascending within a row slice, slices in index order, then one add onto the accumulator; with
 * cols, more rows than fit the workspace -- 2 048 at 8 192 genes -- go in row blocks, one such add each, in row order), no
 * atomics: two calls on the same inputs give bit-identical outputs.  There is more than one row slice only when the
 * triangle's tiles alone (at most 682 of them, against 1024 resident workgroups) do not fill the chip; the plan is a
 * pure function of (B, G), stated above the kernel in dcahip_gram.hip.  B == 0 or no kept row: the accumulators keep their bits.
 * DCAHIP_EINVAL (nothing launched): NULL x / shift / cross / dsum, ldc < G, ldx < 1, G outside 1 .. 8192, B < 0, NULL ws
 * where the call needs one (cols given, or more than one row slice).
 */
long dcahip_gram_workspace_doubles(int B, int G);
int dcahip_gram(const float* x, long ldx, const int* cols, const int* keep, const double* shift,
                int B, int G, double* cross, long ldc, double* dsum, double* ws, void* stream);

/*
 * Deterministic second stage of the loss reduction: loss = scale * sum(partials) with
 * nan -> inf (dca/loss.py:148), written to *loss_out (fp32, device).
 */
int dcahip_loss_finalize(const double* partials, int n_partials, double scale,
                         float* loss_out, void* stream);

/*
 * End-of-step bookkeeping in one tiny launch: hist[*cursor / rows_per_slot] = *loss (if
 * hist), *acc += *loss * weight (Keras' sample-weighted epoch mean, if acc), *cursor += advance.
 */
int dcahip_step_end(const float* loss, double weight, float* hist, int rows_per_slot,
                    double* acc, long long* cursor, int advance, void* stream);

/*
 * Inference heads: mean*sf, theta, pi from pre-activations (in-place allowed: out == in).
 * Replaces model.predict / extra_models['dispersion'|'pi'].predict (dca/network.py:188-211,
 * 395-405).  sf is indexed by batch row (no gather).  Outputs may be NULL.  flags &
 * DCAHIP_NLL_MSE: the mean head is linear (ae_type 'normal': mean_sf = a_mean * sf).
 * A NaN pre-activation gives a NaN output in every head (the clips are comparisons, as tf.clip_by_value).
 * DCAHIP_EINVAL (nothing launched): B or G <= 0, NULL sf, an output given without its input.
 */
int dcahip_zinb_heads_infer(const float* a_mean, const float* a_disp, const float* a_pi,
                            long lda, const float* sf, int B, int G,
                            float* mean_sf, float* theta, float* pi, long ldo, int flags,
                            void* stream);

/*
 * K-HEADS: the output heads of one training step in a single pass -- forward GEMM of the heads
 * (pre-activations = H Wh + bh), NB / ZINB NLL + gradient, weight + bias gradient, input
 * gradient -- without materialising the [B, G] pre-activation / gradient planes in HBM.
 * Equivalent to dcahip_sgemm(NN, bias) + dcahip_zinb_nll + dcahip_sgemm(TN, colsum_row) +
 * dcahip_colsum_chain + dcahip_sgemm(NT) on the same operands.
 * Replaces: dca/network.py:369-385 (the three Dense heads, ColwiseMultLayer, SliceLayer, loss
 * closure), dca/loss.py:72-156 and TensorFlow's autodiff of them.
 *
 *   H [B, ldh]      : decoder output (last hidden activation), 16-byte aligned, ldh % 4 == 0
 *   Wh [hL, ldw]    : head weights, head planes in the order [mean | dispersion | pi] (absent
 *                     heads skipped), `plane` columns apart (plane % 4 == 0, G <= plane <=
 *                     roundup32(G)); bh [nheads*plane] the biases in the same layout
 *   theta_w [G]     : log-dispersion (CONST_DISP only)
 *   y, ldy, sf, perm, cursor, inv_n, flags : as dcahip_zinb_nll; ridge likewise, and it must lie in [0, 1e3]
 *   gW [hL+1, ldg]  : OUT weight gradient in the layout of Wh; row hL = bias gradient
 *   g_theta [G]     : OUT d loss / d theta_w (CONST_DISP only)
 *   dH [B, lddh]    : OUT gradient w.r.t. H (columns < hL)
 *   loss_partials   : as dcahip_zinb_nll
 *   workspace       : >= dcahip_heads_fused_workspace_bytes(...) bytes, 16-byte aligned
 * Optional arguments:
 *   yc, ldc, ovf_ptr, ovf_col, ovf_val : the counts read from the compact store of K-SPARSE (below; 4 x fewer count bytes
 *                     per launch): yc != NULL selects it, y / ldy are then unused and may be NULL / 0.  yc == NULL: the
 *                     fp32 counts y (ldc and the overflow list are ignored).
 *   tile_order      : the order in which workgroups take the 32-gene tiles: a device array of
 *                     dcahip_heads_tile_order_len(G) ints, a permutation of 0 .. ceil(G/32)-1 (padded with values >=
 *                     ceil(G/32)); every 2 consecutive entries share a workgroup.  NULL = identity.  Results do not depend
 *                     on it beyond fp32 re-association (the weight gradients are per gene tile: bitwise the same for every
 *                     order, except that a launch whose plan ends in a poorly filled round of workgroups hands the LAST
 *                     tiles of the order to a second launch with more batch splits -- e.g. 25 000 genes x 4 096 rows -- and
 *                     a tile's gradient is then the sum of 8 or 16 partial sums instead of 2); for a FIXED order every
 *                     result is bit for bit reproducible.  A workgroup lasts as long as its slower tile, so pairing tiles
 *                     of similar non-zero load (sort by the non-zero count of the tile's 32 count columns) removes the
 *                     imbalance: measured 15 % between the two tiles of a workgroup in file order, 8 % of the kernel.
 *   loss_out        : != NULL: the batch loss (inv_n * sum of the partials, nan -> inf: what dcahip_loss_finalize
 *                     computes) is written there by the last launch of the call -- one launch less per step.  NULL:
 *                     finish the loss with dcahip_loss_finalize.
 *   d_exp           : in [-24, 0], 0 by default: the kernel carries the gradient planes as g 2^(8 + d_exp) (kDExp0 = 8) in
 *                     two fp16 pieces, g = the UNSCALED d nll / d pre-activation, |g| <= max(theta, ~2 y): |g| <= 117 fits
 *                     at d_exp = 0.  A 32 x 32 tile with a larger value repeats at the exponent its maximum needs (a slow
 *                     path, exact, but the whole tile is then carried at that exponent: 2^-(kDe + 25) absolute on every g of
 *                     it); a caller whose counts reach c throughout passes d_exp = -ceil(log2(2 c / 117))
 *                     (Engine._heads_d_exp) and keeps the tiles on the fast path.
 * Supported: 1 <= hL <= 64 (workspace_bytes query returns 0 otherwise -> use the separate
 * kernels).  Deterministic (fixed summation order, no atomics).
 */
long dcahip_heads_fused_workspace_bytes(int B, int hL, int G, long plane, int flags);
int dcahip_heads_tile_order_len(int G);
int dcahip_heads_fused(const float* H, long ldh, const float* Wh, long ldw, const float* bh,
                       long plane, const float* theta_w,
                       const float* y, long ldy,
                       const unsigned char* yc, long ldc, const int* ovf_ptr, const int* ovf_col,
                       const float* ovf_val, const float* sf,
                       const int* perm, const long long* cursor,
                       int B, int hL, int G, float ridge, float inv_n, int flags,
                       float* gW, long ldg, float* g_theta, float* dH, long lddh,
                       double* loss_partials, int* n_partials_out,
                       void* workspace, long workspace_bytes, const int* tile_order,
                       float* loss_out, int d_exp, void* stream);
/* The arithmetic of K-HEADS' three matrix products, exposed for testing: C [32, 32] = A [32, K] B [K, 32]
 * (row-major fp32, K % 16 == 0) computed as the kernel does -- each operand scaled by the power of two that brings its
 * largest magnitude into [2^13, 2^14) and split into TWO fp16 pieces (round-to-nearest residual: 2^-22 relative, 2^-25
 * absolute where the second piece is an fp16 denormal, which the matrix pipe preserves), the THREE products a1b1, a1b2, a2b1
 * accumulated in fp32 by v_mfma_f32_32x32x16_f16, the scales taken out at the end (exact).  Contract
 * (tests/test_heads_fused_gpu.py): |C - A B| <= 5e-7 sum|a b| per element, i.e. the accuracy of an fp32 dot product
 * (the fp32 MFMA measures 1.8e-7 .. 2.1e-7 on the same inputs; three bf16 pieces with six products, rounds 2-5: <= 2.5e-7). */
int dcahip_x3_product_32x32(const float* A, const float* B, float* C, int K, void* stream);

/*
 * C[M,N] = op(A) * op(B) (+ bias), fp32 in / fp32 out, LDS-tiled, deterministic split-K through `workspace`.
 * Arithmetic: every operand element is split into three bf16 pieces and the six products a1b1, a1b2, a2b1, a1b3,
 * a2b2, a3b1 are accumulated in fp32 on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) -- the accuracy of an fp32
 * dot product (dcahip_x3_product_32x32 states the contract) at 6/16 of the cycles of the fp32 MFMA, which runs at the
 * vector rate on gfx950.  split_k < 0 selects the exact-fp32 MFMA kernel (v_mfma_f32_32x32x2_f32, a k-ordered fmaf
 * chain) with the library's split heuristic: the yardstick of the accuracy tests.
 * Replaces the MatMul/BiasAdd kernels of every keras Dense layer forward and backward
 * (dca/network.py:124-126,369-380 and autodiff).
 *   ta == 0: A stored [M,K] (lda >= K)      ta == 1: A stored [K,M]   (C = A^T B, weight grads)
 *   tb == 0: B stored [K,N]                 tb == 1: B stored [N,K]   (C = A B^T, input grads)
 *   bias     : [N] added to every row of C, or NULL
 *   perm/cursor : gather on A's STORAGE rows (batch rows: m index if ta==0, k index if ta==1)
 *   colsum_row  : if non-zero (ta==1 only) additionally writes colsum_k B[k,:] into row M of
 *                 C (C + M*ldc): the Dense bias gradient, free while B streams through LDS
 *   split_k  : 0 = library heuristic (a pure function of the shape), > 0 forced, < 0 exact-fp32 kernel + heuristic
 *   workspace: >= dcahip_sgemm_workspace_bytes(...) bytes, may be NULL when that is 0
 */
int dcahip_sgemm(int ta, int tb, int M, int N, int K,
                 const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                 const float* bias, const int* perm, const long long* cursor,
                 int colsum_row, int split_k, void* workspace, long workspace_bytes,
                 void* stream);
long dcahip_sgemm_workspace_bytes(int ta, int tb, int M, int N, int K, int colsum_row, int split_k);
/* What dcahip_sgemm would launch for these arguments, exposed for testing (as dcahip_x3_product_32x32 is): nothing is
 * launched, A and B are looked at for their 16-byte alignment only and never dereferenced.  dcahip_sgemm takes its tile, its
 * arithmetic and its loader width from the function that fills `out`, so the answer cannot differ from the launch.
 *   out[0], out[1] : tile rows, tile columns (128x64, 64x128, 128x128 or 64x64)
 *   out[2], out[3] : tiles along M, along N
 *   out[4], out[5] : K splits (1 = none; empty trailing splits are dropped), K elements per split
 *   out[6]         : arithmetic, 0 = exact fp32 MFMA, 1 = three bf16 pieces (the contract above)
 *   out[7]         : floats per load of the tile loaders: 4 (16-byte loads: A and B 16-byte aligned, lda and ldb multiples
 *                    of 4) or 1
 * The ending follows from out[4] and the outputs (M + (colsum_row ? 1 : 0)) * N: no reduce launch for out[4] == 1; else one
 * ordered reduce, 16 lanes per output when out[4] >= 16 and there are at most 65536 outputs, one lane per output otherwise.
 * DCAHIP_EINVAL wherever dcahip_sgemm returns it for the same arguments (non-positive sizes, NULL A or B, ta && tb,
 * colsum_row && tb), and for a NULL out. */
int dcahip_sgemm_plan(int ta, int tb, int M, int N, int K, int colsum_row, int split_k,
                      const float* A, long lda, const float* B, long ldb, int out[8]);
/*
 * The same products from PRE-SPLIT operands.  "Planes" = the three bf16 pieces of a matrix as three images
 * [3][rows][ld] of bf16 (ld % 8 == 0; plane_stride elements from one piece to the next): x = p0 + p1 + p2 to 2^-24 |x|,
 * the split dcahip_sgemm performs on the fly, done ONCE for an operand that enters several products (the gradient
 * planes of the heads, the head weights, the normalised counts) or written directly by the kernel that produces it.
 * dcahip_gemm_p3 has no vector arithmetic in its K loop, and either operand may be contiguous along k or along m / n
 * (the m / n-contiguous one goes through the transposing LDS read), so ONE stored layout serves the products that
 * contract over a matrix's rows and over its columns: no transposed copies.  Same arithmetic and accuracy contract as
 * dcahip_sgemm (dcahip_x3_product_32x32), same argument meaning: ta / tb as there, lda / ldb in elements,
 * perm / cursor gather A's storage rows, colsum_row (tb == 0) writes the column sums of B into row M of C, split_k 0 =
 * library heuristic.  An operand contiguous along k is read in units of 8 k: K % 8 == 0 (pad BOTH operands with zeros);
 * rows of an m / n-contiguous operand must be allocated up to the next multiple of 8 columns.
 * dcahip_split_planes: fp32 [R, C] (rows gathered through perm / cursor when given) -> planes, columns C .. ldp - 1 zero.
 * Replaces the same MatMul kernels as dcahip_sgemm (dca/network.py:124-126, 369-380 and autodiff) where an operand is
 * reused. */
int dcahip_split_planes(const float* src, long ld, const int* perm, const long long* cursor, long R, int C,
                        void* planes, long ldp, long plane_stride, void* stream);
int dcahip_gemm_p3(int ta, int tb, int M, int N, int K, const void* A, long lda, long plane_a,
                   const void* B, long ldb, long plane_b, float* C, long ldc, const float* bias,
                   const int* perm, const long long* cursor, int colsum_row, int split_k,
                   void* workspace, long workspace_bytes, void* stream);
long dcahip_gemm_p3_workspace_bytes(int M, int N, int K, int colsum_row, int split_k);
/* What dcahip_gemm_p3 (pieces == 3) or dcahip_gemm_h2 (pieces == 2, below) would launch for these arguments, exposed for
 * testing (as dcahip_sgemm_plan is): nothing is launched.  gather: non-zero when perm or cursor would be passed.  Both
 * products take their kernel, tiles, K split, tail and workspace from the function that fills `out`, so the answer cannot
 * differ from the launch.
 *   out[0]         : the kernel, 0 = gemm_p3_kernel (128 x 128 tiles, four waves), 1 = the 256 x 256 eight-wave kernel
 *                    (gemm_p3w_kernel, gemm_h2w_kernel), 2 = gemm_h2m_kernel (128 x 256 tiles, four waves; two pieces, NN
 *                    without column sums)
 *   out[1], out[2] : tile rows, tile columns
 *   out[3], out[4] : tiles along M, along N
 *   out[5], out[6] : K splits (1 = none; empty trailing splits are dropped), K elements per split
 *   out[7..9]      : the tail (K splits == 1 only): first tail tile, K slices per tail tile (1 = no tail), K elements per slice
 *   out[10]        : 1 when the column-sum instantiation of the eight-wave kernel is the one launched
 *   out[11]        : the workspace bytes the call will demand (INT_MAX when they are more than that)
 * The ending follows: out[5] > 1 the ordered split-K reduce, else out[8] > 1 the sum of the tail's K slices, else none.
 * DCAHIP_EINVAL wherever the product returns it for reasons of shape (non-positive sizes, colsum_row && tb, K % 8 != 0 with
 * an operand contiguous along k; two pieces: a shape dcahip_gemm_h2_supported refuses, any gather), for pieces other than
 * 2 and 3 and for a NULL out. */
int dcahip_gemm_planes_plan(int pieces, int ta, int tb, int M, int N, int K, int gather, int colsum_row, int split_k, int out[12]);
/*
 * The plane products on TWO fp16 pieces per operand and THREE products per fp32 product (round 6: the arithmetic of K-HEADS,
 * dcahip_x3_product_32x32; half the matrix instructions of dcahip_gemm_p3).  An operand matrix is scaled by the power of two
 * that brings its largest magnitude into [2^13, 2^14) before it is split: the exponent lives in a DEVICE word, so nothing
 * leaves the stream (capturable).
 *   dcahip_absmax_exp       *exp_out = that exponent for src [R, C] (scratch_word: 4 bytes of device memory the call may use),
 *                           clamped to [-60, 60]; NaN entries are ignored; 0 for an all-zero block and for one that holds
 *                           +-Inf.  Supported range: a largest magnitude in [2^-46, 2^74).  Below it the clamp at +60
 *                           leaves the scaled block under 2^13 and the pieces keep their ABSOLUTE floor only (2^-25 of the
 *                           scaled value, i.e. 2^-85 of the data; the split stays correct down to the fp32 denormals);
 *                           from 2^74 on the clamp at -60 leaves a scaled maximum of 2^14 or more, which from 2^76 on
 *                           overflows the fp16 pieces to Inf: the product is then non-finite, never a wrong finite number.
 *   dcahip_split_planes_h2  fp32 [R, C] (rows gathered through perm / cursor) x 2^*exp -> planes [2][R][ldp] fp16 (exp NULL: 0)
 *   dcahip_gemm_h2          C = alpha 2^-(ea + eb) op(A) op(B) (+ bias), ea = (exp_a ? *exp_a : 0) + exp_a_add, eb likewise;
 *                           colsum_row: row M of C = alpha 2^-eb x the column sums of B.  Shapes: those of the 256 x 256 kernel
 *                           (dcahip_gemm_h2_supported; M, N >= 256, M N >= 2^18, K % 16 == 0, no row gather); layouts, ta / tb,
 *                           split_k and the workspace as dcahip_gemm_p3.  The kernels take the scale out as ONE power of
 *                           two, 2^-(ea + eb), which exists for |ea + eb| <= 126: the exponent words must come from
 *                           dcahip_absmax_exp or lie in [-60, 60], and |exp_a_add| + |exp_b_add| <= 6 (DCAHIP_EINVAL
 *                           otherwise, before any launch).  The factor applied is alpha 2^-(ea + eb), formed in fp32: the
 *                           contract holds where that number is a normal one (alpha >= 1 at ea + eb = 126).
 * Contract (tests/test_gemm_h2_gpu.py): |C - alpha op(A) op(B)| <= 1e-6 alpha sum|a b| per element (a priori 3 x 2^-22 = 7.2e-7
 * plus the fp32 accumulation over K; the worst of 3 M elements at K = 512 measured 5.7e-7), deterministic.
 * A producer that writes planes directly (dcahip_zinb_nll_planes_h2: the gradient planes as g 2^d_exp) passes its static
 * exponent through exp_*_add.  Replaces the same MatMul kernels as dcahip_sgemm (dca/network.py:124-126, 369-380 and autodiff).
 */
int dcahip_absmax_exp(const float* src, long ld, long R, int C, int* exp_out, void* scratch_word, void* stream);
int dcahip_split_planes_h2(const float* src, long ld, const int* perm, const long long* cursor, long R, int C,
                           void* planes, long ldp, long plane_stride, const int* exp, void* stream);
int dcahip_gemm_h2_supported(int M, int N, int K);
long dcahip_gemm_h2_workspace_bytes(int M, int N, int K, int colsum_row, int split_k);
int dcahip_gemm_h2(int ta, int tb, int M, int N, int K, const void* A, long lda, long plane_a, const int* exp_a, int exp_a_add,
                   const void* B, long ldb, long plane_b, const int* exp_b, int exp_b_add, float alpha,
                   float* C, long ldc, const float* bias, int colsum_row, int split_k,
                   void* workspace, long workspace_bytes, void* stream);
/* dst [C, ld_dst] = src [R, ld_src]^T.  The first Dense layer's kernel W0 [genes, h1] is transposed once per step at
 * throughput batches so that its forward product X W0 runs in the NT form (both operands contiguous along the
 * contraction: the fast operand path of dcahip_sgemm). */
int dcahip_transpose(const float* src, long ld_src, int R, int C, float* dst, long ld_dst, void* stream);
/* The same with gathered source rows: dst[c][r] = src[perm[*cursor + r]][c] (perm NULL: r).  Wide networks at throughput
 * batches (first layer >= 128 units): the minibatch of the resident matrix is transposed once per step and the first
 * layer's weight gradient X^T dZ runs as a plain product of a k-contiguous A (see dcahip_sgemm). */
int dcahip_transpose_rows(const float* src, long ld_src, const int* perm, const long long* cursor, int R, int C,
                          float* dst, long ld_dst, void* stream);

/*
 * Batch normalisation (center=True, scale=False, eps inside rsqrt) + ReLU, training mode.
 * Replaces keras BatchNormalization + Activation('relu') (dca/network.py:127-135).
 * Three stages so that data-parallel runs can exchange the statistics in between:
 *  1. dcahip_col_moments: per row-chunk (mean, M2) of Z[B,H]  -> part[R][2][H], R returned
 *  2. (DP only) dcahip_moments_combine: merge E entries (counts[e] rows each) into one
 *  3. dcahip_bn_relu_apply: merge the E entries it is given (Chan et al.), then
 *        xhat = (z - mean) * rsqrt(var + eps); h = max(xhat + beta, 0)
 *     writes h, xhat (may be NULL), inv_std[H], and (training) updates
 *        moving = moving - (moving - batch) * (1 - momentum)   (biased variance).
 *     With entries == NULL it runs in INFERENCE mode on moving_mean / moving_var.
 *     `relu` is the activation code: 0 linear, 1 relu, 2 tanh, 3 sigmoid, 4 elu, 5 selu, 6 softplus,
 *     7 softsign, 8 LeakyReLU(0.3), 10 hard_sigmoid, 11 exponential, 12 swish, 13 gelu (exact, erf)
 *     (Activation(self.activation) / advanced activations, dca/network.py:132-135; 9 is PReLU, a
 *     layer of its own behind code 0).  The backward entry points take the same code as `act`.
 *     Codes 0-11 derive the slope from the forward OUTPUT h.  Codes 12 and 13 are not monotonic,
 *     so h does not determine the slope: they derive it from the PRE-activation x instead --
 *       with batch norm    x = xhat + beta[c]: the `beta` argument of the batch-norm backward entries
 *                          (and the `beta` field of dcahip_stack_bwd_layer); for codes 12, 13 it must
 *                          be non-NULL (DCAHIP_EINVAL otherwise), for the other codes it is not read
 *                          and may be NULL;
 *       without batch norm x = Z, which the caller passes in the `Hact` slot of dcahip_relu_bwd /
 *                          dcahip_dense_bn_bwd_small(batchnorm = 0) (the slope is its only use there).
 *     B == 0 is legal (only the moving statistics are updated): a data-parallel rank with an
 *     exhausted shard still joins the exchange.
 */
int dcahip_col_moments_chunks(int B);
int dcahip_col_moments(const float* Z, long ldz, int B, int H, float* part, void* stream);
int dcahip_moments_combine(const float* entries, const float* counts, int E, int H,
                           float* out /*[2][H]*/, void* stream);
int dcahip_bn_relu_apply(const float* Z, long ldz, int B, int H,
                         const float* entries, const float* counts, int E,
                         const float* beta, float* moving_mean, float* moving_var,
                         float momentum, float eps, int relu,
                         float* Hout, long ldh, float* xhat, long ldx, float* inv_std,
                         void* stream);

/* Batch normalisation for small batches on one GPU (B <= dcahip_bn_fused_max_rows()): batch statistics, moving
 * averages, normalisation + activation (dcahip_col_moments + dcahip_bn_relu_apply) in ONE launch, and the backward
 * pass (dcahip_bn_bwd_sums + dcahip_bn_bwd_apply) in one: the reference-default batch of 32 cells (dca/train.py:37)
 * is bound by launch gaps.  Same arguments and formulas as the two-call forms (one chunk of up to 64 rows). */
int dcahip_bn_fused_max_rows(void);
/* A whole hidden layer per launch for the same small batches (B <= dcahip_bn_fused_max_rows(), K <= dcahip_dense_small_max_k()
 * inputs): Dense -> BatchNormalization (batchnorm != 0) -> activation forward (dca/network.py:124-135; Z receives the
 * pre-activation when non-NULL: the latent code of the centre layer), and its backward: d beta, the weight gradient gW
 * [K, h] with the bias gradient in row K, the gradient w.r.t. the layer input dHp (NULL for none); the backward needs
 * h <= dcahip_dense_small_max_k() as well (one workgroup owns the layer).  Equivalent to dcahip_sgemm + the batch-norm
 * kernels (+ 2 x dcahip_sgemm backward) on the same operands. */
int dcahip_dense_small_max_k(void);
int dcahip_dense_bn_small(const float* Hp, long ldp, const float* W, long ldw, const float* bias,
                          int B, int K, int H, int batchnorm, const float* beta,
                          float* moving_mean, float* moving_var, float momentum, float eps, int act,
                          float* Z, long ldz, float* xhat, long ldx, float* Hout, long ldh,
                          float* inv_std, void* stream);
int dcahip_dense_bn_bwd_small(const float* dH, long ldd, const float* Hact, long ldh,
                              const float* xhat, long ldx, const float* inv_std,
                              const float* Hp, long ldp, const float* W, long ldw,
                              int B, int K, int H, int batchnorm, float n_total, int act,
                              float* gW, long ldg, float* dbeta, float* dHp, long lddp, const float* beta,
                              void* stream);
/* The hidden stack behind the first layer's product in ONE launch (every layer <= 64 units, B <= dcahip_bn_fused_max_rows()):
 * entry 0 with W == NULL normalises + activates its own Z (written by dcahip_sgemm), every entry with a kernel is
 * Dense -> BatchNormalization -> activation on the previous entry's Hout (entry 0 with a kernel reads Hin).  Same
 * formulas and outputs as dcahip_bn_relu_train_small / dcahip_dense_bn_small called one after the other
 * (dca/network.py:124-135). */
typedef struct dcahip_small_layer {
    const float* W; long ldw;           /* kernel [K, H] or NULL */
    const float* bias;                  /* [H] */
    int K, H;
    const float* beta; float* moving_mean; float* moving_var;
    float* Z; long ldz;                 /* pre-activation: input when W == NULL, optional output otherwise */
    float* xhat; long ldx; float* Hout; long ldh; float* inv_std;
} dcahip_small_layer;
int dcahip_hidden_small_chain(const dcahip_small_layer* layers, int n, const float* Hin, long ldin, int B,
                              int batchnorm, float momentum, float eps, int act, void* stream);
/* K-STACK: the same hidden stack at THROUGHPUT batches (B up to dcahip_hidden_stack_max_rows(), every layer <= 64
 * units, batch normalisation on, one GPU) in one launch per direction: workgroups own blocks of batch rows and exchange
 * only the batch-norm statistics (and, at the end of the backward pass, the weight-gradient partials) through grid-wide
 * barriers -- at most 256 workgroups, all resident: launch it on an otherwise idle device (the stream order of a training
 * step guarantees that).  Forward: entry 0 (W == NULL) normalises + activates its own Z (written by dcahip_sgemm), every
 * further entry is Dense -> BatchNormalization -> activation (dca/network.py:124-135); outputs as dcahip_bn_relu_apply /
 * dcahip_sgemm (Z optional when the whole pass is one launch).  Backward: per layer dbeta, for every layer
 * behind the first gW [K + 1, H] (row K = bias gradient), and dZ0 = gradient w.r.t. the first layer's pre-activation
 * (dcahip_bn_bwd_* + dcahip_sgemm x 2 per layer on the same operands).  workspace >=
 * dcahip_hidden_stack_workspace_bytes(n, B) bytes, 16-byte aligned, ZERO before the first call (arrival counters; every
 * call leaves them at zero), shared by both directions.  Deterministic. */
typedef struct dcahip_stack_bwd_layer {
    const float* W; long ldw; int K, H;             /* kernel [K, H] (unused for the first layer) */
    const float* Hact; long ldh;                    /* the layer's output (activation derivative through the output) */
    const float* xhat; long ldx; const float* inv_std;
    const float* Hprev; long ldp;                   /* the layer's input activations [B, K] (unused for the first layer) */
    float* gW; long ldg; float* dbeta;              /* OUT (gW unused for the first layer) */
    float* dH; long lddh;                           /* gradient w.r.t. the layer's output: IN for the last layer, scratch
                                                       (written, then read by the next launch) for the others */
    const float* beta;                              /* the layer's batch-norm offset: read for codes 12, 13 only (see
                                                       dcahip_bn_relu_apply), may be NULL otherwise */
} dcahip_stack_bwd_layer;
/* Both passes are a sequence of STEPS separated by a batch-wide dependency (the batch-norm statistics):
 *   forward  (n + 1 steps): 0 = partial statistics of the first layer's pre-activation; 1 + i = layer i (merge the
 *             statistics, normalise + activate, next layer's pre-activation and ITS partial statistics);
 *   backward (n + 2 steps): 0 = dy and the batch sums of the last layer; 1 + j = layer n - 1 - j (dZ, d beta, weight-gradient
 *             partial, input gradient, dy and sums of the layer below); n + 1 = sum of the weight-gradient partials.
 * A call runs steps [first_step, last_step] in ONE launch: a range of several steps synchronises with grid barriers
 * (every workgroup resident: at most 256 of them -- rows_per_wg * 256 >= B), a single step needs none (the kernel
 * boundary is the barrier; up to 1024 workgroups).  rows_per_wg (16 .. 64) fixes the row partition and must be the same
 * for every call of a pass.  A whole backward pass (steps 0 .. n + 1) over B <= 64 rows -- the reference's default batch of
 * 32 -- is ONE workgroup's work: the batch sums are its own, the input gradients stay in registers between layers, the
 * operands of the layer below are requested while a layer computes; that call takes no workspace (NULL, 0). */
int dcahip_hidden_stack_max_rows(void);
long dcahip_hidden_stack_workspace_bytes(int n_layers, int B);
int dcahip_hidden_stack_fwd(const dcahip_small_layer* layers, int n, int B, float momentum, float eps, int act,
                            int rows_per_wg, int first_step, int last_step,
                            void* workspace, long workspace_bytes, void* stream);
int dcahip_hidden_stack_bwd(const dcahip_stack_bwd_layer* layers, int n, int B, float n_total, int act,
                            float* dZ0, long ldz0, int rows_per_wg, int first_step, int last_step,
                            void* workspace, long workspace_bytes, void* stream);

/* K-STACK inside a data-parallel step (SyncBN; dca/network.py:127-128 BatchNormalization with the statistics of the GLOBAL
 * batch): ONE step per call (the steps of dcahip_hidden_stack_fwd / _bwd at 32 rows per workgroup) with the batch-wide
 * quantity of the step's input layer handed in from outside and the one the step produces merged over this rank's row
 * blocks for the exchange that follows:
 *   forward, step s = 0..n: s = 0 only measures layer 0; s >= 1 normalises layer s - 1 with ext_entries [ext_E][2][H]
 *     (mean, M2 per rank) and ext_counts [ext_E] (rows per rank; an entry with count 0 -- a rank without rows -- is IGNORED,
 *     whatever its mean and M2 hold), applies the activation, multiplies by the next layer's
 *     kernel; stat_out [2][H'] <- (mean, M2) of this rank's rows of the layer made (all-gather it; NULL after the last).
 *   backward, step s = 0..n: s = 0 only sums the top layer; s >= 1 handles layer n - s with ext_sums [2][H] (sum dy,
 *     sum dy xhat over ALL ranks, all-reduced); sums_out [2][K] <- this rank's sums of the layer below (all-reduce them),
 *     whose first half is also stored as that layer's LOCAL d beta.  The weight-gradient reduction is step n + 1 of
 *     dcahip_hidden_stack_bwd (rows_per_wg = 32), unchanged.
 *   ONE rank that holds the whole batch computes the bits of the single-GPU steps at 32 rows per workgroup: ONE entry
 *   whose count equals B is taken as this rank's own stat_out, and the forward merges the block statistics the previous
 *   call left in the workspace -- what that entry was rounded from -- instead (so the workspace must be untouched
 *   between the calls of a pass, as for dcahip_hidden_stack_fwd); one entry with any other count (a batch merged
 *   elsewhere) is used as handed in.  The backward sums are added in the step kernel's order.
 * dcahip_hidden_stack_step_blocks(B): workgroups (= row blocks) of these launches. */
int dcahip_hidden_stack_step_blocks(int B);
int dcahip_hidden_stack_fwd_sync(const dcahip_small_layer* layers, int n, int B, float momentum, float eps, int act,
                                 int step, const float* ext_entries, const float* ext_counts, int ext_E,
                                 float* stat_out, void* workspace, long workspace_bytes, void* stream);
int dcahip_hidden_stack_bwd_sync(const dcahip_stack_bwd_layer* layers, int n, int B, float n_total, int act,
                                 float* dZ0, long ldz0, int step, const float* ext_sums, float* sums_out,
                                 void* workspace, long workspace_bytes, void* stream);
int dcahip_bn_relu_train_small(const float* Z, long ldz, int B, int H, const float* beta,
                               float* moving_mean, float* moving_var, float momentum, float eps,
                               int act, float* Hout, long ldh, float* xhat, long ldx,
                               float* inv_std, void* stream);
int dcahip_bn_bwd_small(const float* dH, long ldd, const float* Hact, long ldh,
                        const float* xhat, long ldx, const float* inv_std, float n_total,
                        int B, int H, float* dZ, long ldz, float* dbeta, int act, const float* beta, void* stream);

/*
 * Backward of ReLU + batch norm.  mask = the forward output h (h > 0 <=> pre-ReLU > 0).
 *  1. dcahip_bn_bwd_sums: per row-chunk sums of dy and dy*xhat, dy = dh*[h>0] -> part[R][2][H]
 *  2. (DP only) all-reduce the combined sums
 *  3. dcahip_bn_bwd_apply: dz = inv_std * (dy - S1/n - xhat * S2/n), dbeta = S1
 *     (sums: E entries [E][2][H] are added in order; n_total = global batch rows).
 * Without batch norm use dcahip_relu_bwd (dz = dh*[h>0]).
 * The `beta` argument (the last before `stream`, here and in dcahip_bn_bwd_small / dcahip_dense_bn_bwd_small): the layer's
 * batch-norm offset, read for codes 12, 13 only (pre-activation = xhat + beta); NULL allowed for codes 0-11.
 */
int dcahip_bn_bwd_sums(const float* dH, long ldd, const float* Hact, long ldh,
                       const float* xhat, long ldx, int B, int H, float* part, int act, const float* beta,
                       void* stream);
int dcahip_bn_bwd_apply(const float* dH, long ldd, const float* Hact, long ldh,
                        const float* xhat, long ldx, const float* inv_std,
                        const float* sums, int E, float n_total, int B, int H,
                        float* dZ, long ldz, float* dbeta, int act, const float* beta, void* stream);
int dcahip_relu_bwd(const float* dH, long ldd, const float* Hact, long ldh, int B, int H,
                    float* dZ, long ldz, int act, void* stream);
/* h = max(z, 0): Activation('relu') of a stack built with batchnorm=False (network.py:132-135). */
int dcahip_relu_fwd(const float* Z, long ldz, int B, int H, float* Hout, long ldh, int act, void* stream);
/* Shared heads (NBSharedAutoencoder / ZINBSharedAutoencoder, network.py:343-362, 464-491): dispersion and
 * dropout come from Dense(1) layers and broadcast over the genes inside the loss (loss.py:85-88,130-137).
 * dcahip_bcast_cols: out[r, c] = s[r * lds] for c < G (the scalar pre-activation spread into the plane
 * the loss kernel reads).  dcahip_row_sums_strided: out[r * ldo] = sum_c x[r, c] (the plane of
 * pre-activation gradients folded back into the gradient of the scalar); fp64 accumulation, fixed order. */
/* keras.layers.PReLU (activation='PReLU', network.py:132-133): out = max(x, 0) + alpha[c] min(x, 0), one trainable
 * slope per unit.  x = the batch-norm (or bias) output with the LINEAR activation code.  dcahip_prelu_bwd: d holds
 * dL/dout on entry and dL/dx on return; galpha[c] = sum_r dL/dout min(x, 0) (fp64 partials, fixed order);
 * workspace: dcahip_prelu_workspace_doubles(h) doubles. */
int dcahip_prelu_workspace_doubles(int h);
int dcahip_prelu_fwd(const float* x, long ldx, const float* alpha, int B, int h, float* out, long ldo, void* stream);
int dcahip_prelu_bwd(float* d, long ldd, const float* x, long ldx, const float* alpha, int B, int h,
                     float* galpha, double* workspace, void* stream);
/* zinb-elempi (ZINBAutoencoderElemPi network.py:424-461, ElementwiseDense layers.py:50-82): the mean head's Dense
 * output is negated (m = -a feeds MeanAct) and the dropout logit is a_pi[r, g] = k[g] m[r, g] + c[g].
 * dcahip_elempi_fwd: a_mean <- m in place, a_pi plane written.  dcahip_elempi_bwd: d_mean holds dL/dm on entry and
 * dL/d(Dense output) = -(dL/dm + k dL/da_pi) on return; gk[g] = sum_r dL/da_pi m, gc[g] = sum_r dL/da_pi (fp64
 * partials over a fixed row assignment: deterministic); workspace: dcahip_elempi_workspace_doubles(G) doubles. */
int dcahip_elempi_workspace_doubles(int G);
int dcahip_elempi_fwd(float* a_mean, long lda, const float* k, const float* c, int B, int G,
                      float* a_pi, long ldp, void* stream);
int dcahip_elempi_bwd(const float* m, long lda, float* d_mean, const float* d_pi, long ldd, const float* k,
                      int B, int G, float* gk, float* gc, double* workspace, void* stream);
int dcahip_bcast_cols(const float* s, long lds, int B, int G, float* out, long ldo, void* stream);
int dcahip_row_sums_strided(const float* x, long ldx, int B, int G, float* out, long ldo, void* stream);

/* out[c] (+)= chain(c) * sum_r x[r, c]; chain = d clip(exp(w),1e-3,1e4)/dw if theta_w given
 * (ConstantDispersionLayer gradient, dca/layers.py:17-21), else 1. */
int dcahip_colsum_chain(const float* x, long ldx, int B, int N, const float* theta_w,
                        float* out, void* stream);

/*
 * K-PREP: dca/io.py:88-111 (normalize: scanpy filter counts, normalize_per_cell, log1p, scale)
 * on the resident count matrix Y [n, ldy].
 *   dcahip_prep_row_sums   out[r] = sum_g Y[r, g]                 (n_counts; exact for counts)
 *   dcahip_prep_col_pass   x = Y[r, g]; if fac: x /= fac[r]; if do_log: x = log1p(x);
 *                          X[r, g] = x (X may be NULL, may alias Y); per-gene sums of x and of
 *                          fl32(x*x) in fp64 per row chunk -> col_part[R][2][roundup4(G)],
 *                          R = dcahip_prep_chunks(n)
 *   dcahip_prep_col_finish ordered sum of the R chunks (x E ranks' all-reduced partials:
 *                          pass the summed [1][2][Gp] block with R = 1): sums[g] (gene counts
 *                          of filter_genes, may be NULL) and/or mean[g], std[g] exactly as
 *                          sc.pp.scale: var = (E[x^2] - E[x]^2) n/(n-1), std 0 -> 1
 *   dcahip_prep_scale      X = (X - mean) / std in place (fp32 division)
 */
int dcahip_prep_chunks(int n);
int dcahip_prep_row_sums(const float* Y, long ldy, int n, int G, float* out, void* stream);
int dcahip_prep_col_pass(const float* Y, long ldy, int n, int G, const float* fac, int do_log,
                         float* X, long ldx, double* col_part, void* stream);
int dcahip_prep_col_finish(const double* col_part, int R, int G, double n_total,
                           float* sums, float* mean, float* stdv, void* stream);
int dcahip_prep_scale(float* X, long ldx, int n, int G, const float* mean, const float* stdv,
                      void* stream);
/*
 * CSR expand: the upload of a sparse host count matrix (scipy.sparse .X of an AnnData, a Matrix Market file), read by
 * the reference through sc.read (dca/io.py:58-59) and densified by Keras' batch feed (dca/train.py:82-88).  Only the
 * CSR arrays of a row chunk cross PCIe; this writes the dense fp32 rows of the resident count matrix.
 *   indptr [rows + 1] int32, chunk-relative (indptr[0] = 0, indptr[rows] = nnz); indices [nnz] int32, values [nnz]
 *   fp32 (may be NULL when nnz = 0).  Rows must be canonical: sorted columns, no duplicates (the host sums
 *   duplicates first).  Writes EVERY element Y[r, 0 .. ldy) for r < rows -- the entry's value or 0, pad columns
 *   G .. ldy included -- so Y may be allocated uninitialised.  Never reads or writes outside its buffers, whatever the
 *   chunk holds: *status += a positive count of what it had to ignore (entries with a column outside [0, G), rows
 *   whose indptr entries leave [0, nnz] or decrease); status (one int32, device memory) is zeroed by the caller.
 *   Deterministic: each element is written by one plain store.  rows = 0 launches nothing; ldy < G, G <= 0 or
 *   nnz > INT32_MAX: DCAHIP_EINVAL.
 */
int dcahip_csr_expand(const int* indptr, const int* indices, const float* values, long nnz, int rows, int G,
                      float* Y, long ldy, int* status, void* stream);

/*
 * CSR compress: dense fp32 rows (a row chunk of a dense host count matrix, copied to the device as it is) -> their CSR,
 * in place of the host's scipy.sparse.csr_matrix(dense) on what sc.read hands over (dca/io.py:58-59) when the counts go
 * counts-resident (below).  An entry is stored when x != 0, as scipy decides it: -0.0 is dropped, a NaN is kept.
 *   X [rows, ld] fp32 (ld >= G; columns G .. ld are never interpreted).  indptr [rows + 1] int64: every word written,
 *   indptr[0] = base, indptr[r + 1] = base + the entries of rows 0 .. r (base: the entries of the matrix in front of this
 *   chunk, so that a matrix beyond 2^31 entries is built chunk by chunk).  indices (int32) / values (fp32) [cap]: the
 *   chunk's entries from position 0 on (position = indptr - base), rows in order, columns ascending, the value's bits
 *   unchanged.  cap >= rows * G always suffices; entries beyond cap are not written and counted into *status (one int32,
 *   zeroed by the caller).  Three launches on the stream (counts per row, their prefix sum, the stores): one plain store
 *   per entry, no atomics on the arrays, deterministic; nothing outside the buffers is read or written.  rows = 0 launches
 *   nothing.  ld < G, G <= 0, base < 0 or rows * G > INT32_MAX: DCAHIP_EINVAL.
 *
 * CSR subset: a resident CSR (next comment) without the rows / columns whose keep byte is 0, in place of a second upload
 * after scanpy's filter_genes / filter_cells (dca/io.py:90-92) and normalize_per_cell's drop of empty cells (:99-101).
 *   row_keep [n], col_keep [G] bytes (either may be NULL: keep all).  out_indptr [n_out + 1] int64 from 0, out_indices /
 *   out_values [cap]: the kept rows in order, their kept entries in order, columns renumbered by the prefix sum of
 *   col_keep (computed here).  n_out: the number of kept rows the caller sized out_indptr for (n when row_keep is NULL,
 *   else DCAHIP_EINVAL); if row_keep keeps another number, *status is raised and the result is not to be used.  cap >= nnz
 *   always suffices; what does not fit is counted into *status, as is malformed input (clamped as in the entries below).
 *   ws: n + G int32 of scratch (may be NULL when both masks are).  Plain stores only, deterministic, on the stream.
 */
int dcahip_csr_compress(const float* X, long ld, int rows, int G, long base, long* indptr, int* indices, float* values,
                        long cap, int* status, void* stream);
int dcahip_csr_subset(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                      const unsigned char* row_keep, const unsigned char* col_keep, int n_out, long* out_indptr,
                      int* out_indices, float* out_values, long cap, int* ws, int* status, void* stream);

/*
 * Resident CSR (counts-resident mode): the raw counts stay on the device as CSR -- indptr [n + 1] int64 (absolute offsets),
 * indices int32, values fp32, canonical rows -- and every step builds only its own minibatch.  The preprocessing is that
 * of dca/io.py:88-111 (as dcahip_prep_*), the per-batch rows those of the Keras feed, dca/train.py:83-98.  All these
 * entries share csr_expand's guarantees: a storage row outside [0, n), an indptr entry outside [0, nnz] or decreasing, a
 * column outside [0, G) is clamped / skipped and counted into *status (one int32, zeroed by the caller); nothing outside
 * the buffers is read or written.
 *
 *   dcahip_csr_gather     the minibatch tile: destination row r < B takes storage row perm[*cursor + r] (perm != NULL) or
 *                         row0 + r (perm == NULL).  Writes EVERY element of Y[r, 0 .. ldy) (the count or 0) and, when X
 *                         is given, of X[r, 0 .. ldx): bit for bit what dcahip_prep_col_pass followed by dcahip_prep_scale
 *                         write for that row, x = (f(y / fac[row]) - mean[g]) / std[g], f = log1p if do_log, each step
 *                         optional as there (fac, mean / std may be NULL; mean and std together); pad columns g >= G hold
 *                         f(0 / fac[row]) unscaled, as prep_col_pass leaves them.  sf_out[r] = sf[row] (sf_out may be
 *                         NULL).  Reads nothing from the host: capturable in a step's graph, valid on every replay.
 *                         One plain store per element, no atomics on the tiles.  B = 0 launches nothing.
 *   dcahip_csr_gather_cols
 *                         the minibatch tile of a network that reads all G input genes and fits G_out of them
 *                         (train(output_subset=...), dca/train.py:85-87): dcahip_csr_gather's arguments, then col_out [G]
 *                         int32 -- the output column of input gene g, -1 when the gene is not fitted -- and G_out.
 *                         X[r, 0 .. ldx) is over ALL G input genes, bit for bit dcahip_csr_gather's X tile (pad columns and
 *                         the fac / do_log / mean / std options included).  Y[r, 0 .. ldy), ldy >= G_out: Y[r, col_out[g]]
 *                         = the count of gene g, every other element +0.0, the pad columns G_out .. ldy included.  sf_out,
 *                         the choice of the storage row, the capture guarantee, "one plain store per element" and B = 0 as
 *                         dcahip_csr_gather.  Besides the shared guarantees, an entry whose col_out value lies outside
 *                         [-1, G_out) is skipped and counted into *status (once per entry).  Two genes with the same
 *                         output column are the caller's error: one of the two counts lands there.
 *   dcahip_csr_gather_compact
 *                         the same minibatch tile in the byte-store format of K-SPARSE (below), for the kernels that read
 *                         the compact counts (dcahip_heads_fused, dcahip_enc0_fwd_lut, dcahip_enc0_dw_sparse) with
 *                         storage row = tile row.  Writes EVERY byte of Yc[r, 0 .. ldc), ldc = dcahip_counts_compact_ld(G):
 *                         bit for bit what dcahip_counts_compact writes from dcahip_csr_gather's Y tile (counts 0 .. 254 as
 *                         is, 255 = escape, pad columns 0; a value that is not a count is stored as 0 and counted into
 *                         *status as dcahip_counts_compact counts it into status[0]).  The tile's overflow list: ovf_ptr
 *                         [B + 1] (every word written; a prefix sum over the tile's rows, made on the stream), ovf_col /
 *                         ovf_val [ovf_cap] = (column, count) of the counts >= 255 of row r at ovf_ptr[r] .. ovf_ptr[r + 1]
 *                         - 1 in column order.  Entries beyond ovf_cap are not written, ovf_ptr never points beyond it, and
 *                         their number is added to *status.  All three NULL (ovf_cap ignored): the caller knows that no
 *                         count reaches 255; one met all the same is counted into *status.  sf_out[r] = sf[row],
 *                         fac_out[r] = fac[row] (each may be NULL; fac_out needs fac; a row outside [0, n) gives 0 / 1).
 *                         X (may be NULL): the fp32 input tile, bit for bit dcahip_csr_gather's.  The fp32 Y tile is never
 *                         written.  Yc 16-byte aligned, ldc a multiple of 16.  Capturable, plain stores only, B = 0
 *                         launches nothing.
 *   dcahip_csr_col_pass   the per-gene fp64 partials [R][2][Gp] of x = f(y / fac) and x*x that dcahip_prep_col_pass
 *                         produces for the dense rows, bit for bit (same row chunks R = dcahip_prep_chunks(n), same row
 *                         order; the zeros it skips add +0.0): dcahip_prep_col_finish takes them unchanged (gene totals
 *                         with fac = NULL, do_log = 0; mean / std otherwise).
 *   dcahip_csr_row_sums   out[r] = sum of row r in fp64, rounded to fp32: dcahip_prep_row_sums for counts (exact).
 */
int dcahip_csr_gather(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                      const int* perm, const long long* cursor, long row0, int B, const float* sf,
                      const float* fac, int do_log, const float* mean, const float* stdv, float* Y, long ldy,
                      float* X, long ldx, float* sf_out, int* status, void* stream);
int dcahip_csr_gather_cols(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                           const int* perm, const long long* cursor, long row0, int B, const float* sf,
                           const float* fac, int do_log, const float* mean, const float* stdv, float* Y, long ldy,
                           float* X, long ldx, float* sf_out, int* status, const int* col_out, int G_out, void* stream);
int dcahip_csr_gather_compact(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                              const int* perm, const long long* cursor, long row0, int B, const float* sf,
                              const float* fac, int do_log, const float* mean, const float* stdv,
                              unsigned char* Yc, long ldc, int* ovf_ptr, int* ovf_col, float* ovf_val, int ovf_cap,
                              float* X, long ldx, float* sf_out, float* fac_out, int* status, void* stream);
int dcahip_csr_col_pass(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                        const float* fac, int do_log, double* col_part, int* status, void* stream);
int dcahip_csr_row_sums(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                        float* out, int* status, void* stream);

/*
 * K-SPLIT: binomial thinning of a resident CSR of counts into two independent parts -- molecular cross-validation (Batson
 * et al. 2019) / count splitting (Neufeld et al. 2022): fit on part A, evaluate the likelihood of part B's molecules with the
 * size factors scaled by (1 - f) / f.  Beyond the reference, which scores a model only on counts its encoder has seen
 * (val_loss, dca/train.py:91-98); no reference call site.
 *
 * The draw.  A stored entry of cell i, gene j with the integer count y, 1 <= y <= 2^24:
 *   a(i, j) = #{ t in [0, y) : word (t & 3) of philox4x32_10(counter = (i, j, t >> 2, 0x7468696E), key = (lo32(seed),
 *               hi32(seed))) < threshold }
 * compared in 64 bits: threshold = 2^32 keeps every molecule, 0 keeps none; a fraction f is threshold = int(f 2^32), and a is
 * Binomial(y, threshold / 2^32) exactly, in integer arithmetic.  Part A receives a, part B y - a.  i = row_ids[r] (row_ids
 * NULL: r), its low 32 bits; j = the entry's column.  Counter word 3 is a constant no K-DROP counter holds there
 * (dcahip_dropout_apply puts its layer code, 0 .. 255, in that word), so the two streams of one seed never meet.  a depends
 * on (seed, i, j, y, threshold) only: not on the launch shape, the order of the rows or how an entry's molecules are shared
 * between lanes (a count above 64 is drawn by the whole wave, its Philox blocks dealt round the lanes and the partial counts
 * added; smaller ones by one lane) -- dca_amd/mcv.py thin_counts_host restates it in numpy and gives the same bits.
 *
 *   indptr / indices / values, nnz, n, G : the resident CSR (as dcahip_csr_gather)
 *   row_ids [n] int64     : the global cell id of every row (a subset or a permutation of a dataset draws what the whole
 *                           dataset draws for those cells); NULL: row r is cell r
 *   indptr_a, indptr_b [n + 1] int64 from 0 (every word written); indices_x / values_x [cap]: each part's entries, rows in
 *                           order, every row in the column order of the source row, values fp32 integers.  Explicit stored
 *                           zeros are dropped from both parts, entries with a = 0 from A, with y - a = 0 from B.
 *                           cap >= nnz always suffices; what does not fit is counted into *status.
 *   workspace             : >= dcahip_csr_thin_workspace_bytes(n, nnz) bytes (a per stored entry: the draws are made once,
 *                           in the count phase, and read back by the store phase); needs no initialisation
 *   status                : one int32, zeroed by the caller: += malformed row pointers and columns (clamped / skipped as in
 *                           the entries above) and every value that is negative, not an integer or above 2^24 (such an
 *                           entry goes to neither part) -- the result is not to be used then
 * Four launches on the stream (draw + count per row, one prefix sum per part, the stores); one plain store per entry, no
 * atomics except the status counter: two calls give the same bits.  Nothing outside the buffers is read or written.
 * DCAHIP_EINVAL (nothing launched): n < 0, G <= 0, nnz < 0, cap < 0, threshold > 2^32, a missing pointer.  n = 0 launches
 * nothing and returns 0; nnz = 0 writes two zero row pointers.
 */
long dcahip_csr_thin_workspace_bytes(int n, long nnz);
int dcahip_csr_thin(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                    const long* row_ids, unsigned long long threshold, unsigned long long seed,
                    long* indptr_a, int* indices_a, float* values_a,
                    long* indptr_b, int* indices_b, float* values_b, long cap,
                    void* workspace, int* status, void* stream);

/*
 * Keras clipvalue + Keras RMSprop (momentum 0) on one flat parameter buffer:
 *   g = clip(g, -clip, clip); ms = rho*ms + (1-rho)*g*g; w -= lr * g / (sqrt(ms) + eps)
 * (epsilon OUTSIDE the root: standalone keras 2.2 / 2.3 `p - lr * g / (K.sqrt(new_a) + self.epsilon)` and tf.keras
 * OptimizerV2's dense update without momentum `var - lr_t * grad / (sqrt(rms_t) + epsilon)` alike; only TF's fused
 * ApplyRMSProp kernel, taken with momentum > 0, puts it inside.)
 * Replaces opt.RMSprop(lr, clipvalue) (dca/train.py:54-57).  *lr is read from device memory
 * so ReduceLROnPlateau does not invalidate a captured graph.  clip <= 0 disables clipping.
 * When at least one of loss, hist, acc, cursor is given, the same launch goes on with what dcahip_step_end does with
 * them (loss slot -> history / epoch accumulator, batch cursor += advance): one launch less per step, which is what the
 * reference-default batch of 32 is made of.  All four NULL: the update alone.
 */
int dcahip_rmsprop_clip(float* w, const float* g, float* ms, long n, const float* lr,
                        float rho, float eps, float clip, const float* loss, double weight,
                        float* hist, int rows_per_slot, double* acc, long long* cursor, int advance,
                        void* stream);

/*
 * K-OPT: the other Keras optimizers selectable through dca/train.py:54-57 and the l1 / l2 kernel
 * regularisers of dca/network.py:114-126,144-146,369-380, on the flat parameter buffer.
 * dcahip_optimizer_step: g clipped to [-clip, clip] (clip <= 0: off), then the tf.keras update
 * with default hyper-parameters (formulas in dcahip_opt.hip); slot1 / slot2 are the optimizer's
 * state buffers ([n], may be NULL where the optimizer has none: SGD none, Adagrad slot1 (init 0.1),
 * Adadelta / Adam / Adamax both).  *iter = completed steps (device memory; Adam / Adamax bias
 * correction), advanced by dcahip_counter_add.  RMSprop is dcahip_rmsprop_clip.
 * dcahip_l1l2_apply: for each segment [start, end) of the flat buffer: g += l1 sign(w) + 2 l2 w
 * (g may be NULL: penalty only) and *loss_inout += sum l1 |w| + l2 w^2 (Keras adds the
 * regularisation losses to the reported loss, training and validation).
 */
#define DCAHIP_OPT_SGD       0
#define DCAHIP_OPT_RMSPROP   1
#define DCAHIP_OPT_ADAGRAD   2
#define DCAHIP_OPT_ADADELTA  3
#define DCAHIP_OPT_ADAM      4
#define DCAHIP_OPT_ADAMAX    5
int dcahip_optimizer_step(int kind, float* w, const float* g, float* slot1, float* slot2, long n,
                          const float* lr, const long long* iter, float clip, void* stream);
int dcahip_counter_add(long long* counter, int v, void* stream);
/* tf.keras Nadam (beta_1 .9, beta_2 .999, epsilon 1e-7, schedule decay .004): m, v = the two slots ([n], zero
 * initialised), *m_schedule = running product of the momentum schedule (device float, initialised to 1 by the
 * host; the call multiplies it by mu_t after the update has read it), *iter = completed steps as above. */
int dcahip_nadam_step(float* w, const float* g, float* m, float* v, long n, const float* lr,
                      const long long* iter, float* m_schedule, float clip, void* stream);
#define DCAHIP_REG_MAX_SEGS 16
typedef struct {
    int nseg;
    long start[DCAHIP_REG_MAX_SEGS];
    long end[DCAHIP_REG_MAX_SEGS];
    float l1[DCAHIP_REG_MAX_SEGS];
    float l2[DCAHIP_REG_MAX_SEGS];
} dcahip_reg_desc;
int dcahip_l1l2_workspace_doubles(void);
int dcahip_l1l2_apply(const dcahip_reg_desc* d, const float* w, float* g, float* loss_inout,
                      double* workspace, void* stream);

/*
 * K-DROP: Keras Dropout of dca/network.py:98-99 (input_dropout) and :137-138 (hidden_dropout),
 * training mode only: out[r, c] = x[src(r), c] * keep(r, c) / (1 - rate).
 * src(r) = perm[*cursor + r] when perm != NULL (the minibatch gather of the input layer), else r;
 * in place (out == x) is allowed when perm == NULL.  The same call applied to the incoming
 * gradient is the backward pass (the mask is recomputed, never stored).
 * keep(r, c): Philox4x32-10 (Salmon et al., SC'11) with key = seed, counter =
 * (group lo, group hi, (uint32)*step, layer), group = (row0 + r) * ceil(h / 4) + c / 4, word c % 4
 * of the output block; u = (word >> 8) * 2^-24 and the unit is kept when u >= rate (TF:
 * random_uniform >= rate).  row0 = index of this rank's first row inside the global batch, so a
 * data-parallel run draws the masks of the single-process run.  *step is device memory (captured
 * step graphs stay valid); the host advances it with dcahip_counter_add.  The reference's masks
 * come from TF's stateful RNG and are not reproducible across TF builds: parity here is statistical
 * (keep frequency, scaling) and exact against oracle/net_np.py's restatement of this generator,
 * which is pinned on the published Random123 known-answer vectors.
 */
int dcahip_dropout_apply(const float* x, long ldx, const int* perm, const long long* cursor, int B, int h,
                         float rate, unsigned long long seed, const long long* step, int layer, long row0,
                         float* out, long ldo, void* stream);

/*
 * K-SPARSE: compact count storage and the first Dense layer on the non-zero counts only.
 *
 * The reference turns the ~93 %-zero count matrix into a DENSE fp32 input X = scale(log1p(counts / size factor))
 * (dca/io.py:88-111; scanpy normalize_per_cell, log1p, scale) and feeds it to the first Dense layer
 * (dca/network.py:124-126); TensorFlow's autodiff forms the weight gradient X^T dZ from the same dense matrix.
 * With x[c, g] = (L[c, g] - mean[g]) / std[g], L = log1p(y / fac[c]) (0 where y = 0; each step optional) both
 * products need the non-zero counts only (formulas in dca_amd/csrc/dcahip_sparse.hip).
 *
 * Compact counts: Yc [n, ldc] bytes, ldc = dcahip_counts_compact_ld(G) (G rounded up to 16, pad columns 0); a count
 * 0 .. 254 is stored as is, 255 is an escape whose value is looked up in a per-row overflow list: entries
 * ovf_ptr[r] .. ovf_ptr[r + 1] - 1 of (ovf_col, ovf_val), sorted by column (all three may be NULL when no count
 * reaches 255).  dcahip_counts_compact writes Yc from the fp32 counts and ADDS to status[0] the number of values that
 * are not counts (negative, fractional, not finite: stored as 0 -- the caller must not use the compact store then)
 * and to status[1] the number of escapes (the caller builds the overflow list from Y >= 255).
 * K-HEADS takes the same store through the `yc` arguments of dcahip_heads_fused (its contract is stated there).
 */
long dcahip_counts_compact_ld(int G);
int dcahip_counts_compact(const float* Y, long ldy, int n, int G, unsigned char* Yc, long ldc, int* status,
                          void* stream);
/* First-layer widths the kernels below take (32, 64, 128). */
int dcahip_enc0_sparse_supported(int H1);
/*
 * Weight (+ bias) gradient of the first Dense layer from the compact counts:
 *   gW [G + 1, ldg]: rows g < G = sum_c x[c, g] dZ[c, :], row G = column sums of dZ (what dcahip_sgemm(ta = 1,
 *   colsum_row = 1) writes from the dense X).  Batch row c = storage row perm[*cursor + row_base + c] (perm NULL:
 *   *cursor + row_base + c) of Yc / fac.  fac NULL: no size-factor division; do_log 0: no log1p; mean NULL: 0;
 *   stdv NULL: 1.  lutp = dcahip_enc0_lut(fac, do_log) of the same cells.  n_cells * ldc must stay below 2^32.
 *   Arithmetic: X^T dZ on the matrix pipe, six bf16 products per fp32 product as dcahip_sgemm; deterministic.
 *   workspace >= dcahip_enc0_dw_sparse_workspace_bytes(B, G, H1), 16-byte aligned.
 * Replaces the autodiff of dca/network.py:124-126 w.r.t. the first kernel on the input of dca/io.py:88-111.
 */
/* lutp [n, dcahip_enc0_lut_entries() = 128] entries of 8 bytes: entry k of cell r = f(k / fac[r]) (f = log1p if do_log,
 * fac NULL: 1) split into the three bf16 pieces the matrix products use ({p0 | p1 << 16, p2}) -- made once per dataset, so
 * that the first-layer kernels LOOK UP their operand instead of dividing, taking logarithms and splitting.  The kernels
 * hold the first 32 (forward), 64 (first weight-gradient kernel) or all 128 (ring weight-gradient kernel) entries of their
 * cells in LDS; counts beyond take the formula (hardware log2 with an exact-ratio correction, ~2e-7 relative). */
int dcahip_enc0_lut(const float* fac, int do_log, int n, void* lutp, void* stream);
int dcahip_enc0_lut_entries(void);
long dcahip_enc0_dw_sparse_workspace_bytes(int B, int G, int H1);
/* The 64-unit weight gradient has two kernels (csrc/dcahip_sparse.hip): enc0_dw_kernel (counts through an LDS tile, lookups
 * and products of a 64-row block between two barriers) and enc0_dw2_kernel (512 genes per workgroup, operands staged
 * global -> LDS into a five-stage ring four K steps ahead, a wave's LDS / vector work behind its own matrix instructions).
 * `form` (an argument of the call: the library keeps no switch): 0 = by the shape -- the ring kernel from 1024 batch rows
 * up, the first kernel below --, 1 = always the first, 2 = always the ring kernel (A/B runs and the parity tests of both).
 * Same products, same row order inside a split; the number of splits differs.  The workspace size covers either. */
int dcahip_enc0_dw_sparse(const unsigned char* Yc, long ldc, const int* ovf_ptr, const int* ovf_col,
                          const float* ovf_val, const float* fac, int do_log, const void* lutp, const float* mean,
                          const float* stdv, const int* perm, const long long* cursor, long row_base,
                          int B, int G, int H1, const float* dZ, long ldz, float* gW, long ldg,
                          void* workspace, long workspace_bytes, int form, void* stream);
/*
 * Forward of the first Dense layer from the compact counts, Z [B, ldz] = X W + bias with X as above, W [G, ldw], on the
 * matrix pipe (H1 = 32 or 64; 0 workspace bytes = width not taken): the A
 * operand is looked up from the byte store through lutp (dcahip_enc0_lut of the same cells: counts 0 .. 31 from the
 * table, larger ones and escapes by the formula), W / std is split into bf16 pieces once per call, six bf16 products per
 * fp32 product as dcahip_sgemm, gene chunks added in a fixed order: deterministic.  workspace >=
 * dcahip_enc0_fwd_lut_workspace_bytes(B, G, H1), 16-byte aligned, any content; n_cells * ldc must stay below 2^32 (lutp).
 * Alignment: Z 16 bytes and ldz a multiple of 4 (else DCAHIP_EINVAL); W, mean, stdv and bias need only that of a float
 * (bias NULL: none; a bias that is not 16-byte aligned is read with scalar loads, same values).
 * Replaces Dense(hidden_size[0]) of dca/network.py:124-126 on the input of dca/io.py:88-111.
 */
long dcahip_enc0_fwd_lut_workspace_bytes(int B, int G, int H1);
int dcahip_enc0_fwd_lut(const unsigned char* Yc, long ldc, const int* ovf_ptr, const int* ovf_col,
                        const float* ovf_val, const float* fac, int do_log, const void* lutp, const float* mean,
                        const float* stdv, const int* perm, const long long* cursor, long row_base,
                        int B, int G, int H1, const float* W, long ldw, const float* bias,
                        float* Z, long ldz, void* workspace, long workspace_bytes, void* stream);

/*
 * K-NEIGHBOURS (dca_amd/csrc/dcahip_knn.hip): exact (brute-force) Euclidean k-nearest neighbours of every query row among
 * the candidate rows, distance evaluation and top-k selection fused: no nq x n matrix exists.  Beyond the reference, which
 * leaves the neighbour graph of obsm['X_dca'] to scanpy on the host; no reference call site.
 *
 *   Q [nq, ldq], X [n, ldx] : queries and candidates, d columns each (ldq, ldx >= d); Q may be X
 *   k                       : neighbours per query, 1 .. 64;  d: 1 .. 128;  n < 2^31
 *   self_offset             : query row q IS candidate row self_offset + q and is left out BY INDEX (other copies of the
 *                             row stay, at distance 0); -1: nothing is left out
 *   splits                  : 0 = the library's choice, dcahip_knn_splits(nq, n, d, k): enough workgroups to fill the part
 *                             when the query blocks are few, every split keeping about 1 000 candidates; 1 .. 64: this
 *                             many contiguous candidate ranges (an argument of the call: the library keeps no switch)
 *   idx_out [nq, ldo] int32, d2_out [nq, ldo] fp32 (ldo >= k): columns 0 .. k-1 of every row are written, nothing else
 *   ws                      : >= dcahip_knn_workspace_bytes(nq, n, d, k, splits) bytes, 16-byte aligned, any content: the
 *                             sorted list of every (split, query), and X zero-padded when d is not 8, 16, 32, 64 or 128
 *   status                  : one int32, zeroed by the caller: += the non-finite coordinates met in Q and in X (a matrix
 *                             passed as both is counted twice); the outputs are unspecified then, but written in bounds
 *
 * The distance: d2(a, b) = s0 + s1, s_p = fma(a_j - b_j, a_j - b_j, s_p) over the j of parity p in ascending order, all in
 * fp32 -- the direct form (the Gram form |a|^2 + |b|^2 - 2 a.b cancels catastrophically on clusters far from the origin,
 * exactly what a ReLU latent is).  The order is a function of d alone, so d2(a, b) and d2(b, a) are the same bits, d2 >= 0,
 * equal rows are at exactly 0, and the relative error is at most (d + 3) 2^-24 to first order.
 * The result: per query the k smallest candidates under the total order (d2, index) ascending, in that order, SQUARED
 * distances; with fewer than k candidates the tail is index -1 at +inf.  Because the order is total the output is the same
 * bits for every `splits`.  Three launches on the stream (check / pad, scan, merge), plain stores only (the status counter
 * aside), every index formed in 64 bits; nothing outside the operands is read or written.
 * DCAHIP_EINVAL (nothing launched): k outside 1 .. 64, d outside 1 .. 128, nq < 0, n < 0, splits outside 0 .. 64, a leading
 * dimension below its row length, self_offset < -1, a missing pointer (the two size functions return it for the same
 * shapes).  nq = 0 launches nothing and returns 0.
 */
int dcahip_knn_splits(int nq, int n, int d, int k);
long dcahip_knn_workspace_bytes(int nq, int n, int d, int k, int splits);
int dcahip_knn(const float* Q, long ldq, int nq, const float* X, long ldx, int n, int d, int k,
               long self_offset, int splits, int* idx_out, float* d2_out, long ldo,
               void* ws, int* status, void* stream);

/*
 * K-MEANS (dca_amd/csrc/dcahip_kmeans.hip): Lloyd's k-means of the rows of X and its k-means++ seeding, on the device.  Beyond
 * the reference, which leaves clustering of obsm['X_dca'] to the host; no reference call site.
 *
 *   X [n, ldx]              : the points, d columns (ldx >= d);  1 <= d <= 128, 1 <= k <= 256, 0 <= n < 2^31 (k may exceed n)
 *   ws                      : >= dcahip_kmeans_workspace_bytes(n, d, k) bytes, 16-byte aligned, any content (the same size
 *                             serves the step and the seeding; nothing in it is carried from one call to the next)
 *   status                  : one int32, zeroed by the caller: += the non-finite coordinates met in X and in C_in (seeding: in
 *                             X); the outputs are unspecified then, but written in bounds
 *
 * The distance is dcahip_knn's, the same function compiled from the same definition (csrc/knn_dist.hpp): d2 = s0 + s1, fma
 * over the coordinates of each parity ascending, fp32.  A (point, centre) pair gets the bits the neighbour search gives it.
 *
 * dcahip_kmeans_step: one Lloyd iteration, two launches, no floating-point atomic.
 *   C_in [k, ldc]           : the centres (ldc >= d);  C_out [k, ldco] (ldco >= d) the new ones; C_out may be C_in
 *   labels [n] int32        : IN the labels of the previous iteration (-1 everywhere before the first), OUT labels[i] = the c
 *                             that minimises the total order (d2(x_i, C_in[c]), c): what dcahip_knn(Q = X, X = C_in, k = 1,
 *                             self_offset = -1) returns, bit for bit
 *   d2_out [n] fp32         : that squared distance
 *   counts [k] int32        : the members of every cluster;  sums [k, lds] double (lds >= d): sums[c][j] = the sum of
 *                             (double)x_ij over the members of c (columns 0 .. d-1 are written)
 *   inertia [1] double      : the sum of (double)d2_out[i];  changed [1] int32: the i whose label differs from the one passed in
 *   C_out[c] = (float)(sums[c] / counts[c]): the division in double, one rounding to fp32.  An empty cluster keeps C_in[c],
 *   except that, when a cluster is empty and the largest d2 of the iteration is > 0, the LOWEST-NUMBERED empty cluster takes
 *   the coordinates of the point with the largest key (d2, index) (re-seeding; at most one cluster per iteration; its count
 *   and sums of this iteration stay 0).  reseeded [1] int32: 1 for such an iteration, else 0.
 *   state [1] int32, iter   : zeroed by the caller before the first iteration; the first iteration number `iter` (>= 1) with
 *                             changed == 0 and reseeded == 0 is stored in it, later iterations leave it.  An iteration after
 *                             that one (C_in = its C_out) is a no-op bit for bit -- same labels, d2, sums, centres -- so a host
 *                             may read state every few iterations only.
 *   Sums and inertia are added in an order that depends on (n, d, k) alone: two calls on the same inputs give the same bits.
 *   Plan (a pure function of the shape): the per-workgroup cluster sums live in LDS while k * pad(d) <= 5120 doubles (pad = the
 *   next of 8, 16, 32, 64, 128), else in the workgroup's slice of the workspace.
 *
 * dcahip_kmeans_seed: k-means++ (Arthur & Vassilvitskii 2007), k rounds on the stream without a host round trip, integer
 * arithmetic after the distances and so reproducible on the host to the row.  Round t = 0 .. k-1 takes one Philox4x32-10 block,
 * key = seed, counter (t, init, 0, 0x6B6D2B2B), r64 = (word1 << 32) | word0.  Round 0: row floor(r64 n / 2^64).  Round t >= 1:
 * m_i = min(m_i, d2(x_i, last centre)), M = max m_i; M = 0: row floor(r64 n / 2^64); else e with M 2^e in [2^30, 2^31),
 * q_i = floor(m_i 2^e) (exact), S = sum q_i (< 2^62), T = floor(r64 S / 2^64), the row is the smallest i whose inclusive prefix
 * sum of q exceeds T.  A point whose weight is below 2^-30 of the largest has q_i = 0 and cannot be drawn (a bias of order
 * 1e-9).  init (>= 0) numbers the initialisation.
 *   rows_out [k] int32      : the rows drawn;  C_out [k, ldc] (ldc >= d): those rows of X
 *
 * Every index is formed in 64 bits; nothing outside the documented outputs and the workspace is written.
 * DCAHIP_EINVAL (nothing launched): k outside 1 .. 256, d outside 1 .. 128, n < 0, a leading dimension below d, iter < 1,
 * init < 0, a missing pointer (the size function returns it for the same shapes).  n = 0 launches nothing and returns 0.
 */
long dcahip_kmeans_workspace_bytes(int n, int d, int k);
int dcahip_kmeans_step(const float* X, long ldx, int n, int d, int k, const float* C_in, long ldc, float* C_out, long ldco,
                       int* labels, float* d2_out, int* counts, double* sums, long lds, double* inertia,
                       int* changed, int* reseeded, int* state, int iter, void* ws, int* status, void* stream);
int dcahip_kmeans_seed(const float* X, long ldx, int n, int d, int k, unsigned long long seed, int init,
                       int* rows_out, float* C_out, long ldc, void* ws, int* status, void* stream);

/*
 * K-SILHOUETTE (dca_amd/csrc/dcahip_silhouette.hip): the silhouette coefficient (Rousseeuw 1987) of every labelled row of X
 * under a clustering, Euclidean, exact: every pair of labelled points is visited, no n x n and no n x k matrix exists.  Beyond
 * the reference, which leaves the quality of a clustering of obsm['X_dca'] to the host; no reference call site.
 *
 *   X [n, ldx]              : the points, d columns (ldx >= d);  1 <= d <= 128, 0 <= n < 2^31
 *   labels [n] int32        : codes in [0, k), 2 <= k <= 256 (k may exceed n); ANY other value, -1 included, means "in no
 *                             cluster": such a point is neither a query nor a candidate
 *   splits                  : 0 = the library's choice, dcahip_silhouette_splits(n, d, k): enough workgroups to fill the part
 *                             when the query blocks of 256 are few, every split keeping about 1 000 candidates, and the
 *                             segment partials (below) staying under 256 MiB -- 1 from 392 961 points on; 1 .. 64: this many
 *                             equal ranges of the sorted candidates (an argument of the call: the library keeps no switch)
 *   s_out, a_out, b_out [n] double, nearest_out [n] int32 : per point, at its ORIGINAL row (below)
 *   counts [k] int32        : n_c, the members of every cluster
 *   cluster_mean [k] double : the mean of s over the members of c (NaN when empty);  mean [1]: over all labelled points
 *   ws                      : >= dcahip_silhouette_workspace_bytes(n, d, k, splits) bytes, 16-byte aligned, any content.  With
 *                             r16 = rounding up to 16, DP = the next of 8, 16, 32, 64, 128 from d and nb = the workgroups of
 *                             the counting sort (<= 1024):  r16(4 nb k) + r16(4 (k + 1)) + 2 r16(4 n) + r16(8 n) + r16(4 n DP)
 *                             + (splits > 1 ? r16(8 (splits + k - 1) n) : 0)
 *   status                  : one int32, zeroed by the caller: += the non-finite coordinates met in X (of unlabelled rows
 *                             too); the outputs are unspecified then, but written in bounds
 *
 * delta(i, j) = the correctly rounded fp32 square root of d2(x_i, x_j), d2 the distance of dcahip_knn compiled from the same
 * definition (csrc/knn_dist.hpp).  S(i, c) = the sum over the j of label c of (double)delta(i, j), in double, j ascending
 * (j = i included: it adds exactly 0).  a_i = S(i, own) / (n_own - 1);  b_i = the minimum over the non-empty c != own of
 * S(i, c) / n_c;  nearest_i = the lowest c that attains it;  s_i = (b_i - a_i) / max(a_i, b_i): double division and
 * subtraction, one rounding each.  Conventions (scikit-learn's where it has one): n_own = 1 gives s = a = 0; max(a, b) = 0
 * gives s = 0; an unlabelled point has s = a = b = NaN and nearest = -1; with fewer than two non-empty clusters b = +inf,
 * nearest = -1 and s = NaN for every labelled point.
 *
 * The plan is a pure function of (n, d, k, splits): a stable counting sort of the labelled points by label (integer work)
 * into a zero-padded copy of X in (label, index) order, so that the candidates of a cluster are contiguous; a scan, grid
 * (query blocks of 256, splits), one lane per query with ONE double accumulator, the candidate row the same for the whole
 * wave; with more than one split the partial sum of every (split, cluster) segment -- at most splits + k - 1 per query -- goes
 * to the workspace and a finishing pass adds them in ascending split order; the two means are fixed trees.  No floating-point
 * atomic: two calls give the same bits, and where the double sums are exact every `splits` gives the same bits.  Plain stores
 * only (the status counter and the integer counters of the sort aside), every index formed in 64 bits; nothing outside the
 * documented outputs and the workspace is written.
 * DCAHIP_EINVAL (nothing launched): k outside 2 .. 256, d outside 1 .. 128, n < 0, splits outside 0 .. 64, ldx < d, a missing
 * pointer (the two size functions return it for the same shapes).  n = 0 launches nothing and returns 0.
 */
int dcahip_silhouette_splits(int n, int d, int k);
long dcahip_silhouette_workspace_bytes(int n, int d, int k, int splits);
int dcahip_silhouette(const float* X, long ldx, int n, int d, const int* labels, int k, int splits,
                      double* s_out, double* a_out, double* b_out, int* nearest_out,
                      int* counts, double* cluster_mean, double* mean,
                      void* ws, int* status, void* stream);

/*
 * K-LOUVAIN (dca_amd/csrc/dcahip_louvain.hip): Louvain modularity optimisation (Blondel et al. 2008) of the neighbour graph
 * dcahip_knn writes, on the device, in integers throughout: the labels equal those of the host restatement
 * (tests/_louvain_ref.py) and are the same on every run.  Beyond the reference, which leaves community detection on
 * obsm['X_dca'] to scanpy on the host; no reference call site.
 *
 * dcahip_graph_symmetrize: W = A + A^T of the directed 0/1 adjacency A of an index array, as a CSR of unit entries.
 *   idx [n, ldi] int32      : k columns (ldi >= k >= 1).  -1 is padding; an entry equal to its row is dropped; any other entry
 *                             outside 0 .. n-1 adds 1 to *status and is never used as an index
 *   rowptr [n + 1] int64    : OUT the row starts; rowptr[n] = 2m, the number of entries
 *   col [cap] int32         : OUT the neighbours, cap >= 2 n k entries of room.  A mutual pair stands twice in both rows.  The
 *                             order inside a row may differ from run to run (an integer atomic hands out the places)
 *   deg [n] int32           : OUT the rows' lengths = the weighted degrees k_i
 *   ws                      : >= dcahip_graph_symmetrize_workspace_bytes(n, k) bytes, 16-byte aligned, any content
 *   status                  : one int32, zeroed by the caller
 *   Six launches (histogram, three of a scan, fill).  DCAHIP_EINVAL (nothing launched): n < 0, k < 1, ldi < k,
 *   2 n k >= 2^31, cap < 2 n k, a missing pointer.  n = 0 writes rowptr[0] = 0.
 *
 * The level.  A CSR graph of n vertices: rowptr [n + 1] int64, col [nnz] int32, wt [nnz] int32 (NULL: every entry weighs 1);
 * an undirected edge stands in both rows, a self-loop (col = row) once, carrying the weight inside a merged community in both
 * directions.  k_i = the sum of row i, 2m = the sum of all k_i < 2^31.  R = 1024, g = round(resolution R) in 1 .. 64 R,
 * M = 2m R.  Every vertex carries a community label in 0 .. n-1; tot_c = the sum of k_i over the members of c.
 *   A sweep is synchronous: every vertex decides from `labels` and `tot` as they stand.  With a its own community and k_{i,c}
 *   the weight from i to community c (self-loop excluded): staying scores k_{i,a} M - g k_i (tot_a - k_i), moving to a
 *   neighbouring c != a scores k_{i,c} M - g k_i tot_c; an even sweep admits only c < a, an odd one only c > a; the vertex
 *   takes the admissible c of the highest score if that is strictly above staying, ties to the lowest c.  The products (up to
 *   2^78) are formed in 128 bits.  Then, from the NEW labels: in = the weight inside the communities (both directions plus
 *   self-loops), tot2 = the sum of tot_c^2, Q = M in - g tot2 (modularity = Q / ((2m)^2 R)).
 *   state [24] int64        : two slots of 8 words, read at slot sweep & 1 and written at the other -- done (0 running, 1 Q did
 *                             not rise, 2 two idle sweeps in a row, 3 max_sweeps), sweeps run, best Q (low word, high word),
 *                             idle sweeps in a row, 1 if this sweep was kept -- and from word 16 two slots of 4 words with the
 *                             sweep's sums: vertices moved, in, tot2 (slot sweep & 1 holds them after the call)
 *   A sweep that moves nothing is idle: two in a row end the level.  A sweep that moves something is kept if its Q exceeds the
 *   best so far -- labels_new and tot_new are copied over labels and tot -- and is otherwise discarded, which ends the level.
 *   After the level's end every sweep is an exact no-op (nothing but the state's other slot is written), so a host may read
 *   the state every few sweeps only: the result does not depend on how often it looks.
 * dcahip_louvain_begin: labels[i] = i, ki = tot = the row sums, state = the start of a level whose best Q is that of the
 *   singletons.  dcahip_louvain_sweep: sweep number `sweep` (0, 1, ..; its parity picks the direction and the slot), four
 *   launches; labels_new [n], tot_new [n] are scratch and outputs (the labels decided, kept or not).
 * Integer atomics only, plain stores, every index formed in 64 bits; a column or label outside 0 .. n-1 is skipped, never an
 * index.  DCAHIP_EINVAL (nothing launched): n < 0, nnz or twom outside 0 .. 2^31 - 1, g outside 1 .. 65536, sweep < 0,
 * max_sweeps < 1, a missing pointer.
 */
long dcahip_graph_symmetrize_workspace_bytes(int n, int k);
int dcahip_graph_symmetrize(const int* idx, long ldi, int n, int k, long* rowptr, int* col, long cap, int* deg,
                            void* ws, int* status, void* stream);
int dcahip_louvain_begin(int n, long nnz, const long* rowptr, const int* col, const int* wt, int* ki, int* labels, int* tot,
                         long twom, int g, long* state, void* stream);
int dcahip_louvain_sweep(int n, long nnz, const long* rowptr, const int* col, const int* wt, const int* ki, int* labels,
                         int* tot, int* labels_new, int* tot_new, long twom, int g, int sweep, int max_sweeps, long* state,
                         void* stream);

/*
 * K-PEER (dca_amd/csrc/dcahip_peer.hip): the small exchanges of the data-parallel step without a library call.
 *   slots[q], flags[q]: device arrays of `world` pointers to every rank's exchange buffers (rank's own: its local
 *   allocation; the others: mapped with hipIpcOpenMemHandle), each dcahip_peer_slot_bytes(world, nmax) /
 *   dcahip_peer_flag_bytes(world) bytes, zero-initialised once, in FINE-GRAINED device memory
 *   (hipExtMallocWithFlags(hipDeviceMallocFinegrained)): a peer's stores over xGMI are not guaranteed visible to the owner's
 *   spinning loads in a coarse-grained (plain hipMalloc) allocation.  epoch: one device counter per communicator, 0 at the start,
 *   advanced by every call (all ranks call in the same order).  reduce = 0: out [world * n] = concatenation of the ranks'
 *   vectors (all-gather); reduce = 1: out [n] = their sum in rank order (all-reduce; out may be local).  A peer that does
 *   not arrive within timeout_us microseconds (100 MHz wall clock) sets *status |= 1 and `out` is filled with NaN: a missed
 *   exchange poisons the step visibly instead of feeding it stale statistics (the caller checks status at its next
 *   synchronisation).  Asynchronous on `stream`; one workgroup.  Replaces torch.distributed.all_gather_into_tensor /
 *   all_reduce on <= nmax floats (SyncBN statistics); no reference call site (the reference is single-process).
 */
long dcahip_peer_slot_bytes(int world, int nmax);
long dcahip_peer_flag_bytes(int world);
int dcahip_peer_exchange(const float* local, int n, float* const* slots, unsigned* const* flags, int rank, int world, int nmax,
                         unsigned long long* epoch, float* out, int reduce, int* status, long timeout_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCAHIP_H */
