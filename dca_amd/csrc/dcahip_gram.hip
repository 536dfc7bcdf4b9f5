// K-GRAM: centred cross-products of selected gene columns of an fp32 plane, in double (dcahip_gram, include/dcahip.h) --
// what a gene-gene correlation of the denoised expression starts from, without the cells x genes matrix leaving the
// device.  With d[r][j] = (double)x[r][cols[j]] - shift[j] over the kept rows:
//     cross[i][j] += sum_r d[r][i] d[r][j]  (the full G x G square),   dsum[j] += sum_r d[r][j].
// A SYRK, not a GEMM: only the 64 x 64 tiles with tile_i <= tile_j are computed and the value that is added at [i][j] is
// added at [j][i] too (the same double), so an accumulator that was symmetric stays symmetric bit for bit.
//
// Launch plan (a pure function of (B, G); tests/_gram_ref.py restates it):
//   T = ceil(G / 64) tile columns, Gp = 64 T, NT = T (T + 1) / 2 tiles of the upper triangle;
//   capmax = 1 when NT >= 1024 (the triangle alone fills the chip: 256 CUs x 4 workgroups), else min(64, 1024 / NT
//   rounded to the nearest integer: more than one slice up to 682 tiles; rounding down, one slice from 513 tiles on, was
//   measured 7 % slower at 528 tiles, where 16 CUs then hold three workgroups of 4 096 rows and the others two);
//   part(c) = c > 1 ? c (NT 4096 + T 64) doubles : 0, the slices' partial tiles;
//   rows_max = (64 MiB - 8 part(capmax)) / (4 Gp) rounded down to a multiple of 32: the rows whose gathered columns fit
//   beside the partial tiles;
//   with cols the B rows go in n = ceil(B / rows_max) row blocks of ceil(B / n) rounded up to a multiple of 32 rows, one
//   after the other on the stream (cols == NULL: one block of B rows, read in place); per row block of b rows:
//     gram_gather_kernel copies the selected columns into a compact fp32 image [b][Gp] (zeros behind gene G), so that the
//     scattered reads happen once and not once per tile column;
//     cap = min(capmax, ceil(b / 32)), rows_per = ceil(b / cap) rounded up to a multiple of 32, S = ceil(b / rows_per) row
//     slices; gram_kernel on grid (NT, S), 256 lanes; blockIdx.x -> (ti, tj) row by row of the triangle: (0,0) (0,1) ..
//     (0,T-1) (1,1) ..; with S > 1 gram_finish_kernel behind it;
//   workspace (query): with bq = min(B rounded up to 32, rows_max): part(min(capmax, bq / 32)) + bq Gp / 2 doubles --
//   an upper bound of every row block's need that does not decrease with B; capmax NT <= 1024 + NT / 2 < 1536 tiles of
//   32 KiB, and rows_max takes what is left of 64 MiB.
// One workgroup: its slice 32 rows at a time.  Wave w stages rows r0 + w, r0 + w + 4, .. (lane = gene of the tile: the 64
// genes of the i side and, off the diagonal, of the j side; the next 32 rows are requested before the products of the
// current ones), converted to double, shifted, 0.0 for a masked row, a row past the slice or a gene >= G, into LDS as
// [row][gene] (row stride 80 doubles: the four rows one operand read touches fall on different banks).  Each wave owns a
// 32 x 32 quarter of the tile as 2 x 2 products of v_mfma_f64_16x16x4_f64; both operands have the index form [k = lane >> 4]
// [gene = lane & 15], so both are read from that one layout; rows ascend with k and k-steps follow each other: the order
// of the sum is fixed.  The result layout of the f64 instruction is col = lane & 15, row = (lane >> 4) + 4 reg (NOT the
// f32 one).  On a diagonal tile only i <= j is used (the lower-left wave computes nothing) and dsum is taken in the
// staging pass (per lane the rows of its wave in ascending order, then the four waves in index order).
//   * S == 1: the lane that owns (i, j) adds its sum to cross[i][j] and to cross[j][i] itself;
//   * S > 1: the tile goes to part[slice][tile][64][64] (dsum: [slice][ti][64] behind it), every word on every call, and
//     gram_finish_kernel adds the slices in index order, then once onto the accumulators.
// No atomics, no sum that depends on scheduling: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "dcahip.h"

namespace {

constexpr int kGramTile = 64, kGramDepth = 32, kGramLd = 80;
constexpr int kGramBlocks = 1024, kGramMaxSlices = 64, kGramMaxG = 8192;
constexpr long kGramWsBytes = 64L << 20;
constexpr int kGramRowsPerLane = kGramDepth / 4;        // rows one lane stages per side and step

typedef double gram_d4 __attribute__((ext_vector_type(4)));

struct GramArgs {
    const float* x;                         // the plane itself (no cols) or the gathered image: gene j is column j
    const int* keep;                        // nullptr: every row
    const double* shift;
    long ldx, ldc;
    double *cross, *dsum, *part;
    int B, G, T, NT, S, rows_per;
};

inline int gram_up32(int v) { return (v + kGramDepth - 1) / kGramDepth * kGramDepth; }

// what depends on G alone
struct GramShape {
    int T, NT, capmax, rows_max;
    long part(int c) const { return c > 1 ? (long)c * ((long)NT * 4096 + (long)T * kGramTile) : 0; }
};

GramShape gram_shape(int G) {
    GramShape g;
    g.T = (G + kGramTile - 1) / kGramTile;
    g.NT = g.T * (g.T + 1) / 2;
    g.capmax = g.NT >= kGramBlocks ? 1 : (kGramBlocks + g.NT / 2) / g.NT;
    if (g.capmax > kGramMaxSlices) g.capmax = kGramMaxSlices;
    g.rows_max = (int)((kGramWsBytes - 8 * g.part(g.capmax)) / (4L * g.T * kGramTile)) / kGramDepth * kGramDepth;
    return g;
}

// the slices of one row block of b >= 1 rows
struct GramPlan {
    int cap, S, rows_per;
};

GramPlan gram_plan(const GramShape& g, int b) {
    GramPlan p;
    const int steps = (b + kGramDepth - 1) / kGramDepth;
    p.cap = g.capmax < steps ? g.capmax : steps;
    p.rows_per = gram_up32((b + p.cap - 1) / p.cap);
    p.S = (b + p.rows_per - 1) / p.rows_per;
    return p;
}

__device__ __forceinline__ void gram_tile_of(int p, int T, int& ti, int& tj) {
    ti = 0;
    while (p >= T - ti) {
        p -= T - ti;
        ++ti;
    }
    tj = ti + p;
}

template <bool KEEP>
__global__ __launch_bounds__(256, 4) void gram_kernel(GramArgs a) {         // four workgroups per CU: 128 registers, 40 KiB
    __shared__ double lds[2 * kGramDepth * kGramLd];
    int ti, tj;
    gram_tile_of(blockIdx.x, a.T, ti, tj);
    const bool diag = ti == tj;
    double* sA = lds;
    double* sB = diag ? lds : lds + kGramDepth * kGramLd;
    const int slice = blockIdx.y;
    const int r_begin = slice * a.rows_per;
    const int r_end = r_begin + a.rows_per < a.B ? r_begin + a.rows_per : a.B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int gi = ti * kGramTile + lane, gj = tj * kGramTile + lane;
    const bool vi = gi < a.G, vj = !diag && gj < a.G;
    const long ci = vi ? gi : ti * kGramTile, cj = gj < a.G ? gj : tj * kGramTile;    // a column the lane may read
    const double shi = vi ? a.shift[gi] : 0.0, shj = vj ? a.shift[gj] : 0.0;

    // every load is unconditional (a clamped row, the tile's first gene for a lane past G) and the select comes at the
    // LDS write: a branch per element would make each load wait for the one before it
    float fa[kGramRowsPerLane], fb[kGramRowsPerLane];
    int kf[kGramRowsPerLane];               // keep flag of row r0 + 4 u + wave
    auto fetch = [&](int r0) {
#pragma unroll
        for (int u = 0; u < kGramRowsPerLane; ++u) {
            const int r = r0 + 4 * u + wave;
            kf[u] = KEEP ? a.keep[r < r_end ? r : r_end - 1] : 1;
        }
#pragma unroll
        for (int u = 0; u < kGramRowsPerLane; ++u) {
            const int r = r0 + 4 * u + wave;
            fa[u] = a.x[(long)(r < r_end ? r : r_end - 1) * a.ldx + ci];
        }
        if (!diag) {
#pragma unroll
            for (int u = 0; u < kGramRowsPerLane; ++u) {
                const int r = r0 + 4 * u + wave;
                fb[u] = a.x[(long)(r < r_end ? r : r_end - 1) * a.ldx + cj];
            }
        }
    };

    gram_d4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = gram_d4{0.0, 0.0, 0.0, 0.0};
    double ds = 0.0;
    const bool idle = diag && wr > wc;      // the lower-left quarter of a diagonal tile: all i > j
    const int kq = lane >> 4, gq = lane & 15;

    if (r_begin < r_end) fetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += kGramDepth) {
        __syncthreads();                    // the products of the previous step have read their operands
#pragma unroll
        for (int u = 0; u < kGramRowsPerLane; ++u) {
            const bool k = r0 + 4 * u + wave < r_end && kf[u] != 0;
            const double da = k && vi ? (double)fa[u] - shi : 0.0;
            sA[(4 * u + wave) * kGramLd + lane] = da;
            if (diag) ds += da;
            else sB[(4 * u + wave) * kGramLd + lane] = k && vj ? (double)fb[u] - shj : 0.0;
        }
        __syncthreads();
        if (r0 + kGramDepth < r_end) fetch(r0 + kGramDepth);
        if (!idle) {
            // all eight k-steps, also behind the slice's last row: those rows were stored as zeros and add nothing
#pragma unroll
            for (int s = 0; s < kGramDepth / 4; ++s) {
                const double* pa = sA + (4 * s + kq) * kGramLd + wr * 32 + gq;
                const double* pb = sB + (4 * s + kq) * kGramLd + wc * 32 + gq;
                const double a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }

    // dsum of a diagonal tile: the four waves' partial sums in index order
    if (diag) {
        __syncthreads();
        lds[wave * kGramTile + lane] = ds;
        __syncthreads();
        if (wave == 0) {
            const double s = ((lds[lane] + lds[kGramTile + lane]) + lds[2 * kGramTile + lane]) + lds[3 * kGramTile + lane];
            if (a.S > 1) a.part[(long)a.S * a.NT * 4096 + ((long)slice * a.T + ti) * kGramTile + lane] = s;
            else if (vi) a.dsum[gi] += s;
        }
    }

    // result layout of v_mfma_f64_16x16x4_f64: register q of the lane holds row (lane >> 4) + 4 q, column lane & 15
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int li = wr * 32 + m * 16 + kq + 4 * q, lj = wc * 32 + n * 16 + gq;
                const double v = acc[m][n][q];
                if (a.S > 1) {
                    a.part[((long)slice * a.NT + blockIdx.x) * 4096 + li * kGramTile + lj] = v;
                    continue;
                }
                const int i = ti * kGramTile + li, j = tj * kGramTile + lj;
                if (i >= a.G || j >= a.G || (diag && li > lj)) continue;
                a.cross[(long)i * a.ldc + j] += v;
                if (i != j) a.cross[(long)j * a.ldc + i] += v;
            }
}

// S > 1: item (tile, li, lj) adds its slices in index order and then once onto cross[i][j] and cross[j][i]; the items
// behind them do the same for dsum
__global__ __launch_bounds__(256) void gram_finish_kernel(GramArgs a) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    const long tiles = (long)a.NT * 4096;
    if (item < tiles) {
        const int p = (int)(item >> 12), li = (int)(item >> 6) & 63, lj = (int)item & 63;
        int ti, tj;
        gram_tile_of(p, a.T, ti, tj);
        const int i = ti * kGramTile + li, j = tj * kGramTile + lj;
        if (i >= a.G || j >= a.G || (ti == tj && li > lj)) return;
        double s = 0.0;
        for (int sl = 0; sl < a.S; ++sl) s += a.part[((long)sl * a.NT + p) * 4096 + (li << 6) + lj];
        a.cross[(long)i * a.ldc + j] += s;
        if (i != j) a.cross[(long)j * a.ldc + i] += s;
        return;
    }
    const long g = item - tiles;
    if (g >= a.G) return;
    const double* dp = a.part + (long)a.S * tiles;
    double s = 0.0;
    for (int sl = 0; sl < a.S; ++sl) s += dp[(long)sl * a.T * kGramTile + g];
    a.dsum[g] += s;
}

// The selected columns of b rows as a compact image out[b][Gp] (Gp = 64 T: 16-byte aligned rows), zeros behind gene G;
// one lane per four genes.  The loads are unconditional (a clamped gene) and selected afterwards, as in gram_kernel.
__global__ __launch_bounds__(256) void gram_gather_kernel(const float* x, long ldx, const int* cols, int b, int G, int Gp,
                                                          float* out) {
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    const int quads = Gp >> 2;
    const long r = item / quads;
    if (r >= b) return;
    const int j = (int)(item - r * quads) << 2;
    const float* row = x + r * ldx;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[cols[j + e < G ? j + e : G - 1]];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = j + e < G ? v[e] : 0.f;
    *reinterpret_cast<float4*>(out + r * Gp + j) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

extern "C" long dcahip_gram_workspace_doubles(int B, int G) {
    if (G < 1 || G > kGramMaxG) return DCAHIP_EINVAL;
    if (B <= 0) return 0;
    const GramShape g = gram_shape(G);
    const int bq = gram_up32(B) < g.rows_max ? gram_up32(B) : g.rows_max;
    const int steps = bq / kGramDepth;
    return g.part(g.capmax < steps ? g.capmax : steps) + (long)bq * g.T * kGramTile / 2;
}

extern "C" int dcahip_gram(const float* x, long ldx, const int* cols, const int* keep, const double* shift,
                           int B, int G, double* cross, long ldc, double* dsum, double* ws, void* stream) {
    if (!x || !shift || !cross || !dsum || G < 1 || G > kGramMaxG || B < 0 || ldc < G || ldx < 1) return DCAHIP_EINVAL;
    if (B == 0) return 0;
    const GramShape g = gram_shape(G);
    const int Gp = g.T * kGramTile;
    const int nblk = cols ? (B + g.rows_max - 1) / g.rows_max : 1;
    const int rows_blk = cols ? gram_up32((B + nblk - 1) / nblk) : B;
    const long image = cols ? (long)rows_blk * Gp / 2 : 0;              // doubles of the gathered image, in front of the tiles
    if (!ws && (cols || gram_plan(g, rows_blk).S > 1)) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int r0 = 0; r0 < B; r0 += rows_blk) {
        const int b = B - r0 < rows_blk ? B - r0 : rows_blk;
        const GramPlan p = gram_plan(g, b);
        if (cols) {
            const long items = (long)b * (Gp >> 2);
            hipLaunchKernelGGL(gram_gather_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                               x + (long)r0 * ldx, ldx, cols, b, G, Gp, reinterpret_cast<float*>(ws));
        }
        GramArgs a{cols ? reinterpret_cast<const float*>(ws) : x, keep ? keep + r0 : nullptr, shift,
                   cols ? (long)Gp : ldx, ldc, cross, dsum, ws ? ws + image : nullptr, b, G, g.T, g.NT, p.S, p.rows_per};
        if (keep) hipLaunchKernelGGL(gram_kernel<true>, dim3(g.NT, p.S), dim3(256), 0, s, a);
        else      hipLaunchKernelGGL(gram_kernel<false>, dim3(g.NT, p.S), dim3(256), 0, s, a);
        if (p.S > 1) {
            const long items = (long)g.NT * 4096 + G;
            hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
        }
    }
    return (int)hipGetLastError();
}
