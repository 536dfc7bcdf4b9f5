// The passes over a fitted model: inference heads (dcahip_zinb_heads_infer), K-SCORE (dcahip_nll_marginals: per-cell and
// per-gene sums of the element-wise NLL) and K-GROUPS (dcahip_group_moments: per-group moments of the denoised expression).
// gfx950 (MI355X), wave64.  Once per dataset, not per training step: readable kernels, both branches of the likelihood under
// divergence.  Each lane owns one 16-byte quad of consecutive genes where the operands allow it (V = 4), one gene otherwise.
//
// Reference arithmetic restated here: dca/network.py:38-39 (MeanAct, DispAct), and through zinb_math.hpp dca/loss.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include "dcahip.h"
#include "zinb_math.hpp"
#include "nll_shared.hpp"

namespace {

struct InferArgs {
    const float *a_mean, *a_disp, *a_pi, *sf;
    float *mean_sf, *theta, *pi;
    long lda, ldo;
    int B, G;
    int linear_mean;
};

// clip_by_value as comparisons: a NaN stays a NaN, as in the reference (fminf / fmaxf return their other argument)
__device__ __forceinline__ float clip_keep_nan(float x, float lo, float hi) {
    return x < lo ? lo : (x > hi ? hi : x);
}

// the mean head's activation (dca/network.py:38 MeanAct; the linear mean of ae_type 'normal'): the one expression
// heads_infer_kernel stores and group_moments_kernel sums
__device__ __forceinline__ float mean_act(float a, bool linear) {
    return linear ? a : clip_keep_nan(expf(a), 1e-5f, 1e6f);
}

template <int V>
__global__ __launch_bounds__(256) void heads_infer_kernel(InferArgs a) {
    const int nvec = (a.G + V - 1) / V;
    const int nseg = (nvec + 255) >> 8;
    const long total = (long)a.B * nseg;
    for (long item = blockIdx.x; item < total; item += gridDim.x) {
        const int row = (int)(item / nseg);
        const int q = (int)(item - (long)row * nseg) * 256 + threadIdx.x;
        if (q >= nvec) continue;
        const int g = q * V;
        const float sf = a.sf[row];
        const long ao = (long)row * a.lda + g, oo = (long)row * a.ldo + g;
        float v[V], o[V];
        if (a.mean_sf) {
            ldv<V>(a.a_mean + ao, v);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = mean_act(v[j], a.linear_mean) * sf;
            stv<V>(a.mean_sf + oo, o);
        }
        if (a.theta) {
            ldv<V>(a.a_disp + ao, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float sp = fmaxf(v[j], 0.f) + log1pf(expf(-fabsf(v[j])));
                o[j] = clip_keep_nan(sp, 1e-4f, 1e4f);
            }
            stv<V>(a.theta + oo, o);
        }
        if (a.pi) {
            ldv<V>(a.a_pi + ao, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float ex = expf(-fabsf(v[j]));
                const float s = 1.f / (1.f + ex);
                o[j] = v[j] >= 0.f ? s : ex * s;
            }
            stv<V>(a.pi + oo, o);
        }
    }
}

// ---- K-SCORE: the two marginals of the element-wise NLL of a fitted model (dcahip_nll_marginals): per-row sums and
// per-gene sums over consecutive rows, every element value accumulated in double.  The grid of zinb_nll_kernel
// (dcahip_zinb.hip): blockIdx.x walks the gene segments (256 lanes x V genes), blockIdx.y = slice strides over the rows.
//   * per gene: every lane keeps the V column sums of its quad over the rows of its slice and stores them to
//     gene_part[slice][g] -- no reduction in the kernel;
//   * per row: every wave adds up its 64 x V genes with shuffles and stores to row_part[segment * 4 + wave][row] -- no
//     barrier in the row loop.
// nll_finish_kernel adds the slices / the segment partials in index order.  Every workspace word it reads is written by
// exactly one lane on every call and no sum depends on scheduling (no atomics): two calls give the same bits.
// One readable kernel, both branches of the likelihood under divergence: scoring is a pass per dataset, not per step.
constexpr int kScoreSlices = 64;

struct MargArgs {
    const float *a_mean, *a_disp, *a_pi, *theta_w, *y, *sf;
    long lda, ldy;
    double *gene_part, *row_part;
    int B, G;
    float ridge;
};

template <bool HAS_PI, bool CONST_DISP, int V, int LOSS>
__global__ __launch_bounds__(256) void nll_marginals_kernel(MargArgs a) {
    const int nvec = (a.G + V - 1) / V;
    const int seg = blockIdx.x, wave = threadIdx.x >> 6;
    const int q = seg * 256 + threadIdx.x;
    const bool qv = q < nvec;
    const int g = (qv ? q : 0) * V;
    bool valid[V];
#pragma unroll
    for (int j = 0; j < V; ++j) valid[j] = qv && (g + j) < a.G;
    float vd[V];
#pragma unroll
    for (int j = 0; j < V; ++j) vd[j] = 0.f;
    if (CONST_DISP && qv) ldv<V>(a.theta_w + g, vd);
    double col[V];
#pragma unroll
    for (int j = 0; j < V; ++j) col[j] = 0.0;
    double* rp = a.row_part + (long)(seg * 4 + wave) * a.B;
    const bool wave_live = seg * 256 + wave * 64 < nvec;         // a wave past the last quad only zeroes its partials
    for (int row = blockIdx.y; row < a.B; row += gridDim.y) {
        if (!wave_live) {
            if ((threadIdx.x & 63) == 0) rp[row] = 0.0;
            continue;
        }
        const float sf = a.sf[row];
        float vm[V], vp[V], vy[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { vm[j] = 0.f; vp[j] = 0.f; vy[j] = 0.f; }
        if (qv) {
            const long ao = (long)row * a.lda + g;
            ldv<V>(a.a_mean + ao, vm);
            if (!CONST_DISP && LOSS == 0) ldv<V>(a.a_disp + ao, vd);
            if (HAS_PI) ldv<V>(a.a_pi + ao, vp);
            ldv<V>(a.y + (long)row * a.ldy + g, vy);
        }
        double racc = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            // the padding of a ragged last quad (columns G .. roundup4(G) - 1) holds anything: evaluated on zeros, not added
            const float am = valid[j] ? vm[j] : 0.f, ad = valid[j] ? vd[j] : 0.f, ap = valid[j] ? vp[j] : 0.f;
            const float y = valid[j] ? vy[j] : 0.f;
            float nll, d0 = 0.f, d1 = 0.f, d2 = 0.f;
            if (LOSS == 1) nll = poisson_elem(am, sf, y, d0);
            else if (LOSS == 2) nll = mse_elem(am, sf, y, d0);
            else nll = nll_elem<HAS_PI, false>(head_acts<HAS_PI, CONST_DISP>(am, ad, ap, sf), y, a.ridge, d0, d1, d2);
            const double v = valid[j] ? (double)nll : 0.0;
            col[j] += v;
            racc += v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) racc += __shfl_down(racc, off, 64);
        if ((threadIdx.x & 63) == 0) rp[row] = racc;
    }
    double* gp = a.gene_part + (long)blockIdx.y * a.G + g;
#pragma unroll
    for (int j = 0; j < V; ++j)
        if (valid[j]) gp[j] = col[j];
}

__global__ __launch_bounds__(256) void nll_finish_kernel(const double* __restrict__ gene_part, int S,
                                                         const double* __restrict__ row_part, int P, int B, int G,
                                                         double* __restrict__ cell_out, double* __restrict__ gene_acc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < G) {
        double s = 0.0;
        for (int k = 0; k < S; ++k) s += gene_part[(long)k * G + i];
        gene_acc[i] += s;
    } else if (i < (long)G + B) {
        const long r = i - G;
        double s = 0.0;
        for (int k = 0; k < P; ++k) s += row_part[(long)k * B + r];
        cell_out[r] = s;
    }
}

// doubles of the two partial arrays: [slices][G] and, for the scalar path's 256-gene segments (the larger count),
// [segments * 4][B]
long marginals_doubles(int B, int G) {
    const long S = B < kScoreSlices ? B : kScoreSlices;
    return S * G + (long)((G + 255) / 256) * 4 * B;
}

// ---- K-GROUPS: per-group first and second moments of the denoised expression (dcahip_group_moments): for every group
// code k and gene g the sums of x and x^2 over the rows that carry k, x = the value heads_infer_kernel stores (mean_act,
// times the row's size factor) or its log1p, every value converted to double before it is added.
//   * blockIdx.x walks the gene segments (256 lanes x V genes), blockIdx.y = group code x row slice (S slices of
//     consecutive rows: enough workgroups when segments x groups alone do not fill the chip);
//   * a workgroup takes its slice 1 024 rows at a time: all four waves compact the indices of the rows that carry its code
//     into LDS in ascending order (ballot + prefix over the wave counts), then every lane walks that list with
//     kGroupLoads independent row loads in flight and adds them up in list order;
//   * S == 1: the lane that owns (code, gene) adds its sums to the accumulators itself; S > 1: they go to
//     part[moment][slice][code][g] and group_finish_kernel adds the slices in index order.
// A row whose code is not in [0, K) matches no workgroup: it is never an index.  Every word of `part` that the finish reads is
// written by exactly one lane on every call (a slice without a row of the code writes zeros); no atomics, no sum that
// depends on scheduling: two calls give the same bits.
constexpr int kGroupTile = 1024;            // rows compacted at a time (4 passes of the 256 lanes)
constexpr int kGroupLoads = 4;              // independent row loads in flight per lane
constexpr int kGroupMaxK = 4096, kGroupMaxSlices = 64, kGroupBlocks = 1024;

struct GroupArgs {
    const float *a_mean, *sf;               // sf == nullptr: DCAHIP_GROUP_NO_SF
    const int* codes;
    long lda, ldg;
    double *sum_acc, *sumsq_acc, *part;
    int B, G, K, S, rows_per;
    int linear_mean, log1p;
};

__device__ __forceinline__ float group_value(float a, float sf, bool has_sf, bool linear, bool log1p) {
    float x = mean_act(a, linear);
    if (has_sf) x = x * sf;
    return log1p ? log1pf(x) : x;
}

template <int V>
__global__ __launch_bounds__(256) void group_moments_kernel(GroupArgs a) {
    __shared__ int list[kGroupTile];
    __shared__ int cnt[kGroupTile / 64];
    constexpr int P = kGroupTile / 256;
    const int nvec = (a.G + V - 1) / V;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool qv = q < nvec;
    const int g = (qv ? q : 0) * V;
    const int code = blockIdx.y / a.S, slice = blockIdx.y - code * a.S;
    const int r_begin = slice * a.rows_per;
    const int r_end = r_begin + a.rows_per < a.B ? r_begin + a.rows_per : a.B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_sf = a.sf != nullptr, linear = a.linear_mean != 0, lg = a.log1p != 0;
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
    bool any = false;
    for (int t0 = r_begin; t0 < r_end; t0 += kGroupTile) {
        // the rows of this tile that carry `code`, ascending: pass p looks at rows t0 + p * 256 + lane id
        bool m[P];
        unsigned long long bal[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int r = t0 + p * 256 + (int)threadIdx.x;
            m[p] = r < r_end && a.codes[r] == code;
            bal[p] = __ballot(m[p]);
            if (lane == 0) cnt[p * 4 + wave] = __popcll(bal[p]);
        }
        __syncthreads();
        int n = 0, base[P];
#pragma unroll
        for (int i = 0; i < P * 4; ++i) {
            if ((i & 3) == wave) base[i >> 2] = n;
            n += cnt[i];
        }
#pragma unroll
        for (int p = 0; p < P; ++p)
            if (m[p]) list[base[p] + __popcll(bal[p] & ((1ull << lane) - 1ull))] = t0 + p * 256 + (int)threadIdx.x;
        __syncthreads();
        any = any || n > 0;
        if (qv) {
            int i = 0;
            for (; i + kGroupLoads <= n; i += kGroupLoads) {
                float v[kGroupLoads][V], f[kGroupLoads];
#pragma unroll
                for (int u = 0; u < kGroupLoads; ++u) {
                    const int row = __builtin_amdgcn_readfirstlane(list[i + u]);
                    ldv<V>(a.a_mean + (long)row * a.lda + g, v[u]);
                    f[u] = has_sf ? a.sf[row] : 1.f;
                }
#pragma unroll
                for (int u = 0; u < kGroupLoads; ++u)
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const double x = (double)group_value(v[u][j], f[u], has_sf, linear, lg);
                        s1[j] += x;
                        s2[j] += x * x;
                    }
            }
            for (; i < n; ++i) {
                const int row = __builtin_amdgcn_readfirstlane(list[i]);
                float v[V];
                ldv<V>(a.a_mean + (long)row * a.lda + g, v);
                const float f = has_sf ? a.sf[row] : 1.f;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double x = (double)group_value(v[j], f, has_sf, linear, lg);
                    s1[j] += x;
                    s2[j] += x * x;
                }
            }
        }
        // no barrier here: the next tile's cnt writes come after this tile's cnt reads (the barrier above), its list writes
        // after its own first barrier, which no wave passes before every wave has finished this walk
    }
    if (!qv) return;
    // columns G .. roundup4(G) - 1 of a ragged last quad were summed in registers only
    if (a.S == 1) {
        if (!any) return;
        double* o1 = a.sum_acc + (long)code * a.ldg + g;
        double* o2 = a.sumsq_acc + (long)code * a.ldg + g;
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (g + j < a.G) { o1[j] += s1[j]; o2[j] += s2[j]; }
    } else {
        const long skg = (long)a.S * a.K * a.G;
        double* o = a.part + ((long)slice * a.K + code) * a.G + g;
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (g + j < a.G) { o[j] = s1[j]; o[skg + j] = s2[j]; }
    }
}

__global__ __launch_bounds__(256) void group_finish_kernel(const double* __restrict__ part, int S, int K, int G, long ldg,
                                                           double* __restrict__ sum_acc, double* __restrict__ sumsq_acc) {
    const long kg = (long)K * G;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= kg) return;
    const long code = i / G, g = i - code * G;
    double t1 = 0.0, t2 = 0.0;
    for (int s = 0; s < S; ++s) {
        t1 += part[(long)s * kg + i];
        t2 += part[(long)(S + s) * kg + i];
    }
    sum_acc[code * ldg + g] += t1;
    sumsq_acc[code * ldg + g] += t2;
}

// most row slices of K-GROUPS for V genes per lane: about kGroupBlocks workgroups, at most one slice per row.  Non-decreasing
// in B and non-increasing in V
long group_slice_cap(int B, int G, int K, int V) {
    const long nseg = ((G + V - 1) / V + 255) / 256;
    long s = (kGroupBlocks + nseg * K - 1) / (nseg * K);
    if (s > kGroupMaxSlices) s = kGroupMaxSlices;
    if (s > B) s = B;
    return s < 1 ? 1 : s;
}

// the slices a call uses: rows_per = ceil(B / cap) consecutive rows each, S = ceil(B / rows_per) <= cap of them (no empty one)
int group_slices(int B, int G, int K, int V, int* rows_per) {
    const long s = group_slice_cap(B, G, K, V);
    *rows_per = (int)((B + s - 1) / s);
    return (B + *rows_per - 1) / *rows_per;
}

// doubles of part, an upper bound that is non-decreasing in B (a workspace sized for a chunk serves every shorter chunk): the
// cap of the 16-byte path, which has the fewest segments and so the most slices
long group_doubles(int B, int G, int K) {
    const long S = group_slice_cap(B, G, K, 4);
    return S > 1 ? 2 * S * K * G : 1;
}

template <bool HAS_PI, bool CONST_DISP, int LOSS>
void launch_marginals(const MargArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((nll_marginals_kernel<HAS_PI, CONST_DISP, 4, LOSS>), grid, dim3(256), 0, s, a);
    else     hipLaunchKernelGGL((nll_marginals_kernel<HAS_PI, CONST_DISP, 1, LOSS>), grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" int dcahip_zinb_heads_infer(const float* a_mean, const float* a_disp, const float* a_pi,
                                       long lda, const float* sf, int B, int G, float* mean_sf,
                                       float* theta, float* pi, long ldo, int flags, void* stream) {
    if (B <= 0 || G <= 0 || !sf) return DCAHIP_EINVAL;
    if ((mean_sf && !a_mean) || (theta && !a_disp) || (pi && !a_pi)) return DCAHIP_EINVAL;
    const int Gp = (G + 3) & ~3;
    bool vec = (lda % 4 == 0) && (ldo % 4 == 0) && lda >= Gp && ldo >= Gp;
    const void* ps[6] = {a_mean, a_disp, a_pi, mean_sf, theta, pi};
    for (const void* p : ps) vec = vec && (p == nullptr || al16(p));
    InferArgs a{a_mean, a_disp, a_pi, sf, mean_sf, theta, pi, lda, ldo, B, G, (flags & DCAHIP_NLL_MSE) ? 1 : 0};
    const int V = vec ? 4 : 1;
    const long total = (long)B * (((G + V - 1) / V + 255) / 256);
    const int grid = (int)(total < 4096 ? total : 4096);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(heads_infer_kernel<4>, dim3(grid), dim3(256), 0, s, a);
    else     hipLaunchKernelGGL(heads_infer_kernel<1>, dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" int dcahip_nll_marginals_workspace_doubles(int B, int G) {
    if (B <= 0 || G <= 0) return 0;
    const long n = marginals_doubles(B, G);
    return n > 0x7fffffffL ? DCAHIP_EINVAL : (int)n;
}

extern "C" int dcahip_nll_marginals(const float* a_mean, const float* a_disp, const float* a_pi, long lda,
                                    const float* theta_w, const float* y, long ldy, const float* sf,
                                    int B, int G, float ridge, int flags,
                                    double* cell_out, double* gene_acc, double* workspace, void* stream) {
    const bool has_pi = flags & DCAHIP_NLL_HAS_PI, cdisp = flags & DCAHIP_NLL_CONST_DISP;
    const int loss = (flags & DCAHIP_NLL_POISSON) ? 1 : ((flags & DCAHIP_NLL_MSE) ? 2 : 0);
    if (B <= 0 || G <= 0 || !a_mean || !y || !sf || !cell_out || !gene_acc || !workspace) return DCAHIP_EINVAL;
    if (loss != 0 && (has_pi || cdisp)) return DCAHIP_EINVAL;
    if (has_pi && !a_pi) return DCAHIP_EINVAL;
    if (loss == 0 && (cdisp ? (theta_w == nullptr) : (a_disp == nullptr))) return DCAHIP_EINVAL;
    if (lda < G || ldy < G || marginals_doubles(B, G) > 0x7fffffffL) return DCAHIP_EINVAL;
    const bool vec = nll_reads_vec(a_mean, a_disp, a_pi, lda, theta_w, y, ldy, G, has_pi, cdisp, loss);
    const int V = vec ? 4 : 1;
    const int nseg = ((G + V - 1) / V + 255) / 256;
    const int S = B < kScoreSlices ? B : kScoreSlices;
    MargArgs a{a_mean, a_disp, a_pi, theta_w, y, sf, lda, ldy, workspace, workspace + (long)S * G, B, G, ridge};
    const dim3 grid(nseg, S);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (loss == 1) launch_marginals<false, false, 1>(a, vec, grid, s);
    else if (loss == 2) launch_marginals<false, false, 2>(a, vec, grid, s);
    else dispatch_pc(has_pi, cdisp, [&](auto P, auto C) { launch_marginals<P.value, C.value, 0>(a, vec, grid, s); });
    const long items = (long)G + B;
    hipLaunchKernelGGL(nll_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                       a.gene_part, S, a.row_part, nseg * 4, B, G, cell_out, gene_acc);
    return (int)hipGetLastError();
}

extern "C" int dcahip_group_moments_workspace_doubles(int B, int G, int K) {
    if (B <= 0 || G <= 0 || K <= 0) return 0;
    if (K > kGroupMaxK) return DCAHIP_EINVAL;
    const long n = group_doubles(B, G, K);
    return n > 0x7fffffffL ? DCAHIP_EINVAL : (int)n;
}

extern "C" int dcahip_group_moments(const float* a_mean, long lda, const float* sf, const int* codes,
                                    int B, int G, int K, int flags,
                                    double* sum_acc, double* sumsq_acc, long ldg,
                                    double* workspace, void* stream) {
    const bool no_sf = flags & DCAHIP_GROUP_NO_SF, lg = flags & DCAHIP_GROUP_LOG1P, linear = flags & DCAHIP_NLL_MSE;
    if (B <= 0 || G <= 0 || K <= 0 || K > kGroupMaxK) return DCAHIP_EINVAL;
    if (!a_mean || !codes || !sum_acc || !sumsq_acc || !workspace || (!no_sf && !sf)) return DCAHIP_EINVAL;
    if (lda < G || ldg < G || (linear && lg) || group_doubles(B, G, K) > 0x7fffffffL) return DCAHIP_EINVAL;
    const bool vec = (lda % 4 == 0) && al16(a_mean);          // lda % 4 == 0 and lda >= G: lda >= roundup4(G)
    const int V = vec ? 4 : 1;
    const int nseg = ((G + V - 1) / V + 255) / 256;
    int rows_per = 0;
    const int S = group_slices(B, G, K, V, &rows_per);
    GroupArgs a{a_mean, no_sf ? nullptr : sf, codes, lda, ldg, sum_acc, sumsq_acc, workspace,
                B, G, K, S, rows_per, linear ? 1 : 0, lg ? 1 : 0};
    const dim3 grid(nseg, K * S);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(group_moments_kernel<4>, grid, dim3(256), 0, s, a);
    else     hipLaunchKernelGGL(group_moments_kernel<1>, grid, dim3(256), 0, s, a);
    if (S > 1) {
        const long items = (long)K * G;
        hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                           workspace, S, K, G, ldg, sum_acc, sumsq_acc);
    }
    return (int)hipGetLastError();
}
