// K-MEANS (include/dcahip.h, dcahip_kmeans_step / dcahip_kmeans_seed): Lloyd's k-means of the latent space and its k-means++
// seeding, on the device.  The distance is the one of K-NEIGHBOURS (knn_dist.hpp), so labels and distances are the bits
// dcahip_knn(Q = X, X = C, k = 1) returns.
//
// One Lloyd iteration = two launches:
//
//   kmeans_assign_kernel  256 lanes, one lane owns one point of a 256-point tile, its coordinates in registers (the shape of
//                         knn_scan_kernel).  The centres are staged zero-padded into LDS, 16 KiB at a time, and read by the
//                         whole wave at one address (a broadcast); a lane keeps the first centre of the smallest distance
//                         (strict <, centres ascending = the total order (d2, c)).  Then the tile is added to the
//                         workgroup's per-cluster sums in double: thread (g, j) owns coordinate j of accumulator copy g and
//                         takes the tile's points g, g + G, g + 2G, .. in that order, so no two threads touch one
//                         accumulator and no atomic is needed.  A workgroup takes `tpb` consecutive tiles and, at its end,
//                         adds its G copies in the order 0 .. G-1 into its partial [k][DP] of the workspace, next to its
//                         member counts (LDS integer atomics), its inertia (every lane's own sum over its tiles, then a
//                         fixed tree), its changed labels and its largest key (d2, index).
//                         Plan per shape (a pure function of n, d, k): k * DP <= 5120 keeps the accumulator copies in LDS
//                         (G = the largest power of two <= 256 / DP with G * k * DP <= 5120, at most 512 workgroups);
//                         above that (256 x 128 doubles do not fit) they live in the workgroup's own slice of the workspace
//                         (G = 256 / DP, at most 128 workgroups) -- the same code through another pointer.
//   kmeans_update_kernel  16 (cluster, coordinate) elements per workgroup, 16 threads per element: thread sl adds the partials
//                         of the workgroups sl, sl + 16, .. in that order, the 16 slices are added in order -> sums, the
//                         new centre = (float)(sum / count) (one rounding), an empty cluster keeps its centre or, the
//                         lowest-numbered one, takes the point of the largest key (re-seeding).  Every workgroup derives the
//                         counts, the lowest empty cluster and the largest key itself (k <= 256 counters); workgroup 0 also
//                         writes counts, inertia, changed, reseeded and the convergence state.
//
// Every order of addition above is a function of (n, d, k) alone: two calls on the same inputs give the same bits, and an
// iteration after convergence (no label changed, nothing re-seeded) reproduces its input centres exactly.
//
// Seeding (k-means++) is integer arithmetic after the distances: per round three launches on the stream, no host round trip --
// seed_dist_kernel (m_i = min(m_i, d2(x_i, last centre)), maximum per workgroup), seed_sum_kernel (the scale 2^e from the
// global maximum, q_i = floor(m_i 2^e), their sum per workgroup as uint64) and seed_pick_kernel (one workgroup: the Philox
// draw, T = floor(r64 S / 2^64), the first row whose inclusive prefix sum exceeds T; the row is copied to C_out).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dcahip.h"
#include "knn_dist.hpp"
#include "philox.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kMaxK = 256, kMaxD = 128, kNT = 256;
constexpr int kStage = 4096;                // floats of one staged chunk of centres (16 KiB)
constexpr int kAccLds = 5120;               // doubles of LDS accumulators (40 KiB)
constexpr int kBlocksLds = 512, kBlocksWs = 128, kSeedBlocks = 1024;


bool shape_ok(int n, int d, int k) { return n >= 0 && d >= 1 && d <= kMaxD && k >= 1 && k <= kMaxK; }

struct Plan {
    int dp, lds, G, tpb, nb;
    long ntiles;
    long o_part, o_gacc, o_inert, o_key, o_cnt, o_chg, step_bytes;      // the step's workspace
    int snb;
    long sper, o_m, o_bmax, o_bsum, seed_bytes;                          // the seeding's
};

Plan make_plan(int n, int d, int k) {
    Plan p;
    p.dp = pad_d(d);
    const long kd = (long)k * p.dp;
    p.lds = kd <= kAccLds ? 1 : 0;
    p.G = kNT / p.dp;
    if (p.lds) while (p.G > 1 && p.G * kd > kAccLds) p.G >>= 1;
    p.ntiles = ((long)n + kNT - 1) / kNT;
    const long cap = p.lds ? kBlocksLds : kBlocksWs;
    long tpb = (p.ntiles + cap - 1) / cap;
    if (tpb < 1) tpb = 1;
    p.tpb = (int)tpb;
    p.nb = (int)((p.ntiles + tpb - 1) / tpb);
    long o = 0;
    p.o_part = o;  o += r16((long)p.nb * kd * 8);
    p.o_gacc = o;  o += p.lds ? 0 : r16((long)p.nb * p.G * kd * 8);
    p.o_inert = o; o += r16((long)p.nb * 8);
    p.o_key = o;   o += r16((long)p.nb * 8);
    p.o_cnt = o;   o += r16((long)p.nb * k * 4);
    p.o_chg = o;   o += r16((long)p.nb * 4);
    p.step_bytes = o;
    long snb = p.ntiles < kSeedBlocks ? p.ntiles : kSeedBlocks;
    if (snb < 1) snb = 1;
    p.sper = ((long)n + snb - 1) / snb;
    if (p.sper < 1) p.sper = 1;
    p.snb = (int)(((long)n + p.sper - 1) / p.sper);
    if (p.snb < 1) p.snb = 1;
    o = 0;
    p.o_m = o;     o += r16((long)n * 4);
    p.o_bmax = o;  o += r16((long)p.snb * 4);
    p.o_bsum = o;  o += r16((long)p.snb * 8);
    p.seed_bytes = o;
    return p;
}

// ---------------------------------------------------------------------------------------------------------- one iteration
struct StepArgs {
    const float* X; long ldx; int n, d, k;
    const float* C; long ldc;
    int* labels; float* d2_out;
    double* part; double* gacc; double* binert; u64* bkey; int* cnt; int* bchg;
    int G, tpb; long ntiles;
    int* status;
};

template <int DP, bool LDSACC>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(StepArgs a) {
    constexpr int KC = kStage / DP;                      // centres per staged chunk
    __shared__ float cs[kStage];
    __shared__ int lab[kNT];
    __shared__ int lcnt[kMaxK];
    __shared__ double red_d[kNT];
    __shared__ u64 red_k[kNT];
    __shared__ int red_i[kNT];
    extern __shared__ double acc_lds[];
    const int t = threadIdx.x, k = a.k, d = a.d, G = a.G;
    const long kd = (long)k * DP;
    double* acc = LDSACC ? acc_lds : a.gacc + (long)blockIdx.x * G * kd;
    for (long e = t; e < G * kd; e += kNT) acc[e] = 0.0;
    lcnt[t] = 0;
    int bad = 0;
    if (blockIdx.x == 0)
        for (int e = t; e < k * d; e += kNT) bad += nonfinite(a.C[(long)(e / d) * a.ldc + e % d]);
    double isum = 0.0;
    int chg = 0;
    u64 mkey = 0;
    const long tile0 = (long)blockIdx.x * a.tpb;
    const long tile1 = tile0 + a.tpb < a.ntiles ? tile0 + a.tpb : a.ntiles;
    const int nchunks = (k + KC - 1) / KC;
    const int j = t % DP, g = t / DP;
    __syncthreads();
    for (long tile = tile0; tile < tile1; ++tile) {
        const long i = tile * kNT + t;
        const bool live = i < a.n;
        v2f qv[DP / 2];
        {
            const float* row = a.X + (live ? i : 0) * a.ldx;
#pragma unroll
            for (int u = 0; u < DP / 2; ++u) {
                qv[u].x = live && 2 * u < d ? row[2 * u] : 0.f;
                qv[u].y = live && 2 * u + 1 < d ? row[2 * u + 1] : 0.f;
                bad += nonfinite(qv[u].x) + nonfinite(qv[u].y);
            }
        }
        float best = __uint_as_float(kInfBits);
        int bl = 0;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * KC;
            const int kc = k - c0 < KC ? k - c0 : KC;
            if (nchunks > 1 || tile == tile0) {          // a single chunk stays staged for every tile
                __syncthreads();
                for (int e = t; e < kc * DP; e += kNT) {
                    const int c = e / DP, col = e % DP;
                    cs[e] = col < d ? a.C[(long)(c0 + c) * a.ldc + col] : 0.f;
                }
                __syncthreads();
            }
            if (live) {
#pragma unroll 2
                for (int c = 0; c < kc; ++c) {
                    const float d2 = dist2<DP>(qv, cs + c * DP);
                    if (d2 < best) { best = d2; bl = c0 + c; }
                }
            }
        }
        if (live) {
            chg += a.labels[i] != bl ? 1 : 0;
            a.labels[i] = bl;
            a.d2_out[i] = best;
            isum += (double)best;
            const u64 key = ((u64)__float_as_uint(best) << 32) | (unsigned)i;
            mkey = key > mkey ? key : mkey;
            atomicAdd(&lcnt[bl], 1);
        }
        lab[t] = live ? bl : -1;
        __syncthreads();
        if (g < G && j < d) {                            // G divides 64: p0 + 3 G < 256 in every trip
            double* mine = acc + (long)g * kd + j;
            for (int p0 = g; p0 < kNT; p0 += 4 * G) {
                int lv[4];
                float xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = p0 + u * G;
                    long ip = tile * kNT + p;
                    ip = ip < a.n ? ip : a.n - 1;
                    lv[u] = lab[p];
                    xv[u] = a.X[ip * a.ldx + j];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (lv[u] >= 0) mine[(long)lv[u] * DP] += (double)xv[u];
            }
        }
        __syncthreads();
    }
    if (!LDSACC) __threadfence_block();
    __syncthreads();
    double* part = a.part + (long)blockIdx.x * kd;
    for (long e = t; e < kd; e += kNT) {
        double s = acc[e];
        for (int gg = 1; gg < G; ++gg) s += acc[gg * kd + e];
        part[e] = s;
    }
    if (t < k) a.cnt[(long)blockIdx.x * k + t] = lcnt[t];
    red_d[t] = isum;
    red_k[t] = mkey;
    red_i[t] = chg;
    __syncthreads();
    for (int s = kNT / 2; s >= 1; s >>= 1) {
        if (t < s) {
            red_d[t] += red_d[t + s];
            red_k[t] = red_k[t + s] > red_k[t] ? red_k[t + s] : red_k[t];
            red_i[t] += red_i[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        a.binert[blockIdx.x] = red_d[0];
        a.bkey[blockIdx.x] = red_k[0];
        a.bchg[blockIdx.x] = red_i[0];
    }
    if (bad) atomicAdd(a.status, bad < 4096 ? bad : 4096);
}

struct UpdArgs {
    const float* X; long ldx; int n, d, k, dp, nb;
    const float* Cin; long ldc; float* Cout; long ldco;
    const double* part; const double* binert; const u64* bkey; const int* cnt; const int* bchg;
    int* counts; double* sums; long lds; double* inertia; int* changed; int* reseeded; int* state; int iter;
};

constexpr int kUE = 16;                     // (cluster, coordinate) elements per workgroup of the update: 16 slices of partials each

__global__ __launch_bounds__(256) void kmeans_update_kernel(UpdArgs a) {
    __shared__ int s_cnt[kNT];
    __shared__ int s_emp[kNT];
    __shared__ u64 s_key[kNT];
    __shared__ double s_d[kNT];
    __shared__ int s_i[kNT];
    const int t = threadIdx.x, k = a.k, d = a.d;
    // the members of every cluster: 256 / k slices of the workgroups' counts per cluster (integers: any order)
    const int cs = kNT / k;
    int cn = 0;
    if (t < cs * k)
        for (int b = t / k; b < a.nb; b += cs) cn += a.cnt[(long)b * k + t % k];
    s_i[t] = cn;
    u64 key = 0;
    for (int b = t; b < a.nb; b += kNT) key = a.bkey[b] > key ? a.bkey[b] : key;
    s_key[t] = key;
    __syncthreads();
    cn = 0;
    if (t < k)
        for (int sl = 0; sl < cs; ++sl) cn += s_i[sl * k + t];
    s_cnt[t] = cn;
    s_emp[t] = t < k && cn == 0 ? t : kNT;
    __syncthreads();
    for (int s = kNT / 2; s >= 1; s >>= 1) {
        if (t < s) {
            s_emp[t] = s_emp[t + s] < s_emp[t] ? s_emp[t + s] : s_emp[t];
            s_key[t] = s_key[t + s] > s_key[t] ? s_key[t + s] : s_key[t];
        }
        __syncthreads();
    }
    const int empty = s_emp[0];
    const u64 mk = s_key[0];
    const bool reseed = empty < kNT && __uint_as_float((unsigned)(mk >> 32)) > 0.f;
    long mi = (long)(unsigned)mk;
    mi = mi < a.n ? mi : a.n - 1;
    // sums[c][j]: slice sl adds the partials of the workgroups sl, sl + 16, .. in that order, then the slices in order
    const int el = t % kUE, sl = t / kUE;
    const int e = blockIdx.x * kUE + el;
    const int c = e < k * d ? e / d : 0, col = e < k * d ? e % d : 0;
    {
        const double* p = a.part + (long)c * a.dp + col;
        const long stride = (long)k * a.dp;
        double s = 0.0;
        if (e < k * d)
            for (int b = sl; b < a.nb; b += kNT / kUE) s += p[b * stride];
        s_d[sl * kUE + el] = s;
    }
    __syncthreads();
    if (sl == 0 && e < k * d) {
        double s = s_d[el];
        for (int q = 1; q < kNT / kUE; ++q) s += s_d[q * kUE + el];
        a.sums[c * a.lds + col] = s;
        const int n_c = s_cnt[c];
        float v = n_c > 0 ? (float)(s / (double)n_c) : a.Cin[c * a.ldc + col];
        if (reseed && c == empty) v = a.X[mi * a.ldx + col];
        a.Cout[c * a.ldco + col] = v;
    }
    if (blockIdx.x == 0) {
        double is = 0.0;
        int ch = 0;
        for (int b = t; b < a.nb; b += kNT) { is += a.binert[b]; ch += a.bchg[b]; }
        __syncthreads();
        s_d[t] = is;
        s_i[t] = ch;
        __syncthreads();
        for (int s = kNT / 2; s >= 1; s >>= 1) {
            if (t < s) { s_d[t] += s_d[t + s]; s_i[t] += s_i[t + s]; }
            __syncthreads();
        }
        if (t < k) a.counts[t] = s_cnt[t];
        if (t == 0) {
            *a.inertia = s_d[0];
            *a.changed = s_i[0];
            *a.reseeded = reseed ? 1 : 0;
            if (*a.state == 0 && s_i[0] == 0 && !reseed) *a.state = a.iter;
        }
    }
}

template <int DP>
int launch_assign(const StepArgs& a, const Plan& p, hipStream_t s) {
    if (p.lds)
        hipLaunchKernelGGL((kmeans_assign_kernel<DP, true>), dim3(p.nb), dim3(kNT), (size_t)p.G * a.k * DP * 8, s, a);
    else
        hipLaunchKernelGGL((kmeans_assign_kernel<DP, false>), dim3(p.nb), dim3(kNT), 0, s, a);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- seeding
struct SeedArgs {
    const float* X; long ldx; int n, d, k;
    float* m; unsigned* bmax; u64* bsum; int nb; long per;
    int* rows; float* Cout; long ldc;
    unsigned k0, k1, init;
    int* status;
    int t;                                               // the round
};

// the largest of v[0 .. n) (a workgroup of 256; every thread gets it)
__device__ __forceinline__ unsigned block_max(const unsigned* v, int n, unsigned* red) {
    const int t = threadIdx.x;
    unsigned m = 0;
    for (int b = t; b < n; b += kNT) m = v[b] > m ? v[b] : m;
    red[t] = m;
    __syncthreads();
    for (int s = kNT / 2; s >= 1; s >>= 1) {
        if (t < s) red[t] = red[t + s] > red[t] ? red[t + s] : red[t];
        __syncthreads();
    }
    m = red[0];
    __syncthreads();
    return m;
}

// 2^e with M 2^e in [2^30, 2^31) for the fp32 M > 0 of these bits (denormals included), as a double
__device__ __forceinline__ double seed_scale(unsigned mbits) {
    const u64 b = (u64)__double_as_longlong((double)__uint_as_float(mbits));
    const int ex = (int)((b >> 52) & 0x7FF) - 1023;      // floor(log2 M)
    return __longlong_as_double((long long)((u64)(30 - ex + 1023) << 52));
}

// floor(m 2^e): a power-of-two scale in double and a truncation, exact; below 2^31 for every finite m <= M
__device__ __forceinline__ u64 seed_weight(float m, double scale) {
    return __float_as_uint(m) < kInfBits ? (u64)((double)m * scale) : 0;
}

template <int DP>
__global__ __launch_bounds__(256) void seed_dist_kernel(SeedArgs a) {
    __shared__ float crow[DP];
    __shared__ unsigned red[kNT];
    const int t = threadIdx.x, d = a.d;
    const long lo = (long)blockIdx.x * a.per;
    const long hi = lo + a.per < a.n ? lo + a.per : a.n;
    if (a.t == 0) {                                      // before the first round: m = +inf, the input is checked once
        int bad = 0;
        for (long i = lo + t; i < hi; i += kNT) {
            for (int c = 0; c < d; ++c) bad += nonfinite(a.X[i * a.ldx + c]);
            a.m[i] = __uint_as_float(kInfBits);
        }
        if (bad) atomicAdd(a.status, bad < 4096 ? bad : 4096);
        return;
    }
    long row = a.rows[a.t - 1];
    row = row < 0 ? 0 : row < a.n ? row : a.n - 1;
    if (t < DP) crow[t] = t < d ? a.X[row * a.ldx + t] : 0.f;
    __syncthreads();
    unsigned mx = 0;
    for (long i = lo + t; i < hi; i += kNT) {
        v2f qv[DP / 2];
        const float* x = a.X + i * a.ldx;
#pragma unroll
        for (int u = 0; u < DP / 2; ++u) {
            qv[u].x = 2 * u < d ? x[2 * u] : 0.f;
            qv[u].y = 2 * u + 1 < d ? x[2 * u + 1] : 0.f;
        }
        const float d2 = dist2<DP>(qv, crow);
        const float old = a.m[i];
        const float mi = d2 < old ? d2 : old;
        a.m[i] = mi;
        mx = __float_as_uint(mi) > mx ? __float_as_uint(mi) : mx;
    }
    red[t] = mx;
    __syncthreads();
    for (int s = kNT / 2; s >= 1; s >>= 1) {
        if (t < s) red[t] = red[t + s] > red[t] ? red[t + s] : red[t];
        __syncthreads();
    }
    if (t == 0) a.bmax[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void seed_sum_kernel(SeedArgs a) {
    __shared__ unsigned red[kNT];
    __shared__ u64 red_s[kNT];
    const int t = threadIdx.x;
    const unsigned M = block_max(a.bmax, a.nb, red);
    const long lo = (long)blockIdx.x * a.per;
    const long hi = lo + a.per < a.n ? lo + a.per : a.n;
    u64 s = 0;
    if (M != 0) {
        const double scale = seed_scale(M);
        for (long i = lo + t; i < hi; i += kNT) s += seed_weight(a.m[i], scale);
    }
    red_s[t] = s;
    __syncthreads();
    for (int w = kNT / 2; w >= 1; w >>= 1) {
        if (t < w) red_s[t] += red_s[t + w];
        __syncthreads();
    }
    if (t == 0) a.bsum[blockIdx.x] = red_s[0];
}

__global__ __launch_bounds__(256) void seed_pick_kernel(SeedArgs a) {
    __shared__ unsigned red[kNT];
    __shared__ u64 sub[kNT];
    __shared__ u64 s_T, s_base;
    __shared__ long s_row;
    __shared__ int s_blk, s_w;
    const int t = threadIdx.x;
    const unsigned M = a.t == 0 ? 0u : block_max(a.bmax, a.nb, red);
    if (t == 0) {
        unsigned o[4];
        philox4x32_10((unsigned)a.t, a.init, 0u, kPhiloxSeedTag, a.k0, a.k1, o);
        const u64 r64 = ((u64)o[1] << 32) | o[0];
        s_row = -1;
        s_blk = -1;
        s_w = -1;
        if (M == 0) {
            s_row = (long)__umul64hi(r64, (u64)a.n);
        } else {
            u64 S = 0;
            for (int b = 0; b < a.nb; ++b) S += a.bsum[b];
            const u64 T = __umul64hi(r64, S);
            u64 pre = 0;
            for (int b = 0; b < a.nb; ++b) {
                if (pre + a.bsum[b] > T) { s_blk = b; break; }
                pre += a.bsum[b];
            }
            s_T = T;
            s_base = pre;
            if (s_blk < 0) s_row = a.n - 1;              // not reached for finite input (T < S)
        }
    }
    __syncthreads();
    if (s_blk >= 0) {                                    // the same for every thread
        const double scale = seed_scale(M);
        const long lo = (long)s_blk * a.per;
        const long hi = lo + a.per < a.n ? lo + a.per : a.n;
        const long len = (hi - lo + kNT - 1) / kNT;
        const long c0 = lo + t * len < hi ? lo + t * len : hi;
        const long c1 = c0 + len < hi ? c0 + len : hi;
        u64 s = 0;
        for (long i = c0; i < c1; ++i) s += seed_weight(a.m[i], scale);
        sub[t] = s;
        __syncthreads();
        if (t == 0) {
            u64 pre = s_base;
            for (int w = 0; w < kNT; ++w) {
                if (pre + sub[w] > s_T) { s_w = w; break; }
                pre += sub[w];
            }
            s_base = pre;
            if (s_w < 0) s_row = a.n - 1;
        }
        __syncthreads();
        if (t == s_w) {
            u64 pre = s_base;
            long r = c1 - 1;
            for (long i = c0; i < c1; ++i) {
                pre += seed_weight(a.m[i], scale);
                if (pre > s_T) { r = i; break; }
            }
            s_row = r;
        }
        __syncthreads();
    }
    long row = s_row;
    row = row < 0 ? 0 : row < a.n ? row : a.n - 1;
    if (t == 0) a.rows[a.t] = (int)row;
    for (int c = t; c < a.d; c += kNT) a.Cout[(long)a.t * a.ldc + c] = a.X[row * a.ldx + c];
}

}  // namespace

extern "C" {

long dcahip_kmeans_workspace_bytes(int n, int d, int k) {
    if (!shape_ok(n, d, k)) return DCAHIP_EINVAL;
    const Plan p = make_plan(n, d, k);
    return p.step_bytes > p.seed_bytes ? p.step_bytes : p.seed_bytes;
}

int dcahip_kmeans_step(const float* X, long ldx, int n, int d, int k, const float* C_in, long ldc, float* C_out, long ldco,
                       int* labels, float* d2_out, int* counts, double* sums, long lds, double* inertia,
                       int* changed, int* reseeded, int* state, int iter, void* ws, int* status, void* stream) {
    if (!shape_ok(n, d, k) || ldx < d || ldc < d || ldco < d || lds < d || iter < 1) return DCAHIP_EINVAL;
    if (n == 0) return 0;
    if (!X || !C_in || !C_out || !labels || !d2_out || !counts || !sums || !inertia || !changed || !reseeded || !state ||
        !ws || !status)
        return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Plan p = make_plan(n, d, k);
    char* w = (char*)ws;
    StepArgs a;
    a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.k = k;
    a.C = C_in; a.ldc = ldc;
    a.labels = labels; a.d2_out = d2_out;
    a.part = (double*)(w + p.o_part); a.gacc = (double*)(w + p.o_gacc); a.binert = (double*)(w + p.o_inert);
    a.bkey = (u64*)(w + p.o_key); a.cnt = (int*)(w + p.o_cnt); a.bchg = (int*)(w + p.o_chg);
    a.G = p.G; a.tpb = p.tpb; a.ntiles = p.ntiles;
    a.status = status;
    int rc;
    switch (p.dp) {
    case 8: rc = launch_assign<8>(a, p, s); break;
    case 16: rc = launch_assign<16>(a, p, s); break;
    case 32: rc = launch_assign<32>(a, p, s); break;
    case 64: rc = launch_assign<64>(a, p, s); break;
    default: rc = launch_assign<128>(a, p, s); break;
    }
    if (rc) return rc;
    UpdArgs u;
    u.X = X; u.ldx = ldx; u.n = n; u.d = d; u.k = k; u.dp = p.dp; u.nb = p.nb;
    u.Cin = C_in; u.ldc = ldc; u.Cout = C_out; u.ldco = ldco;
    u.part = a.part; u.binert = a.binert; u.bkey = a.bkey; u.cnt = a.cnt; u.bchg = a.bchg;
    u.counts = counts; u.sums = sums; u.lds = lds; u.inertia = inertia; u.changed = changed; u.reseeded = reseeded;
    u.state = state; u.iter = iter;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((k * d + kUE - 1) / kUE)), dim3(kNT), 0, s, u);
    return (int)hipGetLastError();
}

int dcahip_kmeans_seed(const float* X, long ldx, int n, int d, int k, unsigned long long seed, int init,
                       int* rows_out, float* C_out, long ldc, void* ws, int* status, void* stream) {
    if (!shape_ok(n, d, k) || ldx < d || ldc < d || init < 0) return DCAHIP_EINVAL;
    if (n == 0) return 0;
    if (!X || !rows_out || !C_out || !ws || !status) return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const Plan p = make_plan(n, d, k);
    char* w = (char*)ws;
    SeedArgs a;
    a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.k = k;
    a.m = (float*)(w + p.o_m); a.bmax = (unsigned*)(w + p.o_bmax); a.bsum = (u64*)(w + p.o_bsum);
    a.nb = p.snb; a.per = p.sper;
    a.rows = rows_out; a.Cout = C_out; a.ldc = ldc;
    a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32); a.init = (unsigned)init;
    a.status = status;
    for (int t = 0; t < k; ++t) {
        a.t = t;
        switch (p.dp) {
        case 8: hipLaunchKernelGGL(seed_dist_kernel<8>, dim3(p.snb), dim3(kNT), 0, s, a); break;
        case 16: hipLaunchKernelGGL(seed_dist_kernel<16>, dim3(p.snb), dim3(kNT), 0, s, a); break;
        case 32: hipLaunchKernelGGL(seed_dist_kernel<32>, dim3(p.snb), dim3(kNT), 0, s, a); break;
        case 64: hipLaunchKernelGGL(seed_dist_kernel<64>, dim3(p.snb), dim3(kNT), 0, s, a); break;
        default: hipLaunchKernelGGL(seed_dist_kernel<128>, dim3(p.snb), dim3(kNT), 0, s, a); break;
        }
        if (t > 0) hipLaunchKernelGGL(seed_sum_kernel, dim3(p.snb), dim3(kNT), 0, s, a);
        hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(kNT), 0, s, a);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
