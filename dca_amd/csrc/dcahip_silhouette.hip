// K-SILHOUETTE (include/dcahip.h, dcahip_silhouette): the silhouette coefficient of every labelled point of a clustering,
// Euclidean, exact (every pair is visited) -- no n x n matrix and no n x k matrix exists.  Five or six launches on the stream:
//
//   sil_count_kernel    a workgroup takes `per` consecutive points (at most 1024 workgroups): the members of every cluster
//                       among them (LDS integer atomics) -> bcnt [workgroup][k]; the non-finite coordinates of X -> *status;
//   sil_offsets_kernel  one workgroup: thread c turns column c of bcnt into its exclusive prefix over the workgroups (the place
//                       of a workgroup's first member of c inside cluster c), its total is counts[c]; then the cluster
//                       offsets off [k + 1] (a serial scan over k <= 256);
//   sil_scatter_kernel  the workgroups of the first pass again: a STABLE counting sort of the labelled points by label (the
//                       rank of a point among the equal labels before it in its 256-point tile is counted, not drawn with an
//                       atomic, so the place of every point is a function of the labels alone).  Writes the permutation, the
//                       sorted labels and Xs = the rows of X in (label, index) order, zero-padded to DP; an unlabelled point
//                       gets its NaN / -1 outputs here;
//   sil_scan_kernel     grid (blocks of 256 sorted queries, candidate splits = equal ranges of the sorted candidates).  One
//                       lane owns one query, its coordinates in registers as DP / 2 packed pairs; the candidate row is the same
//                       for the whole wave and comes through the scalar-load path (the loop of knn_scan_kernel).  A lane adds
//                       (double)sqrtf(d2) into ONE double accumulator, candidates ascending; several candidates per trip keep
//                       independent distance chains in flight.  A cluster boundary is the same for the whole grid row: a scalar
//                       branch.  With one split the lane folds the finished cluster's sum into its running a / b / nearest and
//                       forms s at the end; with more the partial sum of the (split, cluster) segment goes to the workspace
//                       (slot split + c: the segments of a query form a monotone staircase, so the slot is theirs alone, at
//                       most splits + k - 1 of them);
//   sil_finish_kernel   (more than one split) per query the partials of every cluster in ascending split order, folded by the
//                       same function;
//   sil_mean_kernel     workgroup c < k: the mean of s over cluster c (its members are contiguous in sorted order: thread t
//                       adds the members t, t + 256, .. in that order, then a fixed tree); workgroup k: over all labelled points.
//
// Why sorted candidates: a [label][lane] accumulator array does not fit LDS at k = 256 and 256 lanes and would make every
// pair a dependent LDS read-modify-write; sorted, a lane needs one register accumulator and the label of a candidate is
// never looked at in the pair loop.
//
// Every order of addition is a function of (n, d, k, splits) and the labels: two calls give the same bits.  Where the double
// sums are exact, every `splits` gives the same bits (a split only moves the places where a sum is cut).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dcahip.h"
#include "knn_dist.hpp"

namespace {

constexpr int kMaxK = 256, kMaxD = 128, kMaxSplits = 64, kNT = 256;
constexpr int kSortBlocks = 1024;           // workgroups of the counting sort: [kSortBlocks][k] counters at most (1 MiB)
constexpr int kMinPerSplit = 1024;          // a split keeps about this many candidates
constexpr int kTargetBlocks = 1536;         // six workgroups per CU of the 256-CU part, as K-NEIGHBOURS
constexpr long kPartialBudget = 256l << 20; // bytes of segment partials the library's own choice of splits stays under


bool shape_ok(int n, int d, int k) { return n >= 0 && d >= 1 && d <= kMaxD && k >= 2 && k <= kMaxK; }

int choose_splits(int n, int k) {
    const long qblocks = ((long)n + kNT - 1) / kNT;
    long s = qblocks > 0 ? (kTargetBlocks + qblocks - 1) / qblocks : 1;
    const long cap = n / kMinPerSplit;
    if (s > cap) s = cap;
    if (s > kMaxSplits) s = kMaxSplits;
    while (s > 1 && (s + k - 1) * (long)n * 8 > kPartialBudget) --s;
    return s < 1 ? 1 : (int)s;
}

struct Plan {
    int dp, nb;
    long per;                                // points per workgroup of the counting sort, a multiple of 256
    long o_bcnt, o_off, o_perm, o_slab, o_ss, o_xs, o_part, bytes;
};

Plan make_plan(int n, int d, int k, int splits) {
    Plan p;
    p.dp = pad_d(d);
    const long tiles = ((long)n + kNT - 1) / kNT;
    long tpb = (tiles + kSortBlocks - 1) / kSortBlocks;
    if (tpb < 1) tpb = 1;
    p.per = tpb * kNT;
    p.nb = (int)((tiles + tpb - 1) / tpb);
    if (p.nb < 1) p.nb = 1;
    long o = 0;
    p.o_bcnt = o; o += r16((long)p.nb * k * 4);
    p.o_off = o;  o += r16((long)(k + 1) * 4);
    p.o_perm = o; o += r16((long)n * 4);
    p.o_slab = o; o += r16((long)n * 4);
    p.o_ss = o;   o += r16((long)n * 8);
    p.o_xs = o;   o += r16((long)n * p.dp * 4);
    p.o_part = o; o += splits > 1 ? r16((long)(splits + k - 1) * n * 8) : 0;
    p.bytes = o;
    return p;
}

__device__ __forceinline__ double d_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double d_inf() { return __longlong_as_double(0x7FF0000000000000ll); }

struct SilArgs {
    const float* X; long ldx; int n, d, k, dp, splits;
    const int* labels;
    double* s_out; double* a_out; double* b_out; int* nearest_out;
    int* counts; double* cluster_mean; double* mean;
    int* bcnt; int* off; int* perm; int* slab; double* ss; float* xs; double* part;
    int nb; long per;
    int* status;
};

// ------------------------------------------------------------------------------------------------------ the counting sort
__global__ __launch_bounds__(256) void sil_count_kernel(SilArgs a) {
    __shared__ int cnt[kMaxK];
    const int t = threadIdx.x, k = a.k, d = a.d;
    cnt[t] = 0;
    __syncthreads();
    const long lo = (long)blockIdx.x * a.per;
    const long hi = lo + a.per < a.n ? lo + a.per : a.n;
    for (long i = lo + t; i < hi; i += kNT) {
        const int l = a.labels[i];
        if (l >= 0 && l < k) atomicAdd(&cnt[l], 1);
    }
    int bad = 0;
    const long e1 = (hi - lo) * d;
    for (long e = t; e < e1; e += kNT) bad += nonfinite(a.X[(lo + e / d) * a.ldx + e % d]);
    __syncthreads();
    if (t < k) a.bcnt[(long)blockIdx.x * k + t] = cnt[t];
    if (bad) atomicAdd(a.status, bad < 4096 ? bad : 4096);   // at most 2^18 threads: the word cannot wrap back to 0
}

__global__ __launch_bounds__(256) void sil_offsets_kernel(SilArgs a) {
    __shared__ int tot[kMaxK];
    const int t = threadIdx.x, k = a.k;
    if (t < k) {
        int run = 0;
        for (int b = 0; b < a.nb; ++b) {
            const int v = a.bcnt[(long)b * k + t];
            a.bcnt[(long)b * k + t] = run;
            run += v;
        }
        tot[t] = run;
        a.counts[t] = run;
    }
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int c = 0; c < k; ++c) { a.off[c] = run; run += tot[c]; }
        a.off[k] = run;
    }
}

__global__ __launch_bounds__(256) void sil_scatter_kernel(SilArgs a) {
    __shared__ int base[kMaxK];
    __shared__ int tcnt[kMaxK];
    __shared__ int lab[kNT];
    __shared__ int pos[kNT];
    const int t = threadIdx.x, k = a.k, d = a.d, dp = a.dp;
    base[t] = t < k ? a.off[t] + a.bcnt[(long)blockIdx.x * k + t] : 0;
    tcnt[t] = 0;
    const long lo = (long)blockIdx.x * a.per;
    const long hi = lo + a.per < a.n ? lo + a.per : a.n;
    for (long t0 = lo; t0 < hi; t0 += kNT) {
        const long i = t0 + t;
        int l = -1;
        if (i < hi) {
            l = a.labels[i];
            l = l >= 0 && l < k ? l : -1;
        }
        lab[t] = l;
        __syncthreads();
        int p = -1;
        if (l >= 0) {
            int rank = 0;
            for (int u = 0; u < t; ++u) rank += lab[u] == l ? 1 : 0;     // the whole wave reads one address: a broadcast
            p = base[l] + rank;
            atomicAdd(&tcnt[l], 1);
            a.perm[p] = (int)i;
            a.slab[p] = l;
        } else if (i < hi) {
            a.s_out[i] = d_nan();
            a.a_out[i] = d_nan();
            a.b_out[i] = d_nan();
            a.nearest_out[i] = -1;
        }
        pos[t] = p;
        __syncthreads();
        const int rows = hi - t0 < kNT ? (int)(hi - t0) : kNT;
        for (int e = t; e < rows * dp; e += kNT) {
            const int r = e / dp, col = e % dp;
            const int pr = pos[r];
            if (pr >= 0) a.xs[(long)pr * dp + col] = col < d ? a.X[(t0 + r) * a.ldx + col] : 0.f;
        }
        base[t] += tcnt[t];
        tcnt[t] = 0;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scan
// the running a / b / nearest of one query: cluster c (n_c > 0 members, clusters ascending) adds up to S
struct Fold {
    double a, b;
    int nearest;
    __device__ __forceinline__ void init() { a = 0.0; b = d_inf(); nearest = -1; }
    __device__ __forceinline__ void take(int c, double S, int n_c, int own) {
        if (c == own) {
            a = n_c > 1 ? S / (double)(n_c - 1) : 0.0;
        } else {
            const double m = S / (double)n_c;
            if (m < b) { b = m; nearest = c; }          // strict: the lowest c that attains the minimum
        }
    }
    __device__ __forceinline__ double s(int n_own) const {
        if (nearest < 0) return d_nan();                 // fewer than two non-empty clusters
        if (n_own <= 1) return 0.0;
        const double mx = a > b ? a : b;
        return mx > 0.0 ? (b - a) / mx : 0.0;
    }
};

__device__ __forceinline__ void sil_store(const SilArgs& a, long q, int own, int n_own, const Fold& f) {
    const double s = f.s(n_own);
    const long i = a.perm[q];
    a.s_out[i] = s;
    a.a_out[i] = f.a;
    a.b_out[i] = f.b;
    a.nearest_out[i] = f.nearest;
    a.ss[q] = s;
}

template <int DP, bool SPLIT>
__global__ __launch_bounds__(256) void sil_scan_kernel(SilArgs a) {
    constexpr int CB = DP <= 32 ? 4 : 2;                 // candidates per trip: independent chains for the vector pipe
    __shared__ int soff[kMaxK + 1];
    const int t = threadIdx.x, k = a.k;
    for (int c = t; c <= k; c += kNT) soff[c] = a.off[c];
    __syncthreads();
    const int m = __builtin_amdgcn_readfirstlane(soff[k]);
    const long q = (long)blockIdx.x * kNT + t;
    if ((long)blockIdx.x * kNT >= m) return;             // the whole workgroup
    const bool live = q < m;

    v2f qv[DP / 2];
    {
        const float* qrow = a.xs + (live ? q : 0) * DP;
#pragma unroll
        for (int j = 0; j < DP / 2; ++j) {
            qv[j].x = qrow[2 * j];
            qv[j].y = qrow[2 * j + 1];
        }
    }
    const int own = live ? a.slab[q] : -1;
    int r0 = 0, r1 = m;
    if (SPLIT) {
        const int per = (m + a.splits - 1) / a.splits;
        const long lo = (long)blockIdx.y * per;
        r0 = lo < m ? (int)lo : m;
        r1 = lo + per < m ? (int)(lo + per) : m;
    }
    const float* __restrict__ xs = a.xs;
    Fold f;
    f.init();
    int n_own = 0;
    for (int c = 0; c < k; ++c) {
        const int o0 = __builtin_amdgcn_readfirstlane(soff[c]), o1 = __builtin_amdgcn_readfirstlane(soff[c + 1]);
        const int lo = o0 > r0 ? o0 : r0, hi = o1 < r1 ? o1 : r1;
        if (lo >= hi) continue;                          // an empty cluster, or one outside this split: the whole grid row
        double acc = 0.0;
        long j = lo;
        for (; j + CB <= hi; j += CB) {
            float d2[CB];
#pragma unroll
            for (int u = 0; u < CB; ++u) d2[u] = dist2<DP>(qv, xs + (j + u) * DP);
#pragma unroll
            for (int u = 0; u < CB; ++u) acc += (double)sqrtf(d2[u]);
        }
        for (; j < hi; ++j) acc += (double)sqrtf(dist2<DP>(qv, xs + j * DP));
        if (SPLIT) {
            if (live) a.part[(long)(blockIdx.y + c) * a.n + q] = acc;
        } else {
            const int n_c = o1 - o0;
            f.take(c, acc, n_c, own);
            n_own = c == own ? n_c : n_own;
        }
    }
    if (!SPLIT && live) sil_store(a, q, own, n_own, f);
}

__global__ __launch_bounds__(256) void sil_finish_kernel(SilArgs a) {
    __shared__ int soff[kMaxK + 1];
    const int t = threadIdx.x, k = a.k;
    for (int c = t; c <= k; c += kNT) soff[c] = a.off[c];
    __syncthreads();
    const int m = soff[k];
    const long q = (long)blockIdx.x * kNT + t;
    if (q >= m) return;
    const int per = (m + a.splits - 1) / a.splits;
    const int own = a.slab[q];
    Fold f;
    f.init();
    int n_own = 0;
    for (int c = 0; c < k; ++c) {
        const int o0 = soff[c], o1 = soff[c + 1];
        if (o1 <= o0) continue;
        const int s0 = o0 / per, s1 = (o1 - 1) / per;    // the splits that hold a part of cluster c
        double S = a.part[(long)(s0 + c) * a.n + q];
        for (int s = s0 + 1; s <= s1; ++s) S += a.part[(long)(s + c) * a.n + q];
        f.take(c, S, o1 - o0, own);
        n_own = c == own ? o1 - o0 : n_own;
    }
    sil_store(a, q, own, n_own, f);
}

__global__ __launch_bounds__(256) void sil_mean_kernel(SilArgs a) {
    __shared__ double red[kNT];
    const int t = threadIdx.x, k = a.k, c = blockIdx.x;
    const long lo = c < k ? a.off[c] : 0, hi = c < k ? a.off[c + 1] : a.off[k];
    double s = 0.0;
    for (long j = lo + t; j < hi; j += kNT) s += a.ss[j];
    red[t] = s;
    __syncthreads();
    for (int w = kNT / 2; w >= 1; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double v = hi > lo ? red[0] / (double)(hi - lo) : d_nan();
        if (c < k) a.cluster_mean[c] = v; else a.mean[0] = v;
    }
}

template <int DP>
int launch_scan(const SilArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((long)a.n + kNT - 1) / kNT), (unsigned)a.splits);
    if (a.splits > 1)
        hipLaunchKernelGGL((sil_scan_kernel<DP, true>), grid, dim3(kNT), 0, s, a);
    else
        hipLaunchKernelGGL((sil_scan_kernel<DP, false>), grid, dim3(kNT), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int dcahip_silhouette_splits(int n, int d, int k) {
    if (!shape_ok(n, d, k)) return DCAHIP_EINVAL;
    return choose_splits(n, k);
}

long dcahip_silhouette_workspace_bytes(int n, int d, int k, int splits) {
    if (!shape_ok(n, d, k) || splits < 0 || splits > kMaxSplits) return DCAHIP_EINVAL;
    if (splits == 0) splits = choose_splits(n, k);
    return make_plan(n, d, k, splits).bytes;
}

int dcahip_silhouette(const float* X, long ldx, int n, int d, const int* labels, int k, int splits,
                      double* s_out, double* a_out, double* b_out, int* nearest_out,
                      int* counts, double* cluster_mean, double* mean,
                      void* ws, int* status, void* stream) {
    if (!shape_ok(n, d, k) || splits < 0 || splits > kMaxSplits || ldx < d) return DCAHIP_EINVAL;
    if (n == 0) return 0;
    if (!X || !labels || !s_out || !a_out || !b_out || !nearest_out || !counts || !cluster_mean || !mean || !ws || !status)
        return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (splits == 0) splits = choose_splits(n, k);
    const Plan p = make_plan(n, d, k, splits);
    char* w = (char*)ws;
    SilArgs a;
    a.X = X; a.ldx = ldx; a.n = n; a.d = d; a.k = k; a.dp = p.dp; a.splits = splits;
    a.labels = labels;
    a.s_out = s_out; a.a_out = a_out; a.b_out = b_out; a.nearest_out = nearest_out;
    a.counts = counts; a.cluster_mean = cluster_mean; a.mean = mean;
    a.bcnt = (int*)(w + p.o_bcnt); a.off = (int*)(w + p.o_off); a.perm = (int*)(w + p.o_perm); a.slab = (int*)(w + p.o_slab);
    a.ss = (double*)(w + p.o_ss); a.xs = (float*)(w + p.o_xs); a.part = (double*)(w + p.o_part);
    a.nb = p.nb; a.per = p.per;
    a.status = status;
    hipLaunchKernelGGL(sil_count_kernel, dim3(p.nb), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(sil_offsets_kernel, dim3(1), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(sil_scatter_kernel, dim3(p.nb), dim3(kNT), 0, s, a);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    switch (p.dp) {
    case 8: rc = launch_scan<8>(a, s); break;
    case 16: rc = launch_scan<16>(a, s); break;
    case 32: rc = launch_scan<32>(a, s); break;
    case 64: rc = launch_scan<64>(a, s); break;
    default: rc = launch_scan<128>(a, s); break;
    }
    if (rc) return rc;
    if (splits > 1)
        hipLaunchKernelGGL(sil_finish_kernel, dim3((unsigned)(((long)n + kNT - 1) / kNT)), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(sil_mean_kernel, dim3(k + 1), dim3(kNT), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
