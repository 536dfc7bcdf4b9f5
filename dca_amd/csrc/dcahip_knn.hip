// K-NEIGHBOURS (include/dcahip.h, dcahip_knn): exact Euclidean k-nearest-neighbour search, distance evaluation and top-k
// selection fused -- no n x n matrix exists.  Three launches on the stream:
//
//   knn_prep_kernel   counts the non-finite coordinates of Q and X into *status and, when d is not one of the unroll widths
//                     8 / 16 / 32 / 64 / 128, copies X zero-padded to the next width into the workspace (the scan then reads
//                     whole rows with uniform-address loads and never looks past a row's end);
//   knn_scan_kernel   grid (query blocks, candidate splits).  One lane owns one query, its coordinates in registers.  The
//                     candidate is the same for the whole wave: its row comes through the scalar-load path and the
//                     distance is `d` packed subtract + `d / 2` packed fused multiply-adds per lane.  A lane keeps its k best
//                     keys UNSORTED in LDS ([slot][lane]: conflict free) with the largest of them and its slot in
//                     registers: a candidate below that threshold overwrites the largest and the lane looks for its new
//                     largest (k independent LDS reads) -- about k ln(n / k) times per query, where a sorted list would
//                     pay a dependent read-compare-write chain per slot shifted.  At the end every lane ranks its keys
//                     (k^2 LDS reads, once) and stores them sorted to the workspace;
//   knn_merge_kernel  one wave per query, lane j at the head of split j's sorted list: k times the wave-wide minimum key is
//                     taken and its lane advances.  The same path for one split.
//
// The key of candidate c at squared distance d2 >= 0 is (bits(d2) << 32) | c: unsigned order = (d2, index) order, a total
// order, so the k smallest do not depend on how the candidates are split.  An empty slot s holds (bits(+inf) << 32) |
// (2^31 + s): above every finite key, distinct inside a list, and recognised by its low word (n < 2^31) when it is written
// out as index -1 at +inf.  A NaN distance is above the empty keys and is never inserted.
//
// d2 (knn_dist.hpp, shared with K-MEANS) = (sum over even k) + (sum over odd k) of fma(a_k - b_k, a_k - b_k, .), k
// ascending: a function of d alone (the zero padding adds +0 exactly), symmetric in a and b bit for bit, never negative, 0
// for equal rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dcahip.h"
#include "knn_dist.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kMaxK = 64, kMaxD = 128, kMaxSplits = 64;
constexpr int kMinPerSplit = 1024;          // a split keeps about this many candidates: below, its list fill dominates
constexpr int kTargetBlocks = 1536;         // six workgroups per CU of the 256-CU part: measured, 68 579 x 32 x 15
                                            // takes 24.6 / 14.2 / 11.3 / 11.4 / 13.7 ms at 1 / 2 / 6 / 8 / 32 splits

__host__ __device__ inline u64 empty_key(int slot) { return ((u64)kInfBits << 32) | (0x80000000u + (unsigned)slot); }

inline int pad_k(int k) { return k <= 16 ? 16 : k <= 32 ? 32 : 64; }
inline int scan_threads(int kp) { return kp == 64 ? 128 : 256; }          // [kp][threads] keys = at most 64 KiB of LDS

bool shape_ok(int nq, int n, int d, int k) { return nq >= 0 && n >= 0 && d >= 1 && d <= kMaxD && k >= 1 && k <= kMaxK; }

int choose_splits(int nq, int n, int k) {
    const int threads = scan_threads(pad_k(k));
    const long qblocks = ((long)nq + threads - 1) / threads;
    long s = qblocks > 0 ? (kTargetBlocks + qblocks - 1) / qblocks : 1;
    const long cap = n / kMinPerSplit;
    if (s > cap) s = cap;
    if (s > kMaxSplits) s = kMaxSplits;
    return s < 1 ? 1 : (int)s;
}

struct KnnArgs {
    const float* Q; long ldq; int nq;
    const float* X; long ldx; int n;
    int d, k;
    long self_offset;
    int splits;
    u64* keys;                              // [splits][nq][k]
};

template <int DP, int KP>
__global__ __launch_bounds__(KP == 64 ? 128 : 256) void knn_scan_kernel(KnnArgs a) {
    constexpr int NT = KP == 64 ? 128 : 256;
    constexpr int CB = DP <= 32 ? 4 : 2;                 // candidates per trip: independent chains for the vector pipe
    __shared__ u64 list[KP][NT];
    const int t = threadIdx.x;
    const long q = (long)blockIdx.x * NT + t;
    const bool live = q < a.nq;
    const int k = a.k;

    v2f qv[DP / 2];
    {
        const float* qrow = a.Q + (live ? q : 0) * a.ldq;
#pragma unroll
        for (int j = 0; j < DP / 2; ++j) {
            qv[j].x = live && 2 * j < a.d ? qrow[2 * j] : 0.f;
            qv[j].y = live && 2 * j + 1 < a.d ? qrow[2 * j + 1] : 0.f;
        }
    }
    for (int s = 0; s < k; ++s) list[s][t] = empty_key(s);
    u64 thr = live ? empty_key(k - 1) : 0;               // a lane without a query accepts nothing (every key is >= 0)
    int thr_slot = k - 1;
    const long ex = a.self_offset >= 0 && a.self_offset < a.n ? a.self_offset + q : -1;
    const int excl = ex >= 0 && ex < a.n ? (int)ex : -1;

    auto consider = [&](float d2, int c) {
        const u64 key = ((u64)__float_as_uint(d2) << 32) | (unsigned)c;
        if (key < thr) {
            if (c != excl) {
                list[thr_slot][t] = key;
                u64 m = 0;
                int ms = 0;
#pragma unroll 4
                for (int s = 0; s < k; ++s) {
                    const u64 v = list[s][t];
                    if (v >= m) { m = v; ms = s; }
                }
                thr = m;
                thr_slot = ms;
            }
        }
    };

    const long per = ((long)a.n + a.splits - 1) / a.splits;
    const long c0 = (long)blockIdx.y * per;
    const long c1 = c0 + per < a.n ? c0 + per : a.n;
    const float* __restrict__ X = a.X;
    long c = c0;
    for (; c + CB <= c1; c += CB) {
        float d2[CB];
#pragma unroll
        for (int u = 0; u < CB; ++u) d2[u] = dist2<DP>(qv, X + (c + u) * a.ldx);
        unsigned lo = __float_as_uint(d2[0]);            // one test per trip: an insert is the rare case
#pragma unroll
        for (int u = 1; u < CB; ++u) lo = min(lo, __float_as_uint(d2[u]));
        if (lo <= (unsigned)(thr >> 32)) {
#pragma unroll
            for (int u = 0; u < CB; ++u) consider(d2[u], (int)(c + u));
        }
    }
    for (; c < c1; ++c) consider(dist2<DP>(qv, X + c * a.ldx), (int)c);

    if (live) {
        u64* out = a.keys + ((long)blockIdx.y * a.nq + q) * k;
        for (int i = 0; i < k; ++i) {
            const u64 ki = list[i][t];
            int rank = 0;
#pragma unroll 4
            for (int s = 0; s < k; ++s) rank += list[s][t] < ki ? 1 : 0;
            out[rank] = ki;                              // the keys of a list are distinct: the ranks are a permutation
        }
    }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ keys, int nq, int k, int splits,
                                                        int* __restrict__ idx_out, float* __restrict__ d2_out, long ldo) {
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;                                 // the whole wave
    const bool have = lane < splits;
    const u64* mine = keys + ((long)(have ? lane : 0) * nq + q) * k;
    int p = 0;
    u64 head = have ? mine[0] : ~0ull;
    u64 res = 0;
    for (int o = 0; o < k; ++o) {
        u64 m = head;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 other = __shfl_xor(m, off, 64);
            m = other < m ? other : m;
        }
        const u64 hit = __ballot(head == m);
        if (lane == __ffsll((long long)hit) - 1) {
            ++p;
            head = p < k ? mine[p] : ~0ull;
        }
        if (lane == o) res = m;
    }
    if (lane < k) {
        const unsigned hi = (unsigned)(res >> 32), lo = (unsigned)res;
        const bool empty = lo >= 0x80000000u;            // an empty slot (or a list run dry): no candidate index has this bit
        idx_out[q * ldo + lane] = empty ? -1 : (int)lo;
        d2_out[q * ldo + lane] = empty ? __uint_as_float(kInfBits) : __uint_as_float(hi);
    }
}

// non-finite coordinates of Q [nq, d] and X [n, d] -> *status; Xp (may be NULL) [n, dp] = X zero-padded
__global__ __launch_bounds__(256) void knn_prep_kernel(const float* __restrict__ Q, long ldq, int nq,
                                                       const float* __restrict__ X, long ldx, int n, int d,
                                                       float* __restrict__ Xp, int dp, int* status) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int bad = 0;
    const long eq = (long)nq * d;
    for (long e = t0; e < eq; e += stride) {
        const float v = Q[e / d * ldq + e % d];
        bad += (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u ? 1 : 0;
    }
    const int w = Xp ? dp : d;
    const long ex = (long)n * w;
    for (long e = t0; e < ex; e += stride) {
        const long r = e / w;
        const int col = (int)(e % w);
        const float v = col < d ? X[r * ldx + col] : 0.f;
        bad += (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u ? 1 : 0;
        if (Xp) Xp[e] = v;
    }
    if (bad) atomicAdd(status, bad < 4096 ? bad : 4096);  // at most 2^18 threads: the word cannot wrap back to 0
}

template <int DP>
int launch_scan(const KnnArgs& a, int kp, hipStream_t s) {
    const int threads = scan_threads(kp);
    const dim3 grid((unsigned)(((long)a.nq + threads - 1) / threads), (unsigned)a.splits);
    switch (kp) {
    case 16: hipLaunchKernelGGL((knn_scan_kernel<DP, 16>), grid, dim3(threads), 0, s, a); break;
    case 32: hipLaunchKernelGGL((knn_scan_kernel<DP, 32>), grid, dim3(threads), 0, s, a); break;
    default: hipLaunchKernelGGL((knn_scan_kernel<DP, 64>), grid, dim3(threads), 0, s, a); break;
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int dcahip_knn_splits(int nq, int n, int d, int k) {
    if (!shape_ok(nq, n, d, k)) return DCAHIP_EINVAL;
    return choose_splits(nq, n, k);
}

long dcahip_knn_workspace_bytes(int nq, int n, int d, int k, int splits) {
    if (!shape_ok(nq, n, d, k) || splits < 0 || splits > kMaxSplits) return DCAHIP_EINVAL;
    if (splits == 0) splits = choose_splits(nq, n, k);
    const long keys = r16((long)splits * nq * k * 8);
    const int dp = pad_d(d);
    return keys + (dp != d ? r16((long)n * dp * 4) : 0);
}

int dcahip_knn(const float* Q, long ldq, int nq, const float* X, long ldx, int n, int d, int k,
               long self_offset, int splits, int* idx_out, float* d2_out, long ldo,
               void* ws, int* status, void* stream) {
    if (!shape_ok(nq, n, d, k) || splits < 0 || splits > kMaxSplits || ldq < d || ldx < d || ldo < k || self_offset < -1)
        return DCAHIP_EINVAL;
    if (nq == 0) return 0;
    if (!Q || (n > 0 && !X) || !idx_out || !d2_out || !ws || !status) return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (splits == 0) splits = choose_splits(nq, n, k);
    const int dp = pad_d(d), kp = pad_k(k);
    u64* keys = (u64*)ws;
    float* Xp = dp != d ? (float*)((char*)ws + r16((long)splits * nq * k * 8)) : nullptr;

    const long elems = (long)nq * d + (long)n * dp;
    long blocks = (elems + 256 * 8 - 1) / (256 * 8);
    blocks = blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(knn_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, Q, ldq, nq, X, ldx, n, d, Xp, dp, status);
    int rc = (int)hipGetLastError();
    if (rc) return rc;

    KnnArgs a;
    a.Q = Q; a.ldq = ldq; a.nq = nq;
    a.X = Xp ? Xp : X; a.ldx = Xp ? dp : ldx; a.n = n;
    a.d = d; a.k = k;
    a.self_offset = self_offset;
    a.splits = splits;
    a.keys = keys;
    switch (dp) {
    case 8: rc = launch_scan<8>(a, kp, s); break;
    case 16: rc = launch_scan<16>(a, kp, s); break;
    case 32: rc = launch_scan<32>(a, kp, s); break;
    case 64: rc = launch_scan<64>(a, kp, s); break;
    default: rc = launch_scan<128>(a, kp, s); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)(((long)nq + 3) / 4)), dim3(256), 0, s, keys, nq, k, splits,
                       idx_out, d2_out, ldo);
    return (int)hipGetLastError();
}

}  // extern "C"
