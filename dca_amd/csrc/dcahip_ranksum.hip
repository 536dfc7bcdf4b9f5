// K-RANKS (include/dcahip.h, dcahip_ranksum): per gene (a row of the gene-major matrix x) the labelled cells are sorted by
// value and every group's rank sum (or Mann-Whitney U against one group) and tie term come out as exact integers.
//
// Launches on the stream: a 16-byte clear of the status word, ranks_codes_kernel (the 16-bit group code of every position
// of `order`, by a binary search of gstart; an `order` entry outside [0, n) sets the status word and is never used as an
// index), ranks_kernel.  m == 0: ranks_fill_kernel writes zeros and nothing else runs.
//
// ranks_kernel: a persistent grid of kThreads-thread workgroups, workgroup b takes the rows b, b + grid, ..: one row at a
// time, whole.  The workspace holds, per WORKGROUP, two key arrays (uint32 [n]) and two code arrays (uint16 [n]): it does
// not grow with g.  Per row:
//
//   histogram   one read of the m values through `order` (a gather inside the row): the order-preserving 32-bit image of
//               every float (-0.0f folded onto +0.0f first; a negative value: all bits flipped; otherwise the sign bit set)
//               and the four 256-bin histograms of its bytes (LDS integer atomics; a wave whose lanes all hold the same
//               byte adds its count once).  A NaN marks the row: -1 everywhere, nothing else is done for it.
//   sort        a stable LSD radix sort, 8 bits per pass, least significant byte first.  The first pass that runs reads through
//               `order` again and takes the codes in `order`'s sequence (group after group): equal keys stay in group order
//               from there on, because every pass is stable.  A pass whose byte is the same for all m keys moves nothing
//               and is skipped (a constant row runs one pass, as a copy).  A pass goes in tiles of kThreads * kE keys; a wave owns 64 * kE
//               consecutive keys of the tile and takes them 64 at a time: eight ballots give every lane the set of lanes
//               with its digit, the lanes below it are its rank, and the wave's running count of the digit (LDS, one row
//               of 256 counters per wave, touched by that wave alone) is its offset inside the wave.  After a barrier thread
//               d turns the eight counts of digit d into offsets onto the digit's running global position.  The tile is
//               then laid out in digit order in LDS (in the memory the scans' accumulators use later) and written from
//               there to the other pair of arrays, so that neighbouring lanes write neighbouring places of one digit's
//               range.  No rank comes from an atomic: the place of a key is a function of the keys.
//   forward     positions ascending, kThreads at a time, carries in registers: a(p), the start of p's run of equal keys, is
//               a max-scan of the run heads; with ref the count of ref cells below the run, P(a), is a max-scan of the
//               exclusive prefix count at the heads (it does not decrease).  Every cell adds a (rest) or P(a) (ref) to
//               its group; rest: a run's tail adds t^3 - t; ref: P(a) is stored per position in the key array the sort
//               left free.
//   backward    positions descending: b(p), the end of the run, is a min-scan of the tails; P(b) = n_ref - (ref cells
//               above the tail), a min-scan again.  Every cell adds b + 1 (rest) or P(b) (ref).  ref: the head of a run
//               adds t_r^3 - t_r (t_r = P(b) - P(a), the run's ref cells) to the common term and the head of a same-group
//               sub-run of c != ref adds (t_c + t_r)^3 - t_r^3 - t_c to group c's (t_c from a min-scan of the sub-run
//               tails): together the sum of t^3 - t over the runs of c and ref pooled.
//
// Loads stand ahead of their use: the histogram and a sort tile issue their kE loads per lane before the first of them is
// looked at (the rounds of a tile wait for each other at the wave's counters), and the scans fetch a round ahead.
//
// No thread walks along a run: heads and tails are found by comparing neighbours and carried by scans, so ties never make
// a row dearer (a skipped pass makes it cheaper).  The group accumulators are 64-bit integers in LDS (2 x 4096), each group spread over as many
// copies as fit (lane % copies picks one) so that neighbours of one group do not queue on one address; integer additions
// commute, so the result does not depend on the order the atomics arrive in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dcahip.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 512, kWaves = kThreads / 64, kE = 8, kTile = kThreads * kE;
constexpr int kMaxK = 4096, kMaxN = 2097151;
constexpr int kGridSmall = 512, kGridLarge = 256, kLargeN = 262144;      // workgroups: two per CU | one per CU for long rows
constexpr int kIntMax = 0x7FFFFFFF;

inline long r16(long x) { return (x + 15) / 16 * 16; }
inline int ranks_grid(int g, int n) { const int cap = n > kLargeN ? kGridLarge : kGridSmall; return g < cap ? g : cap; }
inline long per_wg_bytes(int n) { return 2 * r16(4l * n) + 2 * r16(2l * n); }

struct RankArgs {
    const float* x; long ldx; int g, n;
    const int* order; int m; const int* gstart; int K, ref;
    long long* rank2; long long* tie; long ldr;
    const int* status; const unsigned short* code0; char* wg_base; long kbytes, cbytes;
};

__global__ void ranks_fill_kernel(long long* rank2, long long* tie, long ldr, int g, int K, long long v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)g * K) return;
    const long c = i / g, j = i % g;
    rank2[c * ldr + j] = v;
    tie[c * ldr + j] = v;
}

__global__ void ranks_codes_kernel(const int* order, int m, int n, const int* gstart, int K, unsigned short* code0, int* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int o = order[i];
    if (o < 0 || o >= n) *status = 1;
    int lo = 0, hi = K - 1;                   // the group c with gstart[c] <= i < gstart[c + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (gstart[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    code0[i] = (unsigned short)lo;
}

__device__ __forceinline__ unsigned key_of(unsigned u) {
    if (u == 0x80000000u) u = 0u;                                        // -0.0f ties with +0.0f
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int wave_scan_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v = max(v, o); }
    return v;
}
__device__ __forceinline__ int wave_scan_min(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v = min(v, o); }
    return v;
}
__device__ __forceinline__ int wave_scan_add(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}

__device__ __forceinline__ u64 cube(int t) { const u64 u = (u64)t; return u * u * u; }

__global__ __launch_bounds__(kThreads) void ranks_kernel(RankArgs A) {
    __shared__ u64 accmem[2 * kMaxK];        // the scans' group accumulators; during the sort: a tile staged in digit order
    u64* racc = accmem;
    u64* tacc = accmem + kMaxK;
    unsigned* stageK = (unsigned*)accmem;                             // [kTile]
    unsigned short* stageC = (unsigned short*)(accmem + kMaxK);       // [kTile]
    __shared__ unsigned hist[4][256];
    __shared__ unsigned short cnt[kWaves][256];     // a wave's keys of a digit in the tile so far (at most 64 * kE)
    __shared__ unsigned short woff[kWaves][256];    // ... of the waves before it
    __shared__ unsigned gbase[256], tbase[256];      // the digit's next global position | the same at the tile's start
    __shared__ unsigned tdigp[256], wsum[4];         // the digit's first place in the staged tile: tdigp[d] + wsum[< d / 64]
    __shared__ int wtot[2][3][kWaves];
    __shared__ u64 common;                   // rest: sum t^3 - t over the runs; ref: the same over the ref cells alone
    __shared__ int skip[4];
    __shared__ int has_nan;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = A.m, K = A.K, ref = A.ref;
    int copies = 1;
    while (copies < 32 && copies * 2 * K <= kMaxK) copies *= 2;
    const int mycopy = tid & (copies - 1);

    char* base = A.wg_base + (long)blockIdx.x * (2 * A.kbytes + 2 * A.cbytes);
    unsigned* keyA = (unsigned*)base;
    unsigned* keyB = (unsigned*)(base + A.kbytes);
    unsigned short* codeA = (unsigned short*)(base + 2 * A.kbytes);
    unsigned short* codeB = (unsigned short*)(base + 2 * A.kbytes + A.cbytes);

    const bool bad_order = *A.status != 0;
    const int n_ref = ref >= 0 ? A.gstart[ref + 1] - A.gstart[ref] : 0;
    __syncthreads();

    for (int row = blockIdx.x; row < A.g; row += gridDim.x) {
        const float* xr = A.x + (long)row * A.ldx;
        // ---------------------------------------------------------------- histogram of the four bytes, NaN check
        for (int i = tid; i < 4 * 256; i += kThreads) (&hist[0][0])[i] = 0;
        if (tid < 4) skip[tid] = 0;
        if (tid == 0) { has_nan = 0; common = 0; }
        __syncthreads();
        if (!bad_order) {
            for (int t0 = 0; t0 < m; t0 += kTile) {
                unsigned us[kE];
#pragma unroll
                for (int r = 0; r < kE; ++r) {        // kE gathers in flight per lane
                    const int i = t0 + r * kThreads + tid;
                    us[r] = 0;
                    if (i < m) us[r] = __float_as_uint(xr[A.order[i]]);
                }
#pragma unroll
                for (int r = 0; r < kE; ++r) {
                    const bool valid = t0 + r * kThreads + tid < m;
                    const unsigned u = us[r];
                    if (valid && (u & 0x7FFFFFFFu) > 0x7F800000u) has_nan = 1;
                    const unsigned key = key_of(u);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const unsigned d = (key >> (8 * p)) & 255u;
                        const unsigned d0 = __builtin_amdgcn_readfirstlane(d);
                        const u64 act = __ballot(valid);
                        if (__ballot(valid && d != d0) == 0 && (act & 1)) {      // one byte for the whole wave
                            if (lane == 0) atomicAdd(&hist[p][d0], (unsigned)__popcll(act));
                        } else if (valid) {
                            atomicAdd(&hist[p][d], 1u);
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (bad_order || has_nan) {
            for (int c = tid; c < K; c += kThreads) { A.rank2[c * A.ldr + row] = -1; A.tie[c * A.ldr + row] = -1; }
            __syncthreads();
            continue;
        }
        if (tid < 256) {
#pragma unroll
            for (int p = 0; p < 4; ++p) if (hist[p][tid] == (unsigned)m) skip[p] = 1;
        }
        __syncthreads();

        // ---------------------------------------------------------------- the sort
        bool gathered = false;                // false: the source is still x through `order`
        unsigned* srcK = keyB; unsigned* dstK = keyA;
        unsigned short* srcC = codeB; unsigned short* dstC = codeA;
        for (int pass = 0; pass < 4; ++pass) {
            if (skip[pass] && (gathered || pass < 3)) continue;
            const int shift = 8 * pass;
            if (w == 0) {                     // exclusive prefix of the 256 counts: the first position of every digit
                const unsigned h0 = hist[pass][4 * lane], h1 = hist[pass][4 * lane + 1], h2 = hist[pass][4 * lane + 2],
                               h3 = hist[pass][4 * lane + 3];
                const int incl = wave_scan_add((int)(h0 + h1 + h2 + h3), lane);
                unsigned e = (unsigned)incl - (h0 + h1 + h2 + h3);
                gbase[4 * lane] = e; e += h0;
                gbase[4 * lane + 1] = e; e += h1;
                gbase[4 * lane + 2] = e; e += h2;
                gbase[4 * lane + 3] = e;
            }
            for (int i = tid; i < kWaves * 256; i += kThreads) (&cnt[0][0])[i] = 0;
            __syncthreads();
            for (int t0 = 0; t0 < m; t0 += kTile) {
                unsigned key[kE]; unsigned short code[kE]; unsigned off[kE];
                volatile unsigned short* mycnt = cnt[w];
#pragma unroll
                for (int r = 0; r < kE; ++r) {        // all loads of the tile first: the rounds below wait for each other
                    const int i = t0 + w * (64 * kE) + r * 64 + lane;
                    key[r] = 0; code[r] = 0;
                    if (i < m) {
                        if (gathered) { key[r] = srcK[i]; code[r] = srcC[i]; }
                        else { key[r] = __float_as_uint(xr[A.order[i]]); code[r] = A.code0[i]; }
                    }
                }
#pragma unroll
                for (int r = 0; r < kE; ++r) {
                    const int i = t0 + w * (64 * kE) + r * 64 + lane;
                    const bool valid = i < m;
                    if (!gathered) key[r] = key_of(key[r]);
                    const unsigned d = (key[r] >> shift) & 255u;
                    u64 mask = __ballot(valid);
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const bool bit = (d >> b) & 1u;
                        const u64 vote = __ballot(valid && bit);
                        mask &= bit ? vote : ~vote;
                    }
                    const int below = __popcll(mask & ((1ull << lane) - 1ull));
                    unsigned prev = 0;
                    if (valid) prev = mycnt[d];
                    __builtin_amdgcn_wave_barrier();
                    if (valid && below == 0) mycnt[d] = (unsigned short)(prev + (unsigned)__popcll(mask));
                    __builtin_amdgcn_wave_barrier();
                    off[r] = prev + (unsigned)below;
                }
                __syncthreads();
                if (tid < 256) {
                    unsigned run = 0;
#pragma unroll
                    for (int ww = 0; ww < kWaves; ++ww) { const unsigned c = cnt[ww][tid]; woff[ww][tid] = (unsigned short)run; run += c; cnt[ww][tid] = 0; }
                    const unsigned gb = gbase[tid];
                    tbase[tid] = gb;
                    gbase[tid] = gb + run;
                    const unsigned incl = (unsigned)wave_scan_add((int)run, lane);      // waves 0 .. 3, all lanes
                    tdigp[tid] = incl - run;
                    if (lane == 63) wsum[w] = incl;
                }
                __syncthreads();
                // the tile in digit order in LDS, then out: neighbouring lanes write neighbouring places of one digit's
                // range instead of 64 places each
#pragma unroll
                for (int r = 0; r < kE; ++r) {
                    const int i = t0 + w * (64 * kE) + r * 64 + lane;
                    if (i < m) {
                        const unsigned d = (key[r] >> shift) & 255u;
                        const unsigned first = tdigp[d] + (d >= 64 ? wsum[0] : 0u) + (d >= 128 ? wsum[1] : 0u) + (d >= 192 ? wsum[2] : 0u);
                        const unsigned lpos = first + woff[w][d] + off[r];
                        if (lpos < (unsigned)kTile) { stageK[lpos] = key[r]; stageC[lpos] = code[r]; }
                    }
                }
                __syncthreads();
                const int in_tile = min(kTile, m - t0);
#pragma unroll
                for (int r = 0; r < kE; ++r) {
                    const int j = r * kThreads + tid;
                    if (j < in_tile) {
                        const unsigned k = stageK[j];
                        const unsigned d = (k >> shift) & 255u;
                        const unsigned first = tdigp[d] + (d >= 64 ? wsum[0] : 0u) + (d >= 128 ? wsum[1] : 0u) + (d >= 192 ? wsum[2] : 0u);
                        const unsigned dest = tbase[d] + ((unsigned)j - first);
                        if (dest < (unsigned)m) { dstK[dest] = k; dstC[dest] = stageC[j]; }
                    }
                }
            }
            __syncthreads();
            gathered = true;
            unsigned* tk = srcK; srcK = dstK; dstK = tk;
            unsigned short* tc = srcC; srcC = dstC; dstC = tc;
        }
        // the sorted keys and codes are in srcK / srcC; dstK is free
        int* Pa = (int*)dstK;

        // what a scan needs of sorted position p, packed: the group code (clamped), bit 16 head and 17 tail of the run of
        // equal keys, with `sub` bit 18 head and 19 tail of the same-group sub-run; 0 outside [0, m).  The scans fetch a
        // round ahead, so that the loads of the next round are in flight behind the barriers of this one.
        auto fetch = [&](int p, bool sub) -> int {
            if (p < 0 || p >= m) return 0;
            const unsigned k = srcK[p];
            const unsigned short c = srcC[p];
            const bool head = p == 0 || srcK[p - 1] != k, tail = p == m - 1 || srcK[p + 1] != k;
            int v = min((int)c, K - 1) | (head ? 1 << 16 : 0) | (tail ? 1 << 17 : 0);
            if (sub) v |= ((head || srcC[p - 1] != c) ? 1 << 18 : 0) | ((tail || srcC[p + 1] != c) ? 1 << 19 : 0);
            return v;
        };
        for (int i = tid; i < 2 * kMaxK; i += kThreads) accmem[i] = 0;      // the sort is done with it
        __syncthreads();
        // ---------------------------------------------------------------- forward scan
        {
            int carry_a = -1, carry_sum = 0, carry_pa = -1, par = 0;
            int cur = fetch(tid, false);
            for (int p0 = 0; p0 < m; p0 += kThreads, par ^= 1) {
                const int p = p0 + tid;
                const bool valid = p < m;
                const int got = cur;
                cur = fetch(p + kThreads, false);
                const int c = got & 0xFFFF;
                const bool head = (got >> 16) & 1, tail = (got >> 17) & 1;
                if (ref < 0) {
                    const int v = wave_scan_max(head ? p : -1, lane);
                    if (lane == 63) wtot[par][0][w] = v;
                    __syncthreads();
                    int pre = carry_a;
                    for (int ww = 0; ww < kWaves; ++ww) { const int t = wtot[par][0][ww]; if (ww < w) pre = max(pre, t); carry_a = max(carry_a, t); }
                    if (valid) {
                        const int a = max(pre, v);
                        atomicAdd(&racc[c * copies + mycopy], (u64)a);
                        if (tail && p > a) { const int t = p + 1 - a; atomicAdd(&common, cube(t) - (u64)t); }
                    }
                } else {
                    const int isref = valid && c == ref;
                    const int s = wave_scan_add(isref, lane);
                    if (lane == 63) wtot[par][1][w] = s;
                    __syncthreads();
                    int spre = carry_sum;
                    for (int ww = 0; ww < kWaves; ++ww) { const int t = wtot[par][1][ww]; if (ww < w) spre += t; carry_sum += t; }
                    const int pexcl = spre + s - isref;
                    const int v = wave_scan_max(head ? pexcl : -1, lane);
                    if (lane == 63) wtot[par][2][w] = v;
                    __syncthreads();
                    int pre = carry_pa;
                    for (int ww = 0; ww < kWaves; ++ww) { const int t = wtot[par][2][ww]; if (ww < w) pre = max(pre, t); carry_pa = max(carry_pa, t); }
                    if (valid) {
                        const int pa = max(pre, v);
                        Pa[p] = pa;
                        atomicAdd(&racc[c * copies + mycopy], (u64)pa);
                    }
                }
            }
        }
        __syncthreads();
        // ---------------------------------------------------------------- backward scan
        {
            int carry_b = kIntMax, carry_sum = 0, carry_pb = kIntMax, carry_sb = kIntMax, par = 0;
            int cur = fetch(m - 1 - tid, ref >= 0);
            for (int q0 = 0; q0 < m; q0 += kThreads, par ^= 1) {
                const int p = m - 1 - (q0 + tid);
                const bool valid = p >= 0;
                const int got = cur;
                cur = fetch(p - kThreads, ref >= 0);
                const int c = got & 0xFFFF;
                const bool head = (got >> 16) & 1, tail = (got >> 17) & 1, shead = (got >> 18) & 1, stail = (got >> 19) & 1;
                if (ref < 0) {
                    const int v = wave_scan_min(tail ? p + 1 : kIntMax, lane);
                    if (lane == 63) wtot[par][0][w] = v;
                    __syncthreads();
                    int pre = carry_b;
                    for (int ww = 0; ww < kWaves; ++ww) { const int t = wtot[par][0][ww]; if (ww < w) pre = min(pre, t); carry_b = min(carry_b, t); }
                    if (valid) atomicAdd(&racc[c * copies + mycopy], (u64)(min(pre, v) + 1));
                } else {
                    const int isref = valid && c == ref;
                    const int s = wave_scan_add(isref, lane);
                    const int vs = wave_scan_min(stail ? p + 1 : kIntMax, lane);
                    if (lane == 63) { wtot[par][1][w] = s; wtot[par][0][w] = vs; }
                    __syncthreads();
                    int spre = carry_sum, sbpre = carry_sb;
                    for (int ww = 0; ww < kWaves; ++ww) {
                        const int t = wtot[par][1][ww], u = wtot[par][0][ww];
                        if (ww < w) { spre += t; sbpre = min(sbpre, u); }
                        carry_sum += t; carry_sb = min(carry_sb, u);
                    }
                    const int pincl = n_ref - (spre + s) + isref;       // ref cells at positions <= p
                    const int v = wave_scan_min(tail ? pincl : kIntMax, lane);
                    if (lane == 63) wtot[par][2][w] = v;
                    __syncthreads();
                    int pre = carry_pb;
                    for (int ww = 0; ww < kWaves; ++ww) { const int t = wtot[par][2][ww]; if (ww < w) pre = min(pre, t); carry_pb = min(carry_pb, t); }
                    if (valid) {
                        const int pb = min(pre, v);
                        atomicAdd(&racc[c * copies + mycopy], (u64)pb);
                        if (shead) {
                            const int tr = pb - Pa[p];
                            if (head && tr > 0) atomicAdd(&common, cube(tr) - (u64)tr);
                            if (c != ref) {
                                const int tc = min(sbpre, vs) - p;
                                atomicAdd(&tacc[c * copies + mycopy], cube(tc + tr) - cube(tr) - (u64)tc);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---------------------------------------------------------------- the row's results
        for (int c = tid; c < K; c += kThreads) {
            u64 r = 0, t = 0;
            for (int i = 0; i < copies; ++i) { r += racc[c * copies + i]; t += tacc[c * copies + i]; }
            A.rank2[c * A.ldr + row] = (long long)r;
            A.tie[c * A.ldr + row] = (long long)(common + t);
        }
        __syncthreads();
    }
}

bool shape_ok(int g, int n) { return g > 0 && n > 0 && n <= kMaxN; }

}  // namespace

extern "C" long dcahip_ranksum_workspace_bytes(int g, int n) {
    if (!shape_ok(g, n)) return DCAHIP_EINVAL;
    return 16 + r16(2l * n) + (long)ranks_grid(g, n) * per_wg_bytes(n);
}

extern "C" int dcahip_ranksum(const float* x, long ldx, int g, int n, const int* order, int m, const int* gstart, int K,
                              int ref, long long* rank2, long long* tie, long ldr, void* workspace, void* stream) {
    if (!x || !gstart || !rank2 || !tie || !workspace || !shape_ok(g, n) || ldx < n || ldr < g || m < 0 || m > n
        || (m > 0 && !order) || K < 1 || K > kMaxK || ref < -1 || ref >= K)
        return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long items = (long)g * K;
    if (m == 0) {
        hipLaunchKernelGGL(ranks_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, rank2, tie, ldr, g, K, 0ll);
        return (int)hipGetLastError();
    }
    char* ws = static_cast<char*>(workspace);
    int* status = reinterpret_cast<int*>(ws);
    unsigned short* code0 = reinterpret_cast<unsigned short*>(ws + 16);
    hipError_t e = hipMemsetAsync(status, 0, 16, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ranks_codes_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, order, m, n, gstart, K, code0, status);
    RankArgs a{x, ldx, g, n, order, m, gstart, K, ref, rank2, tie, ldr, status, code0, ws + 16 + r16(2l * n), r16(4l * n), r16(2l * n)};
    hipLaunchKernelGGL(ranks_kernel, dim3((unsigned)ranks_grid(g, n)), dim3(kThreads), 0, s, a);
    return (int)hipGetLastError();
}
