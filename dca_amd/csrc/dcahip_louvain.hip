// K-LOUVAIN (include/dcahip.h, dcahip_graph_symmetrize / dcahip_louvain_begin / dcahip_louvain_sweep): Louvain modularity
// optimisation of the neighbour graph on the device, in integers throughout -- no floating point, no hash table, so the
// labels are the ones tests/_louvain_ref.py computes, by equality, and the same on every run.
//
// The graph.  W = A + A^T of the [n, k] index array of dcahip_knn as a CSR of unit entries (a mutual pair stands twice in
// both rows): sym_count_kernel (a histogram of out- plus in-degrees, integer atomics), three scan launches (per-chunk sums,
// one workgroup over the chunk sums, per-chunk exclusive scan -> int64 row pointers and the degrees), sym_fill_kernel (a
// row's cursor is its count, taken down by an integer atomic: the order inside a row depends on the run, nothing
// downstream does).  An entry outside 0 .. n-1 other than -1 raises the status and is never an index.
//
// One sweep = four launches, all of them exact no-ops once the level's state word says it has ended:
//
//   louvain_decide_kernel  one wave per vertex (waves stride over the vertices).  The communities and weights of the first
//                          256 entries of the row sit in registers (four per lane), entries past them are read again per
//                          round.  A round: every lane finds the lowest admissible community id above the last one taken
//                          among its entries and the weight it holds of it; a wave minimum gives the community, a wave sum
//                          over the lanes that hold it gives k_{i,c}; the score k_{i,c} M - g k_i tot_c is formed in 128
//                          bits by every lane alike.  Rounds = distinct admissible neighbouring communities.  Ascending
//                          ids and a strict comparison send ties to the lowest id.
//   louvain_stats_kernel   from the NEW labels: the weight inside the communities (64-bit sum, one integer atomic per wave)
//                          and the communities' totals (32-bit integer atomics).
//   louvain_tot2_kernel    the sum of the squared totals (64-bit; it stays below (2m)^2 < 2^62).
//   louvain_commit_kernel  every thread derives the same verdict from the three sums and the state: Q = M in - g tot2 in
//                          128 bits against the best so far.  A sweep that moved nothing is idle (two in a row, one of
//                          each parity, end the level); one that moved something is kept if Q rose -- labels and totals
//                          are copied over the current ones -- and otherwise discarded, which ends the level.  The state
//                          has two slots, read at sweep & 1 and written at the other, so no thread reads what another
//                          writes.
//
// Integer atomics only: order does not matter to integers, the result is the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "dcahip.h"

namespace {

typedef unsigned long long u64;
typedef __int128 i128;

constexpr int kNT = 256, kWaves = kNT / 64;
constexpr int kChunk = 2048;                 // elements of one scan chunk (8 per thread)
constexpr int kReg = 4;                      // row entries a lane keeps in registers
constexpr int kMaxBlocks = 2048;             // workgroups of the striding kernels
constexpr long kR = 1024;                    // the resolution's denominator
constexpr int kStateWords = 24;              // two state slots of 8 words, two sum slots of 4

inline long r16(long x) { return (x + 15) / 16 * 16; }
inline int blocks_for(long items, int per_block) {
    long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b);
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------------------ the graph
struct SymArgs {
    const int* idx; long ldi; int n, k;
    int* cnt; long* bsum; long nchunks;
    long* rowptr; int* col; int* deg;
    int* status;
};

// the neighbour of entry (i, c) if it is an edge; -1 for padding, a self entry and an entry out of range (counted in *bad)
__device__ __forceinline__ int sym_entry(const SymArgs& a, long i, int c, int* bad) {
    const int j = a.idx[i * a.ldi + c];
    if (j == -1 || j == (int)i) return -1;
    if (j < 0 || j >= a.n) { *bad += 1; return -1; }
    return j;
}

__global__ __launch_bounds__(kNT) void sym_count_kernel(SymArgs a) {
    const long total = (long)a.n * a.k;
    int bad = 0;
    for (long t = (long)blockIdx.x * kNT + threadIdx.x; t < total; t += (long)gridDim.x * kNT) {
        const long i = t / a.k;
        const int j = sym_entry(a, i, (int)(t - i * a.k), &bad);
        if (j >= 0) { atomicAdd(&a.cnt[i], 1); atomicAdd(&a.cnt[j], 1); }
    }
    if (bad) atomicAdd(a.status, bad);
}

__global__ __launch_bounds__(kNT) void scan_chunk_sums_kernel(SymArgs a) {
    __shared__ long red[kNT];
    for (long ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        const long base = ch * kChunk + (long)threadIdx.x * 8;
        long s = 0;
        for (int u = 0; u < 8; ++u) if (base + u < a.n) s += a.cnt[base + u];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = kNT / 2; o >= 1; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.bsum[ch] = red[0];
        __syncthreads();
    }
}

// one workgroup: bsum -> its exclusive prefix, in place
__global__ __launch_bounds__(kNT) void scan_chunk_offsets_kernel(SymArgs a) {
    __shared__ long part[kNT];
    const long per = (a.nchunks + kNT - 1) / kNT;
    const long c0 = (long)threadIdx.x * per;
    const long c1 = c0 + per < a.nchunks ? c0 + per : a.nchunks;
    long s = 0;
    for (long c = c0; c < c1; ++c) s += a.bsum[c];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long pre = 0;
        for (int t = 0; t < kNT; ++t) { const long v = part[t]; part[t] = pre; pre += v; }
    }
    __syncthreads();
    long pre = part[threadIdx.x];
    for (long c = c0; c < c1; ++c) { const long v = a.bsum[c]; a.bsum[c] = pre; pre += v; }
}

__global__ __launch_bounds__(kNT) void scan_rows_kernel(SymArgs a) {
    __shared__ long part[kNT];
    for (long ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
        const long base = ch * kChunk + (long)threadIdx.x * 8;
        int v[8];
        long s = 0;
        for (int u = 0; u < 8; ++u) { v[u] = base + u < a.n ? a.cnt[base + u] : 0; s += v[u]; }
        part[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            long pre = a.bsum[ch];
            for (int t = 0; t < kNT; ++t) { const long x = part[t]; part[t] = pre; pre += x; }
        }
        __syncthreads();
        long pre = part[threadIdx.x];
        for (int u = 0; u < 8; ++u) {
            if (base + u < a.n) { a.rowptr[base + u] = pre; a.deg[base + u] = v[u]; }
            pre += v[u];
            if (base + u == (long)a.n - 1) a.rowptr[a.n] = pre;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kNT) void sym_fill_kernel(SymArgs a) {
    const long total = (long)a.n * a.k;
    int bad = 0;
    for (long t = (long)blockIdx.x * kNT + threadIdx.x; t < total; t += (long)gridDim.x * kNT) {
        const long i = t / a.k;
        const int j = sym_entry(a, i, (int)(t - i * a.k), &bad);
        if (j >= 0) {
            // the counts of the first pass are the rows' lengths: a cursor runs from length - 1 down to 0
            a.col[a.rowptr[i] + (atomicSub(&a.cnt[i], 1) - 1)] = j;
            a.col[a.rowptr[j] + (atomicSub(&a.cnt[j], 1) - 1)] = (int)i;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ the sweep
struct SweepArgs {
    int n; long nnz;
    const long* rowptr; const int* col; const int* wt;
    int* ki; int* labels; int* tot; int* labels_new; int* tot_new;
    long twom; int g, sweep, max_sweeps;
    long* state;
};

// state slot p at state + 8 p: done (0 | 1 Q did not rise | 2 two idle sweeps | 3 max_sweeps), sweeps run, best Q low word,
// best Q high word, idle sweeps in a row.  Sum slot p at state + 16 + 4 p: moved, weight inside, sum of squared totals.
__device__ __forceinline__ long* state_slot(long* state, int p) { return state + 8 * p; }
__device__ __forceinline__ u64* sum_slot(long* state, int p) { return (u64*)(state + 16 + 4 * p); }

__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

__device__ __forceinline__ void row_bounds(const SweepArgs& a, long i, long* p0, long* p1) {
    long b = a.rowptr[i], e = a.rowptr[i + 1];
    b = b < 0 ? 0 : b > a.nnz ? a.nnz : b;
    e = e < b ? b : e > a.nnz ? a.nnz : e;
    *p0 = b; *p1 = e;
}

// entry e of row i for the decision: (community of the neighbour, weight); (-1, 0) for a self-loop, an entry past the row
// and anything out of range
__device__ __forceinline__ void load_entry(const SweepArgs& a, long i, long e, long p1, int* c, int* w) {
    *c = -1; *w = 0;
    if (e >= p1) return;
    const int j = a.col[e];
    if (!in_range(j, a.n) || j == (int)i) return;
    const int cj = a.labels[j];
    if (!in_range(cj, a.n)) return;
    *c = cj;
    *w = a.wt ? a.wt[e] : 1;
}

__global__ __launch_bounds__(kNT) void louvain_decide_kernel(SweepArgs a) {
    if (state_slot(a.state, a.sweep & 1)[0] != 0) return;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = (long)gridDim.x * kWaves;
    const i128 M = (i128)a.twom * kR;
    const bool down = (a.sweep & 1) == 0;            // even sweeps move to lower ids, odd ones to higher
    u64 moved = 0;
    for (long i = wave; i < a.n; i += nwaves) {
        const int own = a.labels[i];
        if (lane == 0) a.tot_new[i] = 0;
        if (!in_range(own, a.n)) { if (lane == 0) a.labels_new[i] = own; continue; }
        long p0, p1;
        row_bounds(a, i, &p0, &p1);
        int rc[kReg], rw[kReg];
#pragma unroll
        for (int r = 0; r < kReg; ++r) load_entry(a, i, p0 + lane + 64 * r, p1, &rc[r], &rw[r]);
        const long tail = p0 + 64 * kReg + lane;
        const int hi = down ? own : a.n;
        int last = down ? -1 : own;
        int kia = 0;
#pragma unroll
        for (int r = 0; r < kReg; ++r) kia += rc[r] == own ? rw[r] : 0;
        for (long e = tail; e < p1; e += 64) {
            int c, w;
            load_entry(a, i, e, p1, &c, &w);
            kia += c == own ? w : 0;
        }
        kia = wave_sum(kia);
        const long ki = a.ki[i];
        const long gk = (long)a.g * ki;                                  // < 2^47
        i128 best = (i128)kia * M - (i128)gk * ((long)a.tot[own] - ki);  // staying
        int best_c = own;
        for (;;) {
            int lmin = INT_MAX, lw = 0;
#pragma unroll
            for (int r = 0; r < kReg; ++r) {
                const int c = rc[r];
                if (c > last && c < hi) {
                    if (c < lmin) { lmin = c; lw = rw[r]; }
                    else if (c == lmin) lw += rw[r];
                }
            }
            for (long e = tail; e < p1; e += 64) {
                int c, w;
                load_entry(a, i, e, p1, &c, &w);
                if (c > last && c < hi) {
                    if (c < lmin) { lmin = c; lw = w; }
                    else if (c == lmin) lw += w;
                }
            }
            const int cmin = wave_min(lmin);
            if (cmin == INT_MAX) break;
            const int kic = wave_sum(lmin == cmin ? lw : 0);
            const i128 score = (i128)kic * M - (i128)gk * (long)a.tot[cmin];
            if (score > best) { best = score; best_c = cmin; }
            last = cmin;
        }
        if (lane == 0) a.labels_new[i] = best_c;
        moved += best_c != own ? 1 : 0;
    }
    if (lane == 0 && moved) atomicAdd(&sum_slot(a.state, a.sweep & 1)[0], moved);
}

__global__ __launch_bounds__(kNT) void louvain_stats_kernel(SweepArgs a) {
    if (state_slot(a.state, a.sweep & 1)[0] != 0) return;
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = (long)gridDim.x * kWaves;
    u64 inside = 0;
    for (long i = wave; i < a.n; i += nwaves) {
        const int li = a.labels_new[i];
        if (!in_range(li, a.n)) continue;
        long p0, p1;
        row_bounds(a, i, &p0, &p1);
        for (long e = p0 + lane; e < p1; e += 64) {
            const int j = a.col[e];
            if (in_range(j, a.n) && a.labels_new[j] == li) inside += (u64)(a.wt ? a.wt[e] : 1);
        }
        if (lane == 0) atomicAdd(&a.tot_new[li], a.ki[i]);
    }
    inside = wave_sum64(inside);
    if (lane == 0 && inside) atomicAdd(&sum_slot(a.state, a.sweep & 1)[1], inside);
}

__global__ __launch_bounds__(kNT) void louvain_tot2_kernel(SweepArgs a) {
    if (state_slot(a.state, a.sweep & 1)[0] != 0) return;
    u64 s = 0;
    for (long c = (long)blockIdx.x * kNT + threadIdx.x; c < a.n; c += (long)gridDim.x * kNT) {
        const u64 t = (u64)(long)a.tot_new[c];
        s += t * t;
    }
    s = wave_sum64(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&sum_slot(a.state, a.sweep & 1)[2], s);
}

__global__ __launch_bounds__(kNT) void louvain_commit_kernel(SweepArgs a) {
    const int p = a.sweep & 1, q = p ^ 1;
    const long* st = state_slot(a.state, p);
    const u64* sm = sum_slot(a.state, p);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    long done = st[0], sweeps = st[1], idle = st[4];
    i128 best = (i128)(((unsigned __int128)(u64)st[3] << 64) | (u64)st[2]);
    bool keep = false;
    if (!done) {
        const u64 moved = sm[0];
        const i128 Q = (i128)a.twom * kR * (i128)(long)sm[1] - (i128)a.g * (i128)(long)sm[2];
        sweeps += 1;
        if (moved == 0) {
            idle += 1;
            if (idle >= 2) done = 2;
        } else if (Q > best) {
            keep = true; best = Q; idle = 0;
        } else {
            done = 1;
        }
        if (!done && sweeps >= a.max_sweeps) done = 3;
    }
    if (first) {
        long* out = state_slot(a.state, q);
        out[0] = done; out[1] = sweeps; out[2] = (long)(u64)best; out[3] = (long)(best >> 64); out[4] = idle;
        out[5] = keep ? 1 : 0; out[6] = 0; out[7] = 0;
        u64* z = sum_slot(a.state, q);
        z[0] = 0; z[1] = 0; z[2] = 0; z[3] = 0;
    }
    if (keep)
        for (long i = (long)blockIdx.x * kNT + threadIdx.x; i < a.n; i += (long)gridDim.x * kNT) {
            a.labels[i] = a.labels_new[i];
            a.tot[i] = a.tot_new[i];
        }
}

// the start of a level: singletons, the degrees, and the Q of that state as the best so far
__global__ __launch_bounds__(kNT) void louvain_begin_kernel(SweepArgs a) {
    const int lane = threadIdx.x & 63;
    u64 self = 0, k2 = 0;
    for (long i = (long)blockIdx.x * kNT + threadIdx.x; i < a.n; i += (long)gridDim.x * kNT) {
        long p0, p1;
        row_bounds(a, i, &p0, &p1);
        long k = 0;
        for (long e = p0; e < p1; ++e) {
            const long w = a.wt ? a.wt[e] : 1;
            k += w;
            if (a.col[e] == (int)i) self += (u64)w;
        }
        a.ki[i] = (int)k; a.tot[i] = (int)k; a.labels[i] = (int)i;
        k2 += (u64)k * (u64)k;
    }
    self = wave_sum64(self);
    k2 = wave_sum64(k2);
    if (lane == 0) {
        if (self) atomicAdd(&sum_slot(a.state, 0)[1], self);
        if (k2) atomicAdd(&sum_slot(a.state, 0)[2], k2);
    }
}

__global__ void louvain_begin_commit_kernel(SweepArgs a) {
    if (blockIdx.x || threadIdx.x) return;
    u64* sm = sum_slot(a.state, 0);
    const i128 Q = (i128)a.twom * kR * (i128)(long)sm[1] - (i128)a.g * (i128)(long)sm[2];
    for (int p = 0; p < 2; ++p) {                    // both slots: the first sweep may be of either parity
        long* st = state_slot(a.state, p);
        st[0] = 0; st[1] = 0; st[2] = (long)(u64)Q; st[3] = (long)(Q >> 64); st[4] = 0; st[5] = 0; st[6] = 0; st[7] = 0;
    }
    sm[0] = 0; sm[1] = 0; sm[2] = 0; sm[3] = 0;
}

bool sweep_ok(int n, long nnz, long twom, int g) {
    return n >= 0 && nnz >= 0 && nnz <= INT_MAX && twom >= 0 && twom <= INT_MAX && g >= 1 && g <= 64 * kR;
}

}  // namespace

extern "C" {

long dcahip_graph_symmetrize_workspace_bytes(int n, int k) {
    if (n < 0 || k < 1) return DCAHIP_EINVAL;
    const long nchunks = ((long)n + kChunk - 1) / kChunk;
    return r16((long)n * 4) + r16(nchunks * 8);
}

int dcahip_graph_symmetrize(const int* idx, long ldi, int n, int k, long* rowptr, int* col, long cap, int* deg,
                            void* ws, int* status, void* stream) {
    if (n < 0 || k < 1 || ldi < k || (long)n * k > INT_MAX / 2 || cap < 2 * (long)n * k) return DCAHIP_EINVAL;
    if (!rowptr) return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return (int)hipMemsetAsync(rowptr, 0, sizeof(long), s);
    if (!idx || !col || !deg || !ws || !status) return DCAHIP_EINVAL;
    SymArgs a;
    a.idx = idx; a.ldi = ldi; a.n = n; a.k = k;
    a.nchunks = ((long)n + kChunk - 1) / kChunk;
    a.cnt = (int*)ws; a.bsum = (long*)((char*)ws + r16((long)n * 4));
    a.rowptr = rowptr; a.col = col; a.deg = deg; a.status = status;
    int rc = (int)hipMemsetAsync(a.cnt, 0, (size_t)n * 4, s);
    if (rc) return rc;
    const int eb = blocks_for((long)n * k, kNT), cb = blocks_for(a.nchunks, 1);
    hipLaunchKernelGGL(sym_count_kernel, dim3(eb), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3(cb), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(scan_chunk_offsets_kernel, dim3(1), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(scan_rows_kernel, dim3(cb), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(sym_fill_kernel, dim3(eb), dim3(kNT), 0, s, a);
    return (int)hipGetLastError();
}

int dcahip_louvain_begin(int n, long nnz, const long* rowptr, const int* col, const int* wt, int* ki, int* labels, int* tot,
                         long twom, int g, long* state, void* stream) {
    if (!sweep_ok(n, nnz, twom, g) || !state) return DCAHIP_EINVAL;
    if (n > 0 && (!rowptr || !ki || !labels || !tot || (nnz > 0 && !col))) return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int rc = (int)hipMemsetAsync(state, 0, kStateWords * sizeof(long), s);
    if (rc) return rc;
    SweepArgs a = {};
    a.n = n; a.nnz = nnz; a.rowptr = rowptr; a.col = col; a.wt = wt; a.ki = ki; a.labels = labels; a.tot = tot;
    a.twom = twom; a.g = g; a.state = state;
    if (n > 0) hipLaunchKernelGGL(louvain_begin_kernel, dim3(blocks_for(n, kNT)), dim3(kNT), 0, s, a);
    hipLaunchKernelGGL(louvain_begin_commit_kernel, dim3(1), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}

int dcahip_louvain_sweep(int n, long nnz, const long* rowptr, const int* col, const int* wt, const int* ki, int* labels,
                         int* tot, int* labels_new, int* tot_new, long twom, int g, int sweep, int max_sweeps, long* state,
                         void* stream) {
    if (!sweep_ok(n, nnz, twom, g) || sweep < 0 || max_sweeps < 1 || !state) return DCAHIP_EINVAL;
    if (n > 0 && (!rowptr || !ki || !labels || !tot || !labels_new || !tot_new || (nnz > 0 && !col))) return DCAHIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    SweepArgs a = {};
    a.n = n; a.nnz = nnz; a.rowptr = rowptr; a.col = col; a.wt = wt; a.ki = (int*)ki; a.labels = labels; a.tot = tot;
    a.labels_new = labels_new; a.tot_new = tot_new;
    a.twom = twom; a.g = g; a.sweep = sweep; a.max_sweeps = max_sweeps; a.state = state;
    const int wb = blocks_for(n, kWaves), tb = blocks_for(n, kNT);
    if (n > 0) {
        hipLaunchKernelGGL(louvain_decide_kernel, dim3(wb), dim3(kNT), 0, s, a);
        hipLaunchKernelGGL(louvain_stats_kernel, dim3(wb), dim3(kNT), 0, s, a);
        hipLaunchKernelGGL(louvain_tot2_kernel, dim3(tb), dim3(kNT), 0, s, a);
    }
    hipLaunchKernelGGL(louvain_commit_kernel, dim3(tb), dim3(kNT), 0, s, a);
    return (int)hipGetLastError();
}

}  // extern "C"
