// K-PREP: the preprocessing of dca/io.py:88-111 (scanpy's filter counts, normalize_per_cell,
// log1p, scale) on the resident count matrix, so that the training inputs are produced in HBM
// from ONE upload of the raw counts.  All kernels are memory-bound streaming passes over the
// [n_cells, n_genes] matrix (float4 per lane, coalesced), gfx950 / wave64.
//
//   row sums          n_counts per cell      (filter_cells, normalize_per_cell: exact -- counts
//                                             are integers, accumulated in fp64)
//   column pass       x = log1p(y / fac[row]) written to X, with per-gene sums of x and x*x
//                     accumulated in fp64 per row chunk (deterministic second stage); the same
//                     pass with the transform switched off yields the per-gene counts of
//                     filter_genes
//   column stats      mean, std (ddof = 1, zero std -> 1) exactly as scanpy's scale
//   scale             x = (x - mean) / std in place
//   CSR expand        rows of a CSR chunk -> dense fp32 rows of the resident count matrix (the
//                     upload of a sparse host matrix: index + value bytes cross PCIe, the zeros
//                     are written here)
//   CSR compress /    dense rows -> CSR, and the resident CSR without some rows / columns: the counts-resident form is
//   subset            built and filtered here, not on the host
//   CSR thin          K-SPLIT: every count of the resident CSR thinned binomially into two parts (molecular cross-validation),
//                     drawn with the counter-based generator of K-DROP: beyond the reference
// Arithmetic follows the host restatement operation by operation (fp32 division, fp32 log1p,
// fp32 square accumulated in fp64) so that host and device inputs agree to the last ulp of
// log1p.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include "dcahip.h"
#include "philox.hpp"

namespace {

constexpr int kMaxRowChunks = 512;

__host__ __device__ inline int prep_chunks(int n) {
    int r = (n + 127) / 128;
    return r < 1 ? 1 : (r > kMaxRowChunks ? kMaxRowChunks : r);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one wave per row
template <int V>
__global__ __launch_bounds__(256) void row_sums_kernel(const float* Y, long ldy, int n, int G, float* out) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    for (int r = wave; r < n; r += nwaves) {
        const float* row = Y + (long)r * ldy;
        double s = 0.0;
        if (V == 4) {
            const int nq = G >> 2;
            for (int q = lane; q < nq; q += 64) {
                const float4 v = reinterpret_cast<const float4*>(row)[q];
                s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
            }
            for (int g = (nq << 2) + lane; g < G; g += 64) s += (double)row[g];
        } else {
            for (int g = lane; g < G; g += 64) s += (double)row[g];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) out[r] = (float)s;
    }
}

struct PassArgs {
    const float* Y; long ldy;
    const float* fac;
    float* X; long ldx;
    double* part;          // [R][2][Gp]
    int n, G, Gp, R;
    int do_log;
};

// grid.x: gene segments (256 lanes x V genes), grid.y: row chunks
template <int V>
__global__ __launch_bounds__(256) void col_pass_kernel(PassArgs a) {
    const int g = (blockIdx.x * 256 + threadIdx.x) * V;
    if (g >= a.G) return;
    const int cr = (a.n + a.R - 1) / a.R;
    const int r0 = blockIdx.y * cr;
    const int r1 = min(a.n, r0 + cr);
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
    for (int r = r0; r < r1; ++r) {
        float v[V];
        const float* src = a.Y + (long)r * a.ldy + g;
        if (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(src);
            v[0] = t.x; v[1 % V] = t.y; v[2 % V] = t.z; v[3 % V] = t.w;
        } else {
            v[0] = src[0];
        }
        const float f = a.fac ? a.fac[r] : 1.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float x = v[j];
            if (a.fac) x = __fdiv_rn(x, f);
            if (a.do_log) x = log1pf(x);
            v[j] = x;
            if (g + j < a.G) {
                s1[j] += (double)x;
                s2[j] += (double)__fmul_rn(x, x);
            }
        }
        if (a.X) {
            float* dst = a.X + (long)r * a.ldx + g;
            if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]);
            else dst[0] = v[0];
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j)
        if (g + j < a.G) {
            a.part[((long)blockIdx.y * 2 + 0) * a.Gp + g + j] = s1[j];
            a.part[((long)blockIdx.y * 2 + 1) * a.Gp + g + j] = s2[j];
        }
}

__global__ __launch_bounds__(256) void col_finish_kernel(const double* part, int R, int Gp, int G,
                                                         double n_total, float* sums, float* mean,
                                                         float* stdv) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    double s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < R; ++r) {
        s1 += part[((long)r * 2 + 0) * Gp + g];
        s2 += part[((long)r * 2 + 1) * Gp + g];
    }
    if (sums) sums[g] = (float)s1;
    if (mean) {
        const double m = s1 / n_total;
        const double msq = s2 / n_total;
        double var = n_total > 1.0 ? (msq - m * m) * (n_total / (n_total - 1.0)) : 0.0;
        if (var < 0.0) var = 0.0;
        double sd = sqrt(var);
        if (sd == 0.0) sd = 1.0;
        mean[g] = (float)m;
        stdv[g] = (float)sd;
    }
}

template <int V>
__global__ __launch_bounds__(256) void scale_kernel(float* X, long ldx, int n, int G, const float* mean,
                                                    const float* stdv) {
    const int nvec = (G + V - 1) / V;
    const long total = (long)n * nvec;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i / nvec);
        const int g = (int)(i - (long)r * nvec) * V;
        float* px = X + (long)r * ldx + g;
        if (V == 4 && g + 4 <= G) {
            float4 v = *reinterpret_cast<float4*>(px);
            const float4 m = *reinterpret_cast<const float4*>(mean + g);
            const float4 s = *reinterpret_cast<const float4*>(stdv + g);
            v.x = __fdiv_rn(v.x - m.x, s.x); v.y = __fdiv_rn(v.y - m.y, s.y);
            v.z = __fdiv_rn(v.z - m.z, s.z); v.w = __fdiv_rn(v.w - m.w, s.w);
            *reinterpret_cast<float4*>(px) = v;
        } else {
            for (int j = 0; j < V && g + j < G; ++j) px[j] = __fdiv_rn(px[j] - mean[g + j], stdv[g + j]);
        }
    }
}

// ---- the row core of the CSR expand and gather kernels -------------------------------------------------------------------
// One workgroup builds one destination row in LDS column segments: zero the segment (seg_clear), scatter the row's entries
// that fall into it (seg_scatter), write it out (seg_store, seg_store_x).  Every kernel below is this loop with its own
// row header, segment type and stores; a further tile format is one more such loop: its own `put` for seg_scatter and its
// own store of the finished segment.
// The contract of all of them: malformed input (unsorted columns, a column outside [0, G), a storage row outside [0, n),
// an indptr that leaves [0, nnz] or decreases) is clamped and counted into *status -- wrong values at worst, never an
// access outside the buffers -- and each element of a tile is written by exactly one plain store: no atomics on a tile.
constexpr int kCsrSeg = 8064;                 // floats per LDS segment (31.5 KiB + the counter: 5 workgroups per CU)

// Resident CSR (counts-resident mode: the counts stay in HBM as CSR, each step builds only its own minibatch).
// indptr is int64 (absolute offsets into indices / values, whose length nnz may exceed 2^31); rows are canonical.
struct GatherArgs {
    const long* indptr; const int* indices; const float* values; long nnz; int n, G;
    const int* perm; const long long* cursor; long row0; int B;
    const float* sf; const float* fac; int do_log; const float* mean; const float* stdv;
    float* Y; long ldy; float* X; long ldx; float* sf_out; int* status;
};

// [s, e) clamped into [0, nnz] and made non-decreasing; true when that changed it
__device__ __forceinline__ bool clamp_span(long s, long e, long nnz, long& s0, long& e0) {
    s0 = s < 0 ? 0 : (s > nnz ? nnz : s);
    e0 = e < s0 ? s0 : (e > nnz ? nnz : e);
    return s0 != s || e0 != e;
}

struct RowSpan { long row; bool ok; long s0, e0; };   // the storage row, whether the CSR has it, its clamped entries

__device__ __forceinline__ long gather_base(const GatherArgs& g) { return g.perm ? (long)*g.cursor : g.row0; }

// Destination row r: storage row perm[*cursor + r] or row0 + r.  A storage row outside [0, n) has no entries; it and a
// clamped span are counted once (thread 0).
__device__ __forceinline__ RowSpan row_span(const GatherArgs& g, long base, int r, int tid, int& bad) {
    RowSpan w;
    w.row = g.perm ? (long)g.perm[base + r] : base + r;
    w.ok = w.row >= 0 && w.row < g.n;
    long s = 0, e = 0;
    if (w.ok) { s = g.indptr[w.row]; e = g.indptr[w.row + 1]; }
    const bool moved = clamp_span(s, e, g.nnz, w.s0, w.e0);
    if (tid == 0 && (!w.ok || moved)) ++bad;
    return w;
}

// The row's normalisation factor f, sf_out[r] and -- where an X tile is written (x) -- t0, the row's transform of a +0
// count: a function of the row only, computed once per row.
__device__ __forceinline__ float row_factor(const GatherArgs& g, const RowSpan& w, int r, int tid, bool x, float& t0) {
    const float f = (g.fac && w.ok) ? g.fac[w.row] : 1.f;
    t0 = 0.f;
    if (x) {
        if (g.fac) t0 = __fdiv_rn(t0, f);
        if (g.do_log) t0 = log1pf(t0);
    }
    if (tid == 0 && g.sf_out) g.sf_out[r] = (w.ok && g.sf) ? g.sf[w.row] : 0.f;
    return f;
}

// x of one element as prep_col_pass + prep_scale write it; the scale applies to the G real columns only (prep_scale leaves
// the pad columns as prep_col_pass wrote them).
__device__ inline float gather_x(float y, float t0, float f, const GatherArgs& a, long col) {
    float t = t0;
    if (__float_as_uint(y) != 0u) {
        t = y;
        if (a.fac) t = __fdiv_rn(t, f);
        if (a.do_log) t = log1pf(t);
    }
    if (a.mean && col < a.G) t = __fdiv_rn(t - a.mean[col], a.stdv[col]);
    return t;
}

// The segment at column c0 of a row of L columns in segments of S: its length, and the first column behind it -- the last
// segment takes every remaining entry (columns >= L are counted, not written); seg_part: what of it lies in a tile of
// leading dimension ld <= L.
__device__ __forceinline__ int seg_len(long L, long c0, int S) { return (int)(L - c0 < S ? L - c0 : S); }
__device__ __forceinline__ long seg_end(long L, long c0, int S) { return c0 + S < L ? c0 + S : (1L << 40); }
__device__ __forceinline__ int seg_part(long ld, long c0, int len) {
    return (int)(ld - c0 < len ? (ld - c0 > 0 ? ld - c0 : 0) : len);
}

// V = 4: 16-byte accesses (len * sizeof(T) is a multiple of 16), V = 1: one element at a time
template <typename T, int V>
__device__ __forceinline__ void seg_clear(T* seg, int len, int tid) {
    if (V == 1) {
        for (int i = tid; i < len; i += 256) seg[i] = T(0);
    } else {
        const int nq = (int)((len * sizeof(T)) >> 4);
        for (int i = tid; i < nq; i += 256) reinterpret_cast<uint4*>(seg)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// The entries of the segment [c0, c0 + len): every thread walks its strided share of the sorted run that starts at p and
// stops at the first column >= c1; put(k, j) places entry j at segment element k, 0 <= k < len.  A column outside [0, G)
// is counted and skipped.  Returns where the next segment's run starts: p + the number of entries the threads found,
// at most e0.  Two barriers: behind the clear, and behind the scatter (the segment is complete when this returns).
template <class Put>
__device__ __forceinline__ long seg_scatter(const int* indices, long p, long e0, long c0, long c1, int len, int G, int tid,
                                            int& bad, int& found, Put put) {
    if (tid == 0) found = 0;
    __syncthreads();
    int mine = 0;
    for (long j = p + tid; j < e0; j += 256) {
        const long c = indices[j];
        if (c >= c1) break;
        ++mine;
        if (c < 0 || c >= G) { ++bad; continue; }
        const long k = c - c0;
        if (k >= 0 && k < len) put(k, j);
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    p += found;
    return p > e0 ? e0 : p;
}

// dst[0 .. n) = seg[0 .. n)
template <typename T, int V>
__device__ __forceinline__ void seg_store(T* dst, const T* seg, int n, int tid) {
    if (V == 1) {
        for (int i = tid; i < n; i += 256) dst[i] = seg[i];
    } else {
        const int nq = (int)((n * sizeof(T)) >> 4);
        for (int i = tid; i < nq; i += 256) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(seg)[i];
    }
}

// dst[0 .. n) = gather_x of the segment's counts; dst[0] is column c0
template <int V>
__device__ __forceinline__ void seg_store_x(float* dst, const float* seg, int n, long c0, float t0, float f,
                                            const GatherArgs& g, int tid) {
    if (V == 4) {
        for (int i = tid; i < (n >> 2); i += 256) {
            const float4 y = reinterpret_cast<const float4*>(seg)[i];
            const long col = c0 + 4 * i;
            float4 x;
            x.x = gather_x(y.x, t0, f, g, col);
            x.y = gather_x(y.y, t0, f, g, col + 1);
            x.z = gather_x(y.z, t0, f, g, col + 2);
            x.w = gather_x(y.w, t0, f, g, col + 3);
            reinterpret_cast<float4*>(dst)[i] = x;
        }
    } else {
        for (int i = tid; i < n; i += 256) dst[i] = gather_x(seg[i], t0, f, g, c0 + i);
    }
}

// CSR expand: rows of an int32 CSR chunk (grid-stride), every element of Y[r, 0 .. ldy) written with V-float stores.
template <int V>
__global__ __launch_bounds__(256) void csr_expand_kernel(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                         const float* __restrict__ values, long nnz, int rows, int G,
                                                         float* __restrict__ Y, long ldy, int* status) {
    __shared__ __attribute__((aligned(16))) float seg[kCsrSeg];
    __shared__ int found;
    const int tid = threadIdx.x;
    int bad = 0;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        long s0, e0;
        if (clamp_span(indptr[r], indptr[r + 1], nnz, s0, e0) && tid == 0) ++bad;
        long p = s0;
        float* yrow = Y + (long)r * ldy;
        for (long c0 = 0; c0 < ldy; c0 += kCsrSeg) {
            const int len = seg_len(ldy, c0, kCsrSeg);
            seg_clear<float, V>(seg, len, tid);
            p = seg_scatter(indices, p, e0, c0, seg_end(ldy, c0, kCsrSeg), len, G, tid, bad, found,
                            [&](long k, long j) { seg[k] = values[j]; });
            seg_store<float, V>(yrow + c0, seg, len, tid);
            __syncthreads();
        }
    }
    if (bad) atomicAdd(status, bad);
}

// CSR gather: one workgroup per destination row r < B (grid-stride); every element of Y[r, 0 .. ldy) and X[r, 0 .. ldx)
// is written (V-float stores when aligned).
template <int V>
__global__ __launch_bounds__(256) void csr_gather_kernel(GatherArgs a) {
    __shared__ __attribute__((aligned(16))) float seg[kCsrSeg];
    __shared__ int found;
    const int tid = threadIdx.x;
    int bad = 0;
    const long base = gather_base(a);
    const long L = (a.X && a.ldx > a.ldy) ? a.ldx : a.ldy;
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        const RowSpan w = row_span(a, base, r, tid, bad);
        float t0;
        const float f = row_factor(a, w, r, tid, true, t0);
        long p = w.s0;
        float* yrow = a.Y + (long)r * a.ldy;
        float* xrow = a.X ? a.X + (long)r * a.ldx : nullptr;
        for (long c0 = 0; c0 < L; c0 += kCsrSeg) {
            const int len = seg_len(L, c0, kCsrSeg);
            seg_clear<float, V>(seg, len, tid);
            p = seg_scatter(a.indices, p, w.e0, c0, seg_end(L, c0, kCsrSeg), len, a.G, tid, bad, found,
                            [&](long k, long j) { seg[k] = a.values[j]; });
            seg_store<float, V>(yrow + c0, seg, seg_part(a.ldy, c0, len), tid);
            if (xrow) seg_store_x<V>(xrow + c0, seg, seg_part(a.ldx, c0, len), c0, t0, f, a, tid);
            __syncthreads();
        }
    }
    if (bad) atomicAdd(a.status, bad);
}

// CSR gather for a network that reads all G input genes and fits G_out of them (train(output_subset=...)): the X tile of
// csr_gather_kernel over the input columns, the Y tile over the OUTPUT columns, Y[r, col_out[g]] = the count of gene g.
struct GatherColsArgs {
    GatherArgs g;                       // g.ldy >= G_out: the Y tile's leading dimension
    const int* col_out; int G_out;      // [G]: output column of input gene g, -1 = not fitted
};

// X pass: the segments of csr_gather_kernel over the input columns.  Y pass: segments of kCsrSeg output columns; output
// order is not input order, so every segment walks all of the row's entries and keeps those whose output column falls
// into it (a gene list is far below kCsrSeg genes: one segment, one walk).  What is counted into *status is counted once
// per entry: a column outside [0, G) in the X pass (without X: in the first Y segment), a col_out value outside
// [-1, G_out) in the first Y segment.
template <int V>
__global__ __launch_bounds__(256) void csr_gather_cols_kernel(GatherColsArgs ca) {
    __shared__ __attribute__((aligned(16))) float seg[kCsrSeg];
    __shared__ int found;
    const GatherArgs& a = ca.g;
    const int tid = threadIdx.x;
    int bad = 0;
    const long base = gather_base(a);
    for (int r = blockIdx.x; r < a.B; r += gridDim.x) {
        const RowSpan w = row_span(a, base, r, tid, bad);
        float t0;
        const float f = row_factor(a, w, r, tid, true, t0);
        if (a.X) {
            long p = w.s0;
            float* xrow = a.X + (long)r * a.ldx;
            for (long c0 = 0; c0 < a.ldx; c0 += kCsrSeg) {
                const int len = seg_len(a.ldx, c0, kCsrSeg);
                seg_clear<float, V>(seg, len, tid);
                p = seg_scatter(a.indices, p, w.e0, c0, seg_end(a.ldx, c0, kCsrSeg), len, a.G, tid, bad, found,
                                [&](long k, long j) { seg[k] = a.values[j]; });
                seg_store_x<V>(xrow + c0, seg, len, c0, t0, f, a, tid);
                __syncthreads();
            }
        }
        float* yrow = a.Y + (long)r * a.ldy;
        for (long c0 = 0; c0 < a.ldy; c0 += kCsrSeg) {
            const int len = seg_len(a.ldy, c0, kCsrSeg);
            const bool count = c0 == 0;
            seg_clear<float, V>(seg, len, tid);
            __syncthreads();
            for (long j = w.s0 + tid; j < w.e0; j += 256) {
                const long c = a.indices[j];
                if (c < 0 || c >= a.G) { if (count && !a.X) ++bad; continue; }
                const long o = ca.col_out[c];
                if (o < -1 || o >= ca.G_out) { if (count) ++bad; continue; }
                const long k = o - c0;
                if (o >= 0 && k >= 0 && k < len) seg[k] = a.values[j];
            }
            __syncthreads();
            seg_store<float, V>(yrow + c0, seg, len, tid);
            __syncthreads();
        }
    }
    if (bad) atomicAdd(a.status, bad);
}

// CSR gather into the byte-store format (the tile the byte-store kernels of K-HEADS and K-SPARSE read): Yc [B, ldc] bytes
// as counts_compact_kernel makes them from csr_gather_kernel's fp32 tile, the tile's overflow list, sf / fac per tile row
// and, optionally, the fp32 X tile of csr_gather_kernel.  Three launches: the gather (which leaves every row's number of
// escapes in ovf_ptr[r + 1]), a one-workgroup prefix sum over them, and the list fill (one wave per row); a caller whose
// dataset holds no count >= 255 passes no list and gets the first launch only.
struct CompactGatherArgs {
    GatherArgs g;                       // the CSR, the rows, the normalisation, X / sf_out / status (g.Y is not used)
    unsigned char* Yc; long ldc;
    int* ovf_ptr; int* ovf_col; float* ovf_val; int cap;
    float* fac_out;
};

constexpr int kCsrSegB = 4 * kCsrSeg;   // columns per LDS segment of the byte-only form (the same 31.5 KiB)

// the byte of one count, as counts_compact_kernel codes it: 0 .. 254, 255 = escape; not a count -> 0 and ++bad
__device__ inline unsigned count_code(float x, int& bad) {
    if (!(x >= 0.f) || x != floorf(x) || x > 16777216.f) { ++bad; return 0u; }
    return x >= 255.f ? 255u : (unsigned)x;
}

__device__ inline int lane_rank64(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// XV = 0: no X tile, the segment holds the bytes themselves (four times the columns per segment); XV = 4 / 1: the segment
// holds the fp32 counts, X is written from them as csr_gather_kernel writes it and the bytes are coded on the way out.
// 16-byte stores of Yc (ldc % 16 == 0; ldx % 4 == 0 where XV = 4).
template <int XV>
__global__ __launch_bounds__(256) void csr_gather_compact_kernel(CompactGatherArgs a) {
    using T = typename std::conditional<XV != 0, float, unsigned char>::type;
    constexpr int kSeg = XV ? kCsrSeg : kCsrSegB;
    constexpr int CV = XV == 1 ? 1 : 4;
    __shared__ __attribute__((aligned(16))) T seg[kSeg];
    __shared__ int found, nesc;
    const GatherArgs& g = a.g;
    const int tid = threadIdx.x;
    int bad = 0;
    const long base = gather_base(g);
    const long L = (XV && g.ldx > a.ldc) ? g.ldx : a.ldc;
    for (int r = blockIdx.x; r < g.B; r += gridDim.x) {
        const RowSpan w = row_span(g, base, r, tid, bad);
        float t0;
        const float f = row_factor(g, w, r, tid, XV != 0, t0);
        if (tid == 0) {
            if (a.fac_out) a.fac_out[r] = f;
            nesc = 0;                   // (the first segment's barrier orders it before the row's additions)
        }
        long p = w.s0;
        unsigned char* crow = a.Yc + (long)r * a.ldc;
        float* xrow = (XV && g.X) ? g.X + (long)r * g.ldx : nullptr;
        for (long c0 = 0; c0 < L; c0 += kSeg) {
            const int len = seg_len(L, c0, kSeg);
            seg_clear<T, CV>(seg, len, tid);
            int esc = 0;
            p = seg_scatter(g.indices, p, w.e0, c0, seg_end(L, c0, kSeg), len, g.G, tid, bad, found, [&](long k, long j) {
                const float v = g.values[j];
                const unsigned code = count_code(v, bad);
                esc += code == 255u;
                if (XV) seg[k] = (T)v; else seg[k] = (T)code;
            });
            if (esc) atomicAdd(&nesc, esc);     // (before the segment's last barrier, which the row's end reads it behind)
            const int lb = seg_part(a.ldc, c0, len);
            if (XV == 0) {
                seg_store<unsigned char, 4>(crow + c0, reinterpret_cast<const unsigned char*>(seg), lb, tid);
            } else {
                for (int i = tid; i < (lb >> 4); i += 256) {
                    unsigned q4[4];
                    int skip = 0;       // (what is not a count was counted when it was scattered)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 y = reinterpret_cast<const float4*>(seg)[4 * i + q];
                        q4[q] = count_code(y.x, skip) | count_code(y.y, skip) << 8 | count_code(y.z, skip) << 16 |
                                count_code(y.w, skip) << 24;
                    }
                    reinterpret_cast<uint4*>(crow + c0)[i] = make_uint4(q4[0], q4[1], q4[2], q4[3]);
                }
            }
            if (XV && xrow)
                seg_store_x<CV>(xrow + c0, reinterpret_cast<const float*>(seg), seg_part(g.ldx, c0, len), c0, t0, f, g, tid);
            __syncthreads();
        }
        if (tid == 0) {
            if (a.ovf_ptr) a.ovf_ptr[r + 1] = nesc;
            else bad += nesc;           // an escape and no list to hold its value
        }
    }
    if (bad) atomicAdd(g.status, bad);
}

// ovf_ptr[1 .. B] hold the rows' escape counts: -> ovf_ptr[0] = 0, ovf_ptr[r + 1] = their running sum, cut at the list's
// capacity (what does not fit is counted, and no consumer is led beyond the list).  One workgroup, in place.
__global__ __launch_bounds__(1024) void ovf_scan_kernel(int* ovf_ptr, int B, int cap, int* status) {
    __shared__ long part[1024];
    const int tid = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int i0 = min(B, tid * per), i1 = min(B, i0 + per);
    long s = 0;
    for (int i = i0; i < i1; ++i) { const int c = ovf_ptr[i + 1]; s += c > 0 ? c : 0; }
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long run = part[tid] - s;
    for (int i = i0; i < i1; ++i) {
        const int c = ovf_ptr[i + 1];
        run += c > 0 ? c : 0;
        ovf_ptr[i + 1] = (int)(run > cap ? cap : run);
    }
    if (tid == 0) ovf_ptr[0] = 0;
    if (tid == 1023 && part[1023] > cap) {
        const long over = part[1023] - cap;
        atomicAdd(status, (int)(over > 0x3fffffffL ? 0x3fffffffL : over));
    }
}

// The tile's overflow list: one wave per destination row walks the row in column order and stores its escapes at
// ovf_ptr[r] ..., never beyond ovf_ptr[r + 1] (<= the capacity).  Rows without an escape leave at once.
__global__ __launch_bounds__(256) void csr_gather_ovf_kernel(CompactGatherArgs a) {
    const GatherArgs& g = a.g;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= g.B) return;
    const int lo = a.ovf_ptr[r], hi = min(a.ovf_ptr[r + 1], a.cap);
    if (lo < 0 || hi <= lo) return;
    int skip = 0;                       // (the gather counted what is wrong with the row and its entries)
    const RowSpan w = row_span(g, gather_base(g), r, lane, skip);
    if (!w.ok) return;
    const long s0 = w.s0, e0 = w.e0;
    int pos = lo;
    for (long j0 = s0; j0 < e0 && pos < hi; j0 += 64) {
        const long j = j0 + lane;
        bool is = false;
        int c = 0;
        float v = 0.f;
        if (j < e0) {
            c = g.indices[j];
            if (c >= 0 && c < g.G) {
                v = g.values[j];
                is = count_code(v, skip) == 255u;
            }
        }
        const unsigned long long m = __ballot(is);
        if (is) {
            const int q = pos + lane_rank64(m);
            if (q < hi) { a.ovf_col[q] = c; a.ovf_val[q] = v; }
        }
        pos += __popcll(m);
    }
}

// Per-gene partials of x and x*x over a resident CSR: one workgroup per row chunk (the chunks of col_pass_kernel), rows in
// ascending order, so every gene receives its non-zero terms in the order col_pass_kernel adds them; the zeros it also adds
// are +0.0 in fp64 and change nothing.  Within a row the columns are distinct (canonical rows), so the threads of the
// workgroup update different genes; the barrier after each row orders the updates of one gene across rows.
__global__ __launch_bounds__(256) void csr_col_pass_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                           const float* __restrict__ values, long nnz, int n, int G, int Gp,
                                                           int R, const float* fac, int do_log, double* part, int* status) {
    const int tid = threadIdx.x;
    const int cr = (n + R - 1) / R;
    const int r0 = blockIdx.x * cr;
    const int r1 = min(n, r0 + cr);
    double* p1 = part + (long)blockIdx.x * 2 * Gp;
    double* p2 = p1 + Gp;
    for (int g = tid; g < G; g += 256) { p1[g] = 0.0; p2[g] = 0.0; }
    __syncthreads();
    int bad = 0;
    for (int r = r0; r < r1; ++r) {
        const long s = indptr[r], e = indptr[r + 1];
        const long s0 = s < 0 ? 0 : (s > nnz ? nnz : s);
        const long e0 = e < s0 ? s0 : (e > nnz ? nnz : e);
        if (tid == 0 && (s0 != s || e0 != e)) ++bad;
        const float f = fac ? fac[r] : 1.f;
        for (long j = s0 + tid; j < e0; j += 256) {
            const long c = indices[j];
            if (c < 0 || c >= G) { ++bad; continue; }
            float x = values[j];
            if (fac) x = __fdiv_rn(x, f);
            if (do_log) x = log1pf(x);
            p1[c] += (double)x;
            p2[c] += (double)__fmul_rn(x, x);
        }
        __syncthreads();
    }
    if (bad) atomicAdd(status, bad);
}

// Per-cell totals over a resident CSR: one wave per row, fp64 (exact for counts, as row_sums_kernel).
__global__ __launch_bounds__(256) void csr_row_sums_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                           const float* __restrict__ values, long nnz, int n, int G, float* out,
                                                           int* status) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    int bad = 0;
    for (int r = wave; r < n; r += nwaves) {
        const long s = indptr[r], e = indptr[r + 1];
        const long s0 = s < 0 ? 0 : (s > nnz ? nnz : s);
        const long e0 = e < s0 ? s0 : (e > nnz ? nnz : e);
        if (lane == 0 && (s0 != s || e0 != e)) ++bad;
        double acc = 0.0;
        for (long j = s0 + lane; j < e0; j += 64) {
            const long c = indices[j];
            if (c < 0 || c >= G) { ++bad; continue; }
            acc += (double)values[j];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) out[r] = (float)acc;
    }
    if (bad) atomicAdd(status, bad);
}

// ---- building and filtering the resident CSR on the device (dcahip_csr_compress, dcahip_csr_subset) ----------------------
// Both are an order-preserving stream compaction in two phases: every output row's number of entries (into ptr[row + 1]),
// one workgroup that turns the counts into offsets (rowptr_scan_kernel), then one plain store per entry at its offset.

// what scipy.sparse.csr_matrix(dense) stores: x != 0 -- not +0.0, not -0.0; a NaN and a subnormal are kept
__device__ inline bool stored(float x) { return (__float_as_uint(x) << 1) != 0u; }

// ptr[1 .. rows] hold the rows' entry counts: -> ptr[0] = base, ptr[r + 1] = base + their running sum.  One workgroup, in
// place; a negative count (never written by the kernels here) counts as 0.
__global__ __launch_bounds__(1024) void rowptr_scan_kernel(long* ptr, int rows, long base) {
    __shared__ long part[1024];
    const int tid = threadIdx.x;
    const int per = (rows + 1023) / 1024;
    const int i0 = min(rows, tid * per), i1 = min(rows, i0 + per);
    long s = 0;
    for (int i = i0; i < i1; ++i) { const long c = ptr[i + 1]; s += c > 0 ? c : 0; }
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long run = base + part[tid] - s;
    for (int i = i0; i < i1; ++i) {
        const long c = ptr[i + 1];
        run += c > 0 ? c : 0;
        ptr[i + 1] = run;
    }
    if (tid == 0) ptr[0] = base;
}

// the V columns a lane holds of dense row `row` from column g on: a 16-byte load (V = 4: the row is 16-byte aligned and
// ld a multiple of 4, so the load stays inside the row's ld floats) whose columns >= G are masked; bit j of the result is
// set when column g + j is stored
template <int V>
__device__ inline unsigned dense_mask(const float* row, int g, int G, float (&v)[4]) {
    unsigned m = 0;
    if (g < G) {
        if (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(row + g);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= (g + j < G && stored(v[j])) ? (1u << j) : 0u;
        } else {
            v[0] = row[g];
            m = stored(v[0]) ? 1u : 0u;
        }
    }
    return m;
}

// phase 1 of csr_compress: one wave per dense row, ptr[r + 1] = the row's number of stored entries
template <int V>
__global__ __launch_bounds__(256) void compress_count_kernel(const float* __restrict__ X, long ld, int rows, int G, long* ptr) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    for (int r = wave; r < rows; r += nwaves) {
        const float* row = X + (long)r * ld;
        int c = 0;
        float v[4];
        for (int g = lane * V; g < G; g += 64 * V) c += __popc(dense_mask<V>(row, g, G, v));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0) ptr[r + 1] = c;
    }
}

// phase 2 of csr_compress: one workgroup per dense row (grid-stride), tiles of 256 * V columns.  Lane l of wave w holds the
// V consecutive columns c0 + (64 w + l) V ..; a ballot per component gives the number of stored entries in the lower lanes
// (the sum of the V mbcnt's), the waves' totals cross in LDS (two alternating slots: one barrier per tile), and the entry
// of column c lands at the row's offset + its rank: column order, one plain store each.  The offsets come from ptr (written
// by rowptr_scan_kernel from the SAME data); a store is made only inside the row's own range and the arrays' capacity, and
// what that refuses is counted into *status.
template <int V>
__global__ __launch_bounds__(256) void compress_store_kernel(const float* __restrict__ X, long ld, int rows, int G, long base,
                                                             const long* __restrict__ ptr, int* __restrict__ indices,
                                                             float* __restrict__ values, long cap, int* status) {
    __shared__ int wtot[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int bad = 0;
    int slot = 0;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = X + (long)r * ld;
        long pos = ptr[r] - base;
        long end = ptr[r + 1] - base;
        if (end > cap) end = cap;
        if (pos < 0) pos = end;                  // (never with the offsets rowptr_scan_kernel wrote: nothing is stored then)
        for (int c0 = 0; c0 < G; c0 += 256 * V) {
            const int g = c0 + tid * V;
            float v[4];
            const unsigned m = dense_mask<V>(row, g, G, v);
            int below = 0, total = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned long long b = __ballot((m >> j) & 1u);
                below += lane_rank64(b);
                total += __popcll(b);
            }
            if (lane == 0) wtot[slot][w] = total;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = wtot[slot][k];
                before += k < w ? t : 0;
                all += t;
            }
            slot ^= 1;
            long q = pos + before + below;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if ((m >> j) & 1u) {
                    if (q < end) { indices[q] = g + j; values[q] = v[j]; }
                    else ++bad;
                    ++q;
                }
            }
            pos += all;
        }
    }
    if (bad) atomicAdd(status, bad);
}

// dst[i] = the number of kept elements in front of i when mask[i] is set, else -1 (the renumbering of the kept columns /
// rows of csr_subset).  One workgroup.  expect >= 0: the number of kept elements the caller sized its output for; another
// total is counted into *status.
__global__ __launch_bounds__(1024) void mask_scan_kernel(const unsigned char* __restrict__ mask, int len, int* dst, int expect,
                                                         int* status) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (len + 1023) / 1024;
    const int i0 = min(len, tid * per), i1 = min(len, i0 + per);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += mask[i] ? 1 : 0;
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = i0; i < i1; ++i) {
        const bool k = mask[i] != 0;
        dst[i] = k ? run : -1;
        run += k ? 1 : 0;
    }
    if (tid == 1023 && expect >= 0 && part[1023] != expect) atomicAdd(status, 1);
}

struct SubsetArgs {
    const long* indptr; const int* indices; const float* values; long nnz; int n, G;
    const int* rowmap; const int* colmap;      // source row -> output row, source column -> output column (-1: dropped;
    int n_out;                                 // NULL: identity)
    long* out_ptr; int* out_indices; float* out_values; long cap; int* status;
};

// One wave per source row (both phases of csr_subset).  STORE = false: out_ptr[dst + 1] = the number of the row's entries
// whose column is kept.  STORE = true: those entries, in the order of the source row, at out_ptr[dst] ...: a ballot per 64
// entries gives the ranks.  Malformed input is clamped and counted as in the other CSR kernels (once: in the count phase).
template <bool STORE>
__global__ __launch_bounds__(256) void csr_subset_kernel(SubsetArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    int bad = 0;
    for (int r = wave; r < a.n; r += nwaves) {
        const int dst = a.rowmap ? a.rowmap[r] : r;
        if (dst < 0) continue;
        if (dst >= a.n_out) { if (!STORE && lane == 0) ++bad; continue; }
        const long s = a.indptr[r], e = a.indptr[r + 1];
        const long s0 = s < 0 ? 0 : (s > a.nnz ? a.nnz : s);
        const long e0 = e < s0 ? s0 : (e > a.nnz ? a.nnz : e);
        if (!STORE && lane == 0 && (s0 != s || e0 != e)) ++bad;
        long pos = 0, end = 0;
        if (STORE) {
            pos = a.out_ptr[dst];
            end = a.out_ptr[dst + 1];
            if (end > a.cap) end = a.cap;
            if (pos < 0) pos = end;
        }
        int cnt = 0;
        for (long j0 = s0; j0 < e0; j0 += 64) {
            const long j = j0 + lane;
            int c = -1;
            if (j < e0) {
                const int cs = a.indices[j];
                if (cs < 0 || cs >= a.G) { if (!STORE) ++bad; }
                else c = a.colmap ? a.colmap[cs] : cs;
            }
            const unsigned long long m = __ballot(c >= 0);
            if (STORE) {
                if (c >= 0) {
                    const long q = pos + lane_rank64(m);
                    if (q < end) { a.out_indices[q] = c; a.out_values[q] = a.values[j]; }
                    else ++bad;
                }
                pos += __popcll(m);
            } else {
                cnt += __popcll(m);
            }
        }
        if (!STORE && lane == 0) a.out_ptr[dst + 1] = cnt;
    }
    if (bad) atomicAdd(a.status, bad);
}

// ---- K-SPLIT: binomial thinning of the resident CSR into two parts (dcahip_csr_thin) -------------------------------------
// Molecule t of the count y of (cell i, gene j) goes to part A when word t & 3 of the Philox block with counter
// (i, j, t >> 2, kPhiloxThinTag) and key = seed is below the threshold (compared in 64 bits: 2^32 keeps every molecule);
// a = the number of such molecules, part A gets a, part B y - a.  a is a function of (seed, i, j, y, threshold) alone.
struct ThinArgs {
    const long* indptr; const int* indices; const float* values; long nnz; int n, G;
    const long* row_ids;
    unsigned long long threshold; unsigned k0, k1;
    long* ptr_a; int* idx_a; float* val_a;
    long* ptr_b; int* idx_b; float* val_b; long cap;
    int* drawn;                                 // [nnz]: a of every stored entry, -1 for an entry neither part takes
    int* status;
};

constexpr unsigned kThinShare = 64;             // counts above it are drawn by the whole wave

// the molecules t of Philox block `blk` (t = 4 blk .. 4 blk + 3, t < y) that go to part A
__device__ __forceinline__ int thin_block(unsigned i, unsigned j, unsigned blk, unsigned y, unsigned long long thr,
                                          unsigned k0, unsigned k1) {
    unsigned o[4];
    philox4x32_10(i, j, blk, kPhiloxThinTag, k0, k1, o);
    const unsigned left = y - 4u * blk;         // >= 1
    int a = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) a += ((unsigned)w < left && (unsigned long long)o[w] < thr) ? 1 : 0;
    return a;
}

// the count of a stored value: true and y in [0, 2^24] for a non-negative integer up to 2^24
__device__ __forceinline__ bool thin_count(float v, unsigned& y) {
    const bool ok = v >= 0.f && v == floorf(v) && v <= 16777216.f;
    y = ok ? (unsigned)v : 0u;
    return ok;
}

// One wave per source row (both phases).  STORE = false: the draws -- a of every entry into drawn[], the number of entries
// with a > 0 into ptr_a[r + 1], with y - a > 0 into ptr_b[r + 1]; malformed input is clamped and counted here, once.
// STORE = true: the entries of both parts at ptr_x[r] ..., in the order of the source row (a ballot per 64 entries gives the
// ranks), a read back from drawn[]: nothing is drawn twice.
template <bool STORE>
__global__ __launch_bounds__(256) void csr_thin_kernel(ThinArgs p) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    int bad = 0;
    for (int r = wave; r < p.n; r += nwaves) {
        const long s = p.indptr[r], e = p.indptr[r + 1];
        long s0, e0;
        const bool moved = clamp_span(s, e, p.nnz, s0, e0);
        if (!STORE && lane == 0 && moved) ++bad;
        const unsigned cell = (unsigned)(p.row_ids ? p.row_ids[r] : (long)r);
        long pa = 0, ea = 0, pb = 0, eb = 0;
        if (STORE) {
            pa = p.ptr_a[r]; ea = p.ptr_a[r + 1];
            if (ea > p.cap) ea = p.cap;
            if (pa < 0) pa = ea;
            pb = p.ptr_b[r]; eb = p.ptr_b[r + 1];
            if (eb > p.cap) eb = p.cap;
            if (pb < 0) pb = eb;
        }
        int cnt_a = 0, cnt_b = 0;
        for (long j0 = s0; j0 < e0; j0 += 64) {
            const long j = j0 + lane;
            int c = 0, a = -1;
            unsigned y = 0;
            if (j < e0) {
                c = p.indices[j];
                const bool okc = c >= 0 && c < p.G;
                const bool okv = thin_count(p.values[j], y);
                if (!STORE) bad += (okc ? 0 : 1) + (okv ? 0 : 1);
                if (!okc) y = 0;
                if (STORE) a = p.drawn[j];
            }
            if (!STORE) {
                // small counts: the lane walks its own entry's blocks
                if (y > 0 && y <= kThinShare) {
                    a = 0;
                    for (unsigned blk = 0; 4u * blk < y; ++blk) a += thin_block(cell, (unsigned)c, blk, y, p.threshold, p.k0, p.k1);
                }
                // large counts: one entry at a time, its blocks dealt round the wave, the 64 partial counts added up
                unsigned long long big = __ballot(y > kThinShare);
                while (big) {
                    const int src = __ffsll((long long)big) - 1;
                    big &= big - 1;
                    const unsigned ys = (unsigned)__shfl((int)y, src, 64);
                    const unsigned cs = (unsigned)__shfl(c, src, 64);
                    const unsigned nblk = (ys + 3u) >> 2;
                    int part = 0;
                    for (unsigned blk = (unsigned)lane; blk < nblk; blk += 64u)
                        part += thin_block(cell, cs, blk, ys, p.threshold, p.k0, p.k1);
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
                    if (lane == src) a = part;
                }
                if (j < e0) p.drawn[j] = y > 0 ? a : -1;
            }
            const bool in_a = y > 0 && a > 0;
            const bool in_b = y > 0 && a >= 0 && (unsigned)a < y;
            const unsigned long long ma = __ballot(in_a), mb = __ballot(in_b);
            if (STORE) {
                if (in_a) {
                    const long q = pa + lane_rank64(ma);
                    if (q < ea) { p.idx_a[q] = c; p.val_a[q] = (float)a; }
                    else ++bad;
                }
                if (in_b) {
                    const long q = pb + lane_rank64(mb);
                    if (q < eb) { p.idx_b[q] = c; p.val_b[q] = (float)(y - (unsigned)a); }
                    else ++bad;
                }
                pa += __popcll(ma);
                pb += __popcll(mb);
            } else {
                cnt_a += __popcll(ma);
                cnt_b += __popcll(mb);
            }
        }
        if (!STORE && lane == 0) { p.ptr_a[r + 1] = cnt_a; p.ptr_b[r + 1] = cnt_b; }
    }
    if (bad) atomicAdd(p.status, bad);
}

// What the three dcahip_csr_gather* entries require alike of their arguments, and the GatherArgs made of them (Y / ldy: the
// fp32 count tile, which each entry checks itself).  False: DCAHIP_EINVAL.
bool gather_args(const long* indptr, const int* indices, const float* values, long nnz, int n, int G, const int* perm,
                 const long long* cursor, long row0, int B, const float* sf, const float* fac, int do_log, const float* mean,
                 const float* stdv, float* Y, long ldy, float* X, long ldx, float* sf_out, int* status, GatherArgs* a) {
    if (n < 0 || G <= 0 || B < 0 || nnz < 0 || !status || !indptr || (nnz > 0 && (!indices || !values))) return false;
    if ((perm && !cursor) || (!perm && row0 < 0) || (X && ldx < G) || (!mean != !stdv) || (sf_out && !sf)) return false;
    *a = GatherArgs{indptr, indices, values, nnz, n, G, perm, cursor, row0, B, sf, fac, do_log, mean, stdv,
                    Y, ldy, X, X ? ldx : 0, sf_out, status};
    return true;
}

inline int gather_grid(int B) { return B < 16384 ? B : 16384; }     // one workgroup per destination row, grid-stride beyond

// V-float stores of both fp32 tiles
inline bool gather_vec(const GatherArgs& a) {
    return al16(a.Y) && (a.ldy & 3) == 0 && (!a.X || (al16(a.X) && (a.ldx & 3) == 0));
}

}  // namespace

extern "C" int dcahip_csr_compress(const float* X, long ld, int rows, int G, long base, long* indptr, int* indices,
                                   float* values, long cap, int* status, void* stream) {
    if (rows < 0 || G <= 0 || ld < G || base < 0 || cap < 0 || !status) return DCAHIP_EINVAL;
    if ((long)rows * G > 0x7fffffffL) return DCAHIP_EINVAL;
    if (rows == 0) return 0;
    if (!X || !indptr || (cap > 0 && (!indices || !values))) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int cgrid = (rows + 3) / 4;
    if (cgrid > 4096) cgrid = 4096;
    const int grid = rows < 16384 ? rows : 16384;
    if (al16(X) && (ld & 3) == 0) {
        hipLaunchKernelGGL(compress_count_kernel<4>, dim3(cgrid), dim3(256), 0, s, X, ld, rows, G, indptr);
        hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, s, indptr, rows, base);
        hipLaunchKernelGGL(compress_store_kernel<4>, dim3(grid), dim3(256), 0, s, X, ld, rows, G, base, indptr, indices, values,
                           cap, status);
    } else {
        hipLaunchKernelGGL(compress_count_kernel<1>, dim3(cgrid), dim3(256), 0, s, X, ld, rows, G, indptr);
        hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, s, indptr, rows, base);
        hipLaunchKernelGGL(compress_store_kernel<1>, dim3(grid), dim3(256), 0, s, X, ld, rows, G, base, indptr, indices, values,
                           cap, status);
    }
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_subset(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                 const unsigned char* row_keep, const unsigned char* col_keep, int n_out, long* out_indptr,
                                 int* out_indices, float* out_values, long cap, int* ws, int* status, void* stream) {
    if (n < 0 || G <= 0 || nnz < 0 || n_out < 0 || n_out > n || cap < 0 || !status || !indptr || !out_indptr)
        return DCAHIP_EINVAL;
    if ((nnz > 0 && (!indices || !values)) || (cap > 0 && (!out_indices || !out_values))) return DCAHIP_EINVAL;
    if ((row_keep || col_keep) && !ws) return DCAHIP_EINVAL;
    if (!row_keep && n_out != n) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int* rowmap = row_keep ? ws : nullptr;
    int* colmap = col_keep ? ws + n : nullptr;
    if (row_keep && n > 0) hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, s, row_keep, n, rowmap, n_out, status);
    if (col_keep) hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, s, col_keep, G, colmap, -1, status);
    SubsetArgs a{indptr, indices, values, nnz, n, G, rowmap, colmap, n_out, out_indptr, out_indices, out_values, cap, status};
    int grid = (n + 3) / 4;
    if (grid > 4096) grid = 4096;
    if (n_out > 0) hipLaunchKernelGGL(csr_subset_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, s, out_indptr, n_out, 0L);
    if (n_out > 0) hipLaunchKernelGGL(csr_subset_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" long dcahip_csr_thin_workspace_bytes(int n, long nnz) {
    if (n < 0 || nnz < 0) return DCAHIP_EINVAL;
    return (nnz * (long)sizeof(int) + 15) & ~15L;
}

extern "C" int dcahip_csr_thin(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                               const long* row_ids, unsigned long long threshold, unsigned long long seed,
                               long* indptr_a, int* indices_a, float* values_a,
                               long* indptr_b, int* indices_b, float* values_b, long cap,
                               void* workspace, int* status, void* stream) {
    if (n < 0 || G <= 0 || nnz < 0 || cap < 0 || threshold > (1ULL << 32) || !status) return DCAHIP_EINVAL;
    if (n == 0) return 0;
    if (!indptr || !indptr_a || !indptr_b || (nnz > 0 && (!indices || !values || !workspace))) return DCAHIP_EINVAL;
    if (cap > 0 && (!indices_a || !values_a || !indices_b || !values_b)) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ThinArgs a{indptr, indices, values, nnz, n, G, row_ids, threshold, (unsigned)seed, (unsigned)(seed >> 32),
               indptr_a, indices_a, values_a, indptr_b, indices_b, values_b, cap, static_cast<int*>(workspace), status};
    int grid = (n + 3) / 4;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(csr_thin_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, s, indptr_a, n, 0L);
    hipLaunchKernelGGL(rowptr_scan_kernel, dim3(1), dim3(1024), 0, s, indptr_b, n, 0L);
    hipLaunchKernelGGL(csr_thin_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_expand(const int* indptr, const int* indices, const float* values, long nnz, int rows, int G,
                                 float* Y, long ldy, int* status, void* stream) {
    if (rows < 0 || G <= 0 || ldy < G || nnz < 0 || nnz > 0x7fffffffL || !status) return DCAHIP_EINVAL;
    if (rows == 0) return 0;
    if (!indptr || !Y || (nnz > 0 && (!indices || !values))) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = rows < 16384 ? rows : 16384;
    if (al16(Y) && (ldy & 3) == 0)
        hipLaunchKernelGGL(csr_expand_kernel<4>, dim3(grid), dim3(256), 0, s, indptr, indices, values, nnz, rows, G, Y, ldy, status);
    else
        hipLaunchKernelGGL(csr_expand_kernel<1>, dim3(grid), dim3(256), 0, s, indptr, indices, values, nnz, rows, G, Y, ldy, status);
    return (int)hipGetLastError();
}

extern "C" int dcahip_prep_chunks(int n) { return prep_chunks(n); }

extern "C" int dcahip_prep_row_sums(const float* Y, long ldy, int n, int G, float* out, void* stream) {
    if (!Y || !out || n <= 0 || G <= 0) return DCAHIP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int grid = (n + 3) / 4;
    if (grid > 4096) grid = 4096;
    if (al16(Y) && (ldy & 3) == 0) hipLaunchKernelGGL(row_sums_kernel<4>, dim3(grid), dim3(256), 0, s, Y, ldy, n, G, out);
    else hipLaunchKernelGGL(row_sums_kernel<1>, dim3(grid), dim3(256), 0, s, Y, ldy, n, G, out);
    return (int)hipGetLastError();
}

extern "C" int dcahip_prep_col_pass(const float* Y, long ldy, int n, int G, const float* fac,
                                    int do_log, float* X, long ldx, double* col_part, void* stream) {
    if (!Y || !col_part || n <= 0 || G <= 0) return DCAHIP_EINVAL;
    const int Gp = (G + 3) & ~3;
    const bool vec = al16(Y) && (ldy & 3) == 0 && ldy >= Gp && (!X || (al16(X) && (ldx & 3) == 0 && ldx >= Gp));
    PassArgs a{Y, ldy, fac, X, ldx, col_part, n, G, Gp, prep_chunks(n), do_log};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) {
        const dim3 grid(((G + 3) / 4 + 255) / 256, a.R);
        hipLaunchKernelGGL(col_pass_kernel<4>, grid, dim3(256), 0, s, a);
    } else {
        const dim3 grid((G + 255) / 256, a.R);
        hipLaunchKernelGGL(col_pass_kernel<1>, grid, dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

extern "C" int dcahip_prep_col_finish(const double* col_part, int R, int G, double n_total,
                                      float* sums, float* mean, float* stdv, void* stream) {
    if (!col_part || R <= 0 || G <= 0 || (mean && !stdv)) return DCAHIP_EINVAL;
    const int Gp = (G + 3) & ~3;
    hipLaunchKernelGGL(col_finish_kernel, dim3((G + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       col_part, R, Gp, G, n_total, sums, mean, stdv);
    return (int)hipGetLastError();
}

extern "C" int dcahip_prep_scale(float* X, long ldx, int n, int G, const float* mean, const float* stdv,
                                 void* stream) {
    if (!X || !mean || !stdv || n <= 0 || G <= 0) return DCAHIP_EINVAL;
    const bool vec = al16(X) && (ldx & 3) == 0 && al16(mean) && al16(stdv);
    const long total = (long)n * ((G + 3) / 4);
    long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(scale_kernel<4>, dim3((int)grid), dim3(256), 0, s, X, ldx, n, G, mean, stdv);
    else hipLaunchKernelGGL(scale_kernel<1>, dim3((int)grid), dim3(256), 0, s, X, ldx, n, G, mean, stdv);
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_gather(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                 const int* perm, const long long* cursor, long row0, int B, const float* sf,
                                 const float* fac, int do_log, const float* mean, const float* stdv, float* Y, long ldy,
                                 float* X, long ldx, float* sf_out, int* status, void* stream) {
    GatherArgs a;
    if (ldy < G || !Y || !gather_args(indptr, indices, values, nnz, n, G, perm, cursor, row0, B, sf, fac, do_log, mean, stdv,
                                      Y, ldy, X, ldx, sf_out, status, &a))
        return DCAHIP_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (gather_vec(a)) hipLaunchKernelGGL(csr_gather_kernel<4>, dim3(gather_grid(B)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(csr_gather_kernel<1>, dim3(gather_grid(B)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_gather_cols(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                      const int* perm, const long long* cursor, long row0, int B, const float* sf,
                                      const float* fac, int do_log, const float* mean, const float* stdv, float* Y, long ldy,
                                      float* X, long ldx, float* sf_out, int* status, const int* col_out, int G_out,
                                      void* stream) {
    GatherColsArgs a{{}, col_out, G_out};
    if (!col_out || G_out <= 0 || ldy < G_out || !Y ||
        !gather_args(indptr, indices, values, nnz, n, G, perm, cursor, row0, B, sf, fac, do_log, mean, stdv, Y, ldy, X, ldx,
                     sf_out, status, &a.g))
        return DCAHIP_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (gather_vec(a.g)) hipLaunchKernelGGL(csr_gather_cols_kernel<4>, dim3(gather_grid(B)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(csr_gather_cols_kernel<1>, dim3(gather_grid(B)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_gather_compact(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                         const int* perm, const long long* cursor, long row0, int B, const float* sf,
                                         const float* fac, int do_log, const float* mean, const float* stdv,
                                         unsigned char* Yc, long ldc, int* ovf_ptr, int* ovf_col, float* ovf_val, int ovf_cap,
                                         float* X, long ldx, float* sf_out, float* fac_out, int* status, void* stream) {
    CompactGatherArgs a{{}, Yc, ldc, ovf_ptr, ovf_col, ovf_val, ovf_ptr ? ovf_cap : 0, fac_out};
    if (ldc < G || (ldc & 15) || !Yc || !al16(Yc) || (fac_out && !fac) || (ovf_ptr && (!ovf_col || !ovf_val || ovf_cap <= 0)) ||
        !gather_args(indptr, indices, values, nnz, n, G, perm, cursor, row0, B, sf, fac, do_log, mean, stdv, nullptr, 0, X, ldx,
                     sf_out, status, &a.g))
        return DCAHIP_EINVAL;
    if (B == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int grid = gather_grid(B);
    if (!X) hipLaunchKernelGGL(csr_gather_compact_kernel<0>, dim3(grid), dim3(256), 0, s, a);
    else if (al16(X) && (ldx & 3) == 0) hipLaunchKernelGGL(csr_gather_compact_kernel<4>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(csr_gather_compact_kernel<1>, dim3(grid), dim3(256), 0, s, a);
    if (ovf_ptr) {
        hipLaunchKernelGGL(ovf_scan_kernel, dim3(1), dim3(1024), 0, s, ovf_ptr, B, a.cap, status);
        hipLaunchKernelGGL(csr_gather_ovf_kernel, dim3((B + 3) / 4), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_col_pass(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                   const float* fac, int do_log, double* col_part, int* status, void* stream) {
    if (!indptr || !col_part || !status || n <= 0 || G <= 0 || nnz < 0 || (nnz > 0 && (!indices || !values)))
        return DCAHIP_EINVAL;
    const int R = prep_chunks(n);
    hipLaunchKernelGGL(csr_col_pass_kernel, dim3(R), dim3(256), 0, static_cast<hipStream_t>(stream), indptr, indices, values,
                       nnz, n, G, (G + 3) & ~3, R, fac, do_log, col_part, status);
    return (int)hipGetLastError();
}

extern "C" int dcahip_csr_row_sums(const long* indptr, const int* indices, const float* values, long nnz, int n, int G,
                                   float* out, int* status, void* stream) {
    if (!indptr || !out || !status || n <= 0 || G <= 0 || nnz < 0 || (nnz > 0 && (!indices || !values)))
        return DCAHIP_EINVAL;
    int grid = (n + 3) / 4;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(csr_row_sums_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), indptr, indices,
                       values, nnz, n, G, out, status);
    return (int)hipGetLastError();
}
