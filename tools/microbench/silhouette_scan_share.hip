// The pair loop of K-SILHOUETTE's scan (dca_amd/csrc/dcahip_silhouette.hip, sil_scan_kernel) over ONE candidate range, in two
// forms, for tools/bench_silhouette.py: MODE 0 adds (double)sqrtf(d2) into a double, as the library does; MODE 1 adds d2 into
// a float -- the same loads, the same d packed operations per pair, without the square root, the conversion and the double
// add.  Their difference is the share of those three in the scan.  Not part of the library; built by the tool into
// tools/_dbg/.  X [n, DP] is zero-padded, grid (query blocks of 256, splits), out [splits, n] double.
#include <hip/hip_runtime.h>
#include "../../dca_amd/csrc/knn_dist.hpp"

namespace {

template <int DP, int MODE>
__global__ __launch_bounds__(256) void scan_share_kernel(const float* __restrict__ xs, int n, int splits, double* out) {
    constexpr int CB = DP <= 32 ? 4 : 2;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = q < n;
    v2f qv[DP / 2];
    const float* qrow = xs + (live ? q : 0) * DP;
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) {
        qv[j].x = qrow[2 * j];
        qv[j].y = qrow[2 * j + 1];
    }
    const long per = ((long)n + splits - 1) / splits;
    const long lo = (long)blockIdx.y * per;
    const long hi = lo + per < n ? lo + per : n;
    double acc = 0.0;
    float facc = 0.f;
    long j = lo;
    for (; j + CB <= hi; j += CB) {
        float d2[CB];
#pragma unroll
        for (int u = 0; u < CB; ++u) d2[u] = dist2<DP>(qv, xs + (j + u) * DP);
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            if (MODE == 0) acc += (double)sqrtf(d2[u]); else facc += d2[u];
        }
    }
    for (; j < hi; ++j) {
        const float d2 = dist2<DP>(qv, xs + j * DP);
        if (MODE == 0) acc += (double)sqrtf(d2); else facc += d2;
    }
    if (live) out[(long)blockIdx.y * n + q] = MODE == 0 ? acc : (double)facc;
}

}  // namespace

extern "C" int scan_share(const float* xs, int n, int dp, int splits, int mode, double* out, void* stream) {
    if (n < 1 || splits < 1 || (dp != 32 && dp != 128) || !xs || !out) return -22;
    const dim3 grid((unsigned)(((long)n + 255) / 256), (unsigned)splits);
    hipStream_t s = (hipStream_t)stream;
    if (dp == 32) {
        if (mode == 0) hipLaunchKernelGGL((scan_share_kernel<32, 0>), grid, dim3(256), 0, s, xs, n, splits, out);
        else hipLaunchKernelGGL((scan_share_kernel<32, 1>), grid, dim3(256), 0, s, xs, n, splits, out);
    } else {
        if (mode == 0) hipLaunchKernelGGL((scan_share_kernel<128, 0>), grid, dim3(256), 0, s, xs, n, splits, out);
        else hipLaunchKernelGGL((scan_share_kernel<128, 1>), grid, dim3(256), 0, s, xs, n, splits, out);
    }
    return (int)hipGetLastError();
}
