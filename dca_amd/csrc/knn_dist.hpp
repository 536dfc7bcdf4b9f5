// What the three latent-space kernels share -- K-NEIGHBOURS (dcahip_knn.hip), K-MEANS (dcahip_kmeans.hip) and K-SILHOUETTE
// (dcahip_silhouette.hip): the squared Euclidean distance, one definition, so that a (point, centre) pair gets the bits the
// neighbour search gives it, and the small helpers around it (the padded row length, 16-byte workspace offsets, the test for
// a non-finite float).  d2 = s0 + s1, s_p = fma(a_j - b_j, a_j - b_j, s_p) over the j of parity p ascending, fp32: a function
// of d alone (rows zero-padded to DP add +0 exactly), symmetric bit for bit, never negative, 0 for equal rows.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr unsigned kInfBits = 0x7F800000u;

inline int pad_d(int d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : 128; }
inline long r16(long x) { return (x + 15) / 16 * 16; }

__device__ __forceinline__ int nonfinite(float v) { return (__float_as_uint(v) & kInfBits) == kInfBits ? 1 : 0; }

typedef float v2f __attribute__((ext_vector_type(2)));

template <int DP>
__device__ __forceinline__ float dist2(const v2f (&q)[DP / 2], const float* __restrict__ x) {
    v2f acc = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < DP / 2; ++j) {
        const v2f xv = {x[2 * j], x[2 * j + 1]};
        const v2f df = q[j] - xv;
        acc = __builtin_elementwise_fma(df, df, acc);
    }
    return acc.x + acc.y;
}

}  // namespace
