// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator
// of K-DROP (dcahip_dropout.hip) and K-SPLIT (dcahip_prep.hip).  One block = four 32-bit words from a 128-bit counter and a
// 64-bit key; oracle/net_np.py and dca_amd/mcv.py restate it in numpy, pinned on the Random123 known-answer vectors.  The two
// users keep their streams apart through counter word 3: K-DROP puts its layer code there (0 .. 255), K-SPLIT kPhiloxThinTag,
// the k-means++ seeding of K-MEANS (dcahip_kmeans.hip) kPhiloxSeedTag.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr unsigned kPhiloxThinTag = 0x7468696Eu;
constexpr unsigned kPhiloxSeedTag = 0x6B6D2B2Bu;

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                               unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

}  // namespace
