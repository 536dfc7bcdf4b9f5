// What the two likelihood sources share beside the element arithmetic of zinb_math.hpp (dcahip_zinb.hip: the training and
// validation likelihood; dcahip_score.hip: the passes over a fitted model): V-wide global access, the test for 16-byte
// vector operands and the (HAS_PI, CONST_DISP) template dispatch.  gfx950, wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace {

template <int V>
__device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
    if (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); o[0] = t.x; o[1 % V] = t.y; o[2 % V] = t.z; o[3 % V] = t.w; }
    else o[0] = *p;
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&o)[V]) {
    if (V == 4) *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
    else *p = o[0];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// whether the operands a likelihood pass READS under (has_pi, cdisp, loss) take 16-byte accesses: row strides of whole quads
// that hold roundup4(G) columns, every pointer the flags read aligned
inline bool nll_reads_vec(const float* a_mean, const float* a_disp, const float* a_pi, long lda, const float* theta_w,
                          const float* y, long ldy, int G, bool has_pi, bool cdisp, int loss) {
    return (lda % 4 == 0) && (ldy % 4 == 0) && al16(a_mean) && al16(y) &&
           (loss != 0 || (cdisp ? al16(theta_w) : al16(a_disp))) && (!has_pi || al16(a_pi)) &&
           lda >= ((G + 3) & ~3) && ldy >= ((G + 3) & ~3);
}

// f(P, C) with the two flags as std::bool_constant values: kernel<P.value, C.value> inside a generic lambda
template <class F>
auto dispatch_pc(bool has_pi, bool cdisp, F&& f) {
    if (has_pi && cdisp) return f(std::true_type{}, std::true_type{});
    if (has_pi) return f(std::true_type{}, std::false_type{});
    if (cdisp) return f(std::false_type{}, std::true_type{});
    return f(std::false_type{}, std::false_type{});
}

}  // namespace
