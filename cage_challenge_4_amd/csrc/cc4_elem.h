// cc4_elem.h -- the element types of the caller's tensors in the kernels that take one of three dtypes (cc4_k_logp.hip, cc4_k_gae.hip): the dtype
// codes of cc4_policy_outputs (1 float16, 2 bfloat16, 3 float32) as a template argument, an element to float32 exactly and back rounded to nearest
// even.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <int DT> struct LpElem { using type = uint16_t; };
template <> struct LpElem<3> { using type = float; };
template <int DT> __device__ __forceinline__ float lp_to_float(typename LpElem<DT>::type v) {
  if constexpr (DT == 3) return v;
  else if constexpr (DT == 2) return __uint_as_float((uint32_t)v << 16);
  else { _Float16 h; __builtin_memcpy(&h, &v, 2); return (float)h; }
}
// ... and back, rounded to nearest even (a NaN stays a quiet NaN)
template <int DT> __device__ __forceinline__ typename LpElem<DT>::type lp_from_float(float v) {
  if constexpr (DT == 3) return v;
  else if constexpr (DT == 2) {
    const uint32_t u = __float_as_uint(v);
    if (v != v) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  } else { const _Float16 h = (_Float16)v; uint16_t r; __builtin_memcpy(&r, &h, 2); return r; }
}
