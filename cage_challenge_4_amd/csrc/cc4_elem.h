// cc4_elem.h -- the element types of the caller's tensors in the kernels that take one of three dtypes (cc4_k_sample.hip, cc4_k_logp.hip,
// cc4_k_gae.hip): the dtype codes of cc4_policy_outputs (1 float16, 2 bfloat16, 3 float32) as a template argument, an element to float32 exactly
// and back rounded to nearest even; and the load of one element where the code is a run-time value.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <int DT> struct Elem { using type = uint16_t; };
template <> struct Elem<3> { using type = float; };
template <int DT> __device__ __forceinline__ float elem_to_float(typename Elem<DT>::type v) {
  if constexpr (DT == 3) return v;
  else if constexpr (DT == 2) return __uint_as_float((uint32_t)v << 16);
  else { _Float16 h; __builtin_memcpy(&h, &v, 2); return (float)h; }
}
// ... and back, rounded to nearest even (a NaN stays a quiet NaN)
template <int DT> __device__ __forceinline__ typename Elem<DT>::type elem_from_float(float v) {
  if constexpr (DT == 3) return v;
  else if constexpr (DT == 2) {
    const uint32_t u = __float_as_uint(v);
    if (v != v) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  } else { const _Float16 h = (_Float16)v; uint16_t r; __builtin_memcpy(&r, &h, 2); return r; }
}
// element f of a row whose dtype code is known at run time only (the two 16-bit types share their load)
__device__ __forceinline__ float elem_load(const void* row, int dtype, int f) {
  if (dtype == 3) return elem_to_float<3>(static_cast<const float*>(row)[f]);
  const uint16_t h = static_cast<const uint16_t*>(row)[f];
  return dtype == 2 ? elem_to_float<2>(h) : elem_to_float<1>(h);
}
