// Device helpers shared by the GEMM-like kernels (skinny_gemm.hip, wgrad_grouped.hip, wgrad_gram.hip,
// wgrad_gathered.hip): the MFMA accumulator type and loads / stores through address space 1.
#pragma once
#include "cgv_common.h"

namespace cgv {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Pointers that come out of a record table are generic to the compiler: loads and stores through them are flat_*, which
// count on lgkmcnt as well as vmcnt -- an LDS wait then also waits for them.  These go through address space 1 (global_*).
typedef float gf32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldg4_global(const float* p) {
  const gf32x4 t = *reinterpret_cast<const __attribute__((address_space(1))) gf32x4*>((const __attribute__((address_space(1))) float*)p);
  return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float ldg_global(const float* p) {
  return *((const __attribute__((address_space(1))) float*)p);
}
__device__ __forceinline__ void stg4_global(float* p, const float4& v) {
  *reinterpret_cast<__attribute__((address_space(1))) gf32x4*>((__attribute__((address_space(1))) float*)p) = gf32x4{v.x, v.y, v.z, v.w};
}

}  // namespace cgv
