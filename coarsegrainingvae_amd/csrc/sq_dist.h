// The bond test shared by the sample-quality kernels (K12 sample_quality.hip, K14 ensemble_check.hip): tile size, class
// limit, the bit-reproducible squared distance and the fixed-tree wave sums.
#pragma once
#include "cgv_common.h"

namespace cgv {

constexpr int SQ_TILE = 64;              // atoms per tile = lanes of the wave that owns the rows
constexpr int SQ_MAX_CLASSES = 32;       // element classes of one launch (threshold table [T,T] in LDS)
constexpr int SQ_MAX_FRAME_ATOMS = 32768;  // 2 * pairs of one frame stay below 2^31

// (dx*dx + dy*dy) + dz*dz, every operation individually rounded: bitwise the host's `.pow(2).sum(-1)` (as K0's pair_hit).
// EVERY FILE THAT INCLUDES THIS IS COMPILED WITH -ffp-contract=off (build.py: SOURCE_FLAGS).  Under the library's
// -ffp-contract=fast the _rn intrinsics are plain operators to the compiler and the backend fuses the products into the
// sums (v_fma_f32) whatever a pragma says: the last bit of s changes and with it the membership of a pair that sits on
// its threshold.
__device__ __forceinline__ float sq_dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ int sq_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  return v;                                 // lane 0 holds the sum
}
__device__ __forceinline__ double sq_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);   // fixed tree: the same bits on every run
  return v;
}

}  // namespace cgv
