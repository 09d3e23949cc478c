// The bit-reproducible squared distance and the fixed-tree wave sums of every kernel whose integers or fp64 sums the host
// restates bit for bit, and the tile size and class limit of the sample-quality kernels' bond test.  Who includes it, and why
// each of them has its entry in build.py's SOURCE_FLAGS:
//   K12 sample_quality.hip, K14 ensemble_check.hip   sq_dist2 against host-derived bond thresholds; the wave sums
//   K16 tica.hip                                     a feature is sqrtf(sq_dist2), restated in numpy.float32
//   K20 contact_map.hip                              sq_dist2 < cutoff2; rg2 through sq_wave_sum(double)
//   K23 sasa.hip                                     sq_dist2 of a rounded sphere point against a rounded r * r
//   K25 hbond.hip                                    sq_dist2 against a cutoff, and a rounded dot product beside it
//   K26 dssp.hip                                     sq_dist2 beside its rounded reciprocal distances
//   K27 pca.hip (through gram_dev.h)                 sq_wave_sum(double) alone; its own fp64 feature needs the flag as well
//   K28 lddt.hip                                     sqrtf(sq_dist2) of a model against that of its reference; the wave sum
//   K29 pair_hist.hip                                the bin of sqrtf(sq_dist2) times a host-made scale; sq_dist2 < rmax2
//   K30 dist_moments.hip                             sqrtf(sq_dist2) minus a centre and its square, rounded to fixed point; the wave sum
//   K31 stereo.hip (through packed_dev.h)            not the distance: the signs of rounded cross and dot products, restated the same way
//   K32 relax.hip (through packed_dev.h)             sq_dist2 as the q of every force and of K28's clash test; the wave sums of its energy
//   K33 saxs_hist.hip                                K29's bin of sqrtf(sq_dist2) and sq_dist2 < rmax2, per structure and weighted
// packed_dev.h and gram_dev.h stand on the same contract.
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
// lane 0 holds the sum.  A fixed tree: the same bits on every run.  An xor tree (every lane holds the sum) gives lane 0
// the same bits: at step d lane 0 adds lane d's value, and in both trees lane d's value was formed at the steps d' > d from
// lanes d + d' <= 63 (in range, and d ^ d' = d + d') in the same pairing.
__device__ __forceinline__ double sq_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
  return v;
}

}  // namespace cgv
