// K12 sample quality: bond-graph difference counts and squared deviations of generated structures against their
// reference frame (see include/cgvae_hip.h).
//
// Restates, for a whole evaluation chunk in one launch, what the reference computes per sample on the host with four
// dense [n,n] distance matrices: get_bond_graphs / compare_graph / count_valid_graphs / compute_rmsd
// (scripts/sampling.py:120-239).  No [n,n] tensor exists here: a wave keeps 64 row atoms in registers, stages 64 column
// atoms (reference + generated coordinates, class words) in LDS and tests the 64 x 64 pairs of its tile pair.
// The heavy-atom graph is the heavy x heavy sub-block of the all-atom one (dropH only removes rows / columns, the pair
// cutoffs stay), so one pass over the pairs yields both sets of counts.  The bond matrices are symmetric with an empty
// diagonal: only tile pairs J >= I and, on the diagonal tiles, only j > i are visited; every count is doubled.
#include "cgv_common.h"
#include "sq_dist.h"   // SQ_TILE, SQ_MAX_CLASSES, sq_dist2 (why this file is compiled with -ffp-contract=off), sq_wave_sum

namespace cgv {

// grid: x = tile pairs (I <= J) of the largest frame, y = sample, z = frame; one wave per block.
__global__ __launch_bounds__(64) void sample_quality_k(const float* __restrict__ ref_xyz, const float* __restrict__ gen_xyz,
                                                       const int* __restrict__ frame_ptr, const int* __restrict__ cls,
                                                       const int* __restrict__ heavy, const float* __restrict__ thr_sq,
                                                       int n_atoms, int n_samples, int n_classes, int n_tiles,
                                                       int* __restrict__ counts, double* __restrict__ sums) {
  __shared__ float col[6][SQ_TILE];                         // x y z of the reference, x y z of the sample
  __shared__ int col_cls[SQ_TILE];                          // class | heavy << 16
  __shared__ float thr[SQ_MAX_CLASSES * SQ_MAX_CLASSES];
  const int lane = threadIdx.x, k = blockIdx.y, f = blockIdx.z;
  const int beg = frame_ptr[f], end = frame_ptr[f + 1], n = end - beg;
  if (beg < 0 || n <= 0 || end > n_atoms) return;           // (uniform) an empty or malformed frame keeps its zeros
  int p = blockIdx.x, I = 0;
  while (I < n_tiles && p >= n_tiles - I) { p -= n_tiles - I; ++I; }
  const int J = I + p;
  if (I >= n_tiles || J * SQ_TILE >= n) return;             // (uniform) tile pair outside this frame
  const float* __restrict__ r = ref_xyz + 3 * (size_t)beg;
  const float* __restrict__ g = gen_xyz + 3 * ((size_t)n_samples * (size_t)beg + (size_t)k * (size_t)n);
  const int* __restrict__ c = cls + beg;
  const int* __restrict__ h = heavy + beg;
  const int out = f * n_samples + k;

  // column tile + threshold table -> LDS
  const int j = J * SQ_TILE + lane;
  if (j < n) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      col[d][lane] = r[3 * j + d];
      col[3 + d][lane] = g[3 * j + d];
    }
    col_cls[lane] = min(max(c[j], 0), n_classes - 1) | (h[j] != 0 ? 0x10000 : 0);
  }
  for (int t = lane; t < n_classes * n_classes; t += SQ_TILE) thr[t] = thr_sq[t];
  // row atom of this lane
  const int i = I * SQ_TILE + lane;
  const bool row = i < n;
  const int ii = row ? i : n - 1;
  const float rx = r[3 * ii], ry = r[3 * ii + 1], rz = r[3 * ii + 2];
  const float gx = g[3 * ii], gy = g[3 * ii + 1], gz = g[3 * ii + 2];
  const int ci = min(max(c[ii], 0), n_classes - 1);
  const bool hi = h[ii] != 0;
  __syncthreads();

  int diff_a = 0, diff_h = 0, sgn_a = 0, sgn_h = 0, ref_a = 0, ref_h = 0;
  const int cols = min(SQ_TILE, n - J * SQ_TILE);
  const int first = (I == J) ? lane + 1 : 0;                // diagonal tile: j > i only
#pragma unroll 4
  for (int t = 0; t < cols; ++t) {
    const int w = col_cls[t];
    // the table is symmetric: [column class][row class] puts the lanes of one read on consecutive words
    const float s_star = thr[(w & 0xffff) * n_classes + ci];
    const bool on = row && t >= first;
    const int br = (on && sq_dist2(rx, ry, rz, col[0][t], col[1][t], col[2][t]) <= s_star) ? 1 : 0;
    const int bg = (on && sq_dist2(gx, gy, gz, col[3][t], col[4][t], col[5][t]) <= s_star) ? 1 : 0;
    const int both = (hi && (w >> 16)) ? 1 : 0;
    diff_a += br ^ bg;
    sgn_a += br - bg;
    ref_a += br;
    diff_h += both & (br ^ bg);
    sgn_h += both * (br - bg);
    ref_h += both & br;
  }
  int v[6] = {diff_a, diff_h, sgn_a, sgn_h, ref_a, ref_h};
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const int tot = sq_wave_sum(v[q]);
    if (lane == 0 && tot != 0) atomicAdd(counts + 6 * (size_t)out + q, 2 * tot);   // integer: exact in any order
  }

  // squared deviations: the block of tile pair (0, 0) walks all atoms of the frame in a fixed order (no fp64 atomics:
  // the sums do not depend on how the launch was cut into blocks)
  if (I == 0 && J == 0) {
    double all = 0.0, hv = 0.0;
    for (int a = lane; a < n; a += SQ_TILE) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double dd = (double)g[3 * a + d] - (double)r[3 * a + d];      // float64 positions (sampling.py:228-232)
        s += dd * dd;
      }
      all += s;
      if (h[a] != 0) hv += s;
    }
    all = sq_wave_sum(all);
    hv = sq_wave_sum(hv);
    if (lane == 0) {
      sums[2 * (size_t)out] = all;
      sums[2 * (size_t)out + 1] = hv;
    }
  }
}

}  // namespace cgv

extern "C" {

int cgv_sample_quality_max_classes(void) { return cgv::SQ_MAX_CLASSES; }

int cgv_sample_quality(const float* ref_xyz, const float* gen_xyz, const int32_t* frame_ptr, const int32_t* cls,
                       const int32_t* heavy, const float* thr_sq, int n_frames, int n_atoms, int n_samples, int n_classes,
                       int max_frame_atoms, int32_t* counts, double* sums, void* stream) {
  CGV_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_samples >= 0, "bad size");
  if (n_frames == 0 || n_samples == 0) return 0;
  CGV_REQUIRE(counts && sums && frame_ptr, "null pointer");
  CGV_REQUIRE(n_classes >= 1 && n_classes <= cgv::SQ_MAX_CLASSES, "1 <= n_classes <= cgv_sample_quality_max_classes()");
  CGV_REQUIRE(max_frame_atoms >= 0 && max_frame_atoms <= n_atoms && max_frame_atoms <= cgv::SQ_MAX_FRAME_ATOMS,
              "max_frame_atoms must be the largest frame's atom count (<= 32768)");
  CGV_REQUIRE(n_frames <= 65535 && n_samples <= 65535, "at most 65535 frames and 65535 samples per launch");
  CGV_REQUIRE((((uintptr_t)sums) & 7) == 0, "sums must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t units = (size_t)n_frames * (size_t)n_samples;
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 6 * units, st);
  if (e == hipSuccess) e = hipMemsetAsync(sums, 0, sizeof(double) * 2 * units, st);
  if (e != hipSuccess) {
    cgv::set_error("cgv_sample_quality: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (max_frame_atoms == 0) return 0;
  CGV_REQUIRE(ref_xyz && gen_xyz && cls && heavy && thr_sq, "null pointer");
  const int n_tiles = (max_frame_atoms + cgv::SQ_TILE - 1) / cgv::SQ_TILE;
  const long long pairs = (long long)n_tiles * (n_tiles + 1) / 2;
  hipLaunchKernelGGL(cgv::sample_quality_k, dim3((unsigned)pairs, (unsigned)n_samples, (unsigned)n_frames), dim3(64), 0, st,
                     ref_xyz, gen_xyz, frame_ptr, cls, heavy, thr_sq, n_atoms, n_samples, n_classes, n_tiles, counts, sums);
  return cgv::check_launch("cgv_sample_quality");
}

}  // extern "C"
