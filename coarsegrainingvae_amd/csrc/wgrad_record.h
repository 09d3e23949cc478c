// The problem record of the grouped weight-gradient launches and what every family that walks a table of them
// shares (wgrad_grouped.hip, wgrad_gram.hip, wgrad_gathered.hip).
#pragma once
#include "cgv_common.h"

namespace cgv {

struct WgradProblem {       // mirrors the 88-byte host record built in python (primitives.WeightGradQueue)
  const float* gy;
  const float* x;
  const float* z;           // pre-activation or NULL
  float* gW;
  float* gb;                // or NULL
  int M, N, K;
  int accumulate, act;
  int block_begin;          // first global block index of this problem
  int tiles_k;              // k tiles per row block
  int tile_w;               // floats per k tile (multiple of 4)
  int seg_rows;             // gathered operands (gathered_wgrad_k): rows per rank segment (multiple of 4) ...
  int seg_stride;           // ... and floats between the segments of consecutive ranks; 0 / 0 = one plain [M, .] block
  int pad;
};
static_assert(sizeof(WgradProblem) == 88, "host/device record layout");
// float offset of operand row m (rows of `width` floats): one plain [M, width] block, or -- gathered operands -- rank
// segment m / seg_rows of the all-gathered buffer
__device__ __forceinline__ size_t wg_row(const WgradProblem& pr, int m, int width) {
  if (pr.seg_rows <= 0) return (size_t)m * width;
  const int seg = m / pr.seg_rows;
  return (size_t)seg * pr.seg_stride + (size_t)(m - seg * pr.seg_rows) * width;
}

// The record of this block: block_begin is ascending, so the index is the number of records that begin at or before
// blockIdx.x, minus one -- every lane reads one record's block_begin (64 records per round trip) and a ballot counts.
// (The binary search this replaces was log2(n) DEPENDENT global loads in front of every block's work: 6 at the 57
// problems of a chignolin step.)
template <typename Problem>
__device__ __forceinline__ int wg_find_problem(const Problem* __restrict__ table, int n_problems, int block) {
  const int lane = threadIdx.x & 63;
  int count = 0;
  for (int base = 0; base < n_problems; base += 64) {
    const int i = base + lane;
    const int bb = i < n_problems ? table[i].block_begin : 0x7fffffff;
    count += __popcll(__ballot(bb <= block));
  }
  return __builtin_amdgcn_readfirstlane(count > 0 ? count - 1 : 0);
}
template <typename Problem>
__device__ __forceinline__ int wg_find_problem(const Problem* __restrict__ table, int n_problems) {
  return wg_find_problem(table, n_problems, (int)blockIdx.x);
}

// Rank update (ADAM = true): the tile of gW is never stored -- it goes, clipped, straight into the Adam update of the
// weights it belongs to.  A bead-level layer sees M = 12 rows against 0.36 - 3.2 M weights: its gradient g^T x has rank
// <= 12 and costs 12 FMAs per weight to form, against 12 bytes per weight to write it, read it for the norm and read it
// again in the parameter pass.  The norm comes from the operands instead (wgrad_gram_k), so the step moves 24 bytes per
// weight of these layers (p, m, v read + written) instead of 36.  The arenas are addressed through gW's offset in the
// gradient arena: p = arena_p + (gW - arena_g), likewise m and v.
struct RankUpdateArgs {
  const float* arena_g;
  float* arena_p;
  float* arena_m;
  float* arena_v;
  const float* state;
  float lr, beta1, beta2, eps;
};

// Rows: a single GPU's bead-level layers have 12 (<= 40: the LDS request stays below 64 KB, two blocks per CU); the
// gathered operands of the data-parallel exchange have world x 12 -- up to 64 (cgv_rank_update_supported), beyond
// which walking M^2 / 2 row pairs and re-forming the tiles stops paying against materialising the gradient.
constexpr int GRAM_MAX_ROWS = 64;

}  // namespace cgv
