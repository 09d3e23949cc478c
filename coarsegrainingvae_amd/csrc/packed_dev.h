// What the pair kernels that stream a packed copy [S, P] float4 of every structure share (K20 contact_map.hip, K25
// hbond.hip, K28 lddt.hip, K29 pair_hist.hip, K30 dist_moments.hip): the rule that cuts the structure axis into slices, the walk over the tiles above the
// diagonal, and the per-structure counters of the chunk of structures a block stages at a time.  Only integers here, but EVERY FILE THAT INCLUDES THIS IS COMPILED WITH -ffp-contract=off
// (build.py: SOURCE_FLAGS): the predicates beside it are restated on the host bit for bit.
#pragma once
#include "cgv_common.h"

namespace cgv {

constexpr int PACKED_TARGET_BLOCKS = 1024;   // 4 blocks on each of 256 CUs
constexpr int PACKED_MIN_SLICE = 64;         // structures of a slice at least: a slice ends in an atomic or two per counted pair

// how many slices the structure axis is cut into for `tiles` independent pieces of work, and the structures of a slice (a
// multiple of `quantum`, the structures a block takes at a time)
static inline int struct_slices(int S, int tiles, int quantum, int* per) {
  int want = (PACKED_TARGET_BLOCKS + tiles - 1) / tiles;
  const int most = (S + PACKED_MIN_SLICE - 1) / PACKED_MIN_SLICE;
  if (want > most) want = most;
  if (want < 1) want = 1;
  int p = (S + want - 1) / want;
  p = (p + quantum - 1) / quantum * quantum;
  *per = p;
  return (S + p - 1) / p;
}

// The pair kernels that take every unordered pair once walk the tiles that hold a pair i < j (K20 contact_map.hip, K29
// pair_hist.hip): rows r0 .. r0 + rows - 1 against columns c0 .. c0 + cols - 1.  A tile is live when its last column is above
// its first row; upper_live_tiles counts them for struct_slices
__host__ __device__ __forceinline__ bool upper_tile_live(int r0, int c0, int cols) { return c0 + cols - 1 > r0; }
static inline int upper_live_tiles(int nr, int nc, int rows, int cols) {
  int live = 0;
  for (int r = 0; r < nr; ++r) {
    const int first = (r * rows + 1) / cols;                 // the first column tile with (c + 1) * cols - 1 > r * rows
    if (first < nc) live += nc - first;
  }
  return live;
}
// bit u: column cb + u is inside the selection of m atoms and above `row` (row < m, cb < m, cb a multiple of 32: one word of
// a mask [m, ceil(m / 32)])
__device__ __forceinline__ uint32_t upper_pair_word(int row, int cb, int m) {
  const uint32_t inside = m - cb >= 32 ? 0xffffffffu : (1u << (m - cb)) - 1u;
  const uint32_t above = row < cb ? 0xffffffffu : row >= cb + 31 ? 0u : 0xffffffffu << (row - cb + 1);
  return inside & above;
}

// The LDS counters of a pair kernel for the CHUNK structures s0 .. s0 + CHUNK - 1 it has staged: per structure the pairs that
// count and the native ones among them.  zero() between the chunk loop's two barriers, add() from the pair loop
template <int CHUNK>
struct ChunkHits {
  int hits[2][CHUNK];
  __device__ __forceinline__ void zero(int tid) { if (tid < 2 * CHUNK) hits[tid / CHUNK][tid % CHUNK] = 0; }
  __device__ __forceinline__ void add(int which, int sl, int v) { atomicAdd(&hits[which][sl], v); }
  __device__ __forceinline__ void flush(int s0, int s_end, int tid, int* __restrict__ n_all, int* __restrict__ n_native) {
    if (tid < 2 * CHUNK) {
      const int which = tid / CHUNK, sl = tid % CHUNK, v = hits[which][sl];
      if (v != 0 && s0 + sl < s_end) atomicAdd((which ? n_native : n_all) + s0 + sl, v);
    }
  }
};

// ChunkHits' sibling for a kernel with N counters per structure, laid out as the caller's table [S, N] (K28 lddt.hip: N = 6)
template <int CHUNK, int N>
struct ChunkCounts {
  int v[CHUNK][N];
  __device__ __forceinline__ void zero(int tid) { if (tid < CHUNK * N) v[tid / N][tid % N] = 0; }
  __device__ __forceinline__ void add(int sl, int k, int x) { atomicAdd(&v[sl][k], x); }
  __device__ __forceinline__ void flush(int s0, int s_end, int tid, int* __restrict__ table) {
    if (tid < CHUNK * N) {
      const int sl = tid / N, k = tid % N, x = v[sl][k];
      if (x != 0 && s0 + sl < s_end) atomicAdd(table + (size_t)(s0 + sl) * N + k, x);
    }
  }
};

}  // namespace cgv
