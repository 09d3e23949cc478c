// What the pair kernels that stream a packed copy [S, P] float4 of every structure share.  EVERY FILE THAT INCLUDES THIS IS
// COMPILED WITH -ffp-contract=off (build.py: SOURCE_FLAGS): the centroid here and the predicates beside it are restated on
// the host bit for bit.
//   host     struct_slices, upper_live_tiles, pair_grid      how a launch cuts tiles and the structure axis into blocks
//            workspace_why                                   the three conditions on a caller's workspace
//   prepare  gather_structure, poison_row                    one wave packs one structure, tests it, sums its centroid
//   pairs    upper_tile_live, word_inside, word_above,       which pairs are a block's, a thread's
//            upper_pair_word, upper_pair_bits
//            stage_chunk                                     CHUNK structures of a tile's rows and columns into LDS
//            ChunkCounts                                     per-structure counters of the staged chunk
// Who uses what (x: all of it; the rest stays local for the reason DESIGN.md section 4 gives):
//   K20 contact_map.hip   x (contact_groups_k: struct_slices alone)
//   K25 hbond.hip         gather_structure, poison_row, ChunkCounts, struct_slices, workspace_why (rows and columns are two tables)
//   K28 lddt.hip          all but stage_chunk (it stages a model and its reference in one loop) and upper_pair_bits (ordered pairs)
//   K29 pair_hist.hip     all but ChunkCounts (its counters are the histogram)
//   K30 dist_moments.hip  x
//   K31 stereo.hip        gather_structure, poison_row, ChunkCounts, struct_slices, workspace_why (its tables are quadruples and a
//                         rectangle of rings against bonds, not pairs of one selection; it does not include sq_dist.h's distance)
//   K32 relax.hip         word_inside alone, with sq_dist.h's sq_dist2 and sq_wave_sum.  It streams no packed copy: a structure
//                         is loaded once into LDS and stays there for all steps, every atom against every atom, so there is no
//                         workspace (workspace_why), no tile or slice (struct_slices, pair_grid, stage_chunk, upper_*), no
//                         selection (gather_structure), and its per-structure results are written once, not counted (ChunkCounts)
//   K33 saxs_hist.hip     gather_structure, upper_tile_live, upper_pair_bits, workspace_why.  Its histograms are one per
//                         structure, so a block stays with ONE structure and the structure axis is not cut (struct_slices,
//                         pair_grid) or staged in chunks (stage_chunk: its staged float4 carries the atom's weight in w), and
//                         its counters are the histogram (ChunkCounts)
#pragma once
#include <math.h>

#include "sq_dist.h"

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

// The pair kernels that take every unordered pair once walk the tiles that hold a pair i < j: rows r0 .. r0 + rows - 1
// against columns c0 .. c0 + cols - 1.  A tile is live when its last column is above its first row; upper_live_tiles counts
// them for struct_slices
__host__ __device__ __forceinline__ bool upper_tile_live(int r0, int c0, int cols) { return c0 + cols - 1 > r0; }
static inline int upper_live_tiles(int nr, int nc, int rows, int cols) {
  int live = 0;
  for (int r = 0; r < nr; ++r) {
    const int first = (r * rows + 1) / cols;                 // the first column tile with (c + 1) * cols - 1 > r * rows
    if (first < nc) live += nc - first;
  }
  return live;
}
// the grid of a pair kernel over m x m atoms in tiles of rows x cols -- x = column tile, y = row tile, z = slice of the
// structure axis -- and the structures of a slice, a multiple of `chunk`.  `full`: every tile works (ordered pairs), not
// only the live ones
static inline dim3 pair_grid(int S, int m, int rows, int cols, int chunk, bool full, int* per) {
  const int nr = (m + rows - 1) / rows, nc = (m + cols - 1) / cols;
  const int slices = struct_slices(S, full ? nr * nc : upper_live_tiles(nr, nc, rows, cols), chunk, per);
  return dim3((unsigned)nc, (unsigned)nr, (unsigned)slices);
}

// nullptr for a workspace a kernel can take; else the message: the caller's own where it is missing or too small
static inline const char* workspace_why(const void* workspace, size_t bytes, size_t need, const char* too_small) {
  if (!workspace || bytes < need) return too_small;
  if (((uintptr_t)workspace & 15) != 0) return "workspace must be 16-byte aligned";
  return nullptr;
}

// One wave gathers the P table atoms at(0) .. at(P - 1) of the structure at `base` [n, 3] into its packed `row` (w = 0);
// true when every coordinate is finite (the same in every lane).  With `centre`, their centroid in fp64 as well: lane l sums
// atoms l, l + 64, ... in ascending order, the 64 lane sums meet in sq_wave_sum's fixed tree, then / (double)P
template <class At>
__device__ __forceinline__ bool gather_structure(const float* __restrict__ base, At at, int n, int P, float4* __restrict__ row,
                                                 int lane, double* centre = nullptr) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  bool ok = true;
  for (int k = lane; k < P; k += 64) {
    const f3 p = ld3(base + 3 * (size_t)sel_atom(at(k), n));
    ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    row[k] = make_float4(p.x, p.y, p.z, 0.f);
    sx += (double)p.x, sy += (double)p.y, sz += (double)p.z;
  }
  if (centre != nullptr) {
    centre[0] = __shfl(sq_wave_sum(sx), 0) / (double)P;
    centre[1] = __shfl(sq_wave_sum(sy), 0) / (double)P;
    centre[2] = __shfl(sq_wave_sum(sz), 0) / (double)P;
  }
  return __any(!ok) == 0;
}
// a bad structure's row becomes NaN, which is within no distance of anything (the wave that gathered it: each lane its own)
__device__ __forceinline__ void poison_row(float4* __restrict__ row, int P, int lane) {
  for (int k = lane; k < P; k += 64) row[k] = make_float4(NAN, NAN, NAN, 0.f);
}

// One word of a mask [m, ceil(m / 32)], columns cb .. cb + 31 (cb < m): bit u of word_inside: column cb + u is inside the
// selection of m atoms; of word_above: it is above `row`; of upper_pair_word: both
__device__ __forceinline__ uint32_t word_inside(int cb, int m) { return m - cb >= 32 ? 0xffffffffu : (1u << (m - cb)) - 1u; }
__device__ __forceinline__ uint32_t word_above(int row, int cb) {
  return row < cb ? 0xffffffffu : row >= cb + 31 ? 0u : 0xffffffffu << (row - cb + 1);
}
__device__ __forceinline__ uint32_t upper_pair_word(int row, int cb, int m) { return word_inside(cb, m) & word_above(row, cb); }
// bit u: the pair (row, cb + u), u < PER, is the thread's to count -- inside the selection, above the diagonal, not excluded
// (excl may be null).  A thread's PER columns lie in one word: PER divides 32, cb is a multiple of PER
template <int PER>
__device__ __forceinline__ uint32_t upper_pair_bits(int row, int cb, int m, const uint32_t* __restrict__ excl, int words) {
  static_assert(32 % PER == 0, "a thread's columns lie in one word of the mask");
  if (row >= m || cb >= m) return 0u;
  uint32_t w = upper_pair_word(row, cb & ~31, m);
  if (excl != nullptr) w &= ~excl[(size_t)row * words + (cb >> 5)];
  return PER == 32 ? w : (w >> (cb & 31)) & ((1u << (PER & 31)) - 1u);
}

// 256 threads stage the structures s0 .. s0 + CHUNK - 1 of the tile at (r0, c0) from the packed copy [S, m]: st[sl] holds
// the tile's ROWS row atoms, then its COLS column atoms; `fill` (x = y = z) past the slice's end or the selection.  With
// `skip`: skip[sl] = 1 for a structure that is bad or past the end.  The caller puts a barrier before and after
template <int CHUNK, int ROWS, int COLS>
__device__ __forceinline__ void stage_chunk(float4 (&st)[CHUNK][ROWS + COLS], const float4* __restrict__ packed, int m, int r0, int c0,
                                            int s0, int s_end, int tid, float fill, const int* __restrict__ bad = nullptr,
                                            int* skip = nullptr) {
  if (skip != nullptr && tid < CHUNK) skip[tid] = s0 + tid < s_end && bad[s0 + tid] == 0 ? 0 : 1;
  for (int e = tid; e < CHUNK * (ROWS + COLS); e += 256) {
    const int sl = e / (ROWS + COLS), a = e - sl * (ROWS + COLS);
    const int at = a < ROWS ? r0 + a : c0 + a - ROWS;
    float4 v = make_float4(fill, fill, fill, 0.f);
    if (s0 + sl < s_end && at < m) v = packed[(size_t)(s0 + sl) * m + at];
    st[sl][a] = v;
  }
}

// The LDS counters of a pair kernel for the CHUNK structures it has staged, N per structure.  zero() between the chunk
// loop's two barriers, add() from the pair loop (one LDS atomic), flush() after a barrier: one global atomic per nonzero
// counter of a structure inside the slice -- to the caller's table [S, N], or with N = 2 to two tables [S]
template <class T, int CHUNK, int N>
struct ChunkCounts {
  T v[CHUNK][N];
  __device__ __forceinline__ void zero(int tid) { if (tid < CHUNK * N) v[tid / N][tid % N] = (T)0; }
  __device__ __forceinline__ void add(int sl, int k, T x) { atomicAdd(&v[sl][k], x); }
  __device__ __forceinline__ void flush(int s0, int s_end, int tid, T* __restrict__ table) {
    if (tid < CHUNK * N) {
      const int sl = tid / N, k = tid % N;
      const T x = v[sl][k];
      if (x != (T)0 && s0 + sl < s_end) atomicAdd(table + (size_t)(s0 + sl) * N + k, x);
    }
  }
  __device__ __forceinline__ void flush(int s0, int s_end, int tid, T* __restrict__ t0, T* __restrict__ t1) {
    static_assert(N == 2, "one table per counter");
    if (tid < CHUNK * N) {
      const int sl = tid / N, k = tid % N;
      const T x = v[sl][k];
      if (x != (T)0 && s0 + sl < s_end) atomicAdd((k ? t1 : t0) + s0 + sl, x);
    }
  }
};

}  // namespace cgv
