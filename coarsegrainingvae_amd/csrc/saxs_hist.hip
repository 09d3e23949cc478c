// K33 weighted pair-distance histograms of an ensemble, ONE PER STRUCTURE: what the small-angle scattering curve I(q), the
// electron-weighted P(r), Rg and Dmax of every structure are made from on the host (saxs.py).  See include/cgvae_hip.h.
// Nothing in the reference computes it.  K29 (pair_hist.hip) cannot serve: it sums over the ensemble, counts without
// weights, stops at 256 bins and leaves bonded neighbours out.
//
// For structure s and EVERY unordered pair {i, j}, i < j, of the m selected atoms (there is no exclusion mask), in fp32 with
// every operation rounded on its own (this file is compiled with -ffp-contract=off; sqrtf is the correctly rounded form) --
// K29's bin rule unchanged:
//   q = sq_dist2(x_i, x_j)                                                               csrc/sq_dist.h
//   in range  iff  q < rmax2                                  strict; false for a NaN
//   b = min((int)(sqrtf(q) * scale), n_bins - 1)              one rounded product, truncation, clamp
// An in-range pair adds the integer wq_i * wq_j to hist[s][b]; every other pair adds ONE to beyond[s] (a count of pairs,
// whatever their weights: a signed sum could cancel to zero and hide an incomplete profile).  wq are the caller's
// fixed-point weights, |wq| <= SX_MAX_WEIGHT = 32767.  The host restates the arithmetic bit for bit, so every integer this
// file produces is exact; no floating-point number leaves the device, and every transcendental function (the sinc of the
// Debye sum) stays on the host in fp64.  A structure with a non-finite selected coordinate is bad: bad[s] = 1 and it enters
// no sum (its rows stay as the caller left them).
//
// The gather, the tile walk, the thread's word of pairs and the workspace check are packed_dev.h's.
// saxs_prep_k     one wave per structure, 4 per block: gather_structure fills the packed copy [S, m] float4 of the workspace
//                 and decides bad -- as pairdist_prep_k.
// saxs_tiles_k    m > SX_SMALL.  256 threads; `nblk` blocks share a structure: block k of them takes the row tiles (64 rows)
//                 k, k + nblk, ... -- interleaved, because the rows near the top of the triangle have more column tiles --
//                 and walks every column tile (128 columns) that holds a pair i < j.  Thread t owns row t & 63 and the 32
//                 columns of wave t >> 6, as in K29; the tile's 192 atoms pass through LDS as float4 whose w holds the
//                 bits of the atom's integer weight (moved, never computed with).  An in-range pair with a nonzero product is one 64-bit LDS integer atomic on
//                 the block's private histogram of n_bins signed 64-bit cells (dynamic LDS, 32 KB at the limit).
// saxs_small_k    m <= SX_SMALL = 64: one tile covers the structure, and a block per structure would leave three waves of
//                 four idle.  `pack` (4, 2 or 1: as many histograms of n_bins cells as fit 32 KB) structures share a block,
//                 a wave each; lane i owns atom i and meets the atoms (i + k) mod m, k = 1 .. m / 2 -- every unordered pair
//                 once (at k = m / 2 of an even m only the lanes i < m / 2), with every lane i < m busy at every step,
//                 where a triangle i < j would idle half of them.
// Both end the same way: every NONZERO cell goes to the caller's hist [S, n_bins] int64 in one 64-bit global atomicAdd (the
// blocks of a structure meet there, and so do the launches of a caller who feeds the same rows twice); `beyond` is counted
// in a register, summed over the wave and added once per wave.
// Overflow: |wq_i * wq_j| < 2^30 in a 32-bit product; a structure has fewer than 8192^2 / 2 = 2^25 pairs, so
// |hist[s][b]| < 2^55 and beyond[s] < 2^25 -- in the LDS cells, the caller's tables and the thread's 32-bit beyond counter
// alike.  Negative sums are two's complement: the unsigned 64-bit atomics add them exactly.
// Sums of integers meet in atomicAdd (LDS and global), whose order does not matter: two runs give the same bits, and nothing
// depends on how the caller cuts the structures into launches or on how many blocks share a structure.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int SX_ROWS = 64;                  // rows of a tile: the lanes of a wave
constexpr int SX_COLS = 128;                 // columns of a tile: 4 waves x one word of 32 pairs
constexpr int SX_STAGE = SX_ROWS + SX_COLS;  // float4 of a staged tile
constexpr int SX_SMALL = 64;                 // at most this many atoms: a wave per structure
constexpr int SX_MAX_PACK = 4;               // structures of a block on the small path: its waves
constexpr int SX_MAX_ATOMS = 8192;           // fewer than 2^25 pairs
constexpr int SX_MAX_STRUCTURES = 1 << 20;   // per launch: at most 2^20 x 128 row tiles = 2^27 blocks
constexpr int SX_MAX_BINS = 4096;            // 32 KB of 64-bit cells
constexpr int SX_MAX_WEIGHT = 32767;         // |wq|: a product stays below 2^30
constexpr int SX_TARGET_BLOCKS = 2048;       // 8 blocks on each of 256 CUs: a structure is split until the launch has these
constexpr int SX_LDS_BYTES = 64 * 1024;      // what a launch may ask for without an attribute
constexpr int SX_TILE_STATIC = SX_STAGE * 16;                         // the staged tile
constexpr int SX_SMALL_STATIC = SX_MAX_PACK * SX_SMALL * 16;          // the staged structures
static_assert(SX_MAX_BINS * 8 + SX_TILE_STATIC <= SX_LDS_BYTES, "the histogram at the limit and the staged tile fit 64 KB");
static_assert(SX_MAX_BINS * 8 + SX_SMALL_STATIC <= SX_LDS_BYTES, "the histograms of a packed block and its structures fit 64 KB");
static_assert((long long)SX_MAX_ATOMS * (SX_MAX_ATOMS - 1) / 2 < (1ll << 25), "fewer than 2^25 pairs: the header's bound");
static_assert((long long)SX_MAX_WEIGHT * SX_MAX_WEIGHT < (1ll << 30), "a product of two weights fits 32 bits");

// the bin of an in-range pair; the product is >= 0: max only fences the table
__device__ __forceinline__ int sx_bin(float q, float scale, int last) { return max(min((int)__fmul_rn(sqrtf(q), scale), last), 0); }

// the block's cells -> the caller's row; a wave's `far` -> the caller's counter.  `T` threads scan the `n_bins` cells
__device__ __forceinline__ void sx_flush(const unsigned long long* __restrict__ cells, int n_bins, int t, int T,
                                         unsigned long long* __restrict__ row) {
  for (int e = t; e < n_bins; e += T) {
    const unsigned long long v = cells[e];
    if (v != 0ull) atomicAdd(row + e, v);
  }
}
__device__ __forceinline__ void sx_flush_far(int far, int lane, unsigned long long* __restrict__ counter) {
  const int all = sq_wave_sum(far);
  if (lane == 0 && all != 0) atomicAdd(counter, (unsigned long long)all);
}

// grid: 4 structures per block
__global__ __launch_bounds__(256) void saxs_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int S, int n, int m,
                                                   float4* __restrict__ packed, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  const bool ok = gather_structure(xyz + (size_t)s * n * 3, [=](int k) { return sel[k]; }, n, m, packed + (size_t)s * m, lane);
  if (lane == 0) bad[s] = ok ? 0 : 1;
}

// grid: x = structure * nblk + the block's place among the nblk of its structure; dynamic LDS: n_bins cells
__global__ __launch_bounds__(256) void saxs_tiles_k(const float4* __restrict__ packed, const int* __restrict__ wq,
                                                    const int* __restrict__ bad, int m, int nblk, int n_bins, float rmax2, float scale,
                                                    unsigned long long* __restrict__ hist, unsigned long long* __restrict__ beyond) {
  __shared__ float4 st[SX_STAGE];                            // the tile's rows, then its columns; w: the bits of the atom's weight
  extern __shared__ unsigned long long cells[];              // [n_bins]
  const int s = (int)(blockIdx.x / (unsigned)nblk), k = (int)(blockIdx.x % (unsigned)nblk);
  if (bad[s] != 0) return;                                   // the same for the whole block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float4* __restrict__ x = packed + (size_t)s * m;
  for (int e = tid; e < n_bins; e += 256) cells[e] = 0ull;
  const int nr = (m + SX_ROWS - 1) / SX_ROWS, nc = (m + SX_COLS - 1) / SX_COLS, last = n_bins - 1;
  int far = 0;
  for (int rt = k; rt < nr; rt += nblk) {
    const int r0 = rt * SX_ROWS, row = r0 + lane;
    for (int ct = (r0 + 1) / SX_COLS; ct < nc; ++ct) {       // the first column tile with a column above r0
      const int c0 = ct * SX_COLS;
      if (!upper_tile_live(r0, c0, SX_COLS)) continue;
      __syncthreads();                                       // the previous tile has been read; the first time: cells are zero
      if (tid < SX_STAGE) {
        const int at = tid < SX_ROWS ? r0 + tid : c0 + tid - SX_ROWS;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);           // past the selection: weight 0, and outside `ok`
        if (at < m) v = x[at], v.w = __int_as_float(wq[at]);
        st[tid] = v;
      }
      __syncthreads();
      const int cb = c0 + 32 * wave;
      // bit u: the pair (row, cb + u) is this thread's -- inside the selection and above the diagonal
      const uint32_t ok = upper_pair_bits<32>(row, cb, m, nullptr, 0);
      if (__any(ok != 0) == 0) continue;                     // the whole wave; the barriers are above
      const float4 a = st[lane];
      const int wr = __float_as_int(a.w);
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const float4 b = st[SX_ROWS + 32 * wave + u];
        const float q = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z);
        const bool mine = ((ok >> u) & 1u) != 0, in = q < rmax2;
        const int w = wr * __float_as_int(b.w);
        far += mine && !in ? 1 : 0;
        if (mine && in && w != 0) atomicAdd(cells + sx_bin(q, scale, last), (unsigned long long)(long long)w);
      }
    }
  }
  __syncthreads();
  sx_flush(cells, n_bins, tid, 256, hist + (size_t)s * n_bins);
  sx_flush_far(far, lane, beyond + s);
}

// grid: `pack` structures per block, 64 * pack threads; dynamic LDS: pack x n_bins cells
__global__ __launch_bounds__(256) void saxs_small_k(const float4* __restrict__ packed, const int* __restrict__ wq,
                                                    const int* __restrict__ bad, int S, int m, int pack, int n_bins, float rmax2,
                                                    float scale, unsigned long long* __restrict__ hist,
                                                    unsigned long long* __restrict__ beyond) {
  __shared__ float4 st[SX_MAX_PACK][SX_SMALL];               // w: the bits of the atom's weight
  extern __shared__ unsigned long long cells[];              // [pack][n_bins]
  const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;       // wave < pack: the block has 64 * pack threads
  const int s = (int)blockIdx.x * pack + wave;
  const bool live = s < S && bad[s] == 0;                    // the same for the whole wave
  unsigned long long* mine = cells + (size_t)wave * n_bins;
  for (int e = lane; e < n_bins; e += 64) mine[e] = 0ull;
  {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && lane < m) v = packed[(size_t)s * m + lane], v.w = __int_as_float(wq[lane]);
    st[wave][lane] = v;
  }
  __syncthreads();                                           // every wave is here: none has left
  int far = 0;
  if (live && lane < m) {
    const float4 a = st[wave][lane];
    const int wr = __float_as_int(a.w);
    const int half = m >> 1, last = n_bins - 1;
    for (int d = 1; d <= half; ++d) {
      if (2 * d == m && lane >= half) break;                 // the pairs half a turn apart come up twice: the lower lanes take them
      int j = lane + d;
      j -= j >= m ? m : 0;
      const float4 b = st[wave][j];
      const float q = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z);
      const int w = wr * __float_as_int(b.w);
      if (!(q < rmax2)) far += 1;
      else if (w != 0) atomicAdd(mine + sx_bin(q, scale, last), (unsigned long long)(long long)w);
    }
  }
  __syncthreads();
  if (live) {
    sx_flush(mine, n_bins, lane, 64, hist + (size_t)s * n_bins);
    sx_flush_far(far, lane, beyond + s);
  }
}

static inline bool sx_sizes_ok(int S, int m) { return S >= 0 && m >= 0 && S <= SX_MAX_STRUCTURES && m <= SX_MAX_ATOMS; }
static inline size_t sx_workspace(int S, int m) { return (size_t)S * (size_t)m * sizeof(float4); }
// structures of a block on the small path: as many histograms as fit the cells of one at the limit
static inline int sx_pack(int n_bins) {
  int pack = SX_MAX_PACK;
  while (pack > 1 && pack * n_bins > SX_MAX_BINS) pack >>= 1;
  return pack;
}
// blocks that share a structure on the tiled path: `split` when the caller names it, else until the launch has
// SX_TARGET_BLOCKS; at most one per row tile
static inline int sx_blocks(int S, int m, int split) {
  const int nr = (m + SX_ROWS - 1) / SX_ROWS;
  int nblk = split > 0 ? split : (SX_TARGET_BLOCKS + S - 1) / (S > 0 ? S : 1);
  if (nblk > nr) nblk = nr;
  return nblk < 1 ? 1 : nblk;
}

}  // namespace cgv

extern "C" {

int cgv_saxs_max_atoms(void) { return cgv::SX_MAX_ATOMS; }
int cgv_saxs_max_structures(void) { return cgv::SX_MAX_STRUCTURES; }
int cgv_saxs_max_bins(void) { return cgv::SX_MAX_BINS; }
int cgv_saxs_max_weight(void) { return cgv::SX_MAX_WEIGHT; }
int cgv_saxs_row_tile(void) { return cgv::SX_ROWS; }
int cgv_saxs_col_tile(void) { return cgv::SX_COLS; }
int cgv_saxs_small(void) { return cgv::SX_SMALL; }
int cgv_saxs_pack(int m, int n_bins) { return m >= 1 && m <= cgv::SX_SMALL && n_bins >= 1 && n_bins <= cgv::SX_MAX_BINS ? cgv::sx_pack(n_bins) : 1; }
int cgv_saxs_blocks(int n_structures, int m, int split) {
  return cgv::sx_sizes_ok(n_structures, m) && m > cgv::SX_SMALL ? cgv::sx_blocks(n_structures, m, split) : 1;
}

size_t cgv_saxs_workspace_bytes(int n_structures, int m) {
  return cgv::sx_sizes_ok(n_structures, m) ? cgv::sx_workspace(n_structures, m) : 0;
}

int cgv_saxs_hist(const float* xyz, const int32_t* sel, const int32_t* wq, int n_structures, int n_atoms, int m, int n_bins,
                  float rmax2, float scale, int split, int64_t* hist, int64_t* beyond, int32_t* bad, void* workspace,
                  size_t workspace_bytes, void* stream) {
  const int S = n_structures;
  CGV_REQUIRE(S >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::SX_MAX_STRUCTURES, "structures per launch <= cgv_saxs_max_structures()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(m <= cgv::SX_MAX_ATOMS, "m <= cgv_saxs_max_atoms()");
  CGV_REQUIRE(n_bins >= 1 && n_bins <= cgv::SX_MAX_BINS, "1 <= n_bins <= cgv_saxs_max_bins()");
  CGV_REQUIRE(rmax2 >= 0.f && rmax2 <= 3.0e38f, "rmax2 must be a finite number >= 0");
  CGV_REQUIRE(scale > 0.f && scale <= 3.0e38f, "scale must be a finite number > 0");
  CGV_REQUIRE(split >= 0, "split >= 0 (0: the library decides)");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && sel && wq && hist && beyond && bad, "null pointer");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::sx_workspace(S, m), "workspace smaller than cgv_saxs_workspace_bytes()");
  CGV_REQUIRE(why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::saxs_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, S, n_atoms, m, packed, bad);
  int rc = cgv::check_launch("cgv_saxs_hist (preparation)");
  if (rc || m < 2) return rc;
  if (m <= cgv::SX_SMALL) {
    const int pack = cgv::sx_pack(n_bins);
    hipLaunchKernelGGL(cgv::saxs_small_k, dim3((unsigned)((S + pack - 1) / pack)), dim3(64 * pack), (size_t)pack * n_bins * 8, st,
                       (const float4*)packed, wq, (const int*)bad, S, m, pack, n_bins, rmax2, scale, (unsigned long long*)hist,
                       (unsigned long long*)beyond);
  } else {
    const int nblk = cgv::sx_blocks(S, m, split);
    hipLaunchKernelGGL(cgv::saxs_tiles_k, dim3((unsigned)S * (unsigned)nblk), dim3(256), (size_t)n_bins * 8, st, (const float4*)packed,
                       wq, (const int*)bad, m, nblk, n_bins, rmax2, scale, (unsigned long long*)hist, (unsigned long long*)beyond);
  }
  return cgv::check_launch("cgv_saxs_hist");
}

}  // extern "C"
