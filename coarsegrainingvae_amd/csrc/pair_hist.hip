// K29 pair-distance distributions of an ensemble: over S structures, the histogram of the distances between the pairs of
// selected atoms, one histogram per unordered pair of atom classes (elements, beads, the caller's labels) -- the radial /
// pair distribution P(r) that coarse-grained models are judged by.  See include/cgvae_hip.h.  Nothing in the reference
// computes it.
//
// For an unordered pair {i, j}, i < j, of the m selected atoms that the mask does not exclude, in fp32 with every operation
// rounded on its own (this file is compiled with -ffp-contract=off; sqrtf is the correctly rounded form, see csrc/tica.hip):
//   q = sq_dist2(x_i, x_j)                                                               csrc/sq_dist.h
//   in range  iff  q < rmax2                                  strict; false for a NaN
//   d = sqrtf(q)      b = min((int)(d * scale), n_bins - 1)   one rounded product, truncation, clamp
//   p = pair_class(cls_i, cls_j) = a * C - a * (a - 1) / 2 + (b' - a),  a = min, b' = max of the two classes
// An in-range pair adds one to hist[p][b], every other pair one to beyond[p].  The host restates the arithmetic bit for bit,
// so every integer this file produces is exact; no floating-point number leaves the device.  A structure with a non-finite
// selected coordinate is bad: bad[s] = 1 and it enters no sum.
//
// The gather, the tile walk, the thread's mask word and the staging are packed_dev.h's.
// pairdist_prep_k    one wave per structure, 4 per block: gather_structure fills the packed copy [S, m] float4 of the
//                    workspace (what the pair kernel streams) and decides bad.
// pairdist_pairs_k   256 threads, grid (column tiles of 128, row tiles of 64, slices of the structure axis); tiles without a
//                    pair i < j return.  Thread t owns row t & 63 and the 32 columns of wave t >> 6 -- one word of the
//                    mask -- and keeps in registers, for each of the 32 pairs, where its class pair's row of the histogram
//                    starts.  PD_CHUNK structures at a time go through LDS (row atom: one ds_read_b128 per lane, column
//                    atom: one address for the wave); bad structures are skipped, so nothing relies on NaN.  The block's histogram is private in LDS, P rows of n_bins + 1 32-bit counters (the last
//                    one is `beyond`).  An in-range pair is one LDS integer atomic; the pairs at r_max or farther -- most
//                    pairs of a large molecule, and ONE address per class pair, on which the lanes of a wave would
//                    serialise -- are counted in 32 registers, as K20 counts its contacts, and reach the LDS counter once
//                    per thread.  Where they fit beside the staging in the 64 KB a launch may ask for without an attribute,
//                    the block keeps `copies` (2 or 4) of the histogram and lane l fills copy l % copies, so that lanes
//                    of a wave that meet in one bin meet in fewer addresses; the copies are summed at the end, when every
//                    NONZERO counter goes to the caller's int64 tables in one 64-bit atomicAdd (DESIGN.md section 8 has the
//                    measurements).
// Overflow: a block adds one per counted pair; it owns at most PD_ROWS x PD_COLS = 2^13 pairs and sees at most
// PD_MAX_STRUCTURES = 2^18 structures of a launch, so ALL its counters together, summed over the copies, hold at most 2^31
// (a thread's register counter at most 2^18): no unsigned 32-bit counter can wrap, and no flush inside the loop is needed.
// The caller's tables are 64 bits wide.
// Sums of integers meet in atomicAdd (LDS and global), whose order does not matter: two runs give the same bits, and nothing
// depends on how the caller cuts the structures into launches.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int PD_ROWS = 64;                  // rows of a tile: the lanes of a wave
constexpr int PD_COLS = 128;                 // columns of a tile: 4 waves x one 32-bit mask word
constexpr int PD_CHUNK = 8;                  // structures staged at once: 8 x 192 x 16 B = 24 KB of LDS
constexpr int PD_STAGE = PD_ROWS + PD_COLS;  // float4 of a staged structure
constexpr int PD_MAX_ATOMS = 8192;           // selected atoms: the mask is 8 MB there
constexpr int PD_MAX_STRUCTURES = 1 << 18;   // per launch: 2^13 pairs of a tile x 2^18 structures = 2^31 (the header's bound)
constexpr int PD_MAX_CLASSES = 8;            // 36 class pairs
constexpr int PD_MAX_BINS = 256;             // 36 x 257 counters = 36.1 KB; with the staging 60.2 KB <= 64 KB
constexpr int PD_LDS_BYTES = 64 * 1024;      // what a launch may ask for without an attribute
constexpr int PD_MAX_COPIES = 4;             // copies of the histogram in a block at most
constexpr int PD_STATIC_BYTES = PD_CHUNK * PD_STAGE * 16 + PD_CHUNK * 4;   // the staging and the skip flags
static_assert(PD_STATIC_BYTES + (PD_MAX_CLASSES * (PD_MAX_CLASSES + 1) / 2) * (PD_MAX_BINS + 1) * 4 <= PD_LDS_BYTES,
              "one histogram at the limits and the staging fit 64 KB");

__host__ __device__ __forceinline__ int pair_class(int a, int b, int C) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * C - lo * (lo - 1) / 2 + (hi - lo);
}

// a class out of the caller's table: one outside [0, C) counts as class 0, so nothing is written out of bounds
__device__ __forceinline__ int pd_class(int c, int C) { return (c >= 0 && c < C) ? c : 0; }

// grid: 4 structures per block
__global__ __launch_bounds__(256) void pairdist_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int S, int n, int m,
                                                       float4* __restrict__ packed, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  const bool ok = gather_structure(xyz + (size_t)s * n * 3, [=](int k) { return sel[k]; }, n, m, packed + (size_t)s * m, lane);
  if (lane == 0) bad[s] = ok ? 0 : 1;
}

// grid: x = column tile, y = row tile, z = slice of the structure axis (`per` structures each, a multiple of PD_CHUNK);
// dynamic LDS: copies x P x (n_bins + 1) counters
__global__ __launch_bounds__(256) void pairdist_pairs_k(const float4* __restrict__ packed, const int* __restrict__ cls,
                                                        const uint32_t* __restrict__ excl, const int* __restrict__ bad, int S, int m,
                                                        int words, int per, int C, int n_bins, int copies, float rmax2, float scale,
                                                        unsigned long long* __restrict__ hist, unsigned long long* __restrict__ beyond) {
  __shared__ float4 st[PD_CHUNK][PD_STAGE];
  __shared__ int skip[PD_CHUNK];                             // 1: bad, or past the slice
  extern __shared__ unsigned int lh[];                       // [copies][P][n_bins + 1]
  const int r0 = (int)blockIdx.y * PD_ROWS, c0 = (int)blockIdx.x * PD_COLS;
  if (!upper_tile_live(r0, c0, PD_COLS)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = r0 + lane, cb = c0 + 32 * wave;            // this thread's row and the first of its 32 columns
  const int stride = n_bins + 1, cells = (C * (C + 1) / 2) * stride;
  for (int e = tid; e < copies * cells; e += 256) lh[e] = 0u;
  // bit u: the pair (row, cb + u) is this thread's to count -- inside the selection, above the diagonal, not excluded
  const uint32_t ok = upper_pair_bits<32>(row, cb, m, excl, words);
  const bool wave_live = __any(ok != 0) != 0;
  int off[32];                                               // where the class pair's row of the histogram starts
  {
    const int ca = row < m ? pd_class(cls[row], C) : 0;
#pragma unroll
    for (int u = 0; u < 32; ++u) off[u] = pair_class(ca, cb + u < m ? pd_class(cls[cb + u], C) : 0, C) * stride;
  }
  unsigned int* mine = lh + (lane & (copies - 1)) * cells;   // copies is a power of two
  int far[32];                                               // the thread's pairs at r_max or farther, over its structures
#pragma unroll
  for (int u = 0; u < 32; ++u) far[u] = 0;
  const int last = n_bins - 1;
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += PD_CHUNK) {
    __syncthreads();                                         // the previous chunk has been read; the first time: lh is zero
    // 0 past the slice or the selection: outside every mask
    stage_chunk<PD_CHUNK, PD_ROWS, PD_COLS>(st, packed, m, r0, c0, s0, s_end, tid, 0.f, bad, skip);
    __syncthreads();
    if (wave_live) {
#pragma unroll 1
      for (int sl = 0; sl < PD_CHUNK; ++sl) {
        if (skip[sl] != 0) continue;                         // the same for the whole block
        const float4 a = st[sl][lane];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const float4 b = st[sl][PD_ROWS + 32 * wave + u];
          const float q = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z);
          const int bin = max(min((int)__fmul_rn(sqrtf(q), scale), last), 0);   // the product is >= 0: max only fences the table
          const bool in = q < rmax2;                         // a good structure has no NaN; an overflowed q is beyond
          far[u] += in ? 0 : 1;                              // pairs outside `ok` count too: they are never written
          if (in && ((ok >> u) & 1u) != 0) atomicAdd(mine + off[u] + bin, 1u);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 32; ++u)
    if (((ok >> u) & 1u) != 0 && far[u] != 0) atomicAdd(mine + off[u] + n_bins, (unsigned int)far[u]);
  __syncthreads();
  for (int e = tid; e < cells; e += 256) {
    unsigned long long v = 0ull;
    for (int c = 0; c < copies; ++c) v += lh[c * cells + e];
    if (v != 0ull) {
      const int p = e / stride, b = e - p * stride;
      atomicAdd(b == n_bins ? beyond + p : hist + (size_t)p * n_bins + b, v);
    }
  }
}

static inline bool pd_sizes_ok(int S, int m) { return S >= 0 && m >= 0 && S <= PD_MAX_STRUCTURES && m <= PD_MAX_ATOMS; }
static inline size_t pd_workspace(int S, int m) { return (size_t)S * (size_t)m * sizeof(float4); }
// the most copies of the histogram (4, 2 or 1) that fit beside the staging
static inline int pd_copies(int C, int n_bins) {
  const size_t one = (size_t)(C * (C + 1) / 2) * (size_t)(n_bins + 1) * sizeof(unsigned int);
  int copies = PD_MAX_COPIES;
  while (copies > 1 && PD_STATIC_BYTES + copies * one > (size_t)PD_LDS_BYTES) copies >>= 1;
  return copies;
}

}  // namespace cgv

extern "C" {

int cgv_pairdist_max_atoms(void) { return cgv::PD_MAX_ATOMS; }
int cgv_pairdist_max_structures(void) { return cgv::PD_MAX_STRUCTURES; }
int cgv_pairdist_max_classes(void) { return cgv::PD_MAX_CLASSES; }
int cgv_pairdist_max_bins(void) { return cgv::PD_MAX_BINS; }
int cgv_pairdist_row_tile(void) { return cgv::PD_ROWS; }
int cgv_pairdist_col_tile(void) { return cgv::PD_COLS; }
int cgv_pairdist_chunk(void) { return cgv::PD_CHUNK; }

size_t cgv_pairdist_workspace_bytes(int n_structures, int m) {
  return cgv::pd_sizes_ok(n_structures, m) ? cgv::pd_workspace(n_structures, m) : 0;
}

int cgv_pairdist_counts(const float* xyz, const int32_t* sel, const int32_t* cls, const uint32_t* excluded, int n_structures,
                        int n_atoms, int m, int n_classes, int n_bins, float rmax2, float scale, int64_t* hist, int64_t* beyond,
                        int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  const int S = n_structures, C = n_classes;
  CGV_REQUIRE(S >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::PD_MAX_STRUCTURES, "structures per launch <= cgv_pairdist_max_structures()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(m <= cgv::PD_MAX_ATOMS, "m <= cgv_pairdist_max_atoms()");
  CGV_REQUIRE(C >= 1 && C <= cgv::PD_MAX_CLASSES, "1 <= n_classes <= cgv_pairdist_max_classes()");
  CGV_REQUIRE(n_bins >= 1 && n_bins <= cgv::PD_MAX_BINS, "1 <= n_bins <= cgv_pairdist_max_bins()");
  CGV_REQUIRE(rmax2 >= 0.f && rmax2 <= 3.0e38f, "rmax2 must be a finite number >= 0");
  CGV_REQUIRE(scale > 0.f && scale <= 3.0e38f, "scale must be a finite number > 0");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && sel && cls && excluded && hist && beyond && bad, "null pointer");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::pd_workspace(S, m), "workspace smaller than cgv_pairdist_workspace_bytes()");
  CGV_REQUIRE(why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::pairdist_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, S, n_atoms, m, packed, bad);
  int rc = cgv::check_launch("cgv_pairdist_counts (preparation)");
  if (rc || m < 2) return rc;
  int per;
  const dim3 grid = cgv::pair_grid(S, m, cgv::PD_ROWS, cgv::PD_COLS, cgv::PD_CHUNK, false, &per);
  const int copies = cgv::pd_copies(C, n_bins);
  const size_t lds = (size_t)copies * (size_t)(C * (C + 1) / 2) * (size_t)(n_bins + 1) * sizeof(unsigned int);
  hipLaunchKernelGGL(cgv::pairdist_pairs_k, grid, dim3(256), lds, st,
                     (const float4*)packed, cls, excluded, (const int*)bad, S, m, (m + 31) / 32, per, C, n_bins, copies, rmax2, scale,
                     (unsigned long long*)hist, (unsigned long long*)beyond);
  return cgv::check_launch("cgv_pairdist_counts");
}

}  // extern "C"
