// K30 distance-matrix moments of an ensemble: over S structures, for every pair of the m selected atoms, the sum and the sum
// of squares of the pair's distance minus a centre -- from which the host has the mean-distance map, the standard-deviation
// map and their difference between two ensembles (ens_dRMS) -- and per structure the sum of the squared deviations of its
// distances from the centre table: the superposition-free distance RMSD to a target map.  See include/cgvae_hip.h.  Nothing
// in the reference computes it.
//
// For a good structure s and an unordered pair {i, j}, i < j, that the mask does not exclude, in fp32 with every operation
// rounded on its own (this file is compiled with -ffp-contract=off; sqrtf is the correctly rounded form, see csrc/tica.hip):
//   q = sq_dist2(x_i, x_j)      d = sqrtf(q)      e = __fsub_rn(d, center[i][j])      f = __fmul_rn(e, e)         csrc/sq_dist.h
//   sum_e[i][j]  += rint(e * 2^20)        sum_e2[i][j] += rint(f * 2^20)        dev2[s] += rint(f * 2^12)          (int64)
// A product by a power of two is exact (in fp32 as in fp64: nothing here overflows, and what underflows rounds to 0 either
// way), and rint of an exact value is the same integer in both widths: the kernel rounds in fp32 (v_rndne_f32), the host
// restates it as numpy.rint of the fp64 product, and every integer this file produces is exact.  No floating-point number
// leaves the device, and no floating-point sum exists on it.
//
// A structure is bad -- bad[s] = 1, a packed row of NaN, it enters no sum -- when a selected coordinate is not finite or a
// selected atom lies more than DM_MAX_RADIUS = 512 A from the centroid of the selection (fp64, lane sums in sq_wave_sum's
// fixed tree, as K20's).  With that every true pair distance is at most 1024 A.  A centre outside [0, 1024] (or a NaN) is
// read as 0 (the host wrapper refuses such tables), so |e| <= 2^10 and f <= 2^20, both times (1 + 2^-20) at the most for the
// five roundings from coordinates to d.
//
// Overflow, for m <= DM_MAX_ATOMS = 2^13, S <= DM_MAX_STRUCTURES = 2^20 per launch and at most DM_MAX_TOTAL = 2^22 good
// structures accumulated into one pair of tables (the host refuses more):
//   a term of sum_e     |rint(e * 2^20)| <= 2^30 (1 + 2^-20) < 2^31: an int32 conversion; 2^22 of them: |sum_e| <= 2^52 (1 + 2^-20)
//   a term of sum_e2    rint(f * 2^20) <= 2^40 (1 + 2^-20); 2^22 of them: sum_e2 <= 2^62 (1 + 2^-20) -- 2^62 is reached only
//                       by 2^22 structures that all hold the pair at 1024 A against a centre of 0, and passed only by the
//                       rounding of d, by 2^42 at the most; int64 holds 2^63
//   a term of dev2      rint(f * 2^12) <= 2^32 (1 + 2^-20); fewer than 2^25 pairs of 2^13 atoms: dev2[s] < 2^58
// A thread's registers hold one pair over the structures of ONE launch (<= 2^20): |.| <= 2^60.
//
// The gather with its centroid, the tile walk, the thread's mask bits, the staging and the chunk's counters are packed_dev.h's.
// dist_prep_k     one wave per structure, 4 per block: gather_structure fills the packed copy [S, m] float4 of the workspace
//                 (what the pair kernel streams) and gives the fp64 centroid; the 512 A test decides bad.
// dist_pairs_k    256 threads, grid (column tiles of 64, row tiles of 64, slices of the structure axis); tiles without a pair
//                 i < j return.  Thread t owns row t & 63 and the 16 columns of wave t >> 6 -- half a word of the mask --
//                 and keeps in registers their 16 centres and 2 x 16 int64 sums (64 VGPRs; K20's 32 columns per thread
//                 would be 128 for the sums alone).  DM_CHUNK structures at a time go through LDS (row atom: one
//                 ds_read_b128 per lane, column atom: one address for the wave); bad structures are skipped, so nothing
//                 relies on NaN.  A lane's sum of rint(f * 2^12) over its counted pairs of a structure goes to the chunk's
//                 int64 counter, which the block adds to dev2 once per structure.  At the end a nonzero sum is added to
//                 [i][j] and [j][i] of the caller's tables, one 64-bit atomicAdd each.
// Sums of integers meet in atomicAdd (LDS and global), whose order does not matter: two runs give the same bits, and
// nothing depends on how the caller cuts the structures into launches or struct_slices cuts a launch into slices.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int DM_ROWS = 64;                  // rows of a tile: the lanes of a wave
constexpr int DM_COLS = 64;                  // columns of a tile: 4 waves x half a 32-bit mask word
constexpr int DM_PER = 16;                   // columns of a thread
constexpr int DM_CHUNK = 8;                  // structures staged at once: 8 x 128 x 16 B = 16 KB of LDS
constexpr int DM_STAGE = DM_ROWS + DM_COLS;  // float4 of a staged structure
constexpr int DM_MAX_ATOMS = 8192;           // selected atoms: a table [m, m] int64 is 512 MB there
constexpr int DM_MAX_STRUCTURES = 1 << 20;   // per launch
constexpr int DM_MAX_TOTAL = 1 << 22;        // good structures accumulated into one pair of tables (the header's budget)
constexpr double DM_MAX_RADIUS = 512.0;      // from the centroid of the selection, in Angstrom
constexpr float DM_MAX_CENTER = 1024.f;      // the largest centre taken as it is
constexpr float DM_SCALE = 1048576.f;        // 2^20: sum_e and sum_e2
constexpr float DM_SCALE_DEV = 4096.f;       // 2^12: dev2
static_assert(DM_COLS == 4 * DM_PER, "four waves share a tile's columns");

// grid: 4 structures per block
__global__ __launch_bounds__(256) void dist_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int S, int n, int m,
                                                   float4* __restrict__ packed, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  float4* row = packed + (size_t)s * m;
  double c[3];
  bool ok = gather_structure(xyz + (size_t)s * n * 3, [=](int k) { return sel[k]; }, n, m, row, lane, c);
  for (int k = lane; k < m; k += 64) {
    const float4 p = row[k];                                 // this lane wrote it
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    ok = ok && ((dx * dx + dy * dy) + dz * dz <= DM_MAX_RADIUS * DM_MAX_RADIUS);     // false for a NaN
  }
  const bool is_bad = __any(!ok) != 0;
  if (is_bad) poison_row(row, m, lane);
  if (lane == 0) bad[s] = is_bad ? 1 : 0;
}

// grid: x = column tile, y = row tile, z = slice of the structure axis (`per` structures each, a multiple of DM_CHUNK)
__global__ __launch_bounds__(256) void dist_pairs_k(const float4* __restrict__ packed, const uint32_t* __restrict__ excl,
                                                    const float* __restrict__ center, const int* __restrict__ bad, int S, int m,
                                                    int words, int per, unsigned long long* __restrict__ sum_e,
                                                    unsigned long long* __restrict__ sum_e2, unsigned long long* __restrict__ dev2) {
  __shared__ float4 st[DM_CHUNK][DM_STAGE];
  __shared__ int skip[DM_CHUNK];                             // 1: bad, or past the slice
  __shared__ ChunkCounts<unsigned long long, DM_CHUNK, 1> dsum;   // per structure: its sum of rint(f * 2^12)
  const int r0 = (int)blockIdx.y * DM_ROWS, c0 = (int)blockIdx.x * DM_COLS;
  if (!upper_tile_live(r0, c0, DM_COLS)) return;             // no column of the tile is above a row of it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = r0 + lane, cb = c0 + DM_PER * wave;        // this thread's row and the first of its 16 columns
  // bit u: the pair (row, cb + u) is this thread's to sum -- inside the selection, above the diagonal, not excluded
  const uint32_t ok = upper_pair_bits<DM_PER>(row, cb, m, excl, words);
  const bool wave_live = __any(ok != 0) != 0;
  float ctr[DM_PER];
  long long a1[DM_PER], a2[DM_PER];                          // sums of rint(e * 2^20) and of rint(f * 2^20) over the slice
#pragma unroll
  for (int u = 0; u < DM_PER; ++u) {
    float c = 0.f;
    if (center != nullptr && ((ok >> u) & 1u) != 0) c = center[(size_t)row * m + cb + u];
    ctr[u] = (c >= 0.f && c <= DM_MAX_CENTER) ? c : 0.f;     // a centre outside the budget (or a NaN) is read as 0
    a1[u] = 0, a2[u] = 0;
  }
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += DM_CHUNK) {
    __syncthreads();                                         // the previous chunk has been read and its sums flushed
    // 0 past the slice or the selection: outside every mask
    stage_chunk<DM_CHUNK, DM_ROWS, DM_COLS>(st, packed, m, r0, c0, s0, s_end, tid, 0.f, bad, skip);
    dsum.zero(tid);
    __syncthreads();
    if (wave_live) {
#pragma unroll 1
      for (int sl = 0; sl < DM_CHUNK; ++sl) {
        if (skip[sl] != 0) continue;                         // the same for the whole block; a good structure has no NaN
        const float4 a = st[sl][lane];
        unsigned long long dev = 0ull;
#pragma unroll
        for (int u = 0; u < DM_PER; ++u) {
          const float4 b = st[sl][DM_ROWS + DM_PER * wave + u];
          const float d = sqrtf(sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z));
          const float e = __fsub_rn(d, ctr[u]);
          const float f = __fmul_rn(e, e);
          a1[u] += (long long)(int)rintf(__fmul_rn(e, DM_SCALE));            // pairs outside `ok` are summed too: they are never written
          a2[u] += (long long)rintf(__fmul_rn(f, DM_SCALE));
          const unsigned long long g = (unsigned long long)rintf(__fmul_rn(f, DM_SCALE_DEV));
          dev += ((ok >> u) & 1u) != 0 ? g : 0ull;
        }
        if (dev != 0ull) dsum.add(sl, 0, dev);
      }
    }
    __syncthreads();
    dsum.flush(s0, s_end, tid, dev2);
  }
#pragma unroll
  for (int u = 0; u < DM_PER; ++u) {
    if (((ok >> u) & 1u) == 0) continue;
    const size_t ij = (size_t)row * m + (cb + u), ji = (size_t)(cb + u) * m + row;
    if (a1[u] != 0) atomicAdd(sum_e + ij, (unsigned long long)a1[u]), atomicAdd(sum_e + ji, (unsigned long long)a1[u]);
    if (a2[u] != 0) atomicAdd(sum_e2 + ij, (unsigned long long)a2[u]), atomicAdd(sum_e2 + ji, (unsigned long long)a2[u]);
  }
}

static inline bool dm_sizes_ok(int S, int m) { return S >= 0 && m >= 0 && S <= DM_MAX_STRUCTURES && m <= DM_MAX_ATOMS; }
static inline size_t dm_workspace(int S, int m) { return (size_t)S * (size_t)m * sizeof(float4); }

}  // namespace cgv

extern "C" {

int cgv_dist_moments_max_atoms(void) { return cgv::DM_MAX_ATOMS; }
int cgv_dist_moments_max_structures(void) { return cgv::DM_MAX_STRUCTURES; }
int cgv_dist_moments_max_total(void) { return cgv::DM_MAX_TOTAL; }
int cgv_dist_moments_row_tile(void) { return cgv::DM_ROWS; }
int cgv_dist_moments_col_tile(void) { return cgv::DM_COLS; }
int cgv_dist_moments_chunk(void) { return cgv::DM_CHUNK; }

size_t cgv_dist_moments_workspace_bytes(int n_structures, int m) {
  return cgv::dm_sizes_ok(n_structures, m) ? cgv::dm_workspace(n_structures, m) : 0;
}

int cgv_dist_moments(const float* xyz, const int32_t* sel, const uint32_t* excluded, const float* center, int n_structures,
                     int n_atoms, int m, int64_t* sum_e, int64_t* sum_e2, int64_t* dev2, int32_t* bad, void* workspace,
                     size_t workspace_bytes, void* stream) {
  const int S = n_structures;
  CGV_REQUIRE(S >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::DM_MAX_STRUCTURES, "structures per launch <= cgv_dist_moments_max_structures()");
  CGV_REQUIRE(m >= 2 && m <= n_atoms, "2 <= m <= n_atoms");
  CGV_REQUIRE(m <= cgv::DM_MAX_ATOMS, "m <= cgv_dist_moments_max_atoms()");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && sel && sum_e && sum_e2 && dev2 && bad, "null pointer");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::dm_workspace(S, m), "workspace smaller than cgv_dist_moments_workspace_bytes()");
  CGV_REQUIRE(why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::dist_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, S, n_atoms, m, packed, bad);
  int rc = cgv::check_launch("cgv_dist_moments (preparation)");
  if (rc) return rc;
  int per;
  const dim3 grid = cgv::pair_grid(S, m, cgv::DM_ROWS, cgv::DM_COLS, cgv::DM_CHUNK, false, &per);
  hipLaunchKernelGGL(cgv::dist_pairs_k, grid, dim3(256), 0, st, (const float4*)packed,
                     excluded, center, (const int*)bad, S, m, (m + 31) / 32, per, (unsigned long long*)sum_e,
                     (unsigned long long*)sum_e2, (unsigned long long*)dev2);
  return cgv::check_launch("cgv_dist_moments");
}

}  // extern "C"
