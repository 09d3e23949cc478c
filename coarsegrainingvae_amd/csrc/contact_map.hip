// K20 contact maps of an ensemble: how often every pair of selected atoms (or of groups of them: beads, residues) is
// within a cutoff over S structures, and per structure the number of contacts, the number of NATIVE contacts (pairs of a
// given set) and the squared radius of gyration -- the non-bonded view of an ensemble (contact probability maps, the
// fraction of native contacts Q, Rg).  See include/cgvae_hip.h.  Nothing in the reference computes it.
//
// A pair (i, j), i != j, not excluded, is in contact in structure s iff sq_dist2(x_i, x_j) < cutoff2 (sq_dist.h: fp32,
// every operation individually rounded, strict <; this file is compiled with -ffp-contract=off): the host restates the
// test bit for bit, so every integer this file produces is exact.
//
// The gather, the tile walk, the staging and the chunk's counters are packed_dev.h's.
// contact_prep_k    one wave per structure, 4 per block.  Pass 1: gather_structure packs the m selected atoms into the
//                   copy P [S, m] float4 of the workspace (what the pair kernels stream), tests them and gives their fp64
//                   centroid.  Pass 2: the squared distances from the centroid, lane l taking atoms l, l + 64, ... in
//                   ascending order, the lane sums meeting in sq_wave_sum's fixed tree: rg2.  A bad structure (a
//                   non-finite selected coordinate) gets rg2 = NaN, n_contacts = n_native = -1 and a packed row of NaN,
//                   which is in contact with nothing: the pair kernels need not know of it.
// contact_pairs_k   256 threads, grid (column tiles of 128, row tiles of 64, slices of the structure axis); tiles without
//                   a pair i < j return.  Thread t owns row t & 63 and the 32 columns of wave t >> 6 -- one word of the
//                   bit masks -- and keeps their 32 counters in registers.  CT_CHUNK structures at a time go through LDS
//                   (the row read is one ds_read_b128 per lane, a column read is the same address in every lane); per
//                   structure a lane's hits under its mask go to the chunk's counters, which the block adds to
//                   n_contacts / n_native once per structure.  At the end a nonzero counter is added to counts[i][j] and
//                   counts[j][i].
// contact_groups_k  one wave per pair of groups A < B, grid (G, G, slices).  The lanes tile the |A| x |B| atom pairs (the
//                   width of B rounded up to a power of two, at most 64); for 64 structures at a time a lane tests its
//                   pairs (the exclusion bit of a pair is read once per 64 structures) and keeps one bit per structure;
//                   the wave ORs the lanes' words: bit s = "any pair in contact in structure s".
// Sums of integers meet in atomicAdd, whose order does not matter; rg2 has a fixed order and no atomic: two runs give the
// same bits, and counts do not depend on how the caller cuts the structures into launches.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int CT_ROWS = 64;                  // rows of a tile: the lanes of a wave
constexpr int CT_COLS = 128;                 // columns of a tile: 4 waves x one 32-bit mask word
constexpr int CT_CHUNK = 8;                  // structures staged at once: 8 x 192 x 16 B = 24 KB of LDS
constexpr int CT_MAX_ATOMS = 1 << 14;        // selected atoms: counts [m,m] int32 is 1 GB there, m^2 / 2 pairs < 2^31
constexpr int CT_MAX_STRUCTURES = 1 << 20;   // per launch
constexpr int CT_MAX_GROUPS = 4096;          // the group kernel's grid is G x G waves

__global__ __launch_bounds__(256) void contact_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int S, int n, int m,
                                                      float4* __restrict__ packed, double* __restrict__ rg2,
                                                      int* __restrict__ bad, int* __restrict__ n_contacts,
                                                      int* __restrict__ n_native) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  float4* row = packed + (size_t)s * m;
  double c[3];
  const bool is_bad = !gather_structure(xyz + (size_t)s * n * 3, [=](int k) { return sel[k]; }, n, m, row, lane, c);
  double g = 0.0;
  for (int k = lane; k < m; k += 64) {
    const float4 p = row[k];                                 // this lane wrote it
    const double dx = (double)p.x - c[0], dy = (double)p.y - c[1], dz = (double)p.z - c[2];
    g += (dx * dx + dy * dy) + dz * dz;
  }
  if (is_bad) poison_row(row, m, lane);
  g = sq_wave_sum(g);
  if (lane == 0) {
    if (rg2 != nullptr) rg2[s] = is_bad ? (double)NAN : g / (double)m;
    bad[s] = is_bad ? 1 : 0;
    n_contacts[s] = is_bad ? -1 : 0;
    n_native[s] = is_bad ? -1 : 0;
  }
}

// grid: x = column tile, y = row tile, z = slice of the structure axis (`per` structures each, a multiple of CT_CHUNK)
__global__ __launch_bounds__(256) void contact_pairs_k(const float4* __restrict__ packed, const uint32_t* __restrict__ excl,
                                                       const uint32_t* __restrict__ native, int S, int m, int words, int per,
                                                       float cutoff2, int* __restrict__ counts, int* __restrict__ n_contacts,
                                                       int* __restrict__ n_native) {
  __shared__ float4 st[CT_CHUNK][CT_ROWS + CT_COLS];
  __shared__ ChunkCounts<int, CT_CHUNK, 2> hits;             // per structure: contacts, native contacts
  const int r0 = (int)blockIdx.y * CT_ROWS, c0 = (int)blockIdx.x * CT_COLS;
  if (!upper_tile_live(r0, c0, CT_COLS)) return;             // no column of the tile is above a row of it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = r0 + lane, cb = c0 + 32 * wave;            // this thread's row and the first of its 32 columns
  // bit u: the pair (row, cb + u) is this thread's to count -- inside the selection, above the diagonal, not excluded
  const uint32_t ok = upper_pair_bits<32>(row, cb, m, excl, words);
  uint32_t nat = 0;
  if (ok != 0 && native != nullptr) nat = ok & native[(size_t)row * words + (cb >> 5)];
  const bool wave_live = __any(ok != 0) != 0;
  int cnt[32];
#pragma unroll
  for (int u = 0; u < 32; ++u) cnt[u] = 0;
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += CT_CHUNK) {
    __syncthreads();                                         // the previous chunk has been read and its hits flushed
    // NaN past the slice or the selection: in contact with nothing
    stage_chunk<CT_CHUNK, CT_ROWS, CT_COLS>(st, packed, m, r0, c0, s0, s_end, tid, NAN);
    hits.zero(tid);
    __syncthreads();
    if (wave_live) {
#pragma unroll 1
      for (int sl = 0; sl < CT_CHUNK; ++sl) {
        const float4 a = st[sl][lane];
        uint32_t hit = 0;
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const float4 b = st[sl][CT_ROWS + 32 * wave + u];
          const bool h = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z) < cutoff2;
          cnt[u] += h ? 1 : 0;                               // pairs outside `ok` count too: they are never written
          hit |= h ? 1u << u : 0u;
        }
        hit &= ok;
        if (hit != 0) {
          hits.add(sl, 0, __popc(hit));
          if ((hit & nat) != 0) hits.add(sl, 1, __popc(hit & nat));
        }
      }
    }
    __syncthreads();
    hits.flush(s0, s_end, tid, n_contacts, n_native);
  }
#pragma unroll
  for (int u = 0; u < 32; ++u) {
    if (((ok >> u) & 1u) != 0 && cnt[u] != 0) {
      const int col = cb + u;
      atomicAdd(counts + (size_t)row * m + col, cnt[u]);
      atomicAdd(counts + (size_t)col * m + row, cnt[u]);
    }
  }
}

// grid: x = group B, y = group A (A < B works), z = slice of the structure axis (`per` structures each, a multiple of 64)
__global__ __launch_bounds__(64) void contact_groups_k(const float4* __restrict__ packed, const int* __restrict__ gstart,
                                                       const uint32_t* __restrict__ excl, const uint32_t* __restrict__ native, int S,
                                                       int m, int words, int G, int gwords, int per, float cutoff2,
                                                       int* __restrict__ group_counts, int* __restrict__ n_contacts,
                                                       int* __restrict__ n_native) {
  const int A = (int)blockIdx.y, B = (int)blockIdx.x;
  if (A >= B) return;
  const int lane = threadIdx.x;
  // the caller's table is ascending from 0 to m; whatever it holds, nothing is read outside the m packed atoms
  const int a0 = max(gstart[A], 0), na = min(gstart[A + 1], m) - a0, b0 = max(gstart[B], 0), nb = min(gstart[B + 1], m) - b0;
  if (na <= 0 || nb <= 0) return;
  int sh = 0;
  while (sh < 6 && (1 << sh) < nb) ++sh;                     // the lanes are (64 >> sh) rows of (1 << sh) columns
  const int la = lane >> sh, lb = lane & ((1 << sh) - 1), arows = 64 >> sh, bcols = 1 << sh;
  const bool is_native = native != nullptr && ((native[(size_t)A * gwords + (B >> 5)] >> (B & 31)) & 1u) != 0;
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  int total = 0;
  for (int s0 = s_begin; s0 < s_end; s0 += 64) {
    const int ns = min(64, s_end - s0);
    unsigned long long any = 0ull;                           // bit sl: one of this lane's pairs is in contact in s0 + sl
    for (int a = a0 + la; a < a0 + na; a += arows) {
      for (int b = b0 + lb; b < b0 + nb; b += bcols) {
        if (((excl[(size_t)a * words + (b >> 5)] >> (b & 31)) & 1u) != 0) continue;
        const float4* pa = packed + (size_t)s0 * m + a;
        const float4* pb = packed + (size_t)s0 * m + b;
#pragma unroll 4
        for (int sl = 0; sl < ns; ++sl) {
          const float4 x = pa[(size_t)sl * m], y = pb[(size_t)sl * m];
          if (sq_dist2(x.x, x.y, x.z, y.x, y.y, y.z) < cutoff2) any |= 1ull << sl;
        }
      }
    }
    uint32_t lo = (uint32_t)any, hi = (uint32_t)(any >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lo |= (uint32_t)__shfl_xor((int)lo, d), hi |= (uint32_t)__shfl_xor((int)hi, d);
    any = ((unsigned long long)hi << 32) | lo;               // every lane: the wave's word
    total += __popcll(any);
    if (lane < ns && ((any >> lane) & 1ull) != 0) {
      atomicAdd(n_contacts + s0 + lane, 1);
      if (is_native) atomicAdd(n_native + s0 + lane, 1);
    }
  }
  if (lane == 0 && total != 0) {
    atomicAdd(group_counts + (size_t)A * G + B, total);
    atomicAdd(group_counts + (size_t)B * G + A, total);
  }
}

static int ct_check(const void* xyz, const void* sel, const void* excl, int S, int n_atoms, int m, float cutoff2,
                    const void* n_contacts, const void* n_native, const void* bad, const void* workspace, size_t workspace_bytes,
                    const char** why) {
  *why = nullptr;
  if (S < 0 || n_atoms < 0) *why = "bad size";
  else if (S > CT_MAX_STRUCTURES) *why = "structures per launch <= cgv_contact_max_structures()";
  else if (m < 1 || m > n_atoms) *why = "1 <= m <= n_atoms";
  else if (m > CT_MAX_ATOMS) *why = "m <= cgv_contact_max_atoms()";
  else if (!(cutoff2 >= 0.f)) *why = "cutoff2 must be a number >= 0";
  else if (S == 0) return 1;
  else if (!xyz || !sel || !excl || !n_contacts || !n_native || !bad) *why = "null pointer";
  else *why = workspace_why(workspace, workspace_bytes, (size_t)S * (size_t)m * sizeof(float4), "workspace smaller than cgv_contact_workspace_bytes()");
  return 0;
}

}  // namespace cgv

extern "C" {

int cgv_contact_max_atoms(void) { return cgv::CT_MAX_ATOMS; }
int cgv_contact_max_structures(void) { return cgv::CT_MAX_STRUCTURES; }

size_t cgv_contact_workspace_bytes(int n_structures, int m) {
  if (n_structures < 0 || m < 0 || n_structures > cgv::CT_MAX_STRUCTURES || m > cgv::CT_MAX_ATOMS) return 0;
  return (size_t)n_structures * (size_t)m * sizeof(float4);
}

int cgv_contact_counts(const float* xyz, const int32_t* sel, const uint32_t* excluded, const uint32_t* native, int n_structures,
                       int n_atoms, int m, float cutoff2, int32_t* counts, int32_t* n_contacts, int32_t* n_native, double* rg2,
                       int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  const char* why;
  const int empty = cgv::ct_check(xyz, sel, excluded, n_structures, n_atoms, m, cutoff2, n_contacts, n_native, bad, workspace,
                                  workspace_bytes, &why);
  CGV_REQUIRE(why == nullptr, why);
  if (empty) return 0;
  CGV_REQUIRE(counts && rg2, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::contact_prep_k, dim3((unsigned)((n_structures + 3) / 4)), dim3(256), 0, st, xyz, sel, n_structures, n_atoms,
                     m, packed, rg2, bad, n_contacts, n_native);
  int rc = cgv::check_launch("cgv_contact_counts (preparation)");
  if (rc || m < 2) return rc;
  int per;
  const dim3 grid = cgv::pair_grid(n_structures, m, cgv::CT_ROWS, cgv::CT_COLS, cgv::CT_CHUNK, false, &per);
  hipLaunchKernelGGL(cgv::contact_pairs_k, grid, dim3(256), 0, st, packed, excluded,
                     native, n_structures, m, (m + 31) / 32, per, cutoff2, counts, n_contacts, n_native);
  return cgv::check_launch("cgv_contact_counts");
}

int cgv_contact_group_counts(const float* xyz, const int32_t* sel, const int32_t* group_start, const uint32_t* excluded,
                             const uint32_t* native, int n_structures, int n_atoms, int m, int n_groups, float cutoff2,
                             int32_t* group_counts, int32_t* n_contacts, int32_t* n_native, double* rg2, int32_t* bad,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* why;
  const int empty = cgv::ct_check(xyz, sel, excluded, n_structures, n_atoms, m, cutoff2, n_contacts, n_native, bad, workspace,
                                  workspace_bytes, &why);
  CGV_REQUIRE(why == nullptr, why);
  CGV_REQUIRE(n_groups >= 1 && n_groups <= m && n_groups <= cgv::CT_MAX_GROUPS, "1 <= n_groups <= min(m, 4096)");
  if (empty) return 0;
  CGV_REQUIRE(group_start && group_counts, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::contact_prep_k, dim3((unsigned)((n_structures + 3) / 4)), dim3(256), 0, st, xyz, sel, n_structures, n_atoms,
                     m, packed, rg2, bad, n_contacts, n_native);
  int rc = cgv::check_launch("cgv_contact_group_counts (preparation)");
  if (rc || n_groups < 2) return rc;
  const long long pairs = (long long)n_groups * (n_groups - 1) / 2;
  int per;
  const int slices = cgv::struct_slices(n_structures, pairs > cgv::PACKED_TARGET_BLOCKS ? cgv::PACKED_TARGET_BLOCKS : (int)pairs, 64, &per);
  hipLaunchKernelGGL(cgv::contact_groups_k, dim3((unsigned)n_groups, (unsigned)n_groups, (unsigned)slices), dim3(64), 0, st, packed,
                     group_start, excluded, native, n_structures, m, (m + 31) / 32, n_groups, (n_groups + 31) / 32, per, cutoff2,
                     group_counts, n_contacts, n_native);
  return cgv::check_launch("cgv_contact_group_counts");
}

}  // extern "C"
