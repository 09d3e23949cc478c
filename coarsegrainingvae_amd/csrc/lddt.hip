// K28 local distance difference test (lDDT, Mariani et al. 2013) and steric clashes of an ensemble: S model structures, each
// scored WITHOUT superposition against the reference structure ref_index names for it.  Per structure and per selected atom:
// the pairs within the inclusion radius in the reference, those of them whose distance the model keeps to within each of four
// thresholds, and the pairs of non-bonded atoms that overlap.  See include/cgvae_hip.h.  Nothing in the reference computes it.
//
// For an unordered pair {i, j}, i != j, of the m selected atoms, in fp32 with every operation rounded on its own (this file is
// compiled with -ffp-contract=off; sqrtf is the correctly rounded form, see csrc/tica.hip):
//   q0 = sq_dist2(ref_i, ref_j)      q = sq_dist2(x_i, x_j)                              csrc/sq_dist.h
//   included     iff  not excl_lddt  and  q0 < radius2
//   e = fabsf(sqrtf(q) - sqrtf(q0))
//   preserved_k  iff  included  and  e < t_k                                             k = 0 .. 3, t ascending
//   c = (r_i + r_j) - tol
//   clash        iff  not excl_clash  and  c > 0  and  q < c * c
// Every comparison is strict and false for a NaN.  The host restates the tests bit for bit, so every integer this file
// produces is exact; no floating-point number leaves the device.  A model structure with a non-finite selected coordinate,
// or scored against a reference with one, is bad: its six counts are -1 and it enters no sum.
//
// lddt_prep_k    one wave per structure, 4 per block; launched for the references, then for the models.  packed_dev.h's
//                gather_structure fills a packed copy [count, m] float4 of the workspace (what the pair kernel streams).
//                The reference launch writes a flag per reference, the model launch reads the flag of its structure's
//                reference and writes bad and the six struct_counts (0 or -1).
// lddt_pairs_k   256 threads, grid (column tiles of 128, row tiles of 64, slices of the structure axis) over the FULL m x m
//                grid of ordered pairs: thread t owns row t & 63 and the 32 columns of wave t >> 6 -- one word of the bit
//                masks -- and keeps the row's six counters in registers, so atom_counts needs no transposed add.  LD_CHUNK
//                structures at a time go through LDS (row atom: one ds_read_b128 per lane, column atom: one address for the
//                wave), staged here and not by stage_chunk: one loop fills a model's slot and, where it is needed, its
//                reference's, and skips a slot by the table the first thread wrote.  What depends on the reference alone -- sqrtf(q0) of the thread's 32 pairs and their inclusion word
//                -- stays in registers and is recomputed (and the reference staged) only when ref_index changes between
//                consecutive good structures: a single native reference costs one distance per pair, not two.  The
//                per-structure counts take the pairs above the diagonal only (tiles wholly below it add nothing): three
//                packed wave sums, lane 0 adds them to the chunk's counters (packed_dev.h: ChunkCounts), the block to
//                struct_counts once per structure.  Bad structures are skipped, so nothing relies on NaN.  At the end a nonzero row counter is
//                added to atom_counts.
// Sums of integers meet in atomicAdd (LDS and global), whose order does not matter: two runs give the same bits, and nothing
// depends on how the caller cuts the structures into launches.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int LD_ROWS = 64;                  // rows of a tile: the lanes of a wave
constexpr int LD_COLS = 128;                 // columns of a tile: 4 waves x one 32-bit mask word
constexpr int LD_STAGE = LD_ROWS + LD_COLS;  // float4 of a staged structure
constexpr int LD_CHUNK = 8;                  // structures staged at once: 2 x 8 x 192 x 16 B = 48 KB of LDS (model + reference)
constexpr int LD_N = 6;                      // included, preserved at four thresholds, clashes
constexpr int LD_MAX_ATOMS = 8192;           // selected atoms: the two masks are 8 MB each there; m^2 / 2 pairs < 2^31
constexpr int LD_MAX_STRUCTURES = 1 << 20;   // per launch
constexpr int LD_MAX_REFERENCES = 1 << 20;   // per launch

// grid: 4 structures per block.  refbad_out != nullptr: the reference launch; otherwise the model launch
__global__ __launch_bounds__(256) void lddt_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int count, int n, int m,
                                                   float4* __restrict__ packed, const int* __restrict__ ridx,
                                                   const int* __restrict__ refbad_in, int* __restrict__ refbad_out,
                                                   int* __restrict__ bad, int* __restrict__ struct_counts) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= count) return;                                    // whole waves leave
  bool is_bad = !gather_structure(xyz + (size_t)s * n * 3, [=](int k) { return sel[k]; }, n, m, packed + (size_t)s * m, lane);
  if (refbad_out != nullptr) {
    if (lane == 0) refbad_out[s] = is_bad ? 1 : 0;
    return;
  }
  is_bad = is_bad || refbad_in[ridx[s]] != 0;                // ridx was checked on the host: inside [0, n_references)
  if (lane < LD_N) struct_counts[(size_t)s * LD_N + lane] = is_bad ? -1 : 0;
  if (lane == 0) bad[s] = is_bad ? 1 : 0;
}

// grid: x = column tile, y = row tile, z = slice of the structure axis (`per` structures each, a multiple of LD_CHUNK)
__global__ __launch_bounds__(256) void lddt_pairs_k(const float4* __restrict__ P, const float4* __restrict__ Q,
                                                    const int* __restrict__ ridx, const int* __restrict__ bad,
                                                    const uint32_t* __restrict__ excl_l, const uint32_t* __restrict__ excl_c,
                                                    const float* __restrict__ radii, int S, int m, int words, int per,
                                                    float radius2, float t0, float t1, float t2, float t3, float tol,
                                                    int* __restrict__ struct_counts, unsigned long long* __restrict__ atom_counts) {
  __shared__ float4 sm[LD_CHUNK][LD_STAGE];                  // the models of the chunk
  __shared__ float4 sr[LD_CHUNK][LD_STAGE];                  // the reference of a model, where it differs from the one before
  __shared__ ChunkCounts<int, LD_CHUNK, LD_N> hits;
  __shared__ int sref[LD_CHUNK];                             // the reference of a structure; -1: skipped (bad, past the slice)
  __shared__ int sneed[LD_CHUNK];                            // 1: its reference is staged
  const int r0 = (int)blockIdx.y * LD_ROWS, c0 = (int)blockIdx.x * LD_COLS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = r0 + lane, cb = c0 + 32 * wave;            // this thread's row and the first of its 32 columns
  // bit u of okl / okc: the ordered pair (row, cb + u) counts for the distance test / as a clash -- inside the selection,
  // off the diagonal, not excluded.  `above`: cb + u > row, the pairs the per-structure counts take
  uint32_t okl = 0, okc = 0, above = 0;
  if (row < m && cb < m) {
    const uint32_t inside = word_inside(cb, m);
    const uint32_t off = row >= cb && row < cb + 32 ? ~(1u << (row - cb)) : 0xffffffffu;
    okl = inside & off & ~excl_l[(size_t)row * words + (cb >> 5)];
    okc = inside & off & ~excl_c[(size_t)row * words + (cb >> 5)];
    above = word_above(row, cb);
  }
  const bool wave_live = __any((okl | okc) != 0) != 0;
  const bool tile_above = upper_tile_live(r0, c0, LD_COLS);  // the same for the whole block
  float cc2[32];                                             // c * c of a pair, -1 where c > 0 fails: q < cc2 is the clash test
  {
    const float ri = row < m ? radii[row] : 0.f;
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const float rj = cb + u < m ? radii[cb + u] : 0.f;
      const float c = __fsub_rn(__fadd_rn(ri, rj), tol);
      cc2[u] = c > 0.f ? __fmul_rn(c, c) : -1.f;
    }
  }
  float d0[32];                                              // sqrtf(q0) of the thread's pairs in the reference `cur`
#pragma unroll
  for (int u = 0; u < 32; ++u) d0[u] = 0.f;
  uint32_t incl = 0;                                         // bit u: the pair is included under `cur`
  int cur = -1, n_incl = 0;                                  // the reference the registers hold (the same in every thread)
  int cnt[LD_N];
#pragma unroll
  for (int k = 0; k < LD_N; ++k) cnt[k] = 0;
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += LD_CHUNK) {
    __syncthreads();                                         // the previous chunk has been read and its hits flushed
    if (tid == 0) {
      int c = cur;
      for (int sl = 0; sl < LD_CHUNK; ++sl) {
        const int s = s0 + sl;
        const int r = s < s_end && bad[s] == 0 ? ridx[s] : -1;
        sref[sl] = r;
        sneed[sl] = r >= 0 && r != c ? 1 : 0;
        if (r >= 0) c = r;
      }
    }
    hits.zero(tid);
    __syncthreads();
    for (int e = tid; e < LD_CHUNK * LD_STAGE; e += 256) {
      const int sl = e / LD_STAGE, a = e - sl * LD_STAGE, r = sref[sl];
      if (r < 0) continue;                                   // a skipped structure's slots are never read
      const int at = a < LD_ROWS ? r0 + a : c0 + a - LD_ROWS;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);            // past the selection: outside every mask
      if (at < m) v = P[(size_t)(s0 + sl) * m + at];
      sm[sl][a] = v;
      if (sneed[sl] != 0) {
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (at < m) w = Q[(size_t)r * m + at];
        sr[sl][a] = w;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < LD_CHUNK; ++sl) {
      const int r = sref[sl];
      if (r < 0) continue;                                   // the same for the whole block
      const bool fresh = r != cur;
      cur = r;
      if (!wave_live) continue;
      if (fresh) {
        const float4 a = sr[sl][lane];
        uint32_t in = 0;
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const float4 b = sr[sl][LD_ROWS + 32 * wave + u];
          const float q0 = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z);
          d0[u] = sqrtf(q0);
          in |= q0 < radius2 ? 1u << u : 0u;
        }
        incl = in & okl;
        n_incl = __popc(incl);
      }
      const float4 a = sm[sl][lane];
      uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0, cl = 0;
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const float4 b = sm[sl][LD_ROWS + 32 * wave + u];
        const float q = sq_dist2(a.x, a.y, a.z, b.x, b.y, b.z);
        const float e = fabsf(__fsub_rn(sqrtf(q), d0[u]));
        p0 |= e < t0 ? 1u << u : 0u;
        p1 |= e < t1 ? 1u << u : 0u;
        p2 |= e < t2 ? 1u << u : 0u;
        p3 |= e < t3 ? 1u << u : 0u;
        cl |= q < cc2[u] ? 1u << u : 0u;
      }
      p0 &= incl, p1 &= incl, p2 &= incl, p3 &= incl, cl &= okc;
      cnt[0] += n_incl, cnt[1] += __popc(p0), cnt[2] += __popc(p1), cnt[3] += __popc(p2), cnt[4] += __popc(p3), cnt[5] += __popc(cl);
      if (tile_above) {
        // a lane has at most 32 of each, the wave at most 2048: two counts to a word
        const int v01 = sq_wave_sum((int)(__popc(incl & above) | (__popc(p0 & above) << 16)));
        const int v23 = sq_wave_sum((int)(__popc(p1 & above) | (__popc(p2 & above) << 16)));
        const int v45 = sq_wave_sum((int)(__popc(p3 & above) | (__popc(cl & above) << 16)));
        if (lane == 0) {
          if ((v01 & 0xffff) != 0) hits.add(sl, 0, v01 & 0xffff);
          if ((v01 >> 16) != 0) hits.add(sl, 1, v01 >> 16);
          if ((v23 & 0xffff) != 0) hits.add(sl, 2, v23 & 0xffff);
          if ((v23 >> 16) != 0) hits.add(sl, 3, v23 >> 16);
          if ((v45 & 0xffff) != 0) hits.add(sl, 4, v45 & 0xffff);
          if ((v45 >> 16) != 0) hits.add(sl, 5, v45 >> 16);
        }
      }
    }
    __syncthreads();
    hits.flush(s0, s_end, tid, struct_counts);
  }
  if (row < m) {
#pragma unroll
    for (int k = 0; k < LD_N; ++k)
      if (cnt[k] != 0) atomicAdd(atom_counts + (size_t)row * LD_N + k, (unsigned long long)cnt[k]);
  }
}

static inline bool ld_sizes_ok(int S, int T, int m) {
  return S >= 0 && T >= 0 && m >= 0 && S <= LD_MAX_STRUCTURES && T <= LD_MAX_REFERENCES && m <= LD_MAX_ATOMS;
}
// the packed models [S, m] and references [T, m] as float4, then ref_index [S] and the references' flags [T] as int32
static inline size_t ld_workspace(int S, int T, int m) {
  const size_t bytes = ((size_t)S + (size_t)T) * (size_t)m * sizeof(float4) + ((size_t)S + (size_t)T) * sizeof(int);
  return (bytes + 15) / 16 * 16;
}
static inline bool ld_length(float v) { return v >= 0.f && v <= 3.0e38f; }   // a finite number >= 0; false for a NaN

}  // namespace cgv

extern "C" {

int cgv_lddt_max_atoms(void) { return cgv::LD_MAX_ATOMS; }
int cgv_lddt_max_structures(void) { return cgv::LD_MAX_STRUCTURES; }
int cgv_lddt_max_references(void) { return cgv::LD_MAX_REFERENCES; }
int cgv_lddt_row_tile(void) { return cgv::LD_ROWS; }
int cgv_lddt_col_tile(void) { return cgv::LD_COLS; }
int cgv_lddt_chunk(void) { return cgv::LD_CHUNK; }

size_t cgv_lddt_workspace_bytes(int n_structures, int n_references, int m) {
  return cgv::ld_sizes_ok(n_structures, n_references, m) ? cgv::ld_workspace(n_structures, n_references, m) : 0;
}

int cgv_lddt_counts(const float* xyz, const float* ref_xyz, const int32_t* ref_index, const int32_t* sel, const uint32_t* excl_lddt,
                    const uint32_t* excl_clash, const float* radii, int n_structures, int n_references, int n_atoms, int m,
                    float radius2, float t0, float t1, float t2, float t3, float tolerance, int32_t* struct_counts,
                    int64_t* atom_counts, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  const int S = n_structures, T = n_references;
  CGV_REQUIRE(S >= 0 && T >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::LD_MAX_STRUCTURES, "structures per launch <= cgv_lddt_max_structures()");
  CGV_REQUIRE(T <= cgv::LD_MAX_REFERENCES, "references per launch <= cgv_lddt_max_references()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(m <= cgv::LD_MAX_ATOMS, "m <= cgv_lddt_max_atoms()");
  CGV_REQUIRE(cgv::ld_length(radius2), "radius2 must be a finite number >= 0");
  CGV_REQUIRE(cgv::ld_length(t0) && cgv::ld_length(t1) && cgv::ld_length(t2) && cgv::ld_length(t3),
              "a threshold must be a finite number >= 0");
  CGV_REQUIRE(t0 < t1 && t1 < t2 && t2 < t3, "the thresholds must be ascending");
  CGV_REQUIRE(cgv::ld_length(tolerance), "the clash tolerance must be a finite number >= 0");
  if (S == 0) return 0;
  CGV_REQUIRE(T >= 1, "structures need at least one reference");
  CGV_REQUIRE(xyz && ref_xyz && ref_index && sel && excl_lddt && excl_clash && radii && struct_counts && atom_counts && bad, "null pointer");
  for (int s = 0; s < S; ++s) CGV_REQUIRE(ref_index[s] >= 0 && ref_index[s] < T, "ref_index outside [0, n_references)");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::ld_workspace(S, T, m), "workspace smaller than cgv_lddt_workspace_bytes()");
  CGV_REQUIRE(why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* P = (float4*)workspace;
  float4* Q = P + (size_t)S * m;
  int* ridx = (int*)(Q + (size_t)T * m);
  int* refbad = ridx + S;
  const hipError_t e = hipMemcpyAsync(ridx, ref_index, (size_t)S * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    cgv::set_error("cgv_lddt_counts (ref_index): %s", hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(cgv::lddt_prep_k, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, ref_xyz, sel, T, n_atoms, m, Q,
                     (const int*)nullptr, (const int*)nullptr, refbad, (int*)nullptr, (int*)nullptr);
  int rc = cgv::check_launch("cgv_lddt_counts (references)");
  if (rc) return rc;
  hipLaunchKernelGGL(cgv::lddt_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, S, n_atoms, m, P, (const int*)ridx,
                     (const int*)refbad, (int*)nullptr, bad, struct_counts);
  rc = cgv::check_launch("cgv_lddt_counts (preparation)");
  if (rc || m < 2) return rc;
  int per;
  const dim3 grid = cgv::pair_grid(S, m, cgv::LD_ROWS, cgv::LD_COLS, cgv::LD_CHUNK, true, &per);   // the full grid: ordered pairs
  hipLaunchKernelGGL(cgv::lddt_pairs_k, grid, dim3(256), 0, st, (const float4*)P,
                     (const float4*)Q, (const int*)ridx, (const int*)bad, excl_lddt, excl_clash, radii, S, m, (m + 31) / 32, per,
                     radius2, t0, t1, t2, t3, tolerance, struct_counts, (unsigned long long*)atom_counts);
  return cgv::check_launch("cgv_lddt_counts");
}

}  // extern "C"
