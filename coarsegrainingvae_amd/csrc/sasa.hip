// K23 solvent-accessible surface of an ensemble (Shrake-Rupley): for every structure and every selected atom, how many
// of P points on the atom's probe-inflated sphere lie inside no other selected atom's inflated sphere.  See
// include/cgvae_hip.h.  Nothing in the reference computes it (its analysis goes through mdtraj).
//
// Point k of atom i is p = c_i + r_i * u_k per component, the product rounded, then the sum; it is BURIED iff some
// selected position j != i has sq_dist2(p, c_j) < r2_j, r2_j = r_j * r_j rounded once (sq_dist.h: fp32, every operation
// individually rounded, strict <; this file is compiled with -ffp-contract=off).  The host restates this bit for bit, and
// "some j" does not depend on the order in which the j are tried: every integer this file produces is exact, whatever the
// pre-filter keeps, in whatever order the list is walked, however often an occluder is tried twice.
//
// sasa_prep_k    one wave per structure, 4 per block: gathers the m selected atoms through sel into the packed copy
//                [S, m] float4 (x, y, z, r2_j) of the workspace, and writes the structure's flag behind it -- SA_BAD (a
//                non-finite selected coordinate), SA_FAR (a coordinate beyond SA_FILTER_MAX_COORD: the pre-filter's
//                derivation does not hold, the structure takes the unfiltered loop) or 0.  It also overwrites bad[s] and
//                the structure's row of class_counts (0, or -1 when bad) and, for a bad structure, its row of counts.
// sasa_points_k  256 threads; block b works on the atom range b % ranges of the structures b / ranges, + grid / ranges,
//                ...: the structure's packed atoms (16 B each) and the sphere points are staged in LDS once per
//                structure.  A wave owns the atoms of the range in turn.  For atom i it compacts the occluders that pass
//                the pre-filter into its own list in LDS (ballot + prefix count; capacity m - 1 rounded up to 4, so the
//                list of a collapsed structure fits), padded to a multiple of 4 by repeating its last entry.  Lanes own
//                points, 4 at a time (k = lane + 64 t); the wave walks the list 4 occluders per step -- one uniform
//                8-byte read of the indices, four broadcast 16-byte reads of the atoms -- a lane clears the bit of a
//                point at its first hit, and the wave leaves the list when no lane has a live point.  The exposed count
//                is the popcount of the ballots.  count, count^2 and the class sums are accumulated in LDS; the class
//                sums go to class_counts once per structure, the per-atom sums to atom_sum / atom_sumsq once per block.
// Sums of integers meet in atomicAdd, whose order does not matter: two runs give the same bits, and nothing depends on
// how the caller cuts the structures into launches.
//
// THE PRE-FILTER keeps j for atom i iff  sq_dist2(c_i, c_j) < fl(fl(qa * qa) * (1 + 2^-18)),  qa = fl(fl(r_i + r_j) + a),
// a = SA_FILTER_MAX_COORD * 2^-22.  It is a superset of the atoms that can bury a point of i.  With e = 2^-24 (one
// rounding), |coordinates| <= M = SA_FILTER_MAX_COORD and D = |c_i - c_j| exactly:
//   the point:  t = fl(r_i u) = r_i u (1 + d1), p = fl(c + t) = (c + t)(1 + d2), so p - c_i = r_i u + err with
//               |err| <= e r_i |u| + sqrt(3) e (M + 1.01 r_i) per vector, and |u| <= 1 + e (u is a unit vector rounded once):
//               |p - c_i| <= r_i (1 + 3.8 e) + 1.74 e M;
//   the test:   sq_dist2 rounds the difference, the square and two sums of non-negative terms: its value is the exact
//               |p - c_j|^2 (1 + th), |th| <= 6 e; r2_j <= r_j^2 (1 + e).  Buried therefore needs |p - c_j| < r_j (1 + 4 e);
//   together:   D <= |p - c_j| + |p - c_i| < X = (r_i + r_j)(1 + 4 e) + 2 e M;
//   the filter: its sq_dist2 is <= D^2 (1 + 6 e) < X^2 (1 + 6 e);  qa >= (r_i + r_j)(1 - 2 e) + 4 e M (1 - e), so
//               X <= qa (1 + 12 e) and X^2 (1 + 6 e) <= qa^2 (1 + 31 e) <= qa^2 (1 - e)^2 (1 + 64 e) <= the threshold.
// (A product that underflows adds less than 2^-126 to a sum: nothing next to a^2 = 2^-20.)  M = 4096 A makes a = 2^-10 A:
// the list holds the geometric neighbours and a shell of a thousandth of an Angstrom.  A structure with a coordinate
// beyond M is not bad: every j != i goes on its lists.
#include <math.h>

#include "cgv_common.h"
#include "sq_dist.h"

namespace cgv {

constexpr int SA_MAX_ATOMS = 4096;           // selected atoms: 64 KB of staged atoms, indices fit the lists' 16 bits
constexpr int SA_MAX_POINTS = 1024;          // 12 KB of staged sphere points, 16 points per lane
constexpr int SA_MAX_CLASSES = 64;
constexpr int SA_MAX_STRUCTURES = 1 << 20;   // per launch: count * structures stays below 2^31 in the LDS sums
constexpr int SA_WAVES = 4;
constexpr int SA_TARGET_BLOCKS = 1024;       // 4 blocks on each of 256 CUs
constexpr int SA_MIN_RANGE = 16;             // atoms of a block at least: every block stages all m atoms of a structure
constexpr float SA_FILTER_MAX_COORD = 4096.f;            // M of the derivation above
constexpr float SA_FILTER_ABS = SA_FILTER_MAX_COORD * (1.f / 4194304.f);   // a = M 2^-22
constexpr float SA_FILTER_REL = 1.f + 1.f / 262144.f;    // 1 + 2^-18
constexpr int SA_BAD = 1, SA_FAR = 2;

__host__ __device__ constexpr size_t sa_packed_bytes(int S, int m) { return (size_t)S * (size_t)m * sizeof(float4); }

__global__ __launch_bounds__(256) void sasa_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel,
                                                   const float* __restrict__ r, int S, int n, int m, int C,
                                                   float4* __restrict__ packed, int* __restrict__ flags, int* __restrict__ counts,
                                                   int* __restrict__ class_counts, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  const float* base = xyz + (size_t)s * n * 3;
  float4* row = packed + (size_t)s * m;
  bool ok = true, near = true;
  for (int k = lane; k < m; k += 64) {
    const f3 p = ld3(base + 3 * (size_t)sel_atom(sel[k], n));
    const float rk = r[k];
    ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    near = near && fabsf(p.x) <= SA_FILTER_MAX_COORD && fabsf(p.y) <= SA_FILTER_MAX_COORD && fabsf(p.z) <= SA_FILTER_MAX_COORD;
    row[k] = make_float4(p.x, p.y, p.z, __fmul_rn(rk, rk));
  }
  const bool is_bad = __any(!ok) != 0, is_far = __any(!near) != 0;
  if (lane == 0) {
    flags[s] = is_bad ? SA_BAD : is_far ? SA_FAR : 0;
    bad[s] = is_bad ? 1 : 0;
  }
  for (int c = lane; c < C; c += 64) class_counts[(size_t)s * C + c] = is_bad ? -1 : 0;
  if (is_bad && counts != nullptr)
    for (int k = lane; k < m; k += 64) counts[(size_t)s * m + k] = -1;
}

// dynamic LDS, in this order: atoms [m] float4 | sum of count^2 [alen] u64 | sum of count [alen rounded up to 2] i32 | class
// sums [SA_MAX_CLASSES] i32 | sphere points [3 P rounded up to 2] f32 | candidate lists [SA_WAVES][mpad] u16, mpad = m
// rounded up to 4: every list starts on 8 bytes
__host__ __device__ constexpr size_t sa_lds_bytes(int m, int alen, int P) {
  return (size_t)m * 16 + (size_t)alen * 8 + (size_t)((alen + 1) & ~1) * 4 + SA_MAX_CLASSES * 4 + (size_t)((3 * P + 1) & ~1) * 4 + (size_t)SA_WAVES * ((m + 3) & ~3) * 2;
}

extern __shared__ __attribute__((aligned(16))) unsigned char sa_smem[];

__global__ __launch_bounds__(256) void sasa_points_k(const float4* __restrict__ packed, const int* __restrict__ flags,
                                                     const float* __restrict__ r, const float* __restrict__ u,
                                                     const int* __restrict__ cls, int S, int m, int P, int C, int ranges, int alen,
                                                     int* __restrict__ counts, int* __restrict__ class_counts,
                                                     unsigned long long* __restrict__ atom_sum,
                                                     unsigned long long* __restrict__ atom_sumsq) {
  const int mpad = (m + 3) & ~3;
  float4* at = reinterpret_cast<float4*>(sa_smem);
  unsigned long long* acc_sq = reinterpret_cast<unsigned long long*>(at + m);
  int* acc = reinterpret_cast<int*>(acc_sq + alen);
  int* cls_acc = acc + ((alen + 1) & ~1);
  float* us = reinterpret_cast<float*>(cls_acc + SA_MAX_CLASSES);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned short* list = reinterpret_cast<unsigned short*>(us + ((3 * P + 1) & ~1)) + (size_t)wave * mpad;

  const int range = (int)blockIdx.x % ranges, s_first = (int)blockIdx.x / ranges, s_step = (int)gridDim.x / ranges;
  const int a0 = range * alen, a1 = min(m, a0 + alen);
  if (a0 >= a1) return;                                      // the whole block
  for (int e = tid; e < 3 * P; e += 256) us[e] = u[e];
  for (int e = tid; e < a1 - a0; e += 256) acc[e] = 0, acc_sq[e] = 0ull;
  if (tid < SA_MAX_CLASSES) cls_acc[tid] = 0;
  const int chunks = (P + 255) >> 8;                         // 4 points per lane at a time

  for (int s = s_first; s < S; s += s_step) {
    const int flag = flags[s];
    if (flag == SA_BAD) continue;                            // its rows were written by the preparation
    __syncthreads();                                         // the previous structure's atoms have been read
    for (int e = tid; e < m; e += 256) at[e] = packed[(size_t)s * m + e];
    __syncthreads();
    for (int i = a0 + wave; i < a1; i += SA_WAVES) {
      const float4 ci = at[i];
      const float ri = r[i];
      // the occluders that can bury a point of i, compacted into this wave's list
      int n_cand = 0;
      for (int j0 = 0; j0 < m; j0 += 64) {
        const int j = j0 + lane;
        bool keep = false;
        if (j < m && j != i) {
          const float4 cj = at[j];
          const float qa = __fadd_rn(__fadd_rn(ri, r[j]), SA_FILTER_ABS);
          keep = flag == SA_FAR || sq_dist2(ci.x, ci.y, ci.z, cj.x, cj.y, cj.z) < __fmul_rn(__fmul_rn(qa, qa), SA_FILTER_REL);
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) list[n_cand + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)j;
        n_cand += __popcll(mask);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the list is written by other lanes of this wave
      if (n_cand > 0 && (n_cand & 3) != 0) {                  // pad with the last entry: trying it again changes nothing
        const unsigned short last = list[n_cand - 1];
        if (lane < 4 - (n_cand & 3)) list[n_cand + lane] = last;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      }
      const int n_pad = (n_cand + 3) & ~3;
      int exposed = 0;
      for (int ch = 0; ch < chunks; ++ch) {
        float px[4], py[4], pz[4];
        unsigned alive = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = (ch * 4 + t) * 64 + lane;
          const int kk = k < P ? k : 0;
          px[t] = __fadd_rn(ci.x, __fmul_rn(ri, us[3 * kk]));
          py[t] = __fadd_rn(ci.y, __fmul_rn(ri, us[3 * kk + 1]));
          pz[t] = __fadd_rn(ci.z, __fmul_rn(ri, us[3 * kk + 2]));
          alive |= k < P ? 1u << t : 0u;
        }
        for (int c0 = 0; c0 < n_pad; c0 += 4) {
          if (__ballot(alive != 0) == 0ull) break;           // every live point of the wave is buried
          const uint2 idx = *reinterpret_cast<const uint2*>(list + c0);
          const float4 o[4] = {at[idx.x & 0xffffu], at[idx.x >> 16], at[idx.y & 0xffffu], at[idx.y >> 16]};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            bool hit = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) hit |= sq_dist2(px[t], py[t], pz[t], o[q].x, o[q].y, o[q].z) < o[q].w;
            alive &= hit ? ~(1u << t) : ~0u;
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) exposed += __popcll(__ballot(((alive >> t) & 1u) != 0));
      }
      if (lane == 0) {
        if (counts != nullptr) counts[(size_t)s * m + i] = exposed;
        acc[i - a0] += exposed;                              // this wave alone owns atom i in this block
        acc_sq[i - a0] += (unsigned long long)exposed * (unsigned long long)exposed;
        const int c = cls[i];
        atomicAdd(&cls_acc[(c >= 0 && c < C) ? c : 0], exposed);
      }
    }
    __syncthreads();
    if (tid < C) {
      const int v = cls_acc[tid];
      if (v != 0) atomicAdd(class_counts + (size_t)s * C + tid, v);
      cls_acc[tid] = 0;
    }
  }
  __syncthreads();
  for (int e = tid; e < a1 - a0; e += 256) {
    if (acc[e] != 0) {
      atomicAdd(atom_sum + a0 + e, (unsigned long long)acc[e]);
      atomicAdd(atom_sumsq + a0 + e, acc_sq[e]);
    }
  }
}

// how a launch is cut: `ranges` atom ranges of `alen` atoms per structure, when the structures alone do not fill the chip
static inline void sa_grid(int S, int m, int* ranges, int* alen, int* blocks) {
  int want = (SA_TARGET_BLOCKS + S - 1) / S;
  const int most = (m + SA_MIN_RANGE - 1) / SA_MIN_RANGE;
  if (want > most) want = most;
  if (want < 1) want = 1;
  *alen = (m + want - 1) / want;
  *ranges = (m + *alen - 1) / *alen;
  int per = SA_TARGET_BLOCKS / *ranges;
  if (per < 1) per = 1;
  if (per > S) per = S;
  *blocks = per * *ranges;
}

}  // namespace cgv

extern "C" {

int cgv_sasa_max_atoms(void) { return cgv::SA_MAX_ATOMS; }
int cgv_sasa_max_points(void) { return cgv::SA_MAX_POINTS; }
int cgv_sasa_max_classes(void) { return cgv::SA_MAX_CLASSES; }
int cgv_sasa_max_structures(void) { return cgv::SA_MAX_STRUCTURES; }

size_t cgv_sasa_workspace_bytes(int n_structures, int m, int n_points) {
  if (n_structures < 0 || m < 1 || n_points < 1 || n_structures > cgv::SA_MAX_STRUCTURES || m > cgv::SA_MAX_ATOMS ||
      n_points > cgv::SA_MAX_POINTS)
    return 0;
  return cgv::sa_packed_bytes(n_structures, m) + (size_t)n_structures * sizeof(int);
}

int cgv_sasa_counts(const float* xyz, const int32_t* sel, const float* r, const float* u, const int32_t* cls, int n_structures,
                    int n_atoms, int m, int n_points, int n_classes, int32_t* counts, int32_t* class_counts, int64_t* atom_sum,
                    int64_t* atom_sumsq, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
  const int S = n_structures;
  CGV_REQUIRE(S >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::SA_MAX_STRUCTURES, "structures per launch <= cgv_sasa_max_structures()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(m <= cgv::SA_MAX_ATOMS, "m <= cgv_sasa_max_atoms()");
  CGV_REQUIRE(n_points >= 1 && n_points <= cgv::SA_MAX_POINTS, "1 <= n_points <= cgv_sasa_max_points()");
  CGV_REQUIRE(n_classes >= 1 && n_classes <= cgv::SA_MAX_CLASSES, "1 <= n_classes <= cgv_sasa_max_classes()");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && sel && r && u && cls && class_counts && atom_sum && atom_sumsq && bad, "null pointer");
  CGV_REQUIRE(workspace && workspace_bytes >= cgv_sasa_workspace_bytes(S, m, n_points), "workspace smaller than cgv_sasa_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  int* flags = (int*)((char*)workspace + cgv::sa_packed_bytes(S, m));
  int ranges, alen, blocks;
  cgv::sa_grid(S, m, &ranges, &alen, &blocks);
  const size_t lds = cgv::sa_lds_bytes(m, alen, n_points);
  static bool attr_done = false;                             // the largest size once: 160 000 of the CU's 163 840 bytes
  if (!attr_done) {
    const size_t most = cgv::sa_lds_bytes(cgv::SA_MAX_ATOMS, cgv::SA_MAX_ATOMS, cgv::SA_MAX_POINTS);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cgv::sasa_points_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) { cgv::set_error("hipFuncSetAttribute(%zu bytes of LDS): %s", most, hipGetErrorString(e)); return (int)e; }
    attr_done = true;
  }
  hipLaunchKernelGGL(cgv::sasa_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, r, S, n_atoms, m, n_classes, packed,
                     flags, counts, class_counts, bad);
  int rc = cgv::check_launch("cgv_sasa_counts (preparation)");
  if (rc) return rc;
  hipLaunchKernelGGL(cgv::sasa_points_k, dim3((unsigned)blocks), dim3(256), lds, st, packed, flags, r, u, cls, S, m, n_points,
                     n_classes, ranges, alen, counts, class_counts, (unsigned long long*)atom_sum, (unsigned long long*)atom_sumsq);
  return cgv::check_launch("cgv_sasa_counts");
}

}  // extern "C"
