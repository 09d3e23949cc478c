// K21 superpose an ensemble onto a target and accumulate what a mean structure and a per-atom fluctuation are made of:
// for every structure the PROPER rotation that best fits its selected atoms onto the target's (superpose_rot.h), applied
// to ALL its atoms, and the running sums  sum [n,3] (aligned coordinates), dev2 [n] (squared distance of each aligned
// atom from the target's atom), n_good, plus rmsd2 and a `bad` flag per structure.  See include/cgvae_hip.h.  Nothing
// in the reference superposes anything.  Compiled with -ffp-contract=off.
//
// Both the structure and the target are centred on the centroid of their selected atoms; coordinates are widened on
// load, everything after is fp64.  rmsd2 = max(0, G_a + G_b - 2 lambda) / m as in K17.
//
// align_accumulate_k<G, APT>  G threads -- a wave (G = 64, four independent groups per block) or the whole block
//                   (G = 256) -- own one contiguous range of `per` structures; thread t of the group owns the atoms
//                   t, t + G, ... (at most APT of them) and keeps their four accumulators in registers for the whole
//                   range.  The selection is a bit mask in LDS, so a structure is read ONCE: the thread's atoms stay in
//                   registers for the centroid, the cross-covariance and the rotation.  Per structure two group sums
//                   (centroid and non-finite count; the nine M_ab and G_a), each a fixed tree: the xor butterfly of the
//                   wave, then, for G = 256, the four wave totals as (w0 + w1) + (w2 + w3).  Every thread then solves
//                   the same key matrix (a wave instruction costs the same for one lane as for 64) and rotates its
//                   atoms.  At the end of the range the accumulators go to the group's slice of the workspace.
// align_merge_k     one thread per atom adds the slices in ascending range order and then to the caller's sum / dev2;
//                   one more block counts the good structures into n_good.
// No floating-point atomics, no order left to the scheduler: the order of every addition is fixed by (S, n, m) and the
// form, so two identical calls give identical bits.  An index of sel outside [0, n) is ignored and an atom named twice
// counts once (the host wrapper refuses both); nothing is read or written out of bounds.
#include <math.h>

#include "cgv_common.h"
#include "superpose_rot.h"

namespace cgv {

constexpr int AL_THREADS = 256;
constexpr int AL_MAX_APT = 16;                          // atoms a thread owns at most
constexpr int AL_MAX_ATOMS = AL_THREADS * AL_MAX_APT;   // 4096
constexpr int AL_WAVE_ATOMS = 256;                      // up to here a wave owns a structure (4 atoms per lane)
constexpr int AL_MAX_STRUCTURES = 1 << 20;              // per launch
constexpr int AL_MIN_PER = 4;                           // structures of a range at least: a range ends in 32 n bytes of partials
constexpr int AL_WAVE_RANGES = 4096;                    // ranges aimed at: 4 waves on each SIMD of 256 CUs
constexpr int AL_BLOCK_RANGES = 512;                    // 2 blocks on each CU

static inline int al_form(int n_atoms, int form) { return form != 0 ? form : (n_atoms <= AL_WAVE_ATOMS ? 1 : 2); }
static inline int al_per(int S, int form) {
  const int target = form == 1 ? AL_WAVE_RANGES : AL_BLOCK_RANGES;
  const int p = (S + target - 1) / target;
  return p < AL_MIN_PER ? AL_MIN_PER : p;
}
static inline int al_ranges(int S, int form) {
  const int p = al_per(S, form);
  return (S + p - 1) / p;
}

// the sum of v[0..NV) over the G threads of a group, in every thread of it; red: [4][NV] doubles of LDS (G = 256)
template <int G, int NV>
__device__ __forceinline__ void al_group_sum(double* v, double* red) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[i] += __shfl_xor(v[i], d);
  }
  if (G == 256) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (red[i] + red[NV + i]) + (red[2 * NV + i] + red[3 * NV + i]);
    __syncthreads();                                         // red may be written again
  }
}

template <int G, int APT>
__global__ __launch_bounds__(AL_THREADS) void align_accumulate_k(const float* __restrict__ xyz, const int* __restrict__ sel,
                                                                 const double* __restrict__ ref, int S, int n, int m, int per,
                                                                 int ranges, double* __restrict__ part, double* __restrict__ rmsd2,
                                                                 int* __restrict__ bad, float* __restrict__ aligned) {
  __shared__ uint32_t mask[AL_MAX_ATOMS / 32];
  __shared__ double red[4 * 10];
  const int tid = threadIdx.x;
  for (int w = tid; w < AL_MAX_ATOMS / 32; w += AL_THREADS) mask[w] = 0u;
  __syncthreads();
  for (int k = tid; k < m; k += AL_THREADS) {
    const int a = sel[k];
    if (a >= 0 && a < n) atomicOr(&mask[a >> 5], 1u << (a & 31));
  }
  __syncthreads();
  const int gl = G == 64 ? (tid & 63) : tid;
  const int range = G == 64 ? (int)blockIdx.x * 4 + (tid >> 6) : (int)blockIdx.x;
  if (range >= ranges) return;                               // G = 64 only: whole waves leave, no barrier follows
  uint32_t own = 0, selected = 0;                            // bit j: atom gl + G j exists / is selected
#pragma unroll
  for (int j = 0; j < APT; ++j) {
    const int i = gl + G * j;
    if (i < n) {
      own |= 1u << j;
      if ((mask[i >> 5] >> (i & 31)) & 1u) selected |= 1u << j;
    }
  }
  // the target: centroid over the selection, G_b
  double t4[4] = {0.0, 0.0, 0.0, (double)__popc(selected)};
#pragma unroll
  for (int j = 0; j < APT; ++j) {
    if ((selected >> j) & 1u) {
      const double* r = ref + 3 * (size_t)(gl + G * j);
      t4[0] += r[0], t4[1] += r[1], t4[2] += r[2];
    }
  }
  al_group_sum<G, 4>(t4, red);
  const double meff = t4[3], bx = t4[0] / meff, by = t4[1] / meff, bz = t4[2] / meff;
  double gb[1] = {0.0};
#pragma unroll
  for (int j = 0; j < APT; ++j) {
    if ((selected >> j) & 1u) {
      const double* r = ref + 3 * (size_t)(gl + G * j);
      const double dx = r[0] - bx, dy = r[1] - by, dz = r[2] - bz;
      gb[0] += (dx * dx + dy * dy) + dz * dz;
    }
  }
  al_group_sum<G, 1>(gb, red);

  double acc[APT][4];
#pragma unroll
  for (int j = 0; j < APT; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0;
  const int s_begin = range * per, s_end = min(S, s_begin + per);
  for (int s = s_begin; s < s_end; ++s) {
    const float* base = xyz + (size_t)s * n * 3;
    float* out = aligned != nullptr ? aligned + (size_t)s * n * 3 : nullptr;
    float x[APT][3];
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < APT; ++j) {
      x[j][0] = x[j][1] = x[j][2] = 0.f;
      if ((own >> j) & 1u) {
        const f3 p = ld3(base + 3 * (size_t)(gl + G * j));
        x[j][0] = p.x, x[j][1] = p.y, x[j][2] = p.z;
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) c4[3] += 1.0;
        if ((selected >> j) & 1u) c4[0] += (double)p.x, c4[1] += (double)p.y, c4[2] += (double)p.z;
      }
    }
    al_group_sum<G, 4>(c4, red);
    if (c4[3] != 0.0) {                                      // the same value in every thread of the group
      if (gl == 0) rmsd2[s] = (double)NAN, bad[s] = 1;
      if (out != nullptr) {
#pragma unroll
        for (int j = 0; j < APT; ++j)
          if ((own >> j) & 1u) st3(out + 3 * (size_t)(gl + G * j), NAN, NAN, NAN);
      }
      continue;
    }
    const double ax = c4[0] / meff, ay = c4[1] / meff, az = c4[2] / meff;
    double mv[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // M_ab row-major, G_a
#pragma unroll
    for (int j = 0; j < APT; ++j) {
      if ((selected >> j) & 1u) {
        const double* r = ref + 3 * (size_t)(gl + G * j);
        const double a[3] = {(double)x[j][0] - ax, (double)x[j][1] - ay, (double)x[j][2] - az};
        const double b[3] = {r[0] - bx, r[1] - by, r[2] - bz};
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int v = 0; v < 3; ++v) mv[3 * u + v] += a[u] * b[v];
        mv[9] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
      }
    }
    al_group_sum<G, 10>(mv, red);
    double R[9], q[4];
    const double lambda = sp_rotation(mv, R, q);
    if (gl == 0) rmsd2[s] = fmax(0.0, mv[9] + gb[0] - 2.0 * lambda) / meff, bad[s] = 0;
#pragma unroll
    for (int j = 0; j < APT; ++j) {
      if ((own >> j) & 1u) {
        const double* r = ref + 3 * (size_t)(gl + G * j);
        const double a0 = (double)x[j][0] - ax, a1 = (double)x[j][1] - ay, a2 = (double)x[j][2] - az;
        const double y0 = (R[0] * a0 + R[1] * a1) + R[2] * a2, y1 = (R[3] * a0 + R[4] * a1) + R[5] * a2,
                     y2 = (R[6] * a0 + R[7] * a1) + R[8] * a2;
        const double dx = y0 - (r[0] - bx), dy = y1 - (r[1] - by), dz = y2 - (r[2] - bz);
        acc[j][0] += y0, acc[j][1] += y1, acc[j][2] += y2;
        acc[j][3] += (dx * dx + dy * dy) + dz * dz;
        if (out != nullptr) st3(out + 3 * (size_t)(gl + G * j), (float)y0, (float)y1, (float)y2);
      }
    }
  }
  double* mine = part + (size_t)range * 4 * n;               // [range][x, y, z, dev2][atom]
#pragma unroll
  for (int j = 0; j < APT; ++j) {
    if ((own >> j) & 1u) {
#pragma unroll
      for (int c = 0; c < 4; ++c) mine[(size_t)c * n + gl + G * j] = acc[j][c];
    }
  }
}

// blocks 0 .. ceil(n / 256) - 1: the atoms; the last block: n_good
__global__ __launch_bounds__(AL_THREADS) void align_merge_k(const double* __restrict__ part, const int* __restrict__ bad, int ranges,
                                                            int n, int S, double* __restrict__ sum, double* __restrict__ dev2,
                                                            int* __restrict__ n_good) {
  __shared__ int good;
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 == gridDim.x) {
    if (tid == 0) good = 0;
    __syncthreads();
    int mine = 0;
    for (int s = tid; s < S; s += AL_THREADS) mine += bad[s] == 0 ? 1 : 0;
    if (mine != 0) atomicAdd(&good, mine);
    __syncthreads();
    if (tid == 0) *n_good += good;
    return;
  }
  const int i = (int)blockIdx.x * AL_THREADS + tid;
  if (i >= n) return;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < ranges; ++r) {                         // ascending ranges: a fixed order
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] += part[((size_t)r * 4 + c) * n + i];
  }
  sum[3 * (size_t)i] += t[0], sum[3 * (size_t)i + 1] += t[1], sum[3 * (size_t)i + 2] += t[2];
  dev2[i] += t[3];
}

template <int G, int APT>
static void al_launch(int blocks, hipStream_t st, const float* xyz, const int* sel, const double* ref, int S, int n, int m, int per,
                      int ranges, double* part, double* rmsd2, int* bad, float* aligned) {
  hipLaunchKernelGGL((align_accumulate_k<G, APT>), dim3((unsigned)blocks), dim3(AL_THREADS), 0, st, xyz, sel, ref, S, n, m, per,
                     ranges, part, rmsd2, bad, aligned);
}

}  // namespace cgv

extern "C" {

int cgv_align_max_atoms(void) { return cgv::AL_MAX_ATOMS; }
int cgv_align_max_structures(void) { return cgv::AL_MAX_STRUCTURES; }
int cgv_align_wave_fits(int n_atoms) { return n_atoms >= 1 && n_atoms <= cgv::AL_WAVE_ATOMS ? 1 : 0; }

size_t cgv_align_workspace_bytes(int n_structures, int n_atoms, int form) {
  if (n_structures < 0 || n_atoms < 0 || n_structures > cgv::AL_MAX_STRUCTURES || n_atoms > cgv::AL_MAX_ATOMS) return 0;
  if (form < 0 || form > 2 || (form == 1 && !cgv_align_wave_fits(n_atoms))) return 0;
  return (size_t)cgv::al_ranges(n_structures, cgv::al_form(n_atoms, form)) * 4 * (size_t)n_atoms * sizeof(double);
}

int cgv_align_accumulate(const float* xyz, const int32_t* sel, const double* ref, int n_structures, int n_atoms, int m, int form,
                         double* sum, double* dev2, int32_t* n_good, double* rmsd2, int32_t* bad, float* aligned, void* workspace,
                         size_t workspace_bytes, void* stream) {
  using namespace cgv;
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 1, "bad size");
  CGV_REQUIRE(n_structures <= AL_MAX_STRUCTURES, "structures per launch <= cgv_align_max_structures()");
  CGV_REQUIRE(n_atoms <= AL_MAX_ATOMS, "n_atoms <= cgv_align_max_atoms()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(form >= 0 && form <= 2, "form: 0 (rule), 1 (a wave per structure), 2 (a block per structure)");
  CGV_REQUIRE(form != 1 || cgv_align_wave_fits(n_atoms), "form 1 holds cgv_align_wave_fits() atoms");
  if (n_structures == 0) return 0;
  CGV_REQUIRE(xyz && sel && ref && sum && dev2 && n_good && rmsd2 && bad, "null pointer");
  const int S = n_structures, n = n_atoms, f = al_form(n, form), per = al_per(S, f), ranges = al_ranges(S, f);
  CGV_REQUIRE(workspace && workspace_bytes >= (size_t)ranges * 4 * (size_t)n * sizeof(double),
              "workspace smaller than cgv_align_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
#define AL_GO(G, APT) al_launch<G, APT>(blocks, st, xyz, sel, ref, S, n, m, per, ranges, part, rmsd2, bad, aligned)
  if (f == 1) {
    const int blocks = (ranges + 3) / 4, apt = (n + 63) / 64;
    if (apt <= 1) AL_GO(64, 1);
    else if (apt <= 2) AL_GO(64, 2);
    else AL_GO(64, 4);
  } else {
    const int blocks = ranges, apt = (n + AL_THREADS - 1) / AL_THREADS;
    if (apt <= 1) AL_GO(256, 1);
    else if (apt <= 2) AL_GO(256, 2);
    else if (apt <= 4) AL_GO(256, 4);
    else if (apt <= 8) AL_GO(256, 8);
    else AL_GO(256, 16);
  }
#undef AL_GO
  int rc = check_launch("cgv_align_accumulate");
  if (rc) return rc;
  hipLaunchKernelGGL(align_merge_k, dim3((unsigned)((n + AL_THREADS - 1) / AL_THREADS + 1)), dim3(AL_THREADS), 0, st, part, bad, ranges,
                     n, S, sum, dev2, n_good);
  return check_launch("cgv_align_accumulate (merge)");
}

}  // extern "C"
