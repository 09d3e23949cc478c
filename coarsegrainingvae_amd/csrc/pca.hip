// K27 Cartesian principal component analysis ("essential dynamics", Amadei et al. 1993) of a superposed ensemble: the
// moments a covariance needs and the projection of structures onto fitted modes.  See include/cgvae_hip.h.
//
// Both entry points read what K21 (align_mean.hip) writes for a chunk: y [S,n,3] fp32, the structures superposed onto a
// target, and bad [S] int32.  The superposition is NOT repeated here -- every tile pair would redo it.
// A feature is one coordinate of one selected atom about a point the caller gives:
//   f[3a + c] = (double)y[s, sel[a], c] - centre[sel[a], c],  a < m, c < 3,  d = 3m
// The widening is exact and the subtraction one fp64 rounding (this file is built without FMA contraction), so a host
// restatement in numpy holds the same bits and everything after it differs by fp64 summation order only.  No [S, d]
// feature tensor exists in memory.  A structure with bad[s] != 0 contributes nothing: its features are staged as +0.0
// (its y is NaN and is never multiplied), as are features past d and structures past a range (adding +0.0 is exact).
//
// cgv_pca_moments, two launches:
//   pca_moments_k   256 threads, grid (upper tile pairs bi <= bj of PM_TILE = 32 features, structure ranges).  Per stage of
//                   PM_STAGE = 16 structures the block stages the features of its row tile and its column tile into LDS as
//                   fp64, structure major; wave w owns the 16 x 16 sub-tile (w >> 1, w & 1) and adds F_i^T F_j per 4
//                   structures with v_mfma_f64_16x16x4_f64 (A: row = lane & 15, depth = lane >> 4; B likewise with the
//                   column; result register r of lane l: row (l >> 4) + 4 r, column l & 15).  Diagonal blocks also sum
//                   their 32 features over the structures in ascending order; the block of tile pair 0 counts the good
//                   structures of its range (integers: a fixed tree, exact).  Each block writes its tile to its range's
//                   slice of the workspace: no floating-point atomics.
//   pca_reduce_k    one thread per output element: the ranges' partials summed in ascending order, added to the caller's
//                   totals; cov below the diagonal is read from above it (exactly symmetric).
// cgv_pca_project: one wave per structure; each lane sums its strided share of the features in ascending order, the fixed
// xor tree combines the lanes (every lane then holds the same sum); lane 0 writes the components and bins two of them into
// the block's LDS histogram (integer atomics), flushed with one integer vector atomic per non-zero slot.
// The bin rule is K16's (cgv_tica_project): for lo <= v < hi in fp64 the bin is floor((v - lo) * n_bins2 / (hi - lo)),
// clamped to [0, n_bins2) against rounding alone; a structure with either component outside its range, a NaN, or a bad
// structure counts once in `outside`.
// The selection is validated in the kernels: an index outside [0, n) reads atom 0, nothing is read out of bounds.
#include "cgv_common.h"

namespace cgv {

constexpr int PM_THREADS = 256;
constexpr int PM_TILE = 32;                   // features of a block's row / column tile: 2 x 2 MFMA tiles, one per wave
constexpr int PM_STAGE = 16;                  // structures of a stage: 4 MFMA steps of depth 4
// what bounds it is total plus workspace bytes: one [d,d] fp64 total is 32 MB at 2048 features; from 1409 features on (45
// tiles, 1035 tile pairs) a launch has ONE range, whose slice of the workspace is as large again: 64 MB together.  Below,
// the ranges' slices together stay under 34 MB (pm_range: about 1024 blocks, whatever d).  m <= 682 atoms, so m = 512
// fits; eigh of 2048 x 2048 is host seconds.
constexpr int PM_MAX_FEATURES = 2048;
constexpr int PM_MAX_ATOMS = 1 << 20;
constexpr int PM_MAX_STRUCTURES = 1 << 20;    // per launch, K21's (the aligned chunk is its output)
constexpr int PM_TARGET_BLOCKS = 1024;        // four per CU, K16's rule
constexpr int PM_MIN_RANGE = 256;             // structures of a range, at least (a range's partials cost a pass of the reduction)
constexpr int PM_MAX_SPLITS = 256;
constexpr int PP_THREADS = 256;
constexpr int PP_MAX_K = 8;
constexpr int PP_MAX_BINS2 = 64;              // 64 x 64 int32 slots of a block's LDS histogram (16 KB)
constexpr int PP_MAX_BLOCKS = 1024;

typedef double pm_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int pm_tiles(int d) { return (d + PM_TILE - 1) / PM_TILE; }

// structures of one range (a multiple of the stage) and the number of ranges for S > 0 structures
static inline long long pm_range(long long S, int d) {
  const long long nt = pm_tiles(d), pairs = nt * (nt + 1) / 2;
  long long want = (PM_TARGET_BLOCKS + pairs - 1) / pairs;
  if (want > PM_MAX_SPLITS) want = PM_MAX_SPLITS;
  long long per = (S + want - 1) / want;
  if (per < PM_MIN_RANGE) per = PM_MIN_RANGE;
  return (per + PM_STAGE - 1) / PM_STAGE * PM_STAGE;
}
static inline int pm_splits(long long S, int d) {
  if (d < 1 || S < 1) return 0;
  const long long per = pm_range(S, d);
  return (int)((S + per - 1) / per);
}
// one range's slice of the workspace (doubles): cov [dp,dp], sum [dp], then the count of good structures; dp = tiles * 32
__host__ __device__ inline size_t pm_slice(int d) {
  const size_t dp = (size_t)pm_tiles(d) * PM_TILE;
  return dp * dp + dp + 1;
}

// where feature `feat` (< d) of a structure lies: 3 * atom + component, the atom validated
__device__ __forceinline__ size_t pca_offset(const int* __restrict__ sel, int feat, int n) {
  const int a = feat / 3, c = feat - 3 * a, v = sel[a];
  return 3 * (size_t)((v >= 0 && v < n) ? v : 0) + (size_t)c;
}

// grid: x = upper tile pair (row-major over bi <= bj), y = structure range
__global__ __launch_bounds__(PM_THREADS) void pca_moments_k(const float* __restrict__ y, const int* __restrict__ sel,
                                                            const double* __restrict__ centre, const int* __restrict__ bad, int S,
                                                            int n, int d, int per_range, double* __restrict__ ws) {
  __shared__ double st[2][PM_STAGE][PM_TILE];                // F_i, F_j of the stage, structure major (8 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = pm_tiles(d);
  int bi = 0, p = (int)blockIdx.x;                           // (uniform) the tile pair
  while (p >= nt - bi) {
    p -= nt - bi;
    ++bi;
  }
  const int bj = bi + p;
  const bool diag = bi == bj;
  // a thread stages one feature of the row tile and the same slot of the column tile, for two structures of the stage
  const int f = tid & 31, k0 = tid >> 5;
  const int fi = bi * PM_TILE + f, fj = bj * PM_TILE + f;
  const bool live_i = fi < d, live_j = fj < d && !diag;
  const size_t oi = live_i ? pca_offset(sel, fi, n) : 0, oj = live_j ? pca_offset(sel, fj, n) : 0;
  const double ci = live_i ? centre[oi] : 0.0, cj = live_j ? centre[oj] : 0.0;
  const int s_begin = (int)blockIdx.y * per_range;           // s_begin < S (the host's grid)
  const int s_end = min(S, s_begin + per_range);
  const size_t per = 3 * (size_t)n;
  const double (*xi)[PM_TILE] = st[0];
  const double (*xj)[PM_TILE] = diag ? st[0] : st[1];
  const int sr = (wave >> 1) * 16, sc = (wave & 1) * 16;     // the wave's sub-tile
  const int ml = lane & 15, mk = lane >> 4;                  // A: row ml, depth mk; B: depth mk, column ml
  pm_d4 acc = {0.0, 0.0, 0.0, 0.0};
  double fsum = 0.0;                                         // diagonal blocks: tid < 32 sums F_i[tid]
  for (int s0 = s_begin; s0 < s_end; s0 += PM_STAGE) {
    __syncthreads();                                         // the previous stage has been read
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = k0 + 8 * u, s = s0 + k;
      const bool in = s < s_end && bad[s] == 0;              // && short-circuits: bad is read inside the range only
      const float* base = y + per * (size_t)(in ? s : s_begin);
      st[0][k][f] = (in && live_i) ? (double)base[oi] - ci : 0.0;
      if (!diag) st[1][k][f] = (in && live_j) ? (double)base[oj] - cj : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PM_STAGE / 4; ++q) {
      const int k = 4 * q + mk;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xi[k][sr + ml], xj[k][sc + ml], acc, 0, 0, 0);
    }
    if (diag && tid < PM_TILE) {
#pragma unroll
      for (int k = 0; k < PM_STAGE; ++k) fsum += st[0][k][tid];
    }
  }
  // result layout of the f64 MFMA: register r of lane l is row (l >> 4) + 4 r, column l & 15
  const size_t dp = (size_t)nt * PM_TILE;
  double* __restrict__ out = ws + (size_t)blockIdx.y * pm_slice(d);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const size_t row = (size_t)(sr + mk + 4 * r), col = (size_t)(sc + ml);
    out[((size_t)bi * PM_TILE + row) * dp + (size_t)bj * PM_TILE + col] = acc[r];
  }
  if (diag && tid < PM_TILE) out[dp * dp + (size_t)bi * PM_TILE + tid] = fsum;
  if (blockIdx.x == 0 && wave == 0) {                        // the good structures of the range, below 2^20: exact as a double
    int good = 0;
    for (int s = s_begin + lane; s < s_end; s += 64) good += bad[s] == 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) good += __shfl_xor(good, w);
    if (lane == 0) out[dp * dp + dp] = (double)good;
  }
}

// one thread per element of [cov | sum | n_good]
__global__ __launch_bounds__(256) void pca_reduce_k(const double* __restrict__ ws, int d, int splits, double* __restrict__ sum,
                                                    double* __restrict__ cov, int* __restrict__ n_good) {
  const size_t dd = (size_t)d * d, total = dd + (size_t)d + 1;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t dp = (size_t)pm_tiles(d) * PM_TILE, slice = pm_slice(d);
  size_t src;
  if (e < dd) {
    const size_t i = e / d, j = e - i * d;
    src = i > j ? j * dp + i : i * dp + j;                   // only the upper triangle is trusted
  } else {
    src = dp * dp + (e - dd < (size_t)d ? e - dd : dp);
  }
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += ws[(size_t)s * slice + src];
  if (e < dd) cov[e] += acc;
  else if (e - dd < (size_t)d) sum[e - dd] += acc;
  else *n_good += (int)acc;                                  // a sum of integers below 2^28
}

template <int K>
__global__ __launch_bounds__(PP_THREADS) void pca_project_k(const float* __restrict__ y, const int* __restrict__ sel,
                                                            const double* __restrict__ centre, const int* __restrict__ bad,
                                                            const double* __restrict__ mean, const double* __restrict__ W, int S,
                                                            int n, int d, double* __restrict__ proj, int ca, int cb, int nb,
                                                            double lo_a, double hi_a, double lo_b, double hi_b,
                                                            int* __restrict__ counts, int* __restrict__ outside) {
  __shared__ int hist[PP_MAX_BINS2 * PP_MAX_BINS2 + 1];      // the last slot: outside
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = counts ? nb * nb : 0;
  if (counts) {
    for (int w = tid; w < words; w += PP_THREADS) hist[w] = 0;
    if (tid == 0) hist[PP_MAX_BINS2 * PP_MAX_BINS2] = 0;
    __syncthreads();
  }
  const size_t per = 3 * (size_t)n;
  for (int s = (int)blockIdx.x * (PP_THREADS / 64) + wave; s < S; s += (int)gridDim.x * (PP_THREADS / 64)) {
    const bool good = bad[s] == 0;                           // (uniform over the wave)
    const float* base = y + per * (size_t)s;
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    if (good) {
      for (int f = lane; f < d; f += 64) {
        const size_t o = pca_offset(sel, f, n);
        const double v = ((double)base[o] - centre[o]) - mean[f];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] += v * W[(size_t)f * K + c];
      }
    }
    double va = 0.0, vb = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      double v = acc[c];
#pragma unroll
      for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w);   // fixed tree: the same bits on every run, in every lane
      if (!good) v = (double)NAN;
      if (proj && lane == 0) proj[(size_t)s * K + c] = v;
      if (c == ca) va = v;
      if (c == cb) vb = v;
    }
    if (counts && lane == 0) {
      // (v - lo) * nb / (hi - lo); lo <= v < hi: rounding alone could leave [0, nb)
      const bool in = va >= lo_a && va < hi_a && vb >= lo_b && vb < hi_b;   // false for a NaN
      if (in) {
        const int ia = min(nb - 1, max(0, (int)floor((va - lo_a) * (double)nb / (hi_a - lo_a))));
        const int ib = min(nb - 1, max(0, (int)floor((vb - lo_b) * (double)nb / (hi_b - lo_b))));
        atomicAdd(&hist[ia * nb + ib], 1);
      } else {
        atomicAdd(&hist[PP_MAX_BINS2 * PP_MAX_BINS2], 1);
      }
    }
  }
  if (counts) {
    __syncthreads();
    for (int w = tid; w < words; w += PP_THREADS) {
      const int c = hist[w];
      if (c != 0) atomicAdd(counts + w, c);
    }
    if (tid == 0 && hist[PP_MAX_BINS2 * PP_MAX_BINS2] != 0) atomicAdd(outside, hist[PP_MAX_BINS2 * PP_MAX_BINS2]);
  }
}

}  // namespace cgv

extern "C" {

int cgv_pca_max_features(void) { return cgv::PM_MAX_FEATURES; }
int cgv_pca_max_atoms(void) { return cgv::PM_MAX_ATOMS; }
int cgv_pca_max_structures(void) { return cgv::PM_MAX_STRUCTURES; }
int cgv_pca_max_components(void) { return cgv::PP_MAX_K; }
int cgv_pca_max_bins2(void) { return cgv::PP_MAX_BINS2; }

int cgv_pca_moments_splits(int n_structures, int d) {
  return (d <= cgv::PM_MAX_FEATURES && n_structures <= cgv::PM_MAX_STRUCTURES) ? cgv::pm_splits(n_structures, d) : 0;
}

size_t cgv_pca_moments_workspace_bytes(int n_structures, int d) {
  if (d < 1 || d > cgv::PM_MAX_FEATURES || n_structures > cgv::PM_MAX_STRUCTURES) return 0;
  const int splits = cgv::pm_splits(n_structures, d);
  return (size_t)(splits > 0 ? splits : 1) * cgv::pm_slice(d) * sizeof(double);
}

int cgv_pca_moments(const float* y, const int32_t* sel, const double* centre, const int32_t* bad, int n_structures, int n_atoms,
                    int m, double* sum, double* cov, int32_t* n_good, void* workspace, size_t workspace_bytes, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && m >= 0, "bad size");
  CGV_REQUIRE(m <= cgv::PM_MAX_FEATURES / 3, "3 m <= cgv_pca_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::PM_MAX_ATOMS, "n_atoms <= cgv_pca_max_atoms()");
  CGV_REQUIRE(n_structures <= cgv::PM_MAX_STRUCTURES, "n_structures <= cgv_pca_max_structures()");
  if (n_structures == 0 || m == 0 || n_atoms == 0) return 0;
  CGV_REQUIRE(y && sel && centre && bad && sum && cov && n_good, "null pointer");
  const int d = 3 * m, splits = cgv::pm_splits(n_structures, d);
  CGV_REQUIRE(workspace && workspace_bytes >= (size_t)splits * cgv::pm_slice(d) * sizeof(double),
              "workspace smaller than cgv_pca_moments_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const int nt = cgv::pm_tiles(d);
  const int per_range = (int)cgv::pm_range(n_structures, d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cgv::pca_moments_k, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)splits), dim3(cgv::PM_THREADS), 0, st, y, sel,
                     centre, bad, n_structures, n_atoms, d, per_range, (double*)workspace);
  int rc = cgv::check_launch("cgv_pca_moments");
  if (rc) return rc;
  const size_t total = (size_t)d * d + (size_t)d + 1;
  hipLaunchKernelGGL(cgv::pca_reduce_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)workspace, d, splits,
                     sum, cov, n_good);
  return cgv::check_launch("cgv_pca_moments (reduction)");
}

int cgv_pca_project(const float* y, const int32_t* sel, const double* centre, const int32_t* bad, const double* mean,
                    const double* W, int n_structures, int n_atoms, int m, int k, double* proj, int comp_a, int comp_b, int n_bins2,
                    double lo_a, double hi_a, double lo_b, double hi_b, int32_t* counts, int32_t* outside, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && m >= 0, "bad size");
  CGV_REQUIRE(m <= cgv::PM_MAX_FEATURES / 3, "3 m <= cgv_pca_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::PM_MAX_ATOMS, "n_atoms <= cgv_pca_max_atoms()");
  CGV_REQUIRE(n_structures <= cgv::PM_MAX_STRUCTURES, "n_structures <= cgv_pca_max_structures()");
  CGV_REQUIRE(k >= 1 && k <= cgv::PP_MAX_K, "1 <= k <= cgv_pca_max_components()");
  CGV_REQUIRE((counts == nullptr) == (outside == nullptr), "counts and outside come together");
  if (counts) {
    CGV_REQUIRE(n_bins2 >= 1 && n_bins2 <= cgv::PP_MAX_BINS2, "1 <= n_bins2 <= cgv_pca_max_bins2()");
    CGV_REQUIRE(comp_a >= 0 && comp_a < k && comp_b >= 0 && comp_b < k, "histogram components must be in [0, k)");
    CGV_REQUIRE(lo_a < hi_a && lo_b < hi_b && hi_a - lo_a < 1e300 && hi_b - lo_b < 1e300 && lo_a > -1e300 && lo_b > -1e300,
                "histogram ranges must be finite with lo < hi");
  }
  if (n_structures == 0 || n_atoms == 0 || (!proj && !counts)) return 0;
  CGV_REQUIRE(y && bad && (m == 0 || (sel && centre && mean && W)), "null pointer");
  const int waves = cgv::PP_THREADS / 64;
  int blocks = (n_structures + waves - 1) / waves;
  if (blocks > cgv::PP_MAX_BLOCKS) blocks = cgv::PP_MAX_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
#define CGV_PCA_PROJECT(KK)                                                                                                \
  case KK:                                                                                                                 \
    hipLaunchKernelGGL(cgv::pca_project_k<KK>, dim3((unsigned)blocks), dim3(cgv::PP_THREADS), 0, st, y, sel, centre, bad, mean, W, \
                       n_structures, n_atoms, 3 * m, proj, comp_a, comp_b, n_bins2, lo_a, hi_a, lo_b, hi_b, counts, outside); \
    break;
  switch (k) {
    CGV_PCA_PROJECT(1) CGV_PCA_PROJECT(2) CGV_PCA_PROJECT(3) CGV_PCA_PROJECT(4)
    CGV_PCA_PROJECT(5) CGV_PCA_PROJECT(6) CGV_PCA_PROJECT(7) CGV_PCA_PROJECT(8)
  }
#undef CGV_PCA_PROJECT
  return cgv::check_launch("cgv_pca_project");
}

}  // extern "C"
