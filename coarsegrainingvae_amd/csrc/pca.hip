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
// (its y is NaN and is never multiplied); in the projection its components are NaN and it counts once in `outside`.
//
// The split into structure ranges, the tile and lane maps, the MFMA step, the stores, the reduction of the ranges' partials
// and the whole projection kernel (gram_project_k<K, PcaFeature> in a profile) are gram_dev.h's, shared with K16.  What is K27's:
//   pca_moments_k   a sample is a structure.  The block stages the features of its row tile and its column tile and adds
//                   one product, F_i^T F_j.  Diagonal blocks also sum F_i over the structures; the block of tile pair 0
//                   counts the good structures of its range (integers: a fixed tree, exact).
//   slice           cov [dp,dp] (exactly symmetric), sum [dp], then the count of good structures.
// The selection is validated in the kernels: an index outside [0, n) reads atom 0, nothing is read out of bounds.
#include "gram_dev.h"

namespace cgv {

// what bounds it is total plus workspace bytes: one [d,d] fp64 total is 32 MB at 2048 features; from 1409 features on (45
// tiles, 1035 tile pairs) a launch has ONE range, whose slice of the workspace is as large again: 64 MB together.  Below,
// the ranges' slices together stay under 34 MB (gram_range: about 1024 blocks, whatever d).  m <= 682 atoms, so m = 512
// fits; eigh of 2048 x 2048 is host seconds.
constexpr int PM_MAX_FEATURES = 2048;
constexpr int PM_MAX_ATOMS = 1 << 20;
constexpr int PM_MAX_STRUCTURES = 1 << 20;    // per launch, K21's (the aligned chunk is its output)

__host__ __device__ inline size_t pm_slice(int d) { return gram_slice(d, 1, 1, 1); }

// where feature `feat` (< d) of a structure lies: 3 * atom + component, the atom validated
__device__ __forceinline__ size_t pca_offset(const int* __restrict__ sel, int feat, int n) {
  const int a = feat / 3, c = feat - 3 * a, v = sel[a];
  return 3 * (size_t)sel_atom(v, n) + (size_t)c;
}

// grid: x = upper tile pair, y = structure range
__global__ __launch_bounds__(GRAM_THREADS) void pca_moments_k(const float* __restrict__ y, const int* __restrict__ sel,
                                                              const double* __restrict__ centre, const int* __restrict__ bad, int S,
                                                              int n, int d, int per_range, double* __restrict__ ws) {
  __shared__ double st[2][GRAM_STAGE][GRAM_TILE];            // F_i, F_j of the stage, structure major (8 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = gram_tiles(d);
  const GramTile g = gram_tile(nt);
  const bool diag = g.diag;
  // a thread stages one feature of the row tile and the same slot of the column tile, for two structures of the stage
  const int f = g.f;
  const int fi = g.bi * GRAM_TILE + f, fj = g.bj * GRAM_TILE + f;
  const bool live_i = fi < d, live_j = fj < d && !diag;
  const size_t oi = live_i ? pca_offset(sel, fi, n) : 0, oj = live_j ? pca_offset(sel, fj, n) : 0;
  const double ci = live_i ? centre[oi] : 0.0, cj = live_j ? centre[oj] : 0.0;
  const int s_begin = (int)blockIdx.y * per_range;           // s_begin < S (the host's grid)
  const int s_end = min(S, s_begin + per_range);
  const size_t per = 3 * (size_t)n;
  const double (*xi)[GRAM_TILE] = st[0];
  const double (*xj)[GRAM_TILE] = diag ? st[0] : st[1];
  gram_d4 acc = {0.0, 0.0, 0.0, 0.0};
  double fsum = 0.0;                                         // diagonal blocks: tid < 32 sums F_i[tid]
  for (int s0 = s_begin; s0 < s_end; s0 += GRAM_STAGE) {
    __syncthreads();                                         // the previous stage has been read
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = g.k0 + 8 * u, s = s0 + k;
      const bool in = s < s_end && bad[s] == 0;              // && short-circuits: bad is read inside the range only
      const float* base = y + per * (size_t)(in ? s : s_begin);
      st[0][k][f] = (in && live_i) ? (double)base[oi] - ci : 0.0;
      if (!diag) st[1][k][f] = (in && live_j) ? (double)base[oj] - cj : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GRAM_STAGE / 4; ++q) gram_mfma(xi[4 * q + g.mk], xj[4 * q + g.mk], g, acc);
    if (diag && tid < GRAM_TILE) gram_add_column(fsum, st[0], tid);
  }
  const size_t dp = (size_t)nt * GRAM_TILE;
  double* __restrict__ out = ws + (size_t)blockIdx.y * pm_slice(d);
  gram_store(out, dp, g.bi, g.bj, g, acc);
  if (diag && tid < GRAM_TILE) out[dp * dp + (size_t)g.bi * GRAM_TILE + tid] = fsum;
  if (blockIdx.x == 0 && wave == 0) {                        // the good structures of the range, below 2^20: exact as a double
    int good = 0;
    for (int s = s_begin + lane; s < s_end; s += 64) good += bad[s] == 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) good += __shfl_xor(good, w);
    if (lane == 0) out[dp * dp + dp] = (double)good;
  }
}

// the projection's features: a structure is good iff K21 said so
struct PcaFeature {
  const float* y;
  const int* sel;
  const double* centre;
  const int* bad;
  int n;
  __device__ bool good(int s) const { return bad[s] == 0; }
  __device__ double value(int s, int f) const {
    const size_t o = pca_offset(sel, f, n);
    return (double)y[3 * (size_t)n * (size_t)s + o] - centre[o];
  }
};

}  // namespace cgv

extern "C" {

int cgv_pca_max_features(void) { return cgv::PM_MAX_FEATURES; }
int cgv_pca_max_atoms(void) { return cgv::PM_MAX_ATOMS; }
int cgv_pca_max_structures(void) { return cgv::PM_MAX_STRUCTURES; }
int cgv_pca_max_components(void) { return cgv::GRAM_MAX_K; }
int cgv_pca_max_bins2(void) { return cgv::GRAM_MAX_BINS2; }

int cgv_pca_moments_splits(int n_structures, int d) {
  return (d <= cgv::PM_MAX_FEATURES && n_structures <= cgv::PM_MAX_STRUCTURES) ? cgv::gram_splits(n_structures, d) : 0;
}

size_t cgv_pca_moments_workspace_bytes(int n_structures, int d) {
  if (d < 1 || d > cgv::PM_MAX_FEATURES || n_structures > cgv::PM_MAX_STRUCTURES) return 0;
  const int splits = cgv::gram_splits(n_structures, d);
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
  const int d = 3 * m, nt = cgv::gram_tiles(d), splits = cgv::gram_splits(n_structures, d);
  CGV_REQUIRE(workspace && workspace_bytes >= (size_t)splits * cgv::pm_slice(d) * sizeof(double),
              "workspace smaller than cgv_pca_moments_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const int per_range = (int)cgv::gram_range(n_structures, d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cgv::pca_moments_k, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)splits), dim3(cgv::GRAM_THREADS), 0, st, y, sel,
                     centre, bad, n_structures, n_atoms, d, per_range, (double*)workspace);
  int rc = cgv::check_launch("cgv_pca_moments");
  if (rc) return rc;
  return cgv::gram_reduce<1, 1, 1, 1>("cgv_pca_moments (reduction)", workspace, d, splits, {{cov}, {sum}, n_good}, st);
}

int cgv_pca_project(const float* y, const int32_t* sel, const double* centre, const int32_t* bad, const double* mean,
                    const double* W, int n_structures, int n_atoms, int m, int k, double* proj, int comp_a, int comp_b, int n_bins2,
                    double lo_a, double hi_a, double lo_b, double hi_b, int32_t* counts, int32_t* outside, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && m >= 0, "bad size");
  CGV_REQUIRE(m <= cgv::PM_MAX_FEATURES / 3, "3 m <= cgv_pca_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::PM_MAX_ATOMS, "n_atoms <= cgv_pca_max_atoms()");
  CGV_REQUIRE(n_structures <= cgv::PM_MAX_STRUCTURES, "n_structures <= cgv_pca_max_structures()");
  const cgv::GramHist h = {comp_a, comp_b, n_bins2, lo_a, hi_a, lo_b, hi_b, counts, outside};
  if (int rc = cgv::gram_project_refuses("pca", k, h)) return rc;
  if (n_structures == 0 || n_atoms == 0 || (!proj && !counts)) return 0;
  CGV_REQUIRE(y && bad && (m == 0 || (sel && centre && mean && W)), "null pointer");
  return cgv::gram_launch_project("cgv_pca_project", cgv::PcaFeature{y, sel, centre, bad, n_atoms}, mean, W, n_structures, 3 * m, k,
                                  proj, h, (hipStream_t)stream);
}

}  // extern "C"
