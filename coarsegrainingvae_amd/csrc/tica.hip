// K16 time-lagged independent component analysis: the moments a TICA fit needs and the projection of structures onto a
// fitted model -- what the reference does offline with pyemma (CoarseGrainingVAE/postanalysis.py: pairwise backbone
// distances, tica(lag), transform).  See include/cgvae_hip.h.
//
// A feature is the distance of one atom pair of one frame: fp32 (dx*dx + dy*dy) + dz*dz exactly as sq_dist2, a
// correctly rounded fp32 square root, then widened to fp64 (this file is built without FMA contraction), so a host
// restatement in float32 holds the same bits and everything after it differs by fp64 summation order only.  No
// [T, d] feature tensor exists in memory.
//
// The split into frame ranges, the tile and lane maps, the MFMA step, the stores, the reduction of the ranges' partials and
// the whole projection kernel (gram_project_k<K, TicaFeature> in a profile) are gram_dev.h's, shared with K27.  What is K16's:
//   tica_moments_k   a sample is a frame pair (t, t + lag), N = T - lag of them.  The block stages the features of its row
//                    tile and its column tile at t (X) and at t + lag (Y) from xyz (n * 12 bytes per frame: L2 resident)
//                    and adds four products: X_i X_j^T, Y_i Y_j^T, X_i Y_j^T and (off the diagonal) X_j Y_i^T, the tile of
//                    cxy below the diagonal.  Diagonal blocks also sum X_i and Y_i over the frames.
//   slice            cxx, cyy, cxy [dp,dp], then sum_x, sum_y [dp]; cxx and cyy are exactly symmetric.
// Pair tables are validated in the kernels: an atom index outside [0, n) reads atom 0, nothing is read out of bounds.
// Non-finite coordinates propagate into the sums (moments) / count in `outside` (projection).
#include "gram_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int TM_MAX_FEATURES = 2048;         // three [d,d] fp64 totals: 96 MB, and as much workspace per range
constexpr int TM_MAX_ATOMS = 1 << 20;

// frame pairs of a segment of T frames
static inline long long tm_pairs(long long T, int lag) { return (lag >= 1 && T > lag) ? T - lag : 0; }
__host__ __device__ inline size_t tm_slice(int d) { return gram_slice(d, 3, 2, 0); }

// the fp32 distance of atoms (a, b) of the frame at `base`, widened.  sqrtf, not __fsqrt_rn: without the library's
// rounded-operation build the intrinsic is the native square root (v_sqrt_f32 alone, 1 ulp), while sqrtf is expanded to
// the correctly rounded sequence (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), which is what numpy gives.
__device__ __forceinline__ double tica_feature(const float* __restrict__ base, int a, int b) {
  const float* p = base + 3 * (size_t)a;
  const float* q = base + 3 * (size_t)b;
  return (double)sqrtf(sq_dist2(p[0], p[1], p[2], q[0], q[1], q[2]));
}

// grid: x = upper tile pair, y = frame range
__global__ __launch_bounds__(GRAM_THREADS) void tica_moments_k(const float* __restrict__ xyz, const int* __restrict__ pairs, int N,
                                                               int n, int d, int lag, int per_range, double* __restrict__ ws) {
  __shared__ double st[4][GRAM_STAGE][GRAM_TILE];            // X_i, Y_i, X_j, Y_j of the stage, frame major (16 KB)
  const int tid = threadIdx.x;
  const int nt = gram_tiles(d);
  const GramTile g = gram_tile(nt);
  const bool diag = g.diag;
  // a thread stages one feature of the row tile and the same slot of the column tile, for two frames of the stage
  const int f = g.f;
  int ai[2], aj[2];
  const int fi = g.bi * GRAM_TILE + f, fj = g.bj * GRAM_TILE + f;
  const bool live_i = fi < d, live_j = fj < d && !diag;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int vi = live_i ? pairs[2 * (size_t)fi + a] : 0, vj = live_j ? pairs[2 * (size_t)fj + a] : 0;
    ai[a] = sel_atom(vi, n), aj[a] = sel_atom(vj, n);
  }
  const int t_begin = (int)blockIdx.y * per_range;           // t_begin < N (the host's grid)
  const int t_end = min(N, t_begin + per_range);
  const size_t per = 3 * (size_t)n;
  const double (*xi)[GRAM_TILE] = st[0];
  const double (*yi)[GRAM_TILE] = st[1];
  const double (*xj)[GRAM_TILE] = diag ? st[0] : st[2];
  const double (*yj)[GRAM_TILE] = diag ? st[1] : st[3];
  gram_d4 cxx = {0.0, 0.0, 0.0, 0.0}, cyy = cxx, cxy = cxx, cyx = cxx;
  double fsum = 0.0;                                         // diagonal blocks: tid < 32 sums X_i[tid], tid < 64 Y_i[tid - 32]
  for (int t0 = t_begin; t0 < t_end; t0 += GRAM_STAGE) {
    __syncthreads();                                         // the previous stage has been read
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = g.k0 + 8 * u, t = t0 + k;
      const bool in = t < t_end;
      const float* bx = xyz + per * (size_t)(in ? t : t_begin);
      const float* by = xyz + per * (size_t)(in ? t + lag : t_begin);
      st[0][k][f] = (in && live_i) ? tica_feature(bx, ai[0], ai[1]) : 0.0;
      st[1][k][f] = (in && live_i) ? tica_feature(by, ai[0], ai[1]) : 0.0;
      if (!diag) {
        st[2][k][f] = (in && live_j) ? tica_feature(bx, aj[0], aj[1]) : 0.0;
        st[3][k][f] = (in && live_j) ? tica_feature(by, aj[0], aj[1]) : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < GRAM_STAGE / 4; ++s) {
      const int k = 4 * s + g.mk;
      gram_mfma(xi[k], xj[k], g, cxx);
      gram_mfma(yi[k], yj[k], g, cyy);
      gram_mfma(xi[k], yj[k], g, cxy);
      if (!diag) gram_mfma(xj[k], yi[k], g, cyx);
    }
    if (diag && tid < 64) gram_add_column(fsum, st[tid >> 5], tid & 31);
  }
  const size_t dp = (size_t)nt * GRAM_TILE;
  double* __restrict__ out = ws + (size_t)blockIdx.y * tm_slice(d);
  gram_store(out, dp, g.bi, g.bj, g, cxx);
  gram_store(out + dp * dp, dp, g.bi, g.bj, g, cyy);
  gram_store(out + 2 * dp * dp, dp, g.bi, g.bj, g, cxy);
  if (!diag) gram_store(out + 2 * dp * dp, dp, g.bj, g.bi, g, cyx);
  if (diag && tid < 64) out[3 * dp * dp + (size_t)(tid >> 5) * dp + (size_t)g.bi * GRAM_TILE + (tid & 31)] = fsum;
}

// the projection's features: every structure is good
struct TicaFeature {
  const float* xyz;
  const int* pairs;
  int n;
  __device__ bool good(int) const { return true; }
  __device__ double value(int s, int f) const {
    const int a = pairs[2 * (size_t)f], b = pairs[2 * (size_t)f + 1];
    return tica_feature(xyz + 3 * (size_t)n * (size_t)s, sel_atom(a, n), sel_atom(b, n));
  }
};

}  // namespace cgv

extern "C" {

int cgv_tica_max_features(void) { return cgv::TM_MAX_FEATURES; }
int cgv_tica_max_atoms(void) { return cgv::TM_MAX_ATOMS; }
int cgv_tica_max_bins2(void) { return cgv::GRAM_MAX_BINS2; }
int cgv_tica_max_components(void) { return cgv::GRAM_MAX_K; }

int cgv_tica_moments_splits(int n_frames, int d, int lag) {
  return (d <= cgv::TM_MAX_FEATURES) ? cgv::gram_splits(cgv::tm_pairs(n_frames, lag), d) : 0;
}

size_t cgv_tica_moments_workspace_bytes(int n_frames, int d, int lag) {
  if (d < 1 || d > cgv::TM_MAX_FEATURES) return 0;
  const int splits = cgv::gram_splits(cgv::tm_pairs(n_frames, lag), d);
  return (size_t)(splits > 0 ? splits : 1) * cgv::tm_slice(d) * sizeof(double);
}

int cgv_tica_moments(const float* xyz, const int32_t* pairs, int n_frames, int n_atoms, int d, int lag, double* sum_x,
                     double* sum_y, double* cxx, double* cyy, double* cxy, void* workspace, size_t workspace_bytes,
                     void* stream) {
  CGV_REQUIRE(n_frames >= 0 && n_atoms >= 0 && d >= 0, "bad size");
  CGV_REQUIRE(lag >= 1, "lag >= 1");
  CGV_REQUIRE(d <= cgv::TM_MAX_FEATURES, "d <= cgv_tica_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::TM_MAX_ATOMS, "n_atoms <= cgv_tica_max_atoms()");
  if (n_frames <= lag || d == 0 || n_atoms == 0) return 0;
  CGV_REQUIRE(xyz && pairs && sum_x && sum_y && cxx && cyy && cxy, "null pointer");
  const int N = n_frames - lag, nt = cgv::gram_tiles(d), splits = cgv::gram_splits(N, d);
  CGV_REQUIRE(workspace && workspace_bytes >= (size_t)splits * cgv::tm_slice(d) * sizeof(double),
              "workspace smaller than cgv_tica_moments_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const int per_range = (int)cgv::gram_range(N, d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cgv::tica_moments_k, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)splits), dim3(cgv::GRAM_THREADS), 0, st, xyz,
                     pairs, N, n_atoms, d, lag, per_range, (double*)workspace);
  int rc = cgv::check_launch("cgv_tica_moments");
  if (rc) return rc;
  return cgv::gram_reduce<3, 2, 2, 0>("cgv_tica_moments (reduction)", workspace, d, splits, {{cxx, cyy, cxy}, {sum_x, sum_y}, nullptr}, st);
}

int cgv_tica_project(const float* xyz, const int32_t* pairs, const double* mean, const double* W, int n_structures,
                     int n_atoms, int d, int k, double* ics, int comp_a, int comp_b, int n_bins2, double lo_a, double hi_a,
                     double lo_b, double hi_b, int32_t* counts, int32_t* outside, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && d >= 0, "bad size");
  CGV_REQUIRE(d <= cgv::TM_MAX_FEATURES, "d <= cgv_tica_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::TM_MAX_ATOMS, "n_atoms <= cgv_tica_max_atoms()");
  const cgv::GramHist h = {comp_a, comp_b, n_bins2, lo_a, hi_a, lo_b, hi_b, counts, outside};
  if (int rc = cgv::gram_project_refuses("tica", k, h)) return rc;
  if (n_structures == 0 || n_atoms == 0 || (!ics && !counts)) return 0;
  CGV_REQUIRE(xyz && (d == 0 || (pairs && mean && W)), "null pointer");
  return cgv::gram_launch_project("cgv_tica_project", cgv::TicaFeature{xyz, pairs, n_atoms}, mean, W, n_structures, d, k, ics, h,
                                  (hipStream_t)stream);
}

}  // extern "C"
