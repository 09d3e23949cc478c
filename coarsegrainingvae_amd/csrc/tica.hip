// K16 time-lagged independent component analysis: the moments a TICA fit needs and the projection of structures onto a
// fitted model -- what the reference does offline with pyemma (CoarseGrainingVAE/postanalysis.py: pairwise backbone
// distances, tica(lag), transform).  See include/cgvae_hip.h.
//
// A feature is the distance of one atom pair of one frame: fp32 (dx*dx + dy*dy) + dz*dz exactly as sq_dist2, a
// correctly rounded fp32 square root, then widened to fp64 (this file is built without FMA contraction), so a host
// restatement in float32 holds the same bits and everything after it differs by fp64 summation order only.  No
// [T, d] feature tensor exists in memory.
//
// cgv_tica_moments, two launches:
//   tica_moments_k   256 threads, grid (upper tile pairs bi <= bj of TM_TILE = 32 features, frame ranges).  Per stage of
//                    TM_STAGE = 16 frame pairs the block computes the features of its row tile and its column tile at t
//                    (X) and at t + lag (Y) from xyz (n * 12 bytes per frame: L2 resident) into LDS as fp64, frame major;
//                    wave w owns the 16 x 16 sub-tile (w >> 1, w & 1) and adds four products per 4 frames with
//                    v_mfma_f64_16x16x4_f64: X_i X_j^T, Y_i Y_j^T, X_i Y_j^T and (off the diagonal) X_j Y_i^T, the tile
//                    of cxy below the diagonal.  Diagonal blocks also sum their 32 features over the frames in ascending
//                    order.  Frames past the range and features past d are staged as +0.0 (adding it is exact).
//                    Each block writes its tiles to its range's slice of the workspace: no floating-point atomics.
//   tica_reduce_k    one thread per output element: the ranges' partials summed in ascending order, added to the
//                    caller's totals; cxx / cyy below the diagonal are read from above it (exactly symmetric).
// cgv_tica_project: one wave per structure; each lane sums its strided share of the features in ascending order, the
// fixed tree of sq_wave_sum combines the lanes; lane 0 writes the components and bins two of them into the block's LDS
// histogram (integer atomics), flushed with one integer vector atomic per non-zero slot.
// Pair tables are validated in the kernels: an atom index outside [0, n) reads atom 0, nothing is read out of bounds.
// Non-finite coordinates propagate into the sums (moments) / count in `outside` (projection).
#include "sq_dist.h"

namespace cgv {

constexpr int TM_THREADS = 256;
constexpr int TM_TILE = 32;                   // features of a block's row / column tile: 2 x 2 MFMA tiles, one per wave
constexpr int TM_STAGE = 16;                  // frame pairs of a stage: 4 MFMA steps of depth 4
constexpr int TM_MAX_FEATURES = 2048;         // three [d,d] fp64 totals: 96 MB, and as much workspace per range
constexpr int TM_MAX_ATOMS = 1 << 20;
constexpr int TM_TARGET_BLOCKS = 1024;        // four per CU
constexpr int TM_MIN_RANGE = 256;             // frame pairs of a range, at least (a range's partials cost a pass of the reduction)
constexpr int TM_MAX_SPLITS = 256;
constexpr int TP_THREADS = 256;
constexpr int TP_MAX_K = 8;
constexpr int TP_MAX_BINS2 = 64;              // 64 x 64 int32 slots of a block's LDS histogram (16 KB)
constexpr int TP_MAX_BLOCKS = 1024;

typedef double tm_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int tm_tiles(int d) { return (d + TM_TILE - 1) / TM_TILE; }

// frame pairs of one range (a multiple of the stage) and the number of ranges for N = T - lag > 0 frame pairs
static inline long long tm_range(long long N, int d) {
  const long long nt = tm_tiles(d), pairs = nt * (nt + 1) / 2;
  long long want = (TM_TARGET_BLOCKS + pairs - 1) / pairs;
  if (want > TM_MAX_SPLITS) want = TM_MAX_SPLITS;
  long long per = (N + want - 1) / want;
  if (per < TM_MIN_RANGE) per = TM_MIN_RANGE;
  return (per + TM_STAGE - 1) / TM_STAGE * TM_STAGE;
}
static inline int tm_splits(long long T, int d, int lag) {
  if (d < 1 || lag < 1 || T <= lag) return 0;
  const long long N = T - lag, per = tm_range(N, d);
  return (int)((N + per - 1) / per);
}
// one range's slice of the workspace (doubles): cxx, cyy, cxy [dp,dp] each, then sum_x, sum_y [dp]; dp = tiles * 32
static inline size_t tm_slice(int d) {
  const size_t dp = (size_t)tm_tiles(d) * TM_TILE;
  return 3 * dp * dp + 2 * dp;
}

// the fp32 distance of atoms (a, b) of the frame at `base`, widened.  sqrtf, not __fsqrt_rn: without the library's
// rounded-operation build the intrinsic is the native square root (v_sqrt_f32 alone, 1 ulp), while sqrtf is expanded to
// the correctly rounded sequence (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), which is what numpy gives.
__device__ __forceinline__ double tica_feature(const float* __restrict__ base, int a, int b) {
  const float* p = base + 3 * (size_t)a;
  const float* q = base + 3 * (size_t)b;
  return (double)sqrtf(sq_dist2(p[0], p[1], p[2], q[0], q[1], q[2]));
}

// grid: x = upper tile pair (row-major over bi <= bj), y = frame range
__global__ __launch_bounds__(TM_THREADS) void tica_moments_k(const float* __restrict__ xyz, const int* __restrict__ pairs, int N,
                                                             int n, int d, int lag, int per_range, double* __restrict__ ws) {
  __shared__ double st[4][TM_STAGE][TM_TILE];                // X_i, Y_i, X_j, Y_j of the stage, frame major (16 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = tm_tiles(d);
  int bi = 0, p = (int)blockIdx.x;                           // (uniform) the tile pair
  while (p >= nt - bi) {
    p -= nt - bi;
    ++bi;
  }
  const int bj = bi + p;
  const bool diag = bi == bj;
  // a thread stages one feature of the row tile and the same slot of the column tile, for two frames of the stage
  const int f = tid & 31, k0 = tid >> 5;
  int ai[2], aj[2];
  const int fi = bi * TM_TILE + f, fj = bj * TM_TILE + f;
  const bool live_i = fi < d, live_j = fj < d && !diag;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int vi = live_i ? pairs[2 * (size_t)fi + a] : 0, vj = live_j ? pairs[2 * (size_t)fj + a] : 0;
    ai[a] = (vi >= 0 && vi < n) ? vi : 0;
    aj[a] = (vj >= 0 && vj < n) ? vj : 0;
  }
  const int t_begin = (int)blockIdx.y * per_range;           // t_begin < N (the host's grid)
  const int t_end = min(N, t_begin + per_range);
  const size_t per = 3 * (size_t)n;
  const double (*xi)[TM_TILE] = st[0];
  const double (*yi)[TM_TILE] = st[1];
  const double (*xj)[TM_TILE] = diag ? st[0] : st[2];
  const double (*yj)[TM_TILE] = diag ? st[1] : st[3];
  const int sr = (wave >> 1) * 16, sc = (wave & 1) * 16;     // the wave's sub-tile
  const int ml = lane & 15, mk = lane >> 4;                  // A: row ml, depth mk; B: depth mk, column ml
  tm_d4 cxx = {0.0, 0.0, 0.0, 0.0}, cyy = cxx, cxy = cxx, cyx = cxx;
  double fsum = 0.0;                                         // diagonal blocks: tid < 32 sums X_i[tid], tid < 64 Y_i[tid - 32]
  for (int t0 = t_begin; t0 < t_end; t0 += TM_STAGE) {
    __syncthreads();                                         // the previous stage has been read
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = k0 + 8 * u, t = t0 + k;
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
    for (int s = 0; s < TM_STAGE / 4; ++s) {
      const int k = 4 * s + mk;
      const double a_x = xi[k][sr + ml], a_y = yi[k][sr + ml], b_x = xj[k][sc + ml], b_y = yj[k][sc + ml];
      cxx = __builtin_amdgcn_mfma_f64_16x16x4f64(a_x, b_x, cxx, 0, 0, 0);
      cyy = __builtin_amdgcn_mfma_f64_16x16x4f64(a_y, b_y, cyy, 0, 0, 0);
      cxy = __builtin_amdgcn_mfma_f64_16x16x4f64(a_x, b_y, cxy, 0, 0, 0);
      if (!diag) cyx = __builtin_amdgcn_mfma_f64_16x16x4f64(xj[k][sr + ml], yi[k][sc + ml], cyx, 0, 0, 0);
    }
    if (diag && tid < 64) {
#pragma unroll
      for (int k = 0; k < TM_STAGE; ++k) fsum += st[tid >> 5][k][tid & 31];
    }
  }
  // result layout of the f64 MFMA: register r of lane l is row (l >> 4) + 4 r, column l & 15
  const size_t dp = (size_t)nt * TM_TILE;
  double* __restrict__ out = ws + (size_t)blockIdx.y * (3 * dp * dp + 2 * dp);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const size_t row = (size_t)(sr + mk + 4 * r), col = (size_t)(sc + ml);
    const size_t at = ((size_t)bi * TM_TILE + row) * dp + (size_t)bj * TM_TILE + col;
    out[at] = cxx[r];
    out[dp * dp + at] = cyy[r];
    out[2 * dp * dp + at] = cxy[r];
    if (!diag) out[2 * dp * dp + ((size_t)bj * TM_TILE + row) * dp + (size_t)bi * TM_TILE + col] = cyx[r];
  }
  if (diag && tid < 64) out[3 * dp * dp + (size_t)(tid >> 5) * dp + (size_t)bi * TM_TILE + (tid & 31)] = fsum;
}

// one thread per element of [cxx | cyy | cxy | sum_x | sum_y]
__global__ __launch_bounds__(256) void tica_reduce_k(const double* __restrict__ ws, int d, int splits, double* __restrict__ sum_x,
                                                     double* __restrict__ sum_y, double* __restrict__ cxx,
                                                     double* __restrict__ cyy, double* __restrict__ cxy) {
  const size_t dd = (size_t)d * d, total = 3 * dd + 2 * (size_t)d;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t dp = (size_t)tm_tiles(d) * TM_TILE, slice = 3 * dp * dp + 2 * dp;
  size_t src;
  double* dst;
  if (e < 3 * dd) {
    const int m = (int)(e / dd);
    const size_t ij = e - (size_t)m * dd, i = ij / d, j = ij - i * d;
    const bool mirror = m < 2 && i > j;                      // cxx, cyy: only the upper triangle is trusted
    src = (size_t)m * dp * dp + (mirror ? j * dp + i : i * dp + j);
    dst = (m == 0 ? cxx : m == 1 ? cyy : cxy) + ij;
  } else {
    const size_t r = e - 3 * dd, m = r / d, i = r - m * d;
    src = 3 * dp * dp + m * dp + i;
    dst = (m == 0 ? sum_x : sum_y) + i;
  }
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += ws[(size_t)s * slice + src];
  *dst += acc;
}

template <int K>
__global__ __launch_bounds__(TP_THREADS) void tica_project_k(const float* __restrict__ xyz, const int* __restrict__ pairs,
                                                             const double* __restrict__ mean, const double* __restrict__ W, int S,
                                                             int n, int d, double* __restrict__ ics, int ca, int cb, int nb,
                                                             double lo_a, double hi_a, double lo_b, double hi_b,
                                                             int* __restrict__ counts, int* __restrict__ outside) {
  __shared__ int hist[TP_MAX_BINS2 * TP_MAX_BINS2 + 1];      // the last slot: outside
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = counts ? nb * nb : 0;
  if (counts) {
    for (int w = tid; w < words; w += TP_THREADS) hist[w] = 0;
    if (tid == 0) hist[TP_MAX_BINS2 * TP_MAX_BINS2] = 0;
    __syncthreads();
  }
  const size_t per = 3 * (size_t)n;
  for (int s = (int)blockIdx.x * (TP_THREADS / 64) + wave; s < S; s += (int)gridDim.x * (TP_THREADS / 64)) {
    const float* base = xyz + per * (size_t)s;
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    for (int f = lane; f < d; f += 64) {
      const int a = pairs[2 * (size_t)f], b = pairs[2 * (size_t)f + 1];
      const double v = tica_feature(base, (a >= 0 && a < n) ? a : 0, (b >= 0 && b < n) ? b : 0) - mean[f];
#pragma unroll
      for (int c = 0; c < K; ++c) acc[c] += v * W[(size_t)f * K + c];
    }
    double va = 0.0, vb = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const double v = sq_wave_sum(acc[c]);                  // lane 0 holds the sum
      if (ics && lane == 0) ics[(size_t)s * K + c] = v;
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
        atomicAdd(&hist[TP_MAX_BINS2 * TP_MAX_BINS2], 1);
      }
    }
  }
  if (counts) {
    __syncthreads();
    for (int w = tid; w < words; w += TP_THREADS) {
      const int c = hist[w];
      if (c != 0) atomicAdd(counts + w, c);
    }
    if (tid == 0 && hist[TP_MAX_BINS2 * TP_MAX_BINS2] != 0) atomicAdd(outside, hist[TP_MAX_BINS2 * TP_MAX_BINS2]);
  }
}

}  // namespace cgv

extern "C" {

int cgv_tica_max_features(void) { return cgv::TM_MAX_FEATURES; }
int cgv_tica_max_atoms(void) { return cgv::TM_MAX_ATOMS; }
int cgv_tica_max_bins2(void) { return cgv::TP_MAX_BINS2; }
int cgv_tica_max_components(void) { return cgv::TP_MAX_K; }

int cgv_tica_moments_splits(int n_frames, int d, int lag) {
  return (d <= cgv::TM_MAX_FEATURES) ? cgv::tm_splits(n_frames, d, lag) : 0;
}

size_t cgv_tica_moments_workspace_bytes(int n_frames, int d, int lag) {
  if (d < 1 || d > cgv::TM_MAX_FEATURES) return 0;
  const int splits = cgv::tm_splits(n_frames, d, lag);
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
  const int splits = cgv::tm_splits(n_frames, d, lag);
  CGV_REQUIRE(workspace && workspace_bytes >= (size_t)splits * cgv::tm_slice(d) * sizeof(double),
              "workspace smaller than cgv_tica_moments_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const int N = n_frames - lag, nt = cgv::tm_tiles(d);
  const int per_range = (int)cgv::tm_range(N, d);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cgv::tica_moments_k, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)splits), dim3(cgv::TM_THREADS), 0, st, xyz,
                     pairs, N, n_atoms, d, lag, per_range, (double*)workspace);
  int rc = cgv::check_launch("cgv_tica_moments");
  if (rc) return rc;
  const size_t total = 3 * (size_t)d * d + 2 * (size_t)d;
  hipLaunchKernelGGL(cgv::tica_reduce_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)workspace, d, splits,
                     sum_x, sum_y, cxx, cyy, cxy);
  return cgv::check_launch("cgv_tica_moments (reduction)");
}

int cgv_tica_project(const float* xyz, const int32_t* pairs, const double* mean, const double* W, int n_structures,
                     int n_atoms, int d, int k, double* ics, int comp_a, int comp_b, int n_bins2, double lo_a, double hi_a,
                     double lo_b, double hi_b, int32_t* counts, int32_t* outside, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && d >= 0, "bad size");
  CGV_REQUIRE(d <= cgv::TM_MAX_FEATURES, "d <= cgv_tica_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::TM_MAX_ATOMS, "n_atoms <= cgv_tica_max_atoms()");
  CGV_REQUIRE(k >= 1 && k <= cgv::TP_MAX_K, "1 <= k <= cgv_tica_max_components()");
  CGV_REQUIRE((counts == nullptr) == (outside == nullptr), "counts and outside come together");
  if (counts) {
    CGV_REQUIRE(n_bins2 >= 1 && n_bins2 <= cgv::TP_MAX_BINS2, "1 <= n_bins2 <= cgv_tica_max_bins2()");
    CGV_REQUIRE(comp_a >= 0 && comp_a < k && comp_b >= 0 && comp_b < k, "histogram components must be in [0, k)");
    CGV_REQUIRE(lo_a < hi_a && lo_b < hi_b && hi_a - lo_a < 1e300 && hi_b - lo_b < 1e300 && lo_a > -1e300 && lo_b > -1e300,
                "histogram ranges must be finite with lo < hi");
  }
  if (n_structures == 0 || n_atoms == 0 || (!ics && !counts)) return 0;
  CGV_REQUIRE(xyz && (d == 0 || (pairs && mean && W)), "null pointer");
  const int waves = cgv::TP_THREADS / 64;
  int blocks = (n_structures + waves - 1) / waves;
  if (blocks > cgv::TP_MAX_BLOCKS) blocks = cgv::TP_MAX_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
#define CGV_TICA_PROJECT(KK)                                                                                              \
  case KK:                                                                                                                \
    hipLaunchKernelGGL(cgv::tica_project_k<KK>, dim3((unsigned)blocks), dim3(cgv::TP_THREADS), 0, st, xyz, pairs, mean, W,  \
                       n_structures, n_atoms, d, ics, comp_a, comp_b, n_bins2, lo_a, hi_a, lo_b, hi_b, counts, outside);   \
    break;
  switch (k) {
    CGV_TICA_PROJECT(1) CGV_TICA_PROJECT(2) CGV_TICA_PROJECT(3) CGV_TICA_PROJECT(4)
    CGV_TICA_PROJECT(5) CGV_TICA_PROJECT(6) CGV_TICA_PROJECT(7) CGV_TICA_PROJECT(8)
  }
#undef CGV_TICA_PROJECT
  return cgv::check_launch("cgv_tica_project");
}

}  // extern "C"
