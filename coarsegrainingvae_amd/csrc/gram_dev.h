// What the analyses that need the Gram matrix of on-the-fly features share (K16 tica.hip, K27 pca.hip): the rule that cuts
// the samples into ranges, the pieces of a moments kernel on the fp64 matrix cores, the reduction of the ranges' partials,
// and the projection of structures onto components with its two-component histogram.
// EVERY FILE THAT INCLUDES THIS IS COMPILED WITH -ffp-contract=off (build.py: SOURCE_FLAGS): the features and
// v = feature - mean are restated on the host bit for bit, and no product here may fuse into a sum.
//
// A moments kernel: 256 threads, grid (upper tile pairs bi <= bj of GRAM_TILE = 32 features, sample ranges).  Per stage of
// GRAM_STAGE = 16 samples the block writes the features of its row tile and its column tile into LDS as fp64, sample
// major ([GRAM_STAGE][GRAM_TILE]; samples past the range and features past d as +0.0: adding it is exact); wave w owns the
// 16 x 16 sub-tile (w >> 1, w & 1) and adds A^T B per 4 samples with v_mfma_f64_16x16x4_f64 (gram_mfma).  Diagonal blocks
// also sum their features over the samples in ascending order (gram_add_column).  Each block stores its tiles into its
// range's slice of the workspace (gram_store: no floating-point atomics), and gram_reduce_k sums the slices.  The kernel's
// own part is what a feature is and how many products it carries.
#pragma once
#include "cgv_common.h"
#include "sq_dist.h"

namespace cgv {

constexpr int GRAM_THREADS = 256;
constexpr int GRAM_TILE = 32;                 // features of a block's row / column tile: 2 x 2 MFMA tiles, one per wave
constexpr int GRAM_STAGE = 16;                // samples of a stage: 4 MFMA steps of depth 4
constexpr int GRAM_TARGET_BLOCKS = 1024;      // four per CU
constexpr int GRAM_MIN_RANGE = 256;           // samples of a range, at least (a range's partials cost a pass of the reduction)
constexpr int GRAM_MAX_SPLITS = 256;
constexpr int GRAM_MAX_K = 8;                 // components of a projection
constexpr int GRAM_MAX_BINS2 = 64;            // 64 x 64 int32 slots of a block's LDS histogram (16 KB)
constexpr int GRAM_PROJECT_BLOCKS = 1024;

typedef double gram_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int gram_tiles(int d) { return (d + GRAM_TILE - 1) / GRAM_TILE; }

// samples of one range (a multiple of the stage) and the number of ranges for N samples of d features: about
// GRAM_TARGET_BLOCKS blocks whatever d, no range shorter than GRAM_MIN_RANGE
static inline long long gram_range(long long N, int d) {
  const long long nt = gram_tiles(d), pairs = nt * (nt + 1) / 2;
  long long want = (GRAM_TARGET_BLOCKS + pairs - 1) / pairs;
  if (want > GRAM_MAX_SPLITS) want = GRAM_MAX_SPLITS;
  long long per = (N + want - 1) / want;
  if (per < GRAM_MIN_RANGE) per = GRAM_MIN_RANGE;
  return (per + GRAM_STAGE - 1) / GRAM_STAGE * GRAM_STAGE;
}
static inline int gram_splits(long long N, int d) {
  if (d < 1 || N < 1) return 0;
  const long long per = gram_range(N, d);
  return (int)((N + per - 1) / per);
}
// one range's slice of the workspace (doubles): `mats` matrices [dp,dp], then `vecs` vectors [dp], then `count` (0 or 1)
// scalars; dp = tiles * 32
__host__ __device__ inline size_t gram_slice(int d, int mats, int vecs, int count) {
  const size_t dp = (size_t)gram_tiles(d) * GRAM_TILE;
  return mats * dp * dp + vecs * dp + count;
}

// ----------------------------------------------------------------------------- the pieces of a moments kernel
// where a thread of a moments block works.  grid x = upper tile pair (row-major over bi <= bj)
struct GramTile {
  int bi, bj;                                 // (uniform) the tile pair
  bool diag;
  int f, k0;                                  // staging: slot f of the row tile and of the column tile, stage rows k0 and k0 + 8
  int sr, sc;                                 // the wave's sub-tile
  int ml, mk;                                 // A: row ml, depth mk; B: depth mk, column ml
};
__device__ __forceinline__ GramTile gram_tile(int nt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bi = 0, p = (int)blockIdx.x;
  while (p >= nt - bi) {
    p -= nt - bi;
    ++bi;
  }
  return GramTile{bi, bi + p, p == 0, tid & 31, tid >> 5, (wave >> 1) * 16, (wave & 1) * 16, lane & 15, lane >> 4};
}

// acc += A^T B over the four samples 4 q .. 4 q + 3 of a stage: `a` and `b` are row 4 q + g.mk of the two staged tiles
__device__ __forceinline__ void gram_mfma(const double* a, const double* b, const GramTile& g, gram_d4& acc) {
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[g.sr + g.ml], b[g.sc + g.ml], acc, 0, 0, 0);
}

// the wave's sub-tile of tile (ti, tj) of a [dp,dp] matrix.  Result layout of the f64 MFMA: register r of lane l is row
// (l >> 4) + 4 r, column l & 15
__device__ __forceinline__ void gram_store(double* __restrict__ out, size_t dp, int ti, int tj, const GramTile& g, const gram_d4& acc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const size_t row = (size_t)(g.sr + g.mk + 4 * r), col = (size_t)(g.sc + g.ml);
    out[((size_t)ti * GRAM_TILE + row) * dp + (size_t)tj * GRAM_TILE + col] = acc[r];
  }
}

// sum += the stage's samples of one feature, in ascending order
__device__ __forceinline__ void gram_add_column(double& sum, const double (*stage)[GRAM_TILE], int col) {
#pragma unroll
  for (int k = 0; k < GRAM_STAGE; ++k) sum += stage[k][col];
}

// ----------------------------------------------------------------------------- the ranges' partials, summed
struct GramTotals {                           // what a launch ADDS to: MATS matrices [d,d], VECS vectors [d], COUNT integers
  double* mat[3];
  double* vec[2];
  int* count;
};
// one thread per output element: the ranges' partials summed in ascending order, added to the caller's totals.  The first
// SYM matrices are exactly symmetric and only their upper triangle is trusted: below the diagonal they are read from above it.
template <int MATS, int SYM, int VECS, int COUNT>
__global__ __launch_bounds__(256) void gram_reduce_k(const double* __restrict__ ws, int d, int splits, GramTotals out) {
  const size_t dd = (size_t)d * d, total = MATS * dd + VECS * (size_t)d + COUNT;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const size_t dp = (size_t)gram_tiles(d) * GRAM_TILE, slice = gram_slice(d, MATS, VECS, COUNT);
  size_t src = MATS * dp * dp + VECS * dp;    // the count
  double* dst = nullptr;
  if (e < MATS * dd) {
    const int m = (int)(e / dd);
    const size_t ij = e - (size_t)m * dd, i = ij / d, j = ij - i * d;
    src = (size_t)m * dp * dp + ((m < SYM && i > j) ? j * dp + i : i * dp + j);
    dst = out.mat[0] + ij;
#pragma unroll
    for (int q = 1; q < MATS; ++q)
      if (m == q) dst = out.mat[q] + ij;
  } else if (e - MATS * dd < VECS * (size_t)d) {
    const size_t r = e - MATS * dd;
    const int m = (int)(r / d);
    const size_t i = r - (size_t)m * d;
    src = MATS * dp * dp + (size_t)m * dp + i;
    dst = out.vec[0] + i;
#pragma unroll
    for (int q = 1; q < VECS; ++q)
      if (m == q) dst = out.vec[q] + i;
  }
  double acc = 0.0;
  for (int s = 0; s < splits; ++s) acc += ws[(size_t)s * slice + src];
  if (!COUNT || dst) *dst += acc;
  else *out.count += (int)acc;                // a sum of integers, each exact as a double
}
template <int MATS, int SYM, int VECS, int COUNT>
static inline int gram_reduce(const char* what, const void* ws, int d, int splits, const GramTotals& out, hipStream_t st) {
  const size_t total = MATS * (size_t)d * d + VECS * (size_t)d + COUNT;
  hipLaunchKernelGGL((gram_reduce_k<MATS, SYM, VECS, COUNT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)ws,
                     d, splits, out);
  return check_launch(what);
}

// ----------------------------------------------------------------------------- projection
struct GramHist {                             // two of the components binned into counts [nb,nb]; counts == nullptr: no histogram
  int ca, cb, nb;
  double lo_a, hi_a, lo_b, hi_b;
  int* counts;
  int* outside;
};

// out [S,K] = (feature - mean) W, one wave per structure.  `Feature` says what a structure's features are:
//   bool good(int s)             (uniform over the wave) false: the structure's components are NaN and it counts in `outside`
//   double value(int s, int f)   feature f < d of a good structure s, the mean not yet subtracted
// Each lane sums its strided share of the features in ascending order, sq_wave_sum combines the lanes; lane 0 writes the
// components and bins two of them into the block's LDS histogram (integer atomics), flushed with one integer vector atomic
// per non-zero slot.  The bin rule: for lo <= v < hi in fp64 the bin is floor((v - lo) * nb / (hi - lo)), clamped to [0, nb)
// against rounding alone; a structure with either component outside its range or NaN counts once in `outside`.
template <int K, class Feature>
__global__ __launch_bounds__(GRAM_THREADS) void gram_project_k(const Feature feat, const double* __restrict__ mean,
                                                               const double* __restrict__ W, int S, int d, double* __restrict__ out,
                                                               const GramHist h) {
  __shared__ int hist[GRAM_MAX_BINS2 * GRAM_MAX_BINS2 + 1];  // the last slot: outside
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = h.nb, words = h.counts ? nb * nb : 0;
  if (h.counts) {
    for (int w = tid; w < words; w += GRAM_THREADS) hist[w] = 0;
    if (tid == 0) hist[GRAM_MAX_BINS2 * GRAM_MAX_BINS2] = 0;
    __syncthreads();
  }
  for (int s = (int)blockIdx.x * (GRAM_THREADS / 64) + wave; s < S; s += (int)gridDim.x * (GRAM_THREADS / 64)) {
    const bool good = feat.good(s);
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    if (good) {
      for (int f = lane; f < d; f += 64) {
        const double v = feat.value(s, f) - mean[f];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] += v * W[(size_t)f * K + c];
      }
    }
    double va = 0.0, vb = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      double v = sq_wave_sum(acc[c]);
      if (!good) v = (double)NAN;
      if (out && lane == 0) out[(size_t)s * K + c] = v;
      if (c == h.ca) va = v;
      if (c == h.cb) vb = v;
    }
    if (h.counts && lane == 0) {
      // (v - lo) * nb / (hi - lo); lo <= v < hi: rounding alone could leave [0, nb)
      const bool in = va >= h.lo_a && va < h.hi_a && vb >= h.lo_b && vb < h.hi_b;   // false for a NaN
      if (in) {
        const int ia = min(nb - 1, max(0, (int)floor((va - h.lo_a) * (double)nb / (h.hi_a - h.lo_a))));
        const int ib = min(nb - 1, max(0, (int)floor((vb - h.lo_b) * (double)nb / (h.hi_b - h.lo_b))));
        atomicAdd(&hist[ia * nb + ib], 1);
      } else {
        atomicAdd(&hist[GRAM_MAX_BINS2 * GRAM_MAX_BINS2], 1);
      }
    }
  }
  if (h.counts) {
    __syncthreads();
    for (int w = tid; w < words; w += GRAM_THREADS) {
      const int c = hist[w];
      if (c != 0) atomicAdd(h.counts + w, c);
    }
    if (tid == 0 && hist[GRAM_MAX_BINS2 * GRAM_MAX_BINS2] != 0) atomicAdd(h.outside, hist[GRAM_MAX_BINS2 * GRAM_MAX_BINS2]);
  }
}

// what cgv_<family>_project checks of k and the histogram, with its reasons
static inline int gram_project_refuses(const char* family, int k, const GramHist& h) {
  auto refuse = [family](const char* why) {                 // `why` may name the family once, as %s
    char msg[96];
    snprintf(msg, sizeof msg, why, family);
    set_error("cgv_%s_project: %s", family, msg);
    return CGV_E_BADARG;
  };
  if (k < 1 || k > GRAM_MAX_K) return refuse("1 <= k <= cgv_%s_max_components()");
  if ((h.counts == nullptr) != (h.outside == nullptr)) return refuse("counts and outside come together");
  if (!h.counts) return 0;
  if (h.nb < 1 || h.nb > GRAM_MAX_BINS2) return refuse("1 <= n_bins2 <= cgv_%s_max_bins2()");
  if (!(h.ca >= 0 && h.ca < k && h.cb >= 0 && h.cb < k)) return refuse("histogram components must be in [0, k)");
  if (!(h.lo_a < h.hi_a && h.lo_b < h.hi_b && h.hi_a - h.lo_a < 1e300 && h.hi_b - h.lo_b < 1e300 && h.lo_a > -1e300 && h.lo_b > -1e300))
    return refuse("histogram ranges must be finite with lo < hi");
  return 0;
}

template <class Feature>
static inline int gram_launch_project(const char* what, const Feature& feat, const double* mean, const double* W, int S, int d, int k,
                                      double* out, const GramHist& h, hipStream_t st) {
  const int waves = GRAM_THREADS / 64;
  int blocks = (S + waves - 1) / waves;
  if (blocks > GRAM_PROJECT_BLOCKS) blocks = GRAM_PROJECT_BLOCKS;
#define CGV_GRAM_PROJECT(KK)                                                                                                      \
  case KK:                                                                                                                        \
    hipLaunchKernelGGL((gram_project_k<KK, Feature>), dim3((unsigned)blocks), dim3(GRAM_THREADS), 0, st, feat, mean, W, S, d, out, h); \
    break;
  switch (k) {
    CGV_GRAM_PROJECT(1) CGV_GRAM_PROJECT(2) CGV_GRAM_PROJECT(3) CGV_GRAM_PROJECT(4)
    CGV_GRAM_PROJECT(5) CGV_GRAM_PROJECT(6) CGV_GRAM_PROJECT(7) CGV_GRAM_PROJECT(8)
  }
#undef CGV_GRAM_PROJECT
  return check_launch(what);
}

}  // namespace cgv
