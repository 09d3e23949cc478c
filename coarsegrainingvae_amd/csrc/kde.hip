// K22 the sums behind a Gaussian kernel density estimate (see include/cgvae_hip.h): for P independent planes
//   sums[p, m] = sum_i exp2(-|points[p,m] - samples[p,i]|^2)        d = 1 or 2 coordinates per row
// The host (density.py) has centred, whitened and scaled the coordinates by sqrt(log2(e) / 2), so the kernel knows nothing
// of bandwidths and its exponential is the hardware's v_exp_f32 (__builtin_amdgcn_exp2f: 1 ulp, results below 2^-126 are
// flushed to zero -- "CDNA3 Instruction Set Architecture", V_EXP_F32).  On a periodic axis (period > 0) a difference is
// reduced to its minimum image, delta - period * rint(delta * (1 / period)), the last step one fused multiply-add.
//
// Every term is computed as exp2(64 - r): the -64 is the addend of the first square's fused multiply-add, so it costs no
// instruction, and it moves the flush from terms below 2^-126 to terms below 2^-190.  A sum that is not itself below
// N 2^-126 therefore loses nothing that counts (flushed terms are 2^-64 of it at most); a term is at most 2^64 and a
// stage's fp32 sum at most 2^74.  The merge scales by 2^-64, which is exact.
//
// kde_sums_k<D, PERIODIC>   grid (point tile, sample range, plane) x 256 threads.  A thread owns KDE_PTS = 4 points
//                   of its tile of 1024 in registers (points t, t + 256, ..: coalesced loads and stores); the block owns
//                   one contiguous range of `per` samples and walks it in stages of at most 1024.  A stage's samples are
//                   copied to LDS once -- a non-finite sample is replaced by +inf there, so that its term is exp2(-inf)
//                   = 0 and nothing in the inner loop asks about it -- and every lane then reads the same float2: one
//                   LDS broadcast read per sample serves the thread's four terms.  (Uniform scalar loads from global
//                   memory would save that read but cannot replace a non-finite sample: the test would move into the
//                   inner loop as one more vector instruction per term, and a read is not on the vector pipe.)
//                   Within a stage a point's accumulator is fp32 (at most 1024 non-negative terms, added in sample
//                   order); after the stage it is added to the point's fp64 accumulator.  The range's fp64 sums go to
//                   its slice of the workspace.  The PERIODIC instance also clamps r to 256 with a minimum, which turns
//                   the NaN of inf - inf into a zero term; the other instance has no such instruction.
// kde_merge_k       blocks [0, ceil(P M / 256)): one thread per (plane, point) adds the ranges' slices in ascending
//                   order; a non-finite point gives NaN.  The last P blocks count the non-finite samples of a plane.
// No floating-point atomics; the split is a function of (P, N, M) or the caller's number: the same input gives the same
// bits on every call.  N = 0 or M = 0 read nothing: an empty range adds no term and writes zeros.
//
// Bound: the vector pipe.  A wave's v_exp_f32 issues in 8 cycles, so the chip's transcendental rate is
// 256 CUs x 4 SIMDs x 8 lanes x 2.4 GHz = 19.7e12 terms/s; beside it a term of the non-periodic 2-D instance needs two
// subtractions, two fused multiply-adds and the accumulation (4 cycles each): 28 cycles per 64 terms, 0.29 of
// the transcendental rate at best.  What is reached: DESIGN.md (K22 row), profiles/kde.txt.
#include <math.h>

#include "cgv_common.h"

namespace cgv {

constexpr int KDE_THREADS = 256;
constexpr int KDE_PTS = 4;                                // points a thread owns
constexpr int KDE_TILE = KDE_THREADS * KDE_PTS;           // 1024 points of a block
constexpr int KDE_STAGE = 1024;                           // samples of a stage (8 KB of LDS)
constexpr float KDE_SHIFT = 64.0f;                        // terms are exp2(KDE_SHIFT - r); the merge scales by 2^-KDE_SHIFT
constexpr int KDE_MIN_RANGE = 256;                        // samples of a range at least, under the automatic split
constexpr int KDE_TARGET_BLOCKS = 1024;                   // four per CU
constexpr int KDE_MAX_SPLITS = 1024;
constexpr int KDE_MAX_PLANES = 4096;
constexpr int KDE_MAX_SAMPLES = 1 << 28;
constexpr int KDE_MAX_POINTS = 1 << 24;
constexpr long long KDE_MAX_OUTPUTS = 1ll << 30;          // planes x points of a launch

static inline int kde_auto_splits(int P, int N, int M) {
  if (P < 1 || N < 1 || M < 1) return 1;
  const long long blocks = (long long)P * ((M + KDE_TILE - 1) / KDE_TILE);
  long long s = (KDE_TARGET_BLOCKS + blocks - 1) / blocks;
  const long long cap = ((long long)N + KDE_MIN_RANGE - 1) / KDE_MIN_RANGE;
  if (s > cap) s = cap;
  if (s > KDE_MAX_SPLITS) s = KDE_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

template <int D, bool PERIODIC>
__global__ __launch_bounds__(KDE_THREADS) void kde_sums_k(const float* __restrict__ samples, const float* __restrict__ points,
                                                          const float* __restrict__ period, int P, int N, int M, int per,
                                                          double* __restrict__ part) {
  __shared__ float2 stage[KDE_STAGE];
  const int tid = threadIdx.x, p = (int)blockIdx.z, range = (int)blockIdx.y;
  const float* __restrict__ S = samples + (size_t)p * (size_t)N * D;
  const float* __restrict__ Q = points + (size_t)p * (size_t)M * D;
  float px[KDE_PTS], py[KDE_PTS];
#pragma unroll
  for (int j = 0; j < KDE_PTS; ++j) {
    const int m = (int)blockIdx.x * KDE_TILE + j * KDE_THREADS + tid;
    px[j] = m < M ? Q[(size_t)m * D] : 0.f;
    py[j] = (D == 2 && m < M) ? Q[(size_t)m * D + 1] : 0.f;
  }
  float wx = 0.f, wy = 0.f, ix = 0.f, iy = 0.f;            // period and its reciprocal (0: the axis is not periodic)
  if (PERIODIC) {
    wx = period[(size_t)p * D];
    wy = D == 2 ? period[(size_t)p * D + 1] : 0.f;
    wx = wx > 0.f ? wx : 0.f, wy = wy > 0.f ? wy : 0.f;
    ix = wx > 0.f ? 1.0f / wx : 0.f, iy = wy > 0.f ? 1.0f / wy : 0.f;
  }
  double acc[KDE_PTS];
#pragma unroll
  for (int j = 0; j < KDE_PTS; ++j) acc[j] = 0.0;
  const long long begin = (long long)range * per;
  const int s_begin = begin < N ? (int)begin : N, s_end = (long long)s_begin + per < N ? s_begin + per : N;
  for (int s0 = s_begin; s0 < s_end; s0 += KDE_STAGE) {
    const int ns = min(KDE_STAGE, s_end - s0);
    __syncthreads();                                         // the previous stage has been read
    for (int i = tid; i < ns; i += KDE_THREADS) {
      const float sx = S[(size_t)(s0 + i) * D], sy = D == 2 ? S[(size_t)(s0 + i) * D + 1] : 0.f;
      const bool ok = isfinite(sx) && isfinite(sy);
      stage[i] = ok ? make_float2(sx, sy) : make_float2(INFINITY, INFINITY);
    }
    __syncthreads();
    float a[KDE_PTS];
#pragma unroll
    for (int j = 0; j < KDE_PTS; ++j) a[j] = 0.f;
#pragma unroll 4
    for (int i = 0; i < ns; ++i) {
      const float2 s = stage[i];                             // the same address in every lane: a broadcast
#pragma unroll
      for (int j = 0; j < KDE_PTS; ++j) {
        float dx = px[j] - s.x, r;
        if (PERIODIC) dx = fmaf(-wx, rintf(dx * ix), dx);
        if (D == 2) {
          float dy = py[j] - s.y;
          if (PERIODIC) dy = fmaf(-wy, rintf(dy * iy), dy);
          r = fmaf(dy, dy, fmaf(dx, dx, -KDE_SHIFT));
        } else {
          r = fmaf(dx, dx, -KDE_SHIFT);
        }
        if (PERIODIC) r = fminf(r, 256.0f);                  // NaN (a replaced sample: inf - inf) -> 256 -> a zero term
        a[j] += __builtin_amdgcn_exp2f(-r);
      }
    }
#pragma unroll
    for (int j = 0; j < KDE_PTS; ++j) acc[j] += (double)a[j];
  }
  double* __restrict__ mine = part + ((size_t)range * P + p) * (size_t)M;
#pragma unroll
  for (int j = 0; j < KDE_PTS; ++j) {
    const int m = (int)blockIdx.x * KDE_TILE + j * KDE_THREADS + tid;
    if (m < M) mine[m] = acc[j];
  }
}

template <int D>
__global__ __launch_bounds__(KDE_THREADS) void kde_merge_k(const double* __restrict__ part, const float* __restrict__ samples,
                                                           const float* __restrict__ points, int P, int N, int M, int splits,
                                                           unsigned sum_blocks, double* __restrict__ sums,
                                                           int* __restrict__ n_skipped) {
  __shared__ int skipped;
  const int tid = threadIdx.x;
  if (blockIdx.x >= sum_blocks) {                            // (uniform) one plane's non-finite samples
    const int p = (int)(blockIdx.x - sum_blocks);
    if (tid == 0) skipped = 0;
    __syncthreads();
    const float* __restrict__ S = samples + (size_t)p * (size_t)N * D;
    int mine = 0;
    for (int i = tid; i < N; i += KDE_THREADS) {
      bool ok = isfinite(S[(size_t)i * D]);
      if (D == 2) ok = ok && isfinite(S[(size_t)i * D + 1]);
      mine += ok ? 0 : 1;
    }
    if (mine != 0) atomicAdd(&skipped, mine);
    __syncthreads();
    if (tid == 0) n_skipped[p] = skipped;
    return;
  }
  const size_t total = (size_t)P * (size_t)M, o = (size_t)blockIdx.x * KDE_THREADS + tid;
  if (o >= total) return;
  double t = 0.0;
  for (int r = 0; r < splits; ++r) t += part[(size_t)r * total + o];   // ascending ranges: a fixed order
  bool ok = isfinite(points[o * D]);
  if (D == 2) ok = ok && isfinite(points[o * D + 1]);
  sums[o] = ok ? t * 0x1p-64 : (double)NAN;
}

}  // namespace cgv

extern "C" {

int cgv_kde_max_planes(void) { return cgv::KDE_MAX_PLANES; }
int cgv_kde_max_samples(void) { return cgv::KDE_MAX_SAMPLES; }
int cgv_kde_max_points(void) { return cgv::KDE_MAX_POINTS; }
int cgv_kde_max_splits(void) { return cgv::KDE_MAX_SPLITS; }

int cgv_kde_splits(int n_planes, int n_samples, int n_points) { return cgv::kde_auto_splits(n_planes, n_samples, n_points); }

size_t cgv_kde_workspace_bytes(int n_planes, int n_points, int splits) {
  if (n_planes < 0 || n_points < 0 || splits < 1 || splits > cgv::KDE_MAX_SPLITS) return 0;
  return (size_t)splits * (size_t)n_planes * (size_t)n_points * sizeof(double);
}

int cgv_kde_sums(const float* samples, const float* points, const float* period, int n_planes, int n_samples, int n_points, int d,
                 int splits, double* sums, int32_t* n_skipped, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace cgv;
  CGV_REQUIRE(n_planes >= 0 && n_samples >= 0 && n_points >= 0, "bad size");
  CGV_REQUIRE(d == 1 || d == 2, "d must be 1 or 2");
  CGV_REQUIRE(n_planes <= KDE_MAX_PLANES, "n_planes <= cgv_kde_max_planes()");
  CGV_REQUIRE(n_samples <= KDE_MAX_SAMPLES, "n_samples <= cgv_kde_max_samples()");
  CGV_REQUIRE(n_points <= KDE_MAX_POINTS, "n_points <= cgv_kde_max_points()");
  CGV_REQUIRE((long long)n_planes * n_points <= KDE_MAX_OUTPUTS, "n_planes * n_points <= 2^30 per launch");
  CGV_REQUIRE(splits >= 0 && splits <= KDE_MAX_SPLITS, "0 (automatic) <= splits <= cgv_kde_max_splits()");
  if (n_planes == 0) return 0;
  CGV_REQUIRE(n_skipped, "null n_skipped");
  CGV_REQUIRE(n_samples == 0 || samples, "null samples");
  CGV_REQUIRE(n_points == 0 || (points && sums), "null points or sums");
  const int P = n_planes, N = n_samples, M = n_points;
  const int sp = splits ? splits : kde_auto_splits(P, N, M);
  const int per = N ? (int)(((long long)N + sp - 1) / sp) : 1;
  const size_t need = cgv_kde_workspace_bytes(P, M, sp);
  CGV_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "workspace smaller than cgv_kde_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const unsigned tiles = (unsigned)((M + KDE_TILE - 1) / KDE_TILE);
  if (tiles) {
    const dim3 grid(tiles, (unsigned)sp, (unsigned)P), block(KDE_THREADS);
    if (d == 2 && period)
      hipLaunchKernelGGL((kde_sums_k<2, true>), grid, block, 0, st, samples, points, period, P, N, M, per, part);
    else if (d == 2)
      hipLaunchKernelGGL((kde_sums_k<2, false>), grid, block, 0, st, samples, points, period, P, N, M, per, part);
    else if (period)
      hipLaunchKernelGGL((kde_sums_k<1, true>), grid, block, 0, st, samples, points, period, P, N, M, per, part);
    else
      hipLaunchKernelGGL((kde_sums_k<1, false>), grid, block, 0, st, samples, points, period, P, N, M, per, part);
    const int rc = check_launch("cgv_kde_sums");
    if (rc) return rc;
  }
  const unsigned sum_blocks = (unsigned)(((size_t)P * (size_t)M + KDE_THREADS - 1) / KDE_THREADS);
  if (d == 2)
    hipLaunchKernelGGL((kde_merge_k<2>), dim3(sum_blocks + (unsigned)P), dim3(KDE_THREADS), 0, st, part, samples, points, P, N, M, sp,
                       sum_blocks, sums, n_skipped);
  else
    hipLaunchKernelGGL((kde_merge_k<1>), dim3(sum_blocks + (unsigned)P), dim3(KDE_THREADS), 0, st, part, samples, points, P, N, M, sp,
                       sum_blocks, sums, n_skipped);
  return check_launch("cgv_kde_sums (merge)");
}

}  // extern "C"
