// Squared norms of rank-update weight gradients from their operands (the gradient itself is never formed):
// the LDS form (<= 64 operand rows) and the fp64 MFMA form (<= 128), over the table of wgrad_grouped.hip.
#include "cgv_common.h"
#include "gemm_dev.h"
#include "wgrad_record.h"

namespace cgv {

// ------------------------------------------------------------------ norm of a weight gradient from its operands
// ||g^T x||_F^2 = sum_{a<=b} c_ab (g_a . g_b)(x_a . x_b),  c = 1 on the diagonal and 2 off it, over the M operand rows
// (g = gy * act'(z)): the squared norm of a rank-update layer's gradient without forming it.
//   wgrad_gram_k         grid (GRAM_SLICES, problems): block s takes the column slices s, s + GRAM_SLICES, ... of the
//                        problem's rows -- first g's N columns, then x's K -- C4 float4 per row at a time, staged in LDS
//                        (activation derivative applied once, at staging); 8 lanes share a pair's partial dot product
//                        over the slice (double), the block's slices are summed per pair in LDS and leave as its own
//                        workspace rows ws[problem][s][g | x][pair].  One global round trip per slice, blocks independent.
//   wgrad_gram_reduce_k  one block per problem: sums the slices per pair (fixed order) and the pairs' products.
// The blocks of wgrad_gram_k also write the bias gradient gb[n] (+)= sum_m g[m, n] (a column slice each), which the
// fused update does not produce.
constexpr int GRAM_SLICES = 8;
constexpr int GRAM_WAVES = 8;
constexpr int GRAM_THREADS = 64 * GRAM_WAVES;
constexpr int GRAM_F4_PER_THREAD = 6;                                // staged float4 per thread and slice (<= 3072)
constexpr int GRAM_TILE_F4 = 3200;                                   // rows are padded by one float4 (bank spread)
constexpr int GRAM_MAX_PAIRS = GRAM_MAX_ROWS * (GRAM_MAX_ROWS + 1) / 2;                         // 2080
constexpr size_t GRAM_WS_DOUBLES = (size_t)GRAM_SLICES * 2 * GRAM_MAX_PAIRS;                    // per problem
static size_t gram_lds_bytes(int max_rows) { return sizeof(float4) * GRAM_TILE_F4 + sizeof(double) * (size_t)max_rows * (max_rows + 1); }

constexpr int GRAM_TICKETS = 512;                                    // >= primitives.WeightGradQueue.MAX_PROBLEMS
__device__ unsigned gram_tickets[GRAM_TICKETS];                      // zero at load, every launch leaves them zero

__global__ __launch_bounds__(GRAM_THREADS) void wgrad_gram_k(const WgradProblem* __restrict__ table, double* __restrict__ ws,
                                                             int pair_cap /* pairs the LDS sums hold per operand */,
                                                             double* __restrict__ out /* [problems] or NULL */) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float4* tile = reinterpret_cast<float4*>(smem);                // [M][C4 + 1]
  double* sums = reinterpret_cast<double*>(tile + GRAM_TILE_F4); // [g | x][pair_cap]: this block's slices, summed
  const WgradProblem pr = table[blockIdx.y];
  const int sl = blockIdx.x;
  const int M = pr.M, N = pr.N, K = pr.K, act = pr.act;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* mine = ws + (size_t)blockIdx.y * GRAM_WS_DOUBLES + (size_t)sl * 2 * GRAM_MAX_PAIRS;
  for (int i = t; i < 2 * pair_cap; i += GRAM_THREADS) sums[i] = 0.0;
  const bool unsupported = M > GRAM_MAX_ROWS || M * (M + 1) / 2 > pair_cap;
  if (pr.gb && unsupported) {                                   // bias gradient (supported shapes: from the staged slices, below)
    for (int n = sl * GRAM_THREADS + t; n < N; n += GRAM_SLICES * GRAM_THREADS) {
      float sum = 0.f;
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const size_t at = wg_row(pr, m, N) + n;
        float g = ldg_global(pr.gy + at);
        if (act) g *= act_bwd(ldg_global(pr.z + at), act);
        sum += g;
      }
      pr.gb[n] = pr.accumulate ? pr.gb[n] + sum : sum;
    }
  }
  if (unsupported) {                                            // (cgv_rank_update_supported): poison the norm
    if (t == 0) mine[0] = __builtin_nan("");
    return;
  }
  int C4 = (GRAM_TILE_F4 / M - 1) & ~63;
  if (C4 == 0) C4 = (GRAM_TILE_F4 / M - 1) & ~15;                // more than 49 rows: 48 / 32 float4 per row and slice
  C4 = C4 > 256 ? 256 : C4;
  const int RS = C4 + 1;                                         // row stride (float4)
  const int n4 = N >> 2, k4 = K >> 2;
  const int g_slices = (n4 + C4 - 1) / C4, slices = g_slices + (k4 + C4 - 1) / C4;
  const int pairs = M * (M + 1) / 2;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fetch = [&](int slice, float4 (&buf)[GRAM_F4_PER_THREAD]) {
    const bool is_g = slice < g_slices;
    const int c0 = (is_g ? slice : slice - g_slices) * C4, cols4 = is_g ? n4 : k4;
#pragma unroll
    for (int u = 0; u < GRAM_F4_PER_THREAD; ++u) {
      const int idx = t + GRAM_THREADS * u;
      const int m = idx / C4, col4 = c0 + idx - m * C4;
      buf[u] = zero4;
      if (m < M && col4 < cols4) {
        if (is_g) {
          float4 g = ldg4_global(pr.gy + wg_row(pr, m, N) + 4 * col4);
          if (act) {
            const float4 z = ldg4_global(pr.z + wg_row(pr, m, N) + 4 * col4);
            g.x *= act_bwd(z.x, act); g.y *= act_bwd(z.y, act); g.z *= act_bwd(z.z, act); g.w *= act_bwd(z.w, act);
          }
          buf[u] = g;
        } else {
          buf[u] = ldg4_global(pr.x + wg_row(pr, m, K) + 4 * col4);
        }
      }
    }
  };
  // 8 lanes share a pair (an eighth of the slice's columns each), a wave pass covers 8 pairs
  const int sub = lane & 7, pl = lane >> 3;
  float4 buf[GRAM_F4_PER_THREAD];
  if (sl < slices) fetch(sl, buf);
  for (int slice = sl; slice < slices; slice += GRAM_SLICES) {
    __syncthreads();                                             // previous slice consumed (and `sums` zeroed)
#pragma unroll
    for (int u = 0; u < GRAM_F4_PER_THREAD; ++u) {
      const int idx = t + GRAM_THREADS * u;
      const int m = idx / C4;
      if (m < M) tile[m * RS + idx - m * C4] = buf[u];
    }
    if (slice + GRAM_SLICES < slices) fetch(slice + GRAM_SLICES, buf);       // in flight while this slice is used
    __syncthreads();
    if (pr.gb && slice < g_slices) {
      // bias gradient of this slice's columns: column sums of the staged g (rows ascending) -- as a loop over global
      // memory in front of the first fetch it was M dependent row loads per column, ~6 round trips before the block started
      const int c0 = slice * C4;
      for (int c = t; c < C4 && c0 + c < n4; c += GRAM_THREADS) {
        float4 sum = zero4;
        for (int m = 0; m < M; ++m) {
          const float4 g = tile[m * RS + c];
          sum.x += g.x; sum.y += g.y; sum.z += g.z; sum.w += g.w;
        }
        float* dst = pr.gb + 4 * (c0 + c);
        if ((reinterpret_cast<uintptr_t>(pr.gb) & 15) == 0) {             // (block-uniform; arena slots are 256-byte aligned)
          if (pr.accumulate) { const float4 old = ldg4_global(dst); sum.x += old.x; sum.y += old.y; sum.z += old.z; sum.w += old.w; }
          stg4_global(dst, sum);
        } else {
          const float v4[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) dst[e] = pr.accumulate ? dst[e] + v4[e] : v4[e];
        }
      }
    }
    double* row = sums + (slice < g_slices ? 0 : pair_cap);
    for (int base = 8 * w; base < pairs; base += 8 * GRAM_WAVES) {
      const int pidx = base + pl;
      const bool live = pidx < pairs;
      // pair index -> (a <= b), row-major upper triangle: rows before a hold S(a) = a M - a (a - 1) / 2 pairs
      const int q = live ? pidx : 0;
      const float disc = (float)((2 * M + 1) * (2 * M + 1) - 8 * q);
      int a = (int)(((float)(2 * M + 1) - sqrtf(disc)) * 0.5f);
      a = a < 0 ? 0 : (a > M - 1 ? M - 1 : a);
      while (a + 1 < M && (a + 1) * M - (a + 1) * a / 2 <= q) ++a;
      while (a > 0 && a * M - a * (a - 1) / 2 > q) --a;
      const int b = a + q - (a * M - a * (a - 1) / 2);
      double acc = 0.0;
      if (live) {
        for (int c = sub; c < C4; c += 8) {
          const float4 u4 = tile[a * RS + c], v4 = tile[b * RS + c];
          acc += (double)u4.x * v4.x + (double)u4.y * v4.y + (double)u4.z * v4.z + (double)u4.w * v4.w;
        }
      }
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 4);
      if (live && sub == 0) row[pidx] += acc;                    // this lane owns the pair in every slice of the block
    }
  }
  __syncthreads();
  // agent-scope stores: the block that arrives LAST at this problem's ticket sums all slices (below)
  for (int i = t; i < pairs; i += GRAM_THREADS) {
    __hip_atomic_store(mine + i, sums[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + GRAM_MAX_PAIRS + i, sums[pair_cap + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (out == nullptr) return;                                     // (two-launch form: wgrad_gram_reduce_k follows)
  // One launch instead of two: the eight slice blocks of a problem meet at a ticket (eight arrivals -- the pattern that is
  // too slow for the 1620 blocks of the flat norm pass pays here); atomicInc wraps to zero at the eighth, so the tickets
  // need no reset and a launch that never finished cannot wedge the next one.
  // (No __threadfence: an agent-scope release writes back the WHOLE L2 -- right behind the backward pass that is 60 us per
  // launch, measured.  The partials travel as agent-scope atomics, which are coherent across the XCDs by themselves; every
  // thread waits for its own stores to be acknowledged before the barrier that precedes the ticket.)
  __shared__ unsigned s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    s_last = atomicInc(gram_tickets + (blockIdx.y % GRAM_TICKETS), (unsigned)GRAM_SLICES - 1u) == (unsigned)GRAM_SLICES - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  const double* all = ws + (size_t)blockIdx.y * GRAM_WS_DOUBLES;
  double local = 0.0;
  for (int p = t; p < pairs; p += GRAM_THREADS) {
    double gg = 0.0, xx = 0.0;
    for (int s2 = 0; s2 < GRAM_SLICES; ++s2) {
      gg += __hip_atomic_load(all + (size_t)s2 * 2 * GRAM_MAX_PAIRS + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      xx += __hip_atomic_load(all + (size_t)s2 * 2 * GRAM_MAX_PAIRS + GRAM_MAX_PAIRS + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int a = 0, rem = p;                                           // diagonal pairs (a, a) count once (see wgrad_gram_reduce_k)
    while (rem >= M - a) { rem -= M - a; ++a; }
    local += (rem == 0 ? 1.0 : 2.0) * gg * xx;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) local += __shfl_xor(local, d);
  __shared__ double wsum[GRAM_WAVES];
  if (lane == 0) wsum[w] = local;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < GRAM_WAVES; ++k) tot += wsum[k];
    out[blockIdx.y] = tot;
  }
}

__global__ __launch_bounds__(256) void wgrad_gram_reduce_k(const WgradProblem* __restrict__ table, const double* __restrict__ ws,
                                                           double* __restrict__ out) {
  __shared__ double part[4];
  const int M = table[blockIdx.x].M;
  const double* mine = ws + (size_t)blockIdx.x * GRAM_WS_DOUBLES;
  const int pairs = M <= GRAM_MAX_ROWS ? M * (M + 1) / 2 : 1;
  double local = 0.0;
  for (int p = threadIdx.x; p < pairs; p += 256) {
    double gg = 0.0, xx = 0.0;
    for (int s = 0; s < GRAM_SLICES; ++s) {
      gg += mine[(size_t)s * 2 * GRAM_MAX_PAIRS + p];
      xx += mine[(size_t)s * 2 * GRAM_MAX_PAIRS + GRAM_MAX_PAIRS + p];
    }
    // diagonal pairs are (a, a): p = a M - a (a - 1) / 2; cheaper to recover a by walking than to store it
    int a = 0, rem = p;
    while (rem >= M - a) { rem -= M - a; ++a; }
    local += (rem == 0 ? 1.0 : 2.0) * gg * (M <= GRAM_MAX_ROWS ? xx : 1.0);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) local += __shfl_xor(local, d);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// The same norm for MANY operand rows (41 .. 128: gathered rows of 4 - 8 ranks, bead rows of a large batch), where walking
// M^2 / 2 row pairs on the vector ALU costs more than forming the gradient tiles (48 rows: 140 us against 82 us for the
// tile pass with a squaring epilogue).  The two Gram matrices G = g g^T and X = x x^T are built from 16 x 16 tiles of
// the upper triangle with v_mfma_f64_16x16x4_f64 -- operands widened on the way out of LDS, so products and sums are the
// doubles of wgrad_gram_k -- and ||g^T x||^2 = sum_ab G_ab X_ab (off-diagonal tiles count twice).
//   wgrad_gram_mfma_k     grid (GRAMM_BLOCKS, problems), the column slices and LDS layout of wgrad_gram_k (rows M .. 16 NT - 1
//                         stay zero); block s takes the slices s, s + GRAMM_BLOCKS, ... -- one or two for the model's
//                         layers: the instruction runs at a quarter of the fp32 rate, the work has to be spread by
//                         columns (with 8 blocks per problem the 5400-column layers' blocks set the launch's length) --
//                         and wave w keeps the tiles w, w + 8, ... in registers over them.  They leave as
//                         ws[problem][block][G | X][tile][lane][4] (G when the block's slices turn from g to x, X at the end).
//                         Bias gradients as in wgrad_gram_k.
//   wgrad_gram_mfma_dot_k grid (tiles, problems): blocks' parts summed per element (fixed order), tile's sum of G_ab X_ab
//   wgrad_gram_mfma_sum_k one thread per problem: the tiles' sums in fixed order.
// A tile's 256 elements sit in the same lanes / registers for G and for X (same instruction), and both operands of a
// step read column c + (lane >> 4) of row (lane & 15), so the result does not depend on the instruction's register map.
constexpr int GRAMM_MAX_ROWS = 128;
constexpr int GRAMM_MAX_TILES = 36;                                  // upper triangle of 8 x 8 row groups
constexpr int GRAMM_BLOCKS = 32;
constexpr int GRAMM_LDS_BYTES = 52 * 1024;
typedef double f64x4 __attribute__((ext_vector_type(4)));
// workspace doubles per problem for a launch whose largest problem has `tiles` tiles: the blocks' parts, then the tiles' sums
__device__ __host__ inline size_t gramm_ws_doubles(int tiles) { return (size_t)GRAMM_BLOCKS * 2 * tiles * 256 + GRAMM_MAX_TILES; }
// columns per slice: 16 NT rows x C / 4 float4 <= 3072 (six per thread), rows padded by one float4, at most 52 KB
__device__ __host__ inline int gramm_cols(int MP) { const int c = (12288 / MP) & ~31; return c > 256 ? 256 : c; }
__device__ __forceinline__ void gramm_tile_of(int tt, int NT, int& a, int& b) {
  a = 0;
  while (tt >= NT - a) { tt -= NT - a; ++a; }
  b = a + tt;
}

template <int TPW>   // tiles per wave: 3 up to 96 rows (21 tiles), 5 up to 128 (36)
__global__ __launch_bounds__(GRAM_THREADS) void wgrad_gram_mfma_k(const WgradProblem* __restrict__ table, double* __restrict__ ws,
                                                                  int launch_tiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float4* tile = reinterpret_cast<float4*>(smem);                // [16 NT][C4 + 1]
  const WgradProblem pr = table[blockIdx.y];
  const int sl = blockIdx.x;
  const int M = pr.M, N = pr.N, K = pr.K, act = pr.act;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int NT = (M + 15) >> 4, MP = 16 * NT, T = NT * (NT + 1) / 2;
  if (M > GRAMM_MAX_ROWS || T > launch_tiles || T > TPW * GRAM_WAVES) return;          // (wgrad_gram_mfma_dot_k poisons the norm)
  const int C4 = gramm_cols(MP) >> 2, RS = C4 + 1;
  const int n4 = N >> 2, k4 = K >> 2;
  const int g_slices = (n4 + C4 - 1) / C4, slices = g_slices + (k4 + C4 - 1) / C4;
  if (sl >= slices) return;
  double* mine = ws + (size_t)blockIdx.y * gramm_ws_doubles(launch_tiles) + (size_t)sl * 2 * launch_tiles * 256;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int idx = t; idx < (MP - M) * RS; idx += GRAM_THREADS) tile[M * RS + idx] = zero4;     // never written again
  auto fetch = [&](int slice, float4 (&buf)[GRAM_F4_PER_THREAD]) {
    const bool is_g = slice < g_slices;
    const int c0 = (is_g ? slice : slice - g_slices) * C4, cols4 = is_g ? n4 : k4;
#pragma unroll
    for (int u = 0; u < GRAM_F4_PER_THREAD; ++u) {
      const int idx = t + GRAM_THREADS * u;
      const int m = idx / C4, col4 = c0 + idx - m * C4;
      buf[u] = zero4;
      if (m < M && col4 < cols4) {
        if (is_g) {
          float4 g = ldg4_global(pr.gy + wg_row(pr, m, N) + 4 * col4);
          if (act) {
            const float4 z = ldg4_global(pr.z + wg_row(pr, m, N) + 4 * col4);
            g.x *= act_bwd(z.x, act); g.y *= act_bwd(z.y, act); g.z *= act_bwd(z.z, act); g.w *= act_bwd(z.w, act);
          }
          buf[u] = g;
        } else {
          buf[u] = ldg4_global(pr.x + wg_row(pr, m, K) + 4 * col4);
        }
      }
    }
  };
  int ta[TPW], tb[TPW];
  f64x4 acc[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    const int tt = w + GRAM_WAVES * u;
    gramm_tile_of(tt < T ? tt : 0, NT, ta[u], tb[u]);
    acc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  const int i = lane & 15, q = lane >> 4;
  const float* tf = reinterpret_cast<const float*>(tile);
  const int RSf = 4 * RS, C = 4 * C4;
  float4 buf[GRAM_F4_PER_THREAD];
  fetch(sl, buf);
  for (int slice = sl; slice < slices; slice += GRAMM_BLOCKS) {
    __syncthreads();                                             // previous slice consumed (and the zero rows written)
#pragma unroll
    for (int u = 0; u < GRAM_F4_PER_THREAD; ++u) {
      const int idx = t + GRAM_THREADS * u;
      const int m = idx / C4;
      if (m < M) tile[m * RS + idx - m * C4] = buf[u];
    }
    if (slice + GRAMM_BLOCKS < slices) fetch(slice + GRAMM_BLOCKS, buf);     // in flight while this slice is used
    __syncthreads();
    if (pr.gb && slice < g_slices) {                             // bias gradient: column sums of the staged g (rows ascending)
      const int c0 = slice * C4;
      for (int c = t; c < C4 && c0 + c < n4; c += GRAM_THREADS) {
        float4 sum = zero4;
        for (int m = 0; m < M; ++m) {
          const float4 g = tile[m * RS + c];
          sum.x += g.x; sum.y += g.y; sum.z += g.z; sum.w += g.w;
        }
        float* dst = pr.gb + 4 * (c0 + c);
        if ((reinterpret_cast<uintptr_t>(pr.gb) & 15) == 0) {
          if (pr.accumulate) { const float4 old = ldg4_global(dst); sum.x += old.x; sum.y += old.y; sum.z += old.z; sum.w += old.w; }
          stg4_global(dst, sum);
        } else {
          const float v4[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) dst[e] = pr.accumulate ? dst[e] + v4[e] : v4[e];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      if (w + GRAM_WAVES * u < T) {                                // (wave-uniform)
        const float* pa = tf + (16 * ta[u] + i) * RSf + q;
        const float* pb = tf + (16 * tb[u] + i) * RSf + q;
        f64x4 c = acc[u];
#pragma unroll 4
        for (int col = 0; col < C; col += 4)
          c = __builtin_amdgcn_mfma_f64_16x16x4f64((double)pa[col], (double)pb[col], c, 0, 0, 0);
        acc[u] = c;
      }
    }
    // the block's g slices are done: their tiles leave as its G part (the x slices start from zero)
    const bool last_g = slice < g_slices && slice + GRAMM_BLOCKS >= g_slices;
    const bool last = slice + GRAMM_BLOCKS >= slices;
    if (last_g || last) {
      double* dst = mine + (slice < g_slices ? 0 : (size_t)launch_tiles * 256);
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        const int tt = w + GRAM_WAVES * u;
        if (tt < T) *reinterpret_cast<f64x4*>(dst + (size_t)tt * 256 + 4 * lane) = acc[u];
        acc[u] = f64x4{0.0, 0.0, 0.0, 0.0};
      }
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_gram_mfma_dot_k(const WgradProblem* __restrict__ table, double* __restrict__ ws,
                                                             int launch_tiles) {
  __shared__ double part[4];
  const WgradProblem pr = table[blockIdx.y];
  const int M = pr.M;
  double* mine = ws + (size_t)blockIdx.y * gramm_ws_doubles(launch_tiles);
  double* sums = mine + (size_t)GRAMM_BLOCKS * 2 * launch_tiles * 256;
  const int tt = blockIdx.x;
  const int NT = (M + 15) >> 4, T = NT * (NT + 1) / 2;
  if (M > GRAMM_MAX_ROWS || T > launch_tiles) { if (threadIdx.x == 0) sums[tt] = __builtin_nan(""); return; }
  if (tt >= T) { if (threadIdx.x == 0) sums[tt] = 0.0; return; }
  const int C4 = gramm_cols(16 * NT) >> 2;
  const int g_slices = ((pr.N >> 2) + C4 - 1) / C4, slices = g_slices + ((pr.K >> 2) + C4 - 1) / C4;
  int a, b;
  gramm_tile_of(tt, NT, a, b);
  double gg = 0.0, xx = 0.0;
  for (int s = 0; s < GRAMM_BLOCKS && s < slices; ++s) {
    const double* blk = mine + (size_t)s * 2 * launch_tiles * 256 + (size_t)tt * 256 + threadIdx.x;
    const int last_slice = s + (slices - 1 - s) / GRAMM_BLOCKS * GRAMM_BLOCKS;      // of block s
    if (s < g_slices) gg += blk[0];
    if (last_slice >= g_slices) xx += blk[(size_t)launch_tiles * 256];
  }
  double local = (a == b ? 1.0 : 2.0) * gg * xx;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) local += __shfl_xor(local, d);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) sums[tt] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void wgrad_gram_mfma_sum_k(const double* __restrict__ ws, double* __restrict__ out, int launch_tiles) {
  if (threadIdx.x != 0) return;
  const double* sums = ws + (size_t)blockIdx.x * gramm_ws_doubles(launch_tiles) + (size_t)GRAMM_BLOCKS * 2 * launch_tiles * 256;
  double sum = 0.0;
  for (int tt = 0; tt < launch_tiles; ++tt) sum += sums[tt];
  out[blockIdx.x] = sum;
}

}  // namespace cgv

extern "C" {

/* Rank-update layers, first half: sumsq[i] = ||gW_i||_F^2 from the operands of record i; bias gradients written.
 * Records must satisfy cgv_rank_update_supported (M <= max_rows <= 64; records may address gathered operands through
 * seg_rows / seg_stride); workspace: cgv_wgrad_gram_workspace_bytes(n_problems). */
int cgv_wgrad_gram(const void* table_dev, int n_problems, int max_rows, double* sumsq, void* workspace, size_t workspace_bytes,
                   void* stream) {
  CGV_REQUIRE(n_problems >= 0, "bad size");
  if (n_problems == 0) return 0;
  CGV_REQUIRE(max_rows >= 1 && max_rows <= cgv::GRAM_MAX_ROWS, "max_rows out of range (1..64)");
  CGV_REQUIRE(table_dev && sumsq && workspace, "null pointer");
  CGV_REQUIRE(workspace_bytes >= cgv_wgrad_gram_workspace_bytes(n_problems), "workspace too small");
  CGV_REQUIRE((((uintptr_t)workspace) & 7) == 0, "workspace must be 8-byte aligned");
  const cgv::WgradProblem* table = reinterpret_cast<const cgv::WgradProblem*>(table_dev);
  const size_t lds = cgv::gram_lds_bytes(max_rows);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cgv::wgrad_gram_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { cgv::set_error("cgv_wgrad_gram: %zu bytes of LDS: %s", lds, hipGetErrorString(e)); return (int)e; }
  }
  // one launch (the last slice block of a problem sums its slices) up to GRAM_TICKETS problems, else the reduce launch follows
  const bool one = n_problems <= cgv::GRAM_TICKETS && cgv::option(CGV_OPT_OPTIM_ONE_LAUNCH) != 2;
  hipLaunchKernelGGL(cgv::wgrad_gram_k, dim3(cgv::GRAM_SLICES, n_problems), dim3(cgv::GRAM_THREADS), lds,
                     (hipStream_t)stream, table, reinterpret_cast<double*>(workspace), max_rows * (max_rows + 1) / 2,
                     one ? sumsq : (double*)nullptr);
  if (!one)
    hipLaunchKernelGGL(cgv::wgrad_gram_reduce_k, dim3(n_problems), dim3(256), 0, (hipStream_t)stream, table,
                       reinterpret_cast<const double*>(workspace), sumsq);
  return cgv::check_launch("cgv_wgrad_gram");
}

size_t cgv_wgrad_gram_workspace_bytes(int n_problems) {
  return n_problems > 0 ? (size_t)n_problems * cgv::GRAM_WS_DOUBLES * sizeof(double) : 0;
}

/* The same for records of up to 128 rows (cgv_wgrad_gram_mfma_max_rows): Gram matrices by fp64 MFMA tiles (csrc:
 * wgrad_gram_mfma_k).  N % 4 == 0 and K % 4 == 0; workspace: cgv_wgrad_gram_mfma_workspace_bytes(n_problems, max_rows). */
int cgv_wgrad_gram_mfma_max_rows(void) { return cgv::GRAMM_MAX_ROWS; }
size_t cgv_wgrad_gram_mfma_workspace_bytes(int n_problems, int max_rows) {
  if (n_problems <= 0 || max_rows < 1 || max_rows > cgv::GRAMM_MAX_ROWS) return 0;
  const int nt = (max_rows + 15) / 16;
  return (size_t)n_problems * cgv::gramm_ws_doubles(nt * (nt + 1) / 2) * sizeof(double);
}
int cgv_wgrad_gram_mfma(const void* table_dev, int n_problems, int max_rows, double* sumsq, void* workspace, size_t workspace_bytes,
                        void* stream) {
  CGV_REQUIRE(n_problems >= 0, "bad size");
  if (n_problems == 0) return 0;
  CGV_REQUIRE(max_rows >= 1 && max_rows <= cgv::GRAMM_MAX_ROWS, "max_rows out of range (1..128)");
  CGV_REQUIRE(table_dev && sumsq && workspace, "null pointer");
  CGV_REQUIRE(workspace_bytes >= cgv_wgrad_gram_mfma_workspace_bytes(n_problems, max_rows), "workspace too small");
  CGV_REQUIRE((((uintptr_t)workspace) & 31) == 0, "workspace must be 32-byte aligned");
  const cgv::WgradProblem* table = reinterpret_cast<const cgv::WgradProblem*>(table_dev);
  const int nt = (max_rows + 15) / 16, tiles = nt * (nt + 1) / 2;
  const bool few = tiles <= 3 * cgv::GRAM_WAVES;
  const void* fn = few ? reinterpret_cast<const void*>(cgv::wgrad_gram_mfma_k<3>) : reinterpret_cast<const void*>(cgv::wgrad_gram_mfma_k<5>);
  static bool lds_set[2] = {false, false};
  if (!lds_set[few]) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, cgv::GRAMM_LDS_BYTES);
    if (e != hipSuccess) { cgv::set_error("cgv_wgrad_gram_mfma: LDS request: %s", hipGetErrorString(e)); return (int)e; }
    lds_set[few] = true;
  }
  hipStream_t st = (hipStream_t)stream;
  double* ws = reinterpret_cast<double*>(workspace);
  const dim3 grid(cgv::GRAMM_BLOCKS, n_problems);
  if (few) hipLaunchKernelGGL(cgv::wgrad_gram_mfma_k<3>, grid, dim3(cgv::GRAM_THREADS), cgv::GRAMM_LDS_BYTES, st, table, ws, tiles);
  else hipLaunchKernelGGL(cgv::wgrad_gram_mfma_k<5>, grid, dim3(cgv::GRAM_THREADS), cgv::GRAMM_LDS_BYTES, st, table, ws, tiles);
  hipLaunchKernelGGL(cgv::wgrad_gram_mfma_dot_k, dim3(tiles, n_problems), dim3(256), 0, st, table, ws, tiles);
  hipLaunchKernelGGL(cgv::wgrad_gram_mfma_sum_k, dim3(n_problems), dim3(64), 0, st, ws, sumsq, tiles);
  return cgv::check_launch("cgv_wgrad_gram_mfma");
}

}  // extern "C"
