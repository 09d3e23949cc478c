// Weight gradients over GATHERED operand rows (data-parallel operand exchange): MFMA tile, strip and 128-tile
// layouts, their bf16 split-operand forms, and the operand pack kernel that fills the send buffer.
#include "cgv_common.h"
#include "gemm_dev.h"
#include "wgrad_record.h"

namespace cgv {

// ------------------------------------------------------------------ grouped weight gradient over GATHERED operands
// Data-parallel exchange of the bead-level layers (trainer.OperandExchange): a weight gradient g^T x has rank <= rows,
// and the bead-level layers see 12 rows per GPU against 0.36 - 3.2 M weights, so the ranks all-gather their operand
// rows (g = gy * act'(z) and x, packed by pack_operands_k) instead of all-reducing gW, and every rank forms the
// global gradient itself:  gW[N,K] (+)= sum over ALL ranks' rows of g[m,:]^T x[m,:]  -- what a single process would
// compute on the concatenated batch.  Row m of the problem lives in rank segment m / seg_rows of the gathered buffer:
//   g_row(m) = gy + (m / seg_rows) * seg_stride + (m % seg_rows) * N        x_row(m) likewise with K
// (seg_rows % 4 == 0 is required by the host protocol; the kernel itself takes any).
// A block owns a 64 x 64 tile of one gW; wave w its rows 16 w .. 16 w + 15.  The operand rows of the tile (64 columns
// of g, 64 of x) are staged through LDS in chunks of GW_CHUNK rows with coalesced 16-byte loads that are all in
// flight at once (the direct-from-L2 version spent 264 us at 8 x 12 rows on dependent load rounds; this one is
// bound by the gW stores).  MFMA 16x16x4 f32 steps over 4 rows: lane (i = l&15, q = l>>4) supplies
// A = g[m0+q][16w+i] and B_s = x[m0+q][4i+s], so that D_s holds gW[n0+16w+4q+r][k0+4i+s] and leaves as 16-byte
// stores.  LDS strides 80 / 64 floats keep the b32 / b128 reads conflict free.  Exact fp32 FMA chains, fixed order.
// Straight-line staging: every request goes to a valid (clamped) address and is zeroed by a select afterwards -- with
// predicated loads the compiler builds a branch and a vmcnt(0) per request.  The clobber keeps the requests above the
// MFMA loop they are meant to travel under (LLVM otherwise sinks them to their first use behind it).
__device__ __forceinline__ float4 ldg4_or_zero(const float* p, bool ok) {
  return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void strip_pin() { asm volatile("" ::: "memory"); }
// Operand pointers come out of the record (generic address space): as they are, the requests become flat_load, which
// counts on lgkmcnt as well -- the first LDS wait of the MFMA loop would then wait for the whole next x tile.
typedef const float __attribute__((address_space(1)))* strip_gptr;
__device__ __forceinline__ float4 strip_ldg4(const float* p) {
  const f32x4 t = *reinterpret_cast<const __attribute__((address_space(1))) f32x4*>((strip_gptr)p);
  return make_float4(t.x, t.y, t.z, t.w);
}
#ifndef CGV_GW_CHUNK
#define CGV_GW_CHUNK 48
#endif
// rows per staged chunk (multiple of 16); -DCGV_GW_CHUNK=<n> for A/B builds: 16 / 32 / 48 are within 3 % of each other
// (chignolin 72 / 76 / 74 us, dipeptide 365 / 360 / 371 us), 96 is 20 % slower (two blocks per CU)
constexpr int GW_CHUNK = CGV_GW_CHUNK;
constexpr int GW_GS = 80, GW_XS = 64;
// gathered_wgrad_k's tile is 64 rows x GW_TW columns of gW: the g columns of a staged chunk (with z: two thirds of the
// staged bytes of an activated layer) serve twice as many FMAs as in a 64 x 64 tile -- 8 instead of 5.3 FMAs per staged
// byte; the kernel is bound by the L2 -> LDS traffic of its four blocks per CU, not by the MFMA pipe.
constexpr int GW_TW = 128, GW_XW = 128;          // tile width in k; LDS row stride of the x chunk

// MODE: GW_STORE writes the tile (and the bias gradient); the other two are the halves of a RANK UPDATE over gathered
// rows too many for the FMA-per-row kernel (grouped_wgrad_t<true>: VALU bound from ~48 rows): GW_SUMSQ forms the tile,
// leaves its sum of squares as this block's entry of `partial` (double; summed per problem in block order by
// gathered_sumsq_reduce_k) and writes the bias gradient; GW_ADAM forms the tile again and runs it, clipped, through
// the Adam update of its weights (p / m / v addressed through gW's offset in the gradient arena) -- the gradient itself
// is never stored.
enum { GW_STORE = 0, GW_SUMSQ = 1, GW_ADAM = 2 };
template <int MODE>
__global__ __launch_bounds__(256) void gathered_wgrad_k(const WgradProblem* __restrict__ table, int n_problems,
                                                        double* __restrict__ partial, RankUpdateArgs ra) {
  __shared__ __attribute__((aligned(16))) float gs[GW_CHUNK * GW_GS];
  __shared__ __attribute__((aligned(16))) float xs[GW_CHUNK * GW_XW];
  if (MODE == GW_ADAM && ra.state[ST_SKIP] != 0.f) return;    // skipped step (utils.py:145): parameters stay
  const int lo = wg_find_problem(table, n_problems);
  const WgradProblem pr = table[lo];
  const int local = blockIdx.x - pr.block_begin;
  const int nb = local / pr.tiles_k, kt = local - nb * pr.tiles_k;
  const int M = pr.M, N = pr.N, K = pr.K;
  const int sr = pr.seg_rows > 0 ? pr.seg_rows : M;
  const int n0 = nb * 64, k0 = kt * GW_TW;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc[8];                                                      // [half h of the tile's columns][component]
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int c4 = threadIdx.x & 15, rr = threadIdx.x >> 4;          // staging: 16 float4 columns x 16 rows per pass
  const bool gcol = n0 + 4 * c4 < N, xcol0 = k0 + 4 * c4 < K, xcol1 = k0 + 64 + 4 * c4 < K;
  constexpr int NP = GW_CHUNK / 16;                                  // staging passes per chunk
  float4 gq[NP], zq[NP], xq[NP][2];
  // operand rows of one chunk into registers: the loads only -- g is multiplied by act'(z) when the chunk is stored to
  // LDS (chunk_store), so that the next chunk's loads really travel under this chunk's MFMAs.  Straight line: every
  // request goes to a valid (clamped) address through a global-address-space pointer and is zeroed by a select when it
  // is stored (a predicated load is a branch with a wait for everything outstanding; a generic-pointer load is a
  // flat_load, which also counts on lgkmcnt and made the MFMA loop's first LDS wait a wait for the whole next chunk).
  const int gcol_at = gcol ? n0 + 4 * c4 : 0, xcol0_at = xcol0 ? k0 + 4 * c4 : 0, xcol1_at = xcol1 ? k0 + 64 + 4 * c4 : 0;
  const float* zsrc = pr.act ? pr.z : pr.gy;                          // (no activation: a second look at g instead of a branch)
  auto chunk_load = [&](int m0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int m = min(m0 + rr + 16 * p, M - 1);
      const int seg = m / sr, row = m - seg * sr;
      const size_t base = (size_t)seg * pr.seg_stride;
      gq[p] = strip_ldg4(pr.gy + base + (size_t)row * N + gcol_at);
      zq[p] = strip_ldg4(zsrc + base + (size_t)row * N + gcol_at);
      xq[p][0] = strip_ldg4(pr.x + base + (size_t)row * K + xcol0_at);
      xq[p][1] = strip_ldg4(pr.x + base + (size_t)row * K + xcol1_at);
    }
    strip_pin();
  };
  auto chunk_store = [&](int m0) {
    if (pr.act == 1) {                                                // Swish: the model's activation, kept free of the switch
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        gq[p].x *= act_bwd(zq[p].x, 1); gq[p].y *= act_bwd(zq[p].y, 1);
        gq[p].z *= act_bwd(zq[p].z, 1); gq[p].w *= act_bwd(zq[p].w, 1);
      }
    } else if (pr.act) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        gq[p].x *= act_bwd(zq[p].x, pr.act); gq[p].y *= act_bwd(zq[p].y, pr.act);
        gq[p].z *= act_bwd(zq[p].z, pr.act); gq[p].w *= act_bwd(zq[p].w, pr.act);
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {                                   // rows beyond M and columns beyond N / K: zeros
      const bool live = m0 + rr + 16 * p < M;
      const bool gk = live && gcol, xk0 = live && xcol0, xk1 = live && xcol1;
      *reinterpret_cast<float4*>(gs + (rr + 16 * p) * GW_GS + 4 * c4) =
          make_float4(gk ? gq[p].x : 0.f, gk ? gq[p].y : 0.f, gk ? gq[p].z : 0.f, gk ? gq[p].w : 0.f);
      *reinterpret_cast<float4*>(xs + (rr + 16 * p) * GW_XW + 4 * c4) =
          make_float4(xk0 ? xq[p][0].x : 0.f, xk0 ? xq[p][0].y : 0.f, xk0 ? xq[p][0].z : 0.f, xk0 ? xq[p][0].w : 0.f);
      *reinterpret_cast<float4*>(xs + (rr + 16 * p) * GW_XW + 64 + 4 * c4) =
          make_float4(xk1 ? xq[p][1].x : 0.f, xk1 ? xq[p][1].y : 0.f, xk1 ? xq[p][1].z : 0.f, xk1 ? xq[p][1].w : 0.f);
    }
  };
  chunk_load(0);
  for (int m0 = 0; m0 < M; m0 += GW_CHUNK) {
    chunk_store(m0);
    __syncthreads();
    chunk_load(min(m0 + GW_CHUNK, M - 1));                           // the next chunk travels under this chunk's MFMAs
                                                                     // (the last trip asks for the last row again: no branch)
    const float* ga = gs + q * GW_GS + 16 * wave + i;
    const float* xb = xs + q * GW_XW + 4 * i;
    // whole trip count (the rows beyond the chunk are zeros): unrolled, LDS reads issued two steps ahead of their MFMAs
#pragma unroll
    for (int st = 0; st < GW_CHUNK / 4; ++st) {
      const float a = ga[(4 * st) * GW_GS];
      const float4 b0 = *reinterpret_cast<const float4*>(xb + (4 * st) * GW_XW);
      const float4 b1 = *reinterpret_cast<const float4*>(xb + (4 * st) * GW_XW + 64);
      bsum += a;
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0.y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0.z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0.w, acc[3], 0, 0, 0);
      acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1.x, acc[4], 0, 0, 0);
      acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1.y, acc[5], 0, 0, 0);
      acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1.z, acc[6], 0, 0, 0);
      acc[7] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1.w, acc[7], 0, 0, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
    for (int st = 0; st < GW_CHUNK / 4 - 2; ++st) {
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
    __syncthreads();
  }
  const int n = n0 + 16 * wave + i;
  if (MODE == GW_STORE) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kcol = k0 + 64 * h + 4 * i;
      if (kcol >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 16 * wave + 4 * q + r;
        if (row >= N) continue;
        float* dst = pr.gW + (size_t)row * K + kcol;
        float4 o = make_float4(acc[4 * h][r], acc[4 * h + 1][r], acc[4 * h + 2][r], acc[4 * h + 3][r]);
        if (pr.accumulate) { const float4 old = ldg4_global(dst); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
        stg4_global(dst, o);
      }
    }
  } else if (MODE == GW_SUMSQ) {
    double sq = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (k0 + 64 * h + 4 * i >= K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (n0 + 16 * wave + 4 * q + r >= N) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) sq += (double)acc[4 * h + c][r] * (double)acc[4 * h + c][r];
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d);
    __shared__ double wave_sq[4];
    if (lane == 0) wave_sq[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_sq[0] + wave_sq[1]) + (wave_sq[2] + wave_sq[3]);
  } else {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const AdamStep a = adam_step_of(ra.state, ra.lr, ra.beta1, ra.beta2, ra.eps);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kcol = k0 + 64 * h + 4 * i;
      if (kcol >= K) continue;
      const size_t at0 = (size_t)(pr.gW - ra.arena_g) + kcol;
      float4 pp[4], mm[4], vv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 16 * wave + 4 * q + r;
        const size_t o = at0 + (size_t)(row < N ? row : 0) * K;
        pp[r] = *reinterpret_cast<const float4*>(ra.arena_p + o);
        const f4v tm = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(ra.arena_m + o));
        const f4v tv = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(ra.arena_v + o));
        mm[r] = make_float4(tm.x, tm.y, tm.z, tm.w);
        vv[r] = make_float4(tv.x, tv.y, tv.z, tv.w);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 16 * wave + 4 * q + r;
        if (row >= N) continue;
        const size_t o = at0 + (size_t)row * K;
        adam_elem(a, pp[r].x, acc[4 * h][r], mm[r].x, vv[r].x); adam_elem(a, pp[r].y, acc[4 * h + 1][r], mm[r].y, vv[r].y);
        adam_elem(a, pp[r].z, acc[4 * h + 2][r], mm[r].z, vv[r].z); adam_elem(a, pp[r].w, acc[4 * h + 3][r], mm[r].w, vv[r].w);
        *reinterpret_cast<float4*>(ra.arena_p + o) = pp[r];
        __builtin_nontemporal_store(f4v{mm[r].x, mm[r].y, mm[r].z, mm[r].w}, reinterpret_cast<f4v*>(ra.arena_m + o));
        __builtin_nontemporal_store(f4v{vv[r].x, vv[r].y, vv[r].z, vv[r].w}, reinterpret_cast<f4v*>(ra.arena_v + o));
      }
    }
    return;                                                         // the bias gradient was written by the GW_SUMSQ pass
  }
  if (pr.gb && kt == 0) {                                           // bias: the 4 row groups q of a step meet by shuffle
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (q == 0 && n < N) pr.gb[n] = pr.accumulate ? pr.gb[n] + bsum : bsum;
  }
}

// block partials of gathered_wgrad_k<GW_SUMSQ> -> one double per problem, summed in block order
__global__ __launch_bounds__(256) void gathered_sumsq_reduce_k(const WgradProblem* __restrict__ table, int n_problems, int total_blocks,
                                                               const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double part[256];
  const int pr = blockIdx.x;
  const int beg = table[pr].block_begin, end = pr + 1 < n_problems ? table[pr + 1].block_begin : total_blocks;
  double local = 0.0;
  for (int b = beg + (int)threadIdx.x; b < end; b += 256) local += partial[b];
  part[threadIdx.x] = local;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[pr] = part[0];
}

// STRIP variant for few operand rows (M <= 128: bead-level layers of a large bead batch, gathered rows of 4 - 8 ranks).
// gathered_wgrad_k gives every 64 x 64 tile its own block, which stages BOTH operand tiles and spends most of its short
// life on the problem lookup and the first loads (PMC at 96 rows: MFMA pipe 55 % busy in the norm pass, 39 % in the
// store pass with act').  Here a block owns a 64-row STRIP of gW: the g columns of those rows are staged (and multiplied
// by act'(z)) ONCE, then the block walks the strip's K / 64 column tiles with the x tile of the next one loading while
// the MFMAs of the current one run (two LDS buffers, one barrier per tile).  Same lane maps, same per-element FMA order
// as gathered_wgrad_k (rows ascending), so results are bit-identical to it.
constexpr int GS_MAX_ROWS = 128;
#ifndef CGV_GS_SINGLE_FROM
#define CGV_GS_SINGLE_FROM 7
#endif
// row classes (NP) from which the x tile has ONE LDS buffer (a second barrier per tile, more blocks per CU)
constexpr int GS_SINGLE_FROM = CGV_GS_SINGLE_FROM;
template <int MODE, int NP>   // NP: staging passes of 16 rows (M <= 16 NP)
__global__ __launch_bounds__(256) void gathered_wgrad_strip_k(const WgradProblem* __restrict__ table, int n_problems,
                                                              double* __restrict__ partial, RankUpdateArgs ra) {
  extern __shared__ __attribute__((aligned(16))) float strip_smem[];
  constexpr int MP = 16 * NP;
  float* gs = strip_smem;                              // [MP][GW_GS]
  constexpr bool DB = NP < GS_SINGLE_FROM;
  float* xs0 = gs + MP * GW_GS;                        // [MP][GW_XS] x 2
  float* xs1 = DB ? xs0 + MP * GW_XS : xs0;
  if (MODE == GW_ADAM && ra.state[ST_SKIP] != 0.f) return;
  const int lo = wg_find_problem(table, n_problems);
  const WgradProblem pr = table[lo];
  const int nb = blockIdx.x - pr.block_begin;
  const int M = pr.M, N = pr.N, K = pr.K;
  const int n0 = nb * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int c4 = threadIdx.x & 15, rr = threadIdx.x >> 4;          // staging: 16 float4 columns x 16 rows per pass
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef float f4v __attribute__((ext_vector_type(4)));
  size_t xrow[NP], grow[NP];                                        // operand row offsets (rank segments resolved once, branch-free)
  bool live[NP];
  {
    const int seg_rows = pr.seg_rows > 0 ? pr.seg_rows : 0x7fffffff;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int m = rr + 16 * p;
      live[p] = m < M;
      const int mm = live[p] ? m : 0;
      const int seg = mm / seg_rows, in_seg = mm - seg * seg_rows;
      xrow[p] = (size_t)seg * pr.seg_stride + (size_t)in_seg * K;
      grow[p] = (size_t)seg * pr.seg_stride + (size_t)in_seg * N;
    }
  }
  const int tiles_k = (K + 63) / 64;
  float4 xq[NP];
  auto x_load = [&](int kt) {
    const int kc = kt * 64 + 4 * c4;
    const int col = kc < K ? kc : 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) xq[p] = strip_ldg4(pr.x + xrow[p] + col);
  };
  auto x_store = [&](float* xs, int kt) {
    const bool xcol = kt * 64 + 4 * c4 < K;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const bool ok = live[p] && xcol;
      *reinterpret_cast<float4*>(xs + (rr + 16 * p) * GW_XS + 4 * c4) =
          make_float4(ok ? xq[p].x : 0.f, ok ? xq[p].y : 0.f, ok ? xq[p].z : 0.f, ok ? xq[p].w : 0.f);
    }
  };
  // ---- the strip's g columns, once
  {
    const bool gcol = n0 + 4 * c4 < N;
    const int col = gcol ? n0 + 4 * c4 : 0;
    const float* zsrc = pr.act ? pr.z : pr.gy;                      // (no activation: a second look at g instead of a branch)
    float4 gq[NP], zq[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      gq[p] = strip_ldg4(pr.gy + grow[p] + col);
      zq[p] = strip_ldg4(zsrc + grow[p] + col);
    }
    x_load(0);                                                      // first x tile: arrives while act'(z) is applied
    strip_pin();
    if (pr.act == 1) {                                              // Swish: the model's activation, kept free of the switch
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        gq[p].x *= act_bwd(zq[p].x, 1); gq[p].y *= act_bwd(zq[p].y, 1);
        gq[p].z *= act_bwd(zq[p].z, 1); gq[p].w *= act_bwd(zq[p].w, 1);
      }
    } else if (pr.act) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        gq[p].x *= act_bwd(zq[p].x, pr.act); gq[p].y *= act_bwd(zq[p].y, pr.act);
        gq[p].z *= act_bwd(zq[p].z, pr.act); gq[p].w *= act_bwd(zq[p].w, pr.act);
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const bool ok = live[p] && gcol;
      *reinterpret_cast<float4*>(gs + (rr + 16 * p) * GW_GS + 4 * c4) =
          make_float4(ok ? gq[p].x : 0.f, ok ? gq[p].y : 0.f, ok ? gq[p].z : 0.f, ok ? gq[p].w : 0.f);
    }
  }
  x_store(xs0, 0);
  __syncthreads();
  double sq = 0.0;
  // Adam: p / m / v of a tile are requested ONE TILE AHEAD (two named register sets, the loop below alternates them): with
  // the requests in front of the tile's own MFMAs a block had 48 KB in flight for about a third of its time and the pass
  // ran at 3 TB/s whatever the row count (365 / 378 us at 48 / 96 rows for 46 M weights).  The last tile requests itself again.
  float4 pA[4], mA[4], vA[4], pB[4], mB[4], vB[4];
  size_t atA = 0, atB = 0;
  // (the step's constants once, in front of the loop: read per tile they put a vmcnt(0) -- every request in flight -- into each trip)
  const AdamStep a = MODE == GW_ADAM ? adam_step_of(ra.state, ra.lr, ra.beta1, ra.beta2, ra.eps) : AdamStep{};
  auto pmv_load = [&](int kt, float4 (&pp)[4], float4 (&mm)[4], float4 (&vv)[4], size_t& at0) {
    const int kc = (kt < tiles_k ? kt : tiles_k - 1) * 64 + 4 * i;
    at0 = (size_t)(pr.gW - ra.arena_g) + (kc < K ? kc : 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + 16 * wave + 4 * q + r;
      const size_t o = at0 + (size_t)(row < N ? row : 0) * K;
      pp[r] = strip_ldg4(ra.arena_p + o);
      const f4v tm = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) f4v*>((strip_gptr)(ra.arena_m + o)));
      const f4v tv = __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) f4v*>((strip_gptr)(ra.arena_v + o)));
      mm[r] = make_float4(tm.x, tm.y, tm.z, tm.w);
      vv[r] = make_float4(tv.x, tv.y, tv.z, tv.w);
    }
  };
  auto tile_step = [&](int kt, float4 (&pp)[4], float4 (&mm)[4], float4 (&vv)[4], size_t at0,
                       float4 (&pn)[4], float4 (&mn)[4], float4 (&vn)[4], size_t& atn) {
    const float* xs = (kt & 1) ? xs1 : xs0;
    const int kcol = kt * 64 + 4 * i;
    const int kn = kt + 1 < tiles_k ? kt + 1 : kt;                  // (the last trip requests its own tile again: no branch)
    x_load(kn);                                                     // travels under this tile's MFMAs
    if (MODE == GW_ADAM) pmv_load(kt + 1, pn, mn, vn, atn);         // used one trip from now
    strip_pin();
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ga = gs + q * GW_GS + 16 * wave + i;
    const float* xb = xs + q * GW_XS + 4 * i;
    // whole trip count of the row class (rows M .. 16 NP - 1 are zeros in LDS): unrolled, so that the LDS reads are
    // scheduled ahead of the MFMAs that use them (a rolled loop waits for each pair of reads in front of its MFMAs)
#pragma unroll
    for (int st = 0; st < 4 * NP; ++st) {
      const float a = ga[(4 * st) * GW_GS];
      const float4 b = *reinterpret_cast<const float4*>(xb + (4 * st) * GW_XS);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.w, acc[3], 0, 0, 0);
    }
    // issue order: the reads of two steps, then { 4 MFMAs, the reads of the step after next } -- the scheduler on its own
    // reuses one register set and waits for every read right in front of its MFMAs
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
    for (int st = 0; st < 4 * NP - 2; ++st) {
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
    if (kcol < K) {
      if (MODE == GW_STORE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = n0 + 16 * wave + 4 * q + r;
          if (row >= N) continue;
          float* dst = pr.gW + (size_t)row * K + kcol;
          float4 o = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
          if (pr.accumulate) { const float4 old = ldg4_global(dst); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
          stg4_global(dst, o);
        }
      } else if (MODE == GW_SUMSQ) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (n0 + 16 * wave + 4 * q + r >= N) continue;
#pragma unroll
          for (int c = 0; c < 4; ++c) sq += (double)acc[c][r] * (double)acc[c][r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = n0 + 16 * wave + 4 * q + r;
          if (row >= N) continue;
          const size_t o = at0 + (size_t)row * K;
          adam_elem(a, pp[r].x, acc[0][r], mm[r].x, vv[r].x); adam_elem(a, pp[r].y, acc[1][r], mm[r].y, vv[r].y);
          adam_elem(a, pp[r].z, acc[2][r], mm[r].z, vv[r].z); adam_elem(a, pp[r].w, acc[3][r], mm[r].w, vv[r].w);
          *reinterpret_cast<float4*>(ra.arena_p + o) = pp[r];
          __builtin_nontemporal_store(f4v{mm[r].x, mm[r].y, mm[r].z, mm[r].w}, reinterpret_cast<f4v*>(ra.arena_m + o));
          __builtin_nontemporal_store(f4v{vv[r].x, vv[r].y, vv[r].z, vv[r].w}, reinterpret_cast<f4v*>(ra.arena_v + o));
        }
      }
    }
    if (!DB) __syncthreads();
    x_store((kt & 1) ? xs0 : xs1, kn);                             // that buffer was last read one trip ago, behind a barrier
    __syncthreads();
  };
  if (MODE == GW_ADAM) pmv_load(0, pA, mA, vA, atA);
  for (int kt = 0; kt < tiles_k; kt += 2) {
    tile_step(kt, pA, mA, vA, atA, pB, mB, vB, atB);
    if (kt + 1 < tiles_k) tile_step(kt + 1, pB, mB, vB, atB, pA, mA, vA, atA);
  }
  if (MODE == GW_SUMSQ) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d);
    __shared__ double wave_sq[4];
    if (lane == 0) wave_sq[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_sq[0] + wave_sq[1]) + (wave_sq[2] + wave_sq[3]);
  }
  if (MODE != GW_ADAM && pr.gb && threadIdx.x < 64 && n0 + (int)threadIdx.x < N) {   // bias gradient: column sums of the staged strip
    float b4[4] = {0.f, 0.f, 0.f, 0.f};                            // rows 4 t + q per group q, groups paired as in the tile layout
    for (int t = 0; t < (M + 3) / 4; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) b4[g] += gs[(4 * t + g) * GW_GS + threadIdx.x];
    }
    const float bsum = (b4[0] + b4[1]) + (b4[2] + b4[3]);
    float* dst = pr.gb + n0 + threadIdx.x;
    *dst = pr.accumulate ? *dst + bsum : bsum;
  }
}

// The same with 128 x 128 output tiles (waves as a 2 x 2 grid of 64 x 64 quadrants: 4 row tiles x one 64-column group
// each): every staged operand row feeds twice the MFMAs, so the L2 -> LDS traffic per gW element halves.  Measured
// SLOWER than the 64 x 64 kernel on every workload (fewer, bigger blocks: 3 per CU; see primitives.wgrad_tile): opt-in.
constexpr int GW2_CHUNK = 32;
constexpr int GW2_GS = 144, GW2_XS = 128;

__global__ __launch_bounds__(256) void gathered_wgrad128_k(const WgradProblem* __restrict__ table, int n_problems) {
  __shared__ __attribute__((aligned(16))) float gs[GW2_CHUNK * GW2_GS];
  __shared__ __attribute__((aligned(16))) float xs[GW2_CHUNK * GW2_XS];
  const int lo = wg_find_problem(table, n_problems);
  const WgradProblem pr = table[lo];
  const int local = blockIdx.x - pr.block_begin;
  const int nb = local / pr.tiles_k, kt = local - nb * pr.tiles_k;
  const int M = pr.M, N = pr.N, K = pr.K;
  const int sr = pr.seg_rows > 0 ? pr.seg_rows : M;
  const int n0 = nb * 128, k0 = kt * 128;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = wave >> 1, wk = wave & 1;                          // quadrant: rows n0 + 64 wn .., columns k0 + 64 wk ..
  const int i = lane & 15, q = lane >> 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const int c4 = threadIdx.x & 31, rr = threadIdx.x >> 5;           // staging: 32 float4 columns x 8 rows per pass
  const bool gcol = n0 + 4 * c4 < N, xcol = k0 + 4 * c4 < K;
  constexpr int NP = GW2_CHUNK / 8;
  float4 gq[NP], xq[NP];
  auto chunk_load = [&](int m0) {
    const int rows = min(GW2_CHUNK, M - m0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = rr + 8 * p;
      const bool ok = r < rows;
      const int m = m0 + (ok ? r : 0);
      const int seg = m / sr, row = m - seg * sr;
      const size_t base = (size_t)seg * pr.seg_stride;
      gq[p] = ldg4_or_zero(pr.gy + base + (size_t)row * N + (gcol ? n0 + 4 * c4 : 0), ok && gcol);
      if (pr.act) {
        const float4 zz = ldg4_or_zero(pr.z + base + (size_t)row * N + (gcol ? n0 + 4 * c4 : 0), ok && gcol);
        gq[p].x *= act_bwd(zz.x, pr.act); gq[p].y *= act_bwd(zz.y, pr.act);
        gq[p].z *= act_bwd(zz.z, pr.act); gq[p].w *= act_bwd(zz.w, pr.act);
      }
      xq[p] = ldg4_or_zero(pr.x + base + (size_t)row * K + (xcol ? k0 + 4 * c4 : 0), ok && xcol);
    }
  };
  chunk_load(0);
  for (int m0 = 0; m0 < M; m0 += GW2_CHUNK) {
    const int rows = min(GW2_CHUNK, M - m0);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      *reinterpret_cast<float4*>(gs + (rr + 8 * p) * GW2_GS + 4 * c4) = gq[p];
      *reinterpret_cast<float4*>(xs + (rr + 8 * p) * GW2_XS + 4 * c4) = xq[p];
    }
    __syncthreads();
    if (m0 + GW2_CHUNK < M) chunk_load(m0 + GW2_CHUNK);
    const int steps = (rows + 3) / 4;
#pragma unroll 2
    for (int st = 0; st < steps; ++st) {
      const float4 b = *reinterpret_cast<const float4*>(xs + (4 * st + q) * GW2_XS + 64 * wk + 4 * i);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float a = gs[(4 * st + q) * GW2_GS + 64 * wn + 16 * t + i];
        bsum[t] += a;
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.x, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.y, acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.z, acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b.w, acc[t][3], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int kcol = k0 + 64 * wk + 4 * i;
  if (kcol < K) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 64 * wn + 16 * t + 4 * q + r;
        if (row >= N) continue;
        float4* dst = reinterpret_cast<float4*>(pr.gW + (size_t)row * K + kcol);
        float4 o = make_float4(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]);
        if (pr.accumulate) { const float4 old = *dst; o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
        *dst = o;
      }
  }
  if (pr.gb && kt == 0 && wk == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float b = bsum[t];
      b += __shfl_xor(b, 16);
      b += __shfl_xor(b, 32);
      const int n = n0 + 64 * wn + 16 * t + i;
      if (q == 0 && n < N) pr.gb[n] = pr.accumulate ? pr.gb[n] + b : b;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same 128 x 128 tiles on the bf16 matrix path at fp32 accuracy ("split operands").  Every fp32 operand value is
// written as the EXACT sum of three bf16 numbers, x = x1 + x2 + x3 (round-to-nearest splits: |x2| <= 2^-8 |x|,
// |x3| <= 2^-16 |x|; each residual is exactly representable, so nothing is lost in the operands), and a product
// sum_m g[m] x[m] is taken as six bf16 MFMA products with fp32 accumulation,
//     g1 x1 + (g1 x2 + g2 x1) + (g1 x3 + g2 x2 + g3 x1)
// -- every bf16 x bf16 product is exact in fp32; the dropped terms (g2 x3, g3 x2, g3 x3) are below 2^-23 of the product,
// i.e. under the rounding of the fp32 accumulation itself.  v_mfma_f32_16x16x32_bf16 retires 16x the MACs per cycle of
// v_mfma_f32_16x16x4_f32, so six of them cost 3/8 of the one fp32 instruction they replace.  The fp32 kernels above
// spend 60 % of their time in the MFMA pipe on the atom-level layers (704 - 2000 operand rows); this one is bound by
// LDS traffic and the split arithmetic instead: three planes per operand mean 3 (T + C) fragment reads per 6 T C MFMAs of a
// wave tile of T x C 16-blocks (0.25 reads per MFMA at 64 x 64) against the 0.5 an LDS of 128 B/clk can deliver per MFMA
// slot, plus the staging writes -- measured 1.15 - 1.3x the fp32 kernel, not the 2.7x of the MFMA rates.
// Measured error against fp64: the same as the fp32 MFMA kernel's
// (tests/test_hip_parity.py::test_split_bf16_weight_gradients_have_fp32_accuracy).
//
// Operands are staged TRANSPOSED ([column][m], 32 rows of m per chunk = one MFMA k step) because a lane's fragment is 8
// consecutive m of one column: a thread loads one float4 of 4 consecutive rows and writes, per column and per split,
// one 8-byte group of 4 bf16.  Rows of x are stored permuted (column 4 i + c of a 64-column group at row 16 c + i) so
// that lane i of the B fragment for c reads row 16 c + i: accumulator c of a lane is then column 4 i + c -- float4 stores.
typedef __bf16 sp_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));
typedef float sp_f32x2 __attribute__((ext_vector_type(2)));
constexpr int SP_CHUNK = 32;                 // rows of m per chunk
constexpr int SP_LD = 40;                    // bf16 per LDS row (80 bytes: 16 consecutive rows hit 16 distinct bank groups)

__device__ __forceinline__ void sp_split(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  const sp_f32x2 v = {a, b};
  const sp_bf16x2 h = __builtin_convertvector(v, sp_bf16x2);
  const sp_f32x2 r = v - __builtin_convertvector(h, sp_f32x2);        // exact
  const sp_bf16x2 m = __builtin_convertvector(r, sp_bf16x2);
  const sp_f32x2 r2 = r - __builtin_convertvector(m, sp_f32x2);       // exact, at most 8 significant bits
  const sp_bf16x2 l = __builtin_convertvector(r2, sp_bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  mid = __builtin_bit_cast(unsigned, m);
  lo = __builtin_bit_cast(unsigned, l);
}
// four consecutive m of one column -> the three 8-byte groups at dst (split s at dst + s * plane)
__device__ __forceinline__ void sp_store4(unsigned short* dst, int plane, float v0, float v1, float v2, float v3) {
  unsigned h0, m0, l0, h1, m1, l1;
  sp_split(v0, v1, h0, m0, l0);
  sp_split(v2, v3, h1, m1, l1);
  *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(dst + plane) = make_uint2(m0, m1);
  *reinterpret_cast<uint2*>(dst + 2 * plane) = make_uint2(l0, l1);
}

__global__ __launch_bounds__(256, 2) void wgrad_split128_k(const WgradProblem* __restrict__ table, int n_problems) {
  constexpr int PLANE = 128 * SP_LD;
  __shared__ __attribute__((aligned(16))) unsigned short gs[3 * PLANE];
  __shared__ __attribute__((aligned(16))) unsigned short xs[3 * PLANE];
  const int item = blockIdx.x;
  const int lo = wg_find_problem(table, n_problems, item);
  const WgradProblem pr = table[lo];
  const int local = item - pr.block_begin;
  const int nb = local / pr.tiles_k, kt = local - nb * pr.tiles_k;
  const int M = pr.M, N = pr.N, K = pr.K;
  const int sr = pr.seg_rows > 0 ? pr.seg_rows : M;
  const int n0 = nb * 128, k0 = kt * 128;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wn = wave >> 1, wk = wave & 1;                          // quadrant: rows n0 + 64 wn .., columns k0 + 64 wk ..
  const int i = lane & 15, q = lane >> 4;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging unit of a thread: float4 column c4 (of 32), rows 4 rq .. 4 rq + 3 of the chunk
  const int c4 = 8 * wave + (lane & 7), rq = lane >> 3;
  const bool gcol = n0 + 4 * c4 < N, xcol = k0 + 4 * c4 < K;
  const int gcol_at = gcol ? n0 + 4 * c4 : 0, xcol_at = xcol ? k0 + 4 * c4 : 0;
  const float* zsrc = pr.act ? pr.z : pr.gy;
  float4 gq[4], zq[4], xq[4];
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  auto chunk_load = [&](int m0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = min(m0 + 4 * rq + r, M - 1);
      const int seg = m / sr, row = m - seg * sr;
      const size_t base = (size_t)seg * pr.seg_stride;
      gq[r] = strip_ldg4(pr.gy + base + (size_t)row * N + gcol_at);
      zq[r] = strip_ldg4(zsrc + base + (size_t)row * N + gcol_at);
      xq[r] = strip_ldg4(pr.x + base + (size_t)row * K + xcol_at);
    }
    strip_pin();
  };
  unsigned short* gdst = gs + (4 * c4) * SP_LD + 4 * rq;
  unsigned short* xdst = xs + (64 * (c4 >> 4) + (c4 & 15)) * SP_LD + 4 * rq;          // + 16 j rows for component j
  auto chunk_store = [&](int m0) {
    if (pr.act == 1) {                                                // Swish: the model's activation, kept free of the switch
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gq[r].x *= act_bwd(zq[r].x, 1); gq[r].y *= act_bwd(zq[r].y, 1);
        gq[r].z *= act_bwd(zq[r].z, 1); gq[r].w *= act_bwd(zq[r].w, 1);
      }
    } else if (pr.act) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gq[r].x *= act_bwd(zq[r].x, pr.act); gq[r].y *= act_bwd(zq[r].y, pr.act);
        gq[r].z *= act_bwd(zq[r].z, pr.act); gq[r].w *= act_bwd(zq[r].w, pr.act);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                    // rows beyond M, columns beyond N / K: zeros
      const bool live = m0 + 4 * rq + r < M;
      if (!(live && gcol)) gq[r] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!(live && xcol)) xq[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bs[0] += (gq[0].x + gq[1].x) + (gq[2].x + gq[3].x);
    bs[1] += (gq[0].y + gq[1].y) + (gq[2].y + gq[3].y);
    bs[2] += (gq[0].z + gq[1].z) + (gq[2].z + gq[3].z);
    bs[3] += (gq[0].w + gq[1].w) + (gq[2].w + gq[3].w);
    sp_store4(gdst, PLANE, gq[0].x, gq[1].x, gq[2].x, gq[3].x);
    sp_store4(gdst + SP_LD, PLANE, gq[0].y, gq[1].y, gq[2].y, gq[3].y);
    sp_store4(gdst + 2 * SP_LD, PLANE, gq[0].z, gq[1].z, gq[2].z, gq[3].z);
    sp_store4(gdst + 3 * SP_LD, PLANE, gq[0].w, gq[1].w, gq[2].w, gq[3].w);
    sp_store4(xdst, PLANE, xq[0].x, xq[1].x, xq[2].x, xq[3].x);
    sp_store4(xdst + 16 * SP_LD, PLANE, xq[0].y, xq[1].y, xq[2].y, xq[3].y);
    sp_store4(xdst + 32 * SP_LD, PLANE, xq[0].z, xq[1].z, xq[2].z, xq[3].z);
    sp_store4(xdst + 48 * SP_LD, PLANE, xq[0].w, xq[1].w, xq[2].w, xq[3].w);
  };
  const unsigned short* ga = gs + (64 * wn + i) * SP_LD + 8 * q;      // + 16 t rows, + s planes
  const unsigned short* xb = xs + (64 * wk + i) * SP_LD + 8 * q;      // + 16 c rows, + s planes
  chunk_load(0);
  for (int m0 = 0; m0 < M; m0 += SP_CHUNK) {
    chunk_store(m0);
    __syncthreads();
    chunk_load(min(m0 + SP_CHUNK, M - 1));                           // the next chunk travels under this chunk's MFMAs
    sp_bf16x8 a[3][4];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) a[s][t] = *reinterpret_cast<const sp_bf16x8*>(ga + s * PLANE + 16 * t * SP_LD);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      sp_bf16x8 b[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) b[s] = *reinterpret_cast<const sp_bf16x8*>(xb + s * PLANE + 16 * c * SP_LD);
      // small terms first; four independent accumulators between two uses of one
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][t], b[2], acc[t][c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][t], b[0], acc[t][c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][t], b[1], acc[t][c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][t], b[1], acc[t][c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][t], b[0], acc[t][c], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][t], b[0], acc[t][c], 0, 0, 0);
    }
    __syncthreads();
  }
  const int kcol = k0 + 64 * wk + 4 * i;
  if (kcol < K) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 64 * wn + 16 * t + 4 * q + r;
        if (row >= N) continue;
        float* dst = pr.gW + (size_t)row * K + kcol;
        float4 o = make_float4(acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]);
        if (pr.accumulate) { const float4 old = ldg4_global(dst); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
        stg4_global(dst, o);
      }
  }
  if (pr.gb && kt == 0) {                                           // bias: the 8 row groups of a column meet by shuffle
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float b = bs[j];
      b += __shfl_xor(b, 8);
      b += __shfl_xor(b, 16);
      b += __shfl_xor(b, 32);
      const int n = n0 + 4 * c4 + j;
      if (rq == 0 && n < N) pr.gb[n] = pr.accumulate ? pr.gb[n] + b : b;
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// STRIP layout on the bf16 matrix path with split operands -- the weight gradients of the bead-level layers of a LARGE bead
// batch (33 .. 96 operand rows: dipeptide's 96 beads, the 64 beads of the 2000-atom graph, 8 ranks x 12 gathered rows).
// gathered_wgrad_strip_k above is bound by the fp32 MFMA pipe there (96 rows: 11.7 GF in 99 us = 118 TF/s for 243 MB of
// gradients that HBM takes in ~50 us); wgrad_split128_k re-derives the three bf16 terms of BOTH operand tiles in every
// 128 x 128 block and ends up no faster (154 us on the same problems).  Here the split is done where it is cheap:
//   * x (M x K, shared by all N / 64 strips of a problem) is split ONCE, by strip_xplanes_k, into its three bf16 planes,
//     laid out as the LDS images the strips stage: [k tile of 64][plane][64 rows][MP] with m contiguous (MP = M rounded up to
//     the MFMA's 32-deep step) and the tile's columns permuted (column 4 j + c at row 16 c + j: accumulator c of lane j is
//     then column 4 j + c -- float4 stores).  3 x K x MP x 2 bytes per problem (345 KB at 96 x 600), L2 resident.
//   * g = gy * act'(z) of a strip's 64 columns is staged once per block (fp32, as the fp32 strip kernel does), each lane
//     takes its A fragments -- 8 consecutive m of one column -- out of it, splits them in registers and KEEPS them for
//     the whole walk over the strip's K / 64 column tiles.
// Per tile a block then copies 3 x 64 x MP bf16 to LDS (no arithmetic), reads 36 fragments per wave and issues 72
// v_mfma_f32_16x16x32_bf16 (at 96 rows) for 64 x 64 outputs: bound by the gW stores.  Same six products per fp32 product as
// wgrad_split128_k (dropped terms below 2^-23 of a product), same accuracy class; NOT bit-identical to the fp32 kernels.
constexpr int SS_MAX_ROWS = 96;
__host__ __device__ constexpr int ss_mp(int M) { return (M + 31) / 32 * 32; }
__host__ __device__ constexpr size_t ss_plane_bytes(int M, int K) { return (size_t)((K + 63) / 64) * 3 * 64 * ss_mp(M) * 2; }

// x planes of every problem of the table: grid (max k tiles, problems); pr.pad = offset of the problem's planes in ws, in
// 256-byte units
__global__ __launch_bounds__(256) void strip_xplanes_k(const WgradProblem* __restrict__ table, unsigned short* __restrict__ ws) {
  const WgradProblem pr = table[blockIdx.y];
  const int kt = blockIdx.x;
  const int K = pr.K, M = pr.M;
  if (kt * 64 >= K) return;
  const int MP = ss_mp(M);
  unsigned short* tile = ws + (size_t)pr.pad * 128 + (size_t)kt * 3 * 64 * MP;
  const int kk = threadIdx.x & 63;                                   // column of the tile
  const int rr = 16 * (kk & 3) + (kk >> 2);                          // its row in the image
  const int col = kt * 64 + kk;
  const bool cok = col < K;
  for (int mg = threadIdx.x >> 6; mg < MP / 8; mg += 4) {            // groups of 8 consecutive m
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int m = 8 * mg + e;
      v[e] = (cok && m < M) ? pr.x[wg_row(pr, m, K) + col] : 0.f;
    }
    unsigned h[4], md[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sp_split(v[2 * e], v[2 * e + 1], h[e], md[e], l[e]);
    unsigned short* dst = tile + (size_t)rr * MP + 8 * mg;
    *reinterpret_cast<uint4*>(dst) = make_uint4(h[0], h[1], h[2], h[3]);
    *reinterpret_cast<uint4*>(dst + 64 * MP) = make_uint4(md[0], md[1], md[2], md[3]);
    *reinterpret_cast<uint4*>(dst + 2 * 64 * MP) = make_uint4(l[0], l[1], l[2], l[3]);
  }
}

template <int KS>   // 32-deep steps of the reduction: M <= 32 KS
__global__ __launch_bounds__(256) void strip_split_k(const WgradProblem* __restrict__ table, int n_problems,
                                                     const unsigned short* __restrict__ ws) {
  constexpr int MP = 32 * KS;
  constexpr int XLD = MP + 8;                                        // bf16 per image row in LDS (16 bytes of padding)
  constexpr int XPLANE = 64 * XLD;
  constexpr int G_FLOATS = MP * GW_GS, X_SHORTS = 3 * XPLANE;
  constexpr int LDS_BYTES = (G_FLOATS * 4 > X_SHORTS * 2) ? G_FLOATS * 4 : X_SHORTS * 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
  float* gs = reinterpret_cast<float*>(smem);                        // [MP][GW_GS] fp32 g' (first phase)
  unsigned short* xs = reinterpret_cast<unsigned short*>(smem);      // [3][64][XLD] bf16 x planes of a tile (afterwards)
  const int lo = wg_find_problem(table, n_problems);
  const WgradProblem pr = table[lo];
  const int nb = blockIdx.x - pr.block_begin;
  const int M = pr.M, N = pr.N, K = pr.K;
  const int n0 = nb * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  // ---- the strip's g columns: staged as fp32 (rows beyond M, columns beyond N: zeros), the bias sum, the A fragments
  {
    const int c4 = threadIdx.x & 15, rr = threadIdx.x >> 4;          // 16 float4 columns x 16 rows per pass
    const bool gcol = n0 + 4 * c4 < N;
    const int col = gcol ? n0 + 4 * c4 : 0;
    const float* zsrc = pr.act ? pr.z : pr.gy;
#pragma unroll
    for (int p = 0; p < MP / 16; ++p) {
      const int m = rr + 16 * p;
      const bool ok = m < M && gcol;
      const size_t at = wg_row(pr, m < M ? m : 0, N) + col;
      float4 g4 = strip_ldg4(pr.gy + at);
      if (pr.act) {
        const float4 z4 = strip_ldg4(zsrc + at);
        g4.x *= act_bwd(z4.x, pr.act); g4.y *= act_bwd(z4.y, pr.act); g4.z *= act_bwd(z4.z, pr.act); g4.w *= act_bwd(z4.w, pr.act);
      }
      *reinterpret_cast<float4*>(gs + m * GW_GS + 4 * c4) = make_float4(ok ? g4.x : 0.f, ok ? g4.y : 0.f, ok ? g4.z : 0.f, ok ? g4.w : 0.f);
    }
  }
  __syncthreads();
  if (pr.gb) {                                                       // bias gradient: column sums (four row classes, added in order)
    const int cI = threadIdx.x & 63, cls = threadIdx.x >> 6;
    float b = 0.f;
    for (int m = cls; m < MP; m += 4) b += gs[m * GW_GS + cI];       // (rows beyond M are zeros)
    __shared__ float bias_part[4][64];
    bias_part[cls][cI] = b;
    __syncthreads();
    if (threadIdx.x < 64) {
      const int n = n0 + (int)threadIdx.x;
      const float t = (bias_part[0][cI] + bias_part[1][cI]) + (bias_part[2][cI] + bias_part[3][cI]);
      if (n < N) pr.gb[n] = pr.accumulate ? pr.gb[n] + t : t;
    }
  }
  sp_bf16x8 a[3][KS];                                                // lane (i, q): rows m = 32 ks + 8 q .. + 7 of column 16 wave + i
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    unsigned h[4], md[4], l[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* src = gs + (32 * ks + 8 * q + 2 * e) * GW_GS + 16 * wave + i;
      sp_split(src[0], src[GW_GS], h[e], md[e], l[e]);
    }
    a[0][ks] = __builtin_bit_cast(sp_bf16x8, make_uint4(h[0], h[1], h[2], h[3]));
    a[1][ks] = __builtin_bit_cast(sp_bf16x8, make_uint4(md[0], md[1], md[2], md[3]));
    a[2][ks] = __builtin_bit_cast(sp_bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
  }
  // ---- walk over the strip's column tiles
  const int tiles_k = (K + 63) / 64;
  const unsigned short* planes = ws + (size_t)pr.pad * 128;
  const int MPp = ss_mp(M);                                          // this problem's plane rows hold MPp <= MP values of m
  constexpr int PIECES = 3 * 64 * MP / 8;                            // 16-byte pieces of a tile's LDS image
  constexpr int PER = (PIECES + 255) / 256;
  typedef unsigned su4 __attribute__((ext_vector_type(4)));
  su4 xr[PER];
  // piece pc of the image: row pc / (MP / 8) (= plane * 64 + image row), 16-byte piece pc % (MP / 8) of it; a problem with
  // fewer rows than the table's largest has shorter plane rows: the pieces beyond them are zeros (their a fragments are
  // zeros too, but what LDS holds there must not be a NaN pattern)
  auto x_load = [&](int kt) {
    const unsigned short* src = planes + (size_t)kt * 3 * 64 * MPp;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int pc = (int)threadIdx.x + 256 * u;
      const int row = pc / (MP / 8), piece = pc - row * (MP / 8);
      const bool ok = pc < PIECES && 8 * piece < MPp;
      const su4 v = *reinterpret_cast<const __attribute__((address_space(1))) su4*>(
          (strip_gptr)(const void*)(src + (ok ? row * MPp + 8 * piece : 0)));
      xr[u] = ok ? v : su4{0u, 0u, 0u, 0u};
    }
    strip_pin();
  };
  auto x_store = [&]() {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int pc = (int)threadIdx.x + 256 * u;
      if (pc < PIECES) {
        const int row = pc / (MP / 8), piece = pc - row * (MP / 8);
        *reinterpret_cast<su4*>(xs + row * XLD + 8 * piece) = xr[u];
      }
    }
  };
  x_load(0);
  const unsigned short* xb = xs + i * XLD + 8 * q;                    // + 16 c rows, + s planes, + 32 ks
  for (int kt = 0; kt < tiles_k; ++kt) {
    __syncthreads();                                                 // the fragments of g' / of the last tile are read
    x_store();
    __syncthreads();
    x_load(kt + 1 < tiles_k ? kt + 1 : kt);                          // travels under this tile's MFMAs
    f32x4v acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      sp_bf16x8 b[4][3];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int s3 = 0; s3 < 3; ++s3) b[c][s3] = *reinterpret_cast<const sp_bf16x8*>(xb + s3 * XPLANE + 16 * c * XLD + 32 * ks);
      // small terms first (as wgrad_split128_k); the four column blocks' accumulators between two uses of one
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][ks], b[c][2], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][ks], b[c][0], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][ks], b[c][1], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][ks], b[c][1], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][ks], b[c][0], acc[c], 0, 0, 0);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][ks], b[c][0], acc[c], 0, 0, 0);
    }
    const int kcol = kt * 64 + 4 * i;
    if (kcol < K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 16 * wave + 4 * q + r;
        if (row >= N) continue;
        float* dst = pr.gW + (size_t)row * K + kcol;
        float4 o = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        if (pr.accumulate) { const float4 old = ldg4_global(dst); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
        stg4_global(dst, o);
      }
    }
  }
}

// Packs the operands of queued weight-gradient problems into one contiguous send buffer:
//   dst_g[M,N] = gy * act'(z)      dst_x[M,K] = x        (float4 granularity; N % 4 == 0, K % 4 == 0)
struct PackProblem {        // mirrors the 64-byte host record built in python (trainer.OperandExchange)
  const float* gy;
  const float* z;           // pre-activation or NULL
  const float* x;
  float* dst_g;
  float* dst_x;
  int M, N, K, act;
  int block_begin;
  int pad[1];
};
static_assert(sizeof(PackProblem) == 64, "host/device record layout");
constexpr int PACK_F4_PER_BLOCK = 1024;

__global__ __launch_bounds__(256) void pack_operands_k(const PackProblem* __restrict__ table, int n_problems) {
  const int lo = wg_find_problem(table, n_problems);
  const PackProblem pr = table[lo];
  const int ng4 = pr.M * pr.N / 4, nx4 = pr.M * pr.K / 4;
  const int base = (blockIdx.x - pr.block_begin) * PACK_F4_PER_BLOCK;
#pragma unroll
  for (int t = 0; t < PACK_F4_PER_BLOCK / 256; ++t) {
    const int idx = base + t * 256 + threadIdx.x;
    if (idx < ng4) {
      float4 g = reinterpret_cast<const float4*>(pr.gy)[idx];
      if (pr.act) {
        const float4 zz = reinterpret_cast<const float4*>(pr.z)[idx];
        g.x *= act_bwd(zz.x, pr.act); g.y *= act_bwd(zz.y, pr.act); g.z *= act_bwd(zz.z, pr.act); g.w *= act_bwd(zz.w, pr.act);
      }
      reinterpret_cast<float4*>(pr.dst_g)[idx] = g;
    } else if (idx < ng4 + nx4) {
      reinterpret_cast<float4*>(pr.dst_x)[idx - ng4] = reinterpret_cast<const float4*>(pr.x)[idx - ng4];
    }
  }
}

template <int MODE, int NP>
static int strip_launch_np(const void* table_dev, int n_problems, int total_blocks, double* partial, RankUpdateArgs ra,
                           hipStream_t st, const char* what) {
  const size_t lds = sizeof(float) * (size_t)(16 * NP) * (GW_GS + (NP < GS_SINGLE_FROM ? 2 : 1) * GW_XS);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gathered_wgrad_strip_k<MODE, NP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("%s: %zu bytes of LDS: %s", what, lds, hipGetErrorString(e)); return (int)e; }
  }
  hipLaunchKernelGGL((gathered_wgrad_strip_k<MODE, NP>), dim3(total_blocks), dim3(256), lds, st,
                     reinterpret_cast<const WgradProblem*>(table_dev), n_problems, partial, ra);
  return check_launch(what);
}
template <int MODE>
static int strip_launch(const void* table_dev, int n_problems, int total_blocks, int max_rows, double* partial, RankUpdateArgs ra,
                        hipStream_t st, const char* what) {
  if (max_rows <= 32) return strip_launch_np<MODE, 2>(table_dev, n_problems, total_blocks, partial, ra, st, what);
  if (max_rows <= 48) return strip_launch_np<MODE, 3>(table_dev, n_problems, total_blocks, partial, ra, st, what);
  if (max_rows <= 64) return strip_launch_np<MODE, 4>(table_dev, n_problems, total_blocks, partial, ra, st, what);
  if (max_rows <= 80) return strip_launch_np<MODE, 5>(table_dev, n_problems, total_blocks, partial, ra, st, what);
  if (max_rows <= 96) return strip_launch_np<MODE, 6>(table_dev, n_problems, total_blocks, partial, ra, st, what);
  return strip_launch_np<MODE, 8>(table_dev, n_problems, total_blocks, partial, ra, st, what);
}
}  // namespace cgv

extern "C" {

/* Weight gradients over gathered operand rows (include/cgvae_hip.h: data-parallel operand exchange). */
int cgv_wgrad_gathered_plan(int M, int N, int K, int seg_rows, int* tiles_k, int* n_blocks) {
  return cgv_wgrad_gathered_plan_tile(M, N, K, seg_rows, 64, tiles_k, n_blocks);
}

/* tile = 64 or 128: output tile edge of the launch (one value per launch, see cgv_grouped_wgrad_gathered_tile) */
int cgv_wgrad_gathered_plan_tile(int M, int N, int K, int seg_rows, int tile, int* tiles_k, int* n_blocks) {
  CGV_REQUIRE(tiles_k && n_blocks, "null pointer");
  CGV_REQUIRE(M >= 1 && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0, "unsupported shape (need N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(seg_rows == 0 || (seg_rows > 0 && seg_rows % 4 == 0), "rank segments must hold a multiple of 4 rows");
  CGV_REQUIRE(tile == 64 || tile == 128, "tile must be 64 or 128");
  const int tile_k = tile == 64 ? cgv::GW_TW : tile;        // (the 64-row tiles are GW_TW = 128 columns wide)
  *tiles_k = (K + tile_k - 1) / tile_k;
  *n_blocks = ((N + tile - 1) / tile) * *tiles_k;
  return 0;
}

/* The grouped weight gradients of cgv_grouped_wgrad_gathered_tile(tile = 128: same table, same plan) on the bf16 matrix
 * path with split operands (three bf16 terms per fp32 value, six products, fp32 accumulation: fp32-class accuracy at
 * 3/8 of the fp32 MFMA time; wgrad_split128_k). */
int cgv_grouped_wgrad_split(const void* table_dev, int n_problems, int total_blocks, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev, "null table");
  hipLaunchKernelGGL(cgv::wgrad_split128_k, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const cgv::WgradProblem*>(table_dev), n_problems);
  return cgv::check_launch("cgv_grouped_wgrad_split");
}

/* Strip layout on the bf16 matrix path with split operands (strip_split_k): records as cgv_grouped_wgrad_strip's with at
 * most cgv_wgrad_strip_split_max_rows() rows, `pad` = offset of the problem's x planes in ws in 256-byte units (each problem
 * needs cgv_wgrad_strip_split_plane_bytes(M, K), rounded up to 256).  Two launches: the x planes of every problem, the strips. */
int cgv_wgrad_strip_split_max_rows(void) { return cgv::SS_MAX_ROWS; }
size_t cgv_wgrad_strip_split_plane_bytes(int M, int K) {
  if (M < 1 || M > cgv::SS_MAX_ROWS || K < 4) return 0;
  return (cgv::ss_plane_bytes(M, K) + 255) & ~(size_t)255;
}
int cgv_grouped_wgrad_strip_split(const void* table_dev, int n_problems, int total_blocks, int max_rows, int max_k, void* ws,
                                  size_t ws_bytes, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && ws && max_rows >= 1 && max_rows <= cgv::SS_MAX_ROWS && max_k >= 4, "bad argument");
  CGV_REQUIRE((((uintptr_t)ws) & 255) == 0 && ws_bytes > 0, "workspace must be 256-byte aligned");
  CGV_REQUIRE(n_problems <= 65535, "too many problems");
  hipStream_t st = (hipStream_t)stream;
  const cgv::WgradProblem* table = reinterpret_cast<const cgv::WgradProblem*>(table_dev);
  hipLaunchKernelGGL(cgv::strip_xplanes_k, dim3((max_k + 63) / 64, n_problems), dim3(256), 0, st, table,
                     reinterpret_cast<unsigned short*>(ws));
  if (int rc = cgv::check_launch("cgv_grouped_wgrad_strip_split (planes)")) return rc;
  const unsigned short* planes = reinterpret_cast<const unsigned short*>(ws);
  if (max_rows <= 32) hipLaunchKernelGGL(cgv::strip_split_k<1>, dim3(total_blocks), dim3(256), 0, st, table, n_problems, planes);
  else if (max_rows <= 64) hipLaunchKernelGGL(cgv::strip_split_k<2>, dim3(total_blocks), dim3(256), 0, st, table, n_problems, planes);
  else hipLaunchKernelGGL(cgv::strip_split_k<3>, dim3(total_blocks), dim3(256), 0, st, table, n_problems, planes);
  return cgv::check_launch("cgv_grouped_wgrad_strip_split");
}

int cgv_grouped_wgrad_gathered(const void* table_dev, int n_problems, int total_blocks, void* stream) {
  return cgv_grouped_wgrad_gathered_tile(table_dev, n_problems, total_blocks, 64, stream);
}

int cgv_grouped_wgrad_gathered_tile(const void* table_dev, int n_problems, int total_blocks, int tile, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  CGV_REQUIRE(tile == 64 || tile == 128, "tile must be 64 or 128");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev, "null table");
  if (tile == 128)
    hipLaunchKernelGGL(cgv::gathered_wgrad128_k, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const cgv::WgradProblem*>(table_dev), n_problems);
  else
    hipLaunchKernelGGL(cgv::gathered_wgrad_k<cgv::GW_STORE>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const cgv::WgradProblem*>(table_dev), n_problems, (double*)nullptr, cgv::RankUpdateArgs{});
  return cgv::check_launch("cgv_grouped_wgrad_gathered");
}

/* Rank update over (gathered) operand rows with MFMA tiles, for row counts beyond the FMA-per-row kernel's range
 * (cgv_grouped_wgrad_adam): the table and plan of cgv_grouped_wgrad_gathered (tile 64), accumulate = 0.
 *   _sumsq: sumsq[i] = ||gW_i||_F^2 for record i (tiles formed, squared, never stored; block partials in `partial`,
 *           total_blocks doubles) and the bias gradients written;
 *   _adam:  the tiles formed again and run through the clipped Adam update of their weights (state from
 *           cgv_optim_prepare_extra with those norms); every gW must lie inside the gradient arena. */
int cgv_grouped_wgrad_gathered_sumsq(const void* table_dev, int n_problems, int total_blocks, double* partial, double* sumsq,
                                     void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && partial && sumsq, "null pointer");
  const cgv::WgradProblem* table = reinterpret_cast<const cgv::WgradProblem*>(table_dev);
  hipLaunchKernelGGL(cgv::gathered_wgrad_k<cgv::GW_SUMSQ>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table,
                     n_problems, partial, cgv::RankUpdateArgs{});
  hipLaunchKernelGGL(cgv::gathered_sumsq_reduce_k, dim3(n_problems), dim3(256), 0, (hipStream_t)stream, table, n_problems,
                     total_blocks, partial, sumsq);
  return cgv::check_launch("cgv_grouped_wgrad_gathered_sumsq");
}

int cgv_grouped_wgrad_gathered_adam(const void* table_dev, int n_problems, int total_blocks, const float* arena_g,
                                    float* arena_p, float* arena_m, float* arena_v, float lr, float beta1, float beta2,
                                    float eps, const float* state, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && arena_g && arena_p && arena_m && arena_v && state, "null pointer");
  CGV_REQUIRE(((((uintptr_t)arena_g | (uintptr_t)arena_p | (uintptr_t)arena_m | (uintptr_t)arena_v)) & 15) == 0,
              "arenas must be 16-byte aligned");
  hipLaunchKernelGGL(cgv::gathered_wgrad_k<cgv::GW_ADAM>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const cgv::WgradProblem*>(table_dev), n_problems, (double*)nullptr,
                     cgv::RankUpdateArgs{arena_g, arena_p, arena_m, arena_v, state, lr, beta1, beta2, eps});
  return cgv::check_launch("cgv_grouped_wgrad_gathered_adam");
}

/* The strip layout of the gathered launches for problems of at most 128 operand rows (csrc: gathered_wgrad_strip_k): a
 * block per 64 ROWS of gW (it walks that strip's column tiles itself).  Plan: n_blocks = ceil(N / 64); records as for
 * cgv_grouped_wgrad_gathered with block_begin counted in these blocks.  Results are bit-identical to the tile layout. */
int cgv_wgrad_strip_max_rows(void) { return cgv::GS_MAX_ROWS; }
int cgv_wgrad_strip_plan(int M, int N, int K, int seg_rows, int* n_blocks) {
  CGV_REQUIRE(n_blocks, "null pointer");
  CGV_REQUIRE(M >= 1 && M <= cgv::GS_MAX_ROWS && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0, "unsupported shape (need M <= 128, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(seg_rows == 0 || (seg_rows > 0 && seg_rows % 4 == 0), "rank segments must hold a multiple of 4 rows");
  *n_blocks = (N + 63) / 64;
  return 0;
}

int cgv_grouped_wgrad_strip(const void* table_dev, int n_problems, int total_blocks, int max_rows, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && max_rows >= 1 && max_rows <= cgv::GS_MAX_ROWS, "bad argument");
  return cgv::strip_launch<cgv::GW_STORE>(table_dev, n_problems, total_blocks, max_rows, nullptr, cgv::RankUpdateArgs{},
                                          (hipStream_t)stream, "cgv_grouped_wgrad_strip");
}

int cgv_grouped_wgrad_strip_sumsq(const void* table_dev, int n_problems, int total_blocks, int max_rows, double* partial,
                                  double* sumsq, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && partial && sumsq && max_rows >= 1 && max_rows <= cgv::GS_MAX_ROWS, "bad argument");
  if (int rc = cgv::strip_launch<cgv::GW_SUMSQ>(table_dev, n_problems, total_blocks, max_rows, partial, cgv::RankUpdateArgs{},
                                                (hipStream_t)stream, "cgv_grouped_wgrad_strip_sumsq")) return rc;
  hipLaunchKernelGGL(cgv::gathered_sumsq_reduce_k, dim3(n_problems), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const cgv::WgradProblem*>(table_dev), n_problems, total_blocks, partial, sumsq);
  return cgv::check_launch("cgv_grouped_wgrad_strip_sumsq");
}

int cgv_grouped_wgrad_strip_adam(const void* table_dev, int n_problems, int total_blocks, int max_rows, const float* arena_g,
                                 float* arena_p, float* arena_m, float* arena_v, float lr, float beta1, float beta2, float eps,
                                 const float* state, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev && arena_g && arena_p && arena_m && arena_v && state && max_rows >= 1 && max_rows <= cgv::GS_MAX_ROWS, "bad argument");
  CGV_REQUIRE(((((uintptr_t)arena_g | (uintptr_t)arena_p | (uintptr_t)arena_m | (uintptr_t)arena_v)) & 15) == 0,
              "arenas must be 16-byte aligned");
  return cgv::strip_launch<cgv::GW_ADAM>(table_dev, n_problems, total_blocks, max_rows, nullptr,
                                         cgv::RankUpdateArgs{arena_g, arena_p, arena_m, arena_v, state, lr, beta1, beta2, eps},
                                         (hipStream_t)stream, "cgv_grouped_wgrad_strip_adam");
}

int cgv_pack_record_bytes(void) { return (int)sizeof(cgv::PackProblem); }

int cgv_pack_plan(int M, int N, int K, int* n_blocks) {
  CGV_REQUIRE(n_blocks, "null pointer");
  CGV_REQUIRE(M >= 1 && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0, "unsupported shape (need N % 4 == 0, K % 4 == 0)");
  const long long f4 = (long long)M * (N + K) / 4;
  *n_blocks = (int)((f4 + cgv::PACK_F4_PER_BLOCK - 1) / cgv::PACK_F4_PER_BLOCK);
  return 0;
}

int cgv_pack_operands(const void* table_dev, int n_problems, int total_blocks, void* stream) {
  CGV_REQUIRE(n_problems >= 0 && total_blocks >= 0, "bad size");
  if (n_problems == 0 || total_blocks == 0) return 0;
  CGV_REQUIRE(table_dev, "null table");
  hipLaunchKernelGGL(cgv::pack_operands_k, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const cgv::PackProblem*>(table_dev), n_problems);
  return cgv::check_launch("cgv_pack_operands");
}

}  // extern "C"
