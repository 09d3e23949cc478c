// Skinny fp32 GEMMs for the node-level Dense layers on the bead graph (M = beads or 3*beads
// rows, 12..64; K, N = n_basis multiples, 600..5400).
//
// Reference: Dense / nn.Linear forward (CoarseGrainingVAE/modules.py:103-114, activation Swish
// modules.py:16-21) and its autograd backward, ~70 layer-uses per training step of the chignolin
// config.  With M <= 64 these products are weight-streaming (GEMV-like): the [N,K] weight
// (1.4 - 13 MB) is read once, the arithmetic is negligible, and what a step pays is mostly the
// NUMBER of launches (measured: ~4-5 us of GPU time per small kernel inside the captured step
// graph, profiles/r01d).  So the design goal here is launches, then bytes:
//   fwd        z = x W^T + b ; y = act(z)          ONE launch (bias + Swish in the epilogue)
//   bwd_input  gx = (gy * act'(z)) W               ONE launch (activation backward in the operand
//                                                   load, N-split over 16 waves reduced in LDS --
//                                                   no partial buffers, no second kernel)
//   wgrad      gW (+)= (gy * act'(z))^T x, gb      ONE launch PER STEP for all layers: wgrad_grouped.hip
//                                                   (norms: wgrad_gram.hip, gathered operands: wgrad_gathered.hip)
// Matrix products use v_mfma_f32_16x16x4_f32: exact fp32 FMA chains (bitwise an fmaf loop).
//
// MFMA 16x16x4 f32 operand map (cdna_hip_programming.md 3): lane l holds A[i = l&15][k = l>>4],
// B[k = l>>4][j = l&15]; D: col j = l&15, row i = 4*(l>>4) + reg.
#include "cgv_common.h"
#include "gemm_dev.h"

namespace cgv {

// ------------------------------------------------------------------ fwd
// Block = 16 output columns n0..n0+15, WAVES waves splitting K in whole 16-float steps.  Lane
// (i = l&15, q = l>>4) loads W[n0+i, 16 s + 4 q .. +3] (16 rows x 64 contiguous bytes per wave
// instruction) and the matching x[m, ...] float4; component c feeds MFMA c (k = 16 s + 4 q + c).
// D: lane holds y[m = 16 mb + (l&15)][n0 + 4 q + r], r = 0..3 -> one 16-byte store per m-block.
template <int MB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void skinny_fwd_k(const float* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ y,
                                                           float* __restrict__ zout, int M, int N, int K, int act) {
  __shared__ float red[(WAVES - 1) * MB * 4 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16;
  {                                     // blockIdx.y: this block's 16 MB rows (more, smaller blocks when there are few column blocks)
    const int m0 = blockIdx.y * 16 * MB;
    x += (size_t)m0 * K; y += (size_t)m0 * N;
    if (zout) zout += (size_t)m0 * N;
    M = min(M - m0, 16 * MB);
  }
  const int nrow = n0 + i;
  const bool nok = nrow < N;
  const float* wrow = W + (size_t)(nok ? nrow : 0) * K;
  const int steps = (K + 15) / 16;
  const int per = (steps + WAVES - 1) / WAVES;
  const int s_beg = wave * per, s_end = min(s_beg + per, steps);
  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Loads are unconditional (rows / columns clamped into range): rows beyond M or N give products that are never
  // stored, and the reduction tail is zeroed on W's side only.  A guarded load is a branch: the loop then neither
  // unrolls nor keeps more than one step's loads in flight (s_waitcnt vmcnt(0) per step), and a wave's 2 - 3 steps
  // each paid a full memory round trip.
  const float* xrow[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) xrow[mb] = x + (size_t)(mb * 16 + i < M ? mb * 16 + i : 0) * K;
  constexpr int SB = MB >= 3 ? 2 : 4;             // steps whose loads are issued together (the compiler does not
  for (int s0 = s_beg; s0 < s_end; s0 += SB) {    // unroll this loop by itself: runtime bounds)
    float4 a[SB], b[SB][MB];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int k = (s0 + u) * 16 + 4 * q;
      const bool kok = s0 + u < s_end && k < K;   // K % 4 == 0: a float4 is entirely in or out
      const int kc = kok ? k : 0;
      a[u] = *reinterpret_cast<const float4*>(wrow + kc);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) b[u][mb] = *reinterpret_cast<const float4*>(xrow[mb] + kc);
    }
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      if (s0 + u < s_end) {                       // wave-uniform
        const bool kok = (s0 + u) * 16 + 4 * q < K;
        const float4 w = make_float4(kok ? a[u].x : 0.f, kok ? a[u].y : 0.f, kok ? a[u].z : 0.f, kok ? a[u].w : 0.f);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b[u][mb].x, acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b[u][mb].y, acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b[u][mb].z, acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b[u][mb].w, acc[mb], 0, 0, 0);
        }
      }
    }
  }
  if (WAVES > 1) {
    if (wave > 0) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(((wave - 1) * MB + mb) * 4 + r) * 64 + lane] = acc[mb][r];
    }
    __syncthreads();
    if (wave != 0) return;
  }
  const int n = n0 + 4 * q;
  if (n >= N) return;                              // N % 4 == 0
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mb * 16 + i;
    f32x4 t = acc[mb];
    for (int w = 0; w < WAVES - 1; ++w)
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] += red[((w * MB + mb) * 4 + r) * 64 + lane];
    if (m < M) {
      const float4 zv = make_float4(t[0] + bv.x, t[1] + bv.y, t[2] + bv.z, t[3] + bv.w);
      if (act) {
        if (zout) *reinterpret_cast<float4*>(zout + (size_t)m * N + n) = zv;
        *reinterpret_cast<float4*>(y + (size_t)m * N + n) =
            make_float4(act_fwd(zv.x, act), act_fwd(zv.y, act), act_fwd(zv.z, act), act_fwd(zv.w, act));
      } else {
        *reinterpret_cast<float4*>(y + (size_t)m * N + n) = zv;
      }
    }
  }
}

// ------------------------------------------------------------------ bwd_input
// gx[m, k] = sum_n g[m, n] W[n, k],  g = gy * act'(z).  The weight is read in ROW-contiguous
// pieces: block (kt, ns) owns 64 columns k0..k0+63 (256 contiguous bytes per weight row) and the
// row slice [ns*rpb, ns*rpb + rpb); wave w of 4 takes rows 4w..4w+3 of every group of 16.
// Lane (j = l&15, q = l>>4) loads the float4 W[n + q, k0 + 4j .. +3]; component c is the B operand
// B[kk = q][col j] of MFMA c, A[i = j][kk = q] = g[m = 16 mb + j][n + q] comes from an LDS stage
// of g (coalesced row reads, activation derivative applied once).  D_c: lane holds
// gx[m = 16 mb + 4 q + r][k0 + 4 j + c] -> the 4 MFMAs give one 16-byte store per r.
// The first version gave each block a 16-column strip over ALL rows: 38 blocks, each touching
// every page of the weight 64 bytes at a time -- 11-22 us per call (profiles/r01l), 48 calls a
// step.  Here ~300 blocks each read a compact [rpb x 256 B] piece with every load in flight at
// once; the row slices meet in a second, tiny launch that sums the ns partials in index order
// (deterministic).  A single-launch "last block reduces" variant behind an agent-scope acq_rel counter
// was measured at 30-85 us: every __threadfence writes back / invalidates the XCD's whole L2.
constexpr int BI_COLS = 64;       // weight columns per block
constexpr int BI_ROUND = 64;      // weight rows per staging round (4 waves x 4 steps x 4 rows)
constexpr int BI_LD = 68;         // LDS row stride of the g stage

template <int MB>
__device__ __forceinline__ void skinny_bwd_input_body(const int bx /* block index within the problem */,
                                                      const float* __restrict__ gy, const float* __restrict__ z,
                                                      const float* __restrict__ W, float* __restrict__ gx,
                                                      float* __restrict__ part, int M, int N, int K, int act, int KT,
                                                      int NS, int rpb) {
  // g stage [16 MB rows][BI_LD], then the wave reduction: up to 4 row blocks all three partner waves deposit at once,
  // beyond that (MB 5..8: 65-128 rows) one wave at a time through a third of the space
  constexpr int SM_RED = (MB <= 4 ? 4 : 1) * MB * 16 * 64, SM_G = MB * 16 * BI_LD;
  __shared__ __attribute__((aligned(16))) float sm[SM_RED > SM_G ? SM_RED : SM_G];
  const int kt = bx % KT, ns = bx / KT;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, q = lane >> 4;
  const int kcol = kt * BI_COLS + 4 * j;
  const bool kok = kcol < K;                                               // K % 4 == 0
  const int n_beg = ns * rpb, n_end = min(n_beg + rpb, N);
  f32x4 acc[MB][4];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[mb][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Up to four rounds (a row slice of <= 256 weight rows: every split product of the model), plain aligned operands, no
  // activation of its own (the usual case since Swish' travels downstream): EVERY round's weights and g tile are requested
  // up front -- a block is alone on its CU and each round used to wait out its own round trip (~2 us of W from HBM in
  // front of 0.45 us of MFMAs: 96 x 5400 -> 600 took 20.5 us) -- then the rounds only stage, meet and multiply.
  constexpr int RMAX = 4;
  const int rounds = (n_end - n_beg + BI_ROUND - 1) / BI_ROUND;
  const bool upfront = act == 0 && rounds <= RMAX && (((uintptr_t)gy) & 15) == 0;
  if (upfront) {
    float4 wA[RMAX][4], gA[RMAX][MB];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int nb = n_beg + min(r, rounds - 1) * BI_ROUND;              // (surplus rounds repeat the last one's addresses; never used)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int row = nb + 16 * s + 4 * wave + q;
        const bool ok = row < n_end && kok;
        wA[r][s] = *reinterpret_cast<const float4*>(W + (size_t)(ok ? row : 0) * K + (ok ? kcol : 0));
      }
#pragma unroll
      for (int u = 0; u < MB; ++u) {
        const int unit = u * 256 + (int)threadIdx.x, m = unit >> 4, n = nb + 4 * (unit & 15);
        const bool ok = m < M && n < n_end;
        gA[r][u] = *reinterpret_cast<const float4*>(gy + (ok ? (size_t)m * N + n : 0));
      }
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      if (r >= rounds) break;                                              // block-uniform
      const int nb = n_beg + r * BI_ROUND;
      if (r) __syncthreads();                                              // readers of the previous round
#pragma unroll
      for (int u = 0; u < MB; ++u) {
        const int unit = u * 256 + (int)threadIdx.x, m = unit >> 4, n = nb + 4 * (unit & 15);
        *reinterpret_cast<float4*>(sm + m * BI_LD + 4 * (unit & 15)) = (m < M && n < n_end) ? gA[r][u] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool ok = nb + 16 * s + 4 * wave + q < n_end && kok;
        const float4 w4 = ok ? wA[r][s] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const float a = sm[(mb * 16 + j) * BI_LD + 16 * s + 4 * wave + q];
          acc[mb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w4.x, acc[mb][0], 0, 0, 0);
          acc[mb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w4.y, acc[mb][1], 0, 0, 0);
          acc[mb][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w4.z, acc[mb][2], 0, 0, 0);
          acc[mb][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w4.w, acc[mb][3], 0, 0, 0);
        }
      }
    }
  }
  for (int nb = upfront ? n_end : n_beg; nb < n_end; nb += BI_ROUND) {
    float4 wv[4];                                                          // weights first: the long latency
    bool wok[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {                                          // unconditional (clamped) requests, zeroed below:
      const int row = nb + 16 * s + 4 * wave + q;                          // a guarded load is a branch and ten instructions
      wok[s] = row < n_end && kok;
      wv[s] = *reinterpret_cast<const float4*>(W + (size_t)(wok[s] ? row : 0) * K + (wok[s] ? kcol : 0));
    }
    float g[MB * 4], zz[MB * 4];
    // Plain operands, 16-byte aligned: the [16 MB x 64] tile of g as MB float4 per thread (row = unit / 16, 4 columns),
    // requested unconditionally -- 6 requests for the 24 + 24 guarded dword loads of a 96-row round, whose address
    // arithmetic alone was ~500 instructions per wave and round (a round took 4 us for 1.5 us of MFMAs)
    const bool vec = (((uintptr_t)gy | (uintptr_t)(act ? z : gy)) & 15) == 0;
    float4 g4[MB], z4[MB];
    if (vec) {
#pragma unroll
      for (int u = 0; u < MB; ++u) {
        const int unit = u * 256 + (int)threadIdx.x, m = unit >> 4, n = nb + 4 * (unit & 15);
        const bool ok = m < M && n < n_end;                                // N % 4 == 0, rounds of 64: a float4 is all in or all out
        const size_t at = ok ? (size_t)m * N + n : 0;
        g4[u] = *reinterpret_cast<const float4*>(gy + at);
        if (act) z4[u] = *reinterpret_cast<const float4*>(z + at);         // wave-uniform
      }
    } else {
#pragma unroll
      for (int t = 0; t < MB * 4; ++t) {                                   // g[:, nb .. nb+63], row m = 4t + wave
        const int m = 4 * t + wave, n = nb + lane;
        const bool ok = m < M && n < n_end;
        g[t] = ok ? gy[(size_t)m * N + n] : 0.f;
        zz[t] = (ok && act) ? z[(size_t)m * N + n] : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (!wok[s]) wv[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nb != n_beg) __syncthreads();                                      // readers of the previous round
    if (vec) {
#pragma unroll
      for (int u = 0; u < MB; ++u) {
        const int unit = u * 256 + (int)threadIdx.x, m = unit >> 4, n = nb + 4 * (unit & 15);
        float4 v = g4[u];
        if (act) { v.x *= act_bwd(z4[u].x, act); v.y *= act_bwd(z4[u].y, act); v.z *= act_bwd(z4[u].z, act); v.w *= act_bwd(z4[u].w, act); }
        if (!(m < M && n < n_end)) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(sm + m * BI_LD + 4 * (unit & 15)) = v;
      }
    } else {
#pragma unroll
      for (int t = 0; t < MB * 4; ++t) sm[(4 * t + wave) * BI_LD + lane] = act ? g[t] * act_bwd(zz[t], act) : g[t];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const float a = sm[(mb * 16 + j) * BI_LD + 16 * s + 4 * wave + q];
        acc[mb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wv[s].x, acc[mb][0], 0, 0, 0);
        acc[mb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wv[s].y, acc[mb][1], 0, 0, 0);
        acc[mb][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wv[s].z, acc[mb][2], 0, 0, 0);
        acc[mb][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wv[s].w, acc[mb][3], 0, 0, 0);
      }
  }
  __syncthreads();
  float4 tot[MB][4];                                                       // [mb][r] = gx[16 mb + 4 q + r][kcol .. +3]
  // Up to 4 row blocks: every wave deposits its partial sums and wave w FINISHES row block w (sums the four partials in
  // wave order -- the same sum as ever -- and stores) instead of wave 0 finishing all of them alone: 192 LDS reads and
  // adds per lane at the end of every launch at 64 rows (the tile kernels' tail of rounds 1-5, see tile_bwd_input_k).
  constexpr bool SHARED_FINISH = MB <= 4;
  if constexpr (MB <= 4) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[(((wave * MB + mb) * 4 + r) * 4 + c) * 64 + lane] = acc[mb][c][r];
    __syncthreads();
    if (wave >= MB) return;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      if (mb != wave) continue;                                            // wave-uniform
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t[c] = sm[(((0 * MB + mb) * 4 + r) * 4 + c) * 64 + lane];
#pragma unroll
          for (int w = 1; w < 4; ++w) t[c] += sm[(((w * MB + mb) * 4 + r) * 4 + c) * 64 + lane];
        }
        tot[mb][r] = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
  } else {
    for (int w = 1; w < 4; ++w) {                                          // waves 1, 2, 3 in turn (same summation order)
      if (wave == w) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[(((mb * 4 + r) * 4 + c) * 64) + lane] = acc[mb][c][r];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mb][c][r] += sm[(((mb * 4 + r) * 4 + c) * 64) + lane];
      }
      __syncthreads();
    }
    if (wave != 0) return;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[mb][r] = make_float4(acc[mb][0][r], acc[mb][1][r], acc[mb][2][r], acc[mb][3][r]);
  }
  if (NS > 1 || (part && !gx)) {    // row slices meet in the next launch on the stream (a reduce kernel)
    float* mine = part + ((size_t)ns * M) * K;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      if (SHARED_FINISH && mb != wave) continue;                           // wave-uniform: this wave's row block
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mb * 16 + 4 * q + r;
        if (m < M && kok) *reinterpret_cast<float4*>(mine + (size_t)m * K + kcol) = tot[mb][r];
      }
    }
    return;
  }
  if (!kok) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (SHARED_FINISH && mb != wave) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mb * 16 + 4 * q + r;
      if (m < M) *reinterpret_cast<float4*>(gx + (size_t)m * K + kcol) = tot[mb][r];
    }
  }
}

template <int MB>
__global__ __launch_bounds__(256) void skinny_bwd_input_k(const float* __restrict__ gy, const float* __restrict__ z,
                                                          const float* __restrict__ W, float* __restrict__ gx,
                                                          float* __restrict__ part, int M, int N, int K, int act, int KT,
                                                          int NS, int rpb) {
  skinny_bwd_input_body<MB>(blockIdx.x, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb);
}

// Two products of one shape in one launch (blockIdx.y picks the problem): the two heads of an MLP pair (mu / sigma:
// cgvae.py:366-371) are independent of each other, as separate launches they are two more dependent links in the chain.
constexpr int BI_MULTI_MAX = 4;
struct BiPair {
  const float* gy[BI_MULTI_MAX]; const float* z[BI_MULTI_MAX]; const float* W[BI_MULTI_MAX];
  float* gx[BI_MULTI_MAX]; float* part[BI_MULTI_MAX];
  int act[BI_MULTI_MAX];
};
template <int MB>
__global__ __launch_bounds__(256) void skinny_bwd_input_pair_k(BiPair p, int M, int N, int K, int KT, int NS, int rpb) {
  const int y = blockIdx.y;
  skinny_bwd_input_body<MB>(blockIdx.x, p.gy[y], p.z[y], p.W[y], p.gx[y], p.part[y], M, N, K, p.act[y], KT, NS, rpb);
}

// gx[i] = sum_p part[p][i] (i over M*K/4 float4s), p ascending: deterministic.  4 lanes share one output
// float4 and take every 4th slice, then combine by two xor-shuffles.  The body of the three reduce kernels: thread
// t = 4 i + sub adds its slices (stride4 float4 apart) to `acc`; the sum is complete in every lane of the four.
__device__ __forceinline__ float4 bwd_input_reduce_slices(const float* __restrict__ part, int i, int sub, int n4, int NS,
                                                          size_t stride4, float4 acc) {
  if (i < n4) {
    const float4* p4 = reinterpret_cast<const float4*>(part) + i;
    // a lane's 5 - 8 slices are loaded together (slice index clamped, the surplus zeroed afterwards): the runtime-bounded
    // loop left a remainder of single loads, each a memory round trip of this 4 us launch; summation order unchanged
    constexpr int RB = 8;
    for (int p0 = sub; p0 < NS; p0 += 4 * RB) {
      float4 v[RB];
#pragma unroll
      for (int u = 0; u < RB; ++u) v[u] = p4[(size_t)min(p0 + 4 * u, NS - 1) * stride4];
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        const bool ok = p0 + 4 * u < NS;
        acc.x += ok ? v[u].x : 0.f; acc.y += ok ? v[u].y : 0.f; acc.z += ok ? v[u].z : 0.f; acc.w += ok ? v[u].w : 0.f;
      }
    }
  }
#pragma unroll
  for (int d = 1; d <= 2; d <<= 1) {
    acc.x += __shfl_xor(acc.x, d); acc.y += __shfl_xor(acc.y, d);
    acc.z += __shfl_xor(acc.z, d); acc.w += __shfl_xor(acc.w, d);
  }
  return acc;
}

// base: added to the sum (the second gradient of a forked input).  slice_stride4: float4 between consecutive slices
// when they are not packed (0: n4).
// z_out: the stored sum is multiplied by act_out'(z_out) -- the gradient of the pre-activation of the layer that produced
// this product's input (see OutAct in tile_gemm.hip: that layer's own backward then runs without an activation).
__global__ __launch_bounds__(256) void skinny_bwd_input_reduce_k(const float* __restrict__ part, float* __restrict__ gx,
                                                                 int n4, int NS, const float* __restrict__ base = nullptr,
                                                                 long long slice_stride4 = 0,
                                                                 const float* __restrict__ z_out = nullptr, int act_out = 0) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int i = t >> 2, sub = t & 3;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4 && base && sub == 0) acc = reinterpret_cast<const float4*>(base)[i];
  acc = bwd_input_reduce_slices(part, i, sub, n4, NS, slice_stride4 ? (size_t)slice_stride4 : (size_t)n4, acc);
  if (i < n4 && sub == 0) {
    if (z_out) {
      const float4 z4 = reinterpret_cast<const float4*>(z_out)[i];
      acc.x *= act_bwd(z4.x, act_out); acc.y *= act_bwd(z4.y, act_out); acc.z *= act_bwd(z4.z, act_out); acc.w *= act_bwd(z4.w, act_out);
    }
    reinterpret_cast<float4*>(gx)[i] = acc;
  }
}

// the reduction launch of up to four outputs: blockIdx.y picks (partials, output); NS slices each
struct ReduceMulti { const float* part[BI_MULTI_MAX]; float* gx[BI_MULTI_MAX]; };
__global__ __launch_bounds__(256) void skinny_bwd_input_reduce_multi_k(ReduceMulti rm, int n4, int NS) {
  const float* __restrict__ part = rm.part[blockIdx.y];
  float* __restrict__ gx = rm.gx[blockIdx.y];
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int i = t >> 2, sub = t & 3;
  const float4 acc = bwd_input_reduce_slices(part, i, sub, n4, NS, (size_t)n4, make_float4(0.f, 0.f, 0.f, 0.f));
  if (i < n4 && sub == 0) reinterpret_cast<float4*>(gx)[i] = acc;
}

// the reduction launch of a pair with two outputs: blockIdx.y picks (partials, output)
__global__ __launch_bounds__(256) void skinny_bwd_input_reduce_pair_k(const float* __restrict__ part0, const float* __restrict__ part1,
                                                                      float* __restrict__ gx0, float* __restrict__ gx1, int n4, int NS) {
  const float* part = blockIdx.y ? part1 : part0;
  float* gx = blockIdx.y ? gx1 : gx0;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int i = t >> 2, sub = t & 3;
  const float4 acc = bwd_input_reduce_slices(part, i, sub, n4, NS, (size_t)n4, make_float4(0.f, 0.f, 0.f, 0.f));
  if (i < n4 && sub == 0) reinterpret_cast<float4*>(gx)[i] = acc;
}

// row slicing of one bwd_input problem: ~320 blocks when a workspace is available
static inline void bwd_input_plan(int N, int K, bool split, int* KT, int* NS, int* rpb) {
  *KT = (K + BI_COLS - 1) / BI_COLS;
  if (!split) { *NS = 1; *rpb = N; return; }
#ifndef CGV_BI_WANT
#define CGV_BI_WANT 250   /* one round of blocks on 256 CUs: 96 x 5400 x 600 21.9 against 31.7 us at 320 (tools/bwd_input_bench.py), 64 rows 15.4 / 17.1 */
#endif
  const int want = (CGV_BI_WANT + *KT - 1) / *KT;
  int r = (N + want - 1) / want;
  r = (r + 15) / 16 * 16;
  if (r < 32) r = 32;
  *rpb = r;
  *NS = (N + r - 1) / r;
}

template <int MB>
static void launch_fwd(dim3 grid, int waves, hipStream_t st, const float* x, const float* W, const float* bias, float* y,
                       float* z, int M, int N, int K, int act) {
  if (waves >= 16) hipLaunchKernelGGL((skinny_fwd_k<MB, 16>), grid, dim3(1024), 0, st, x, W, bias, y, z, M, N, K, act);
  else if (waves >= 8) hipLaunchKernelGGL((skinny_fwd_k<MB, 8>), grid, dim3(512), 0, st, x, W, bias, y, z, M, N, K, act);
  else hipLaunchKernelGGL((skinny_fwd_k<MB, 4>), grid, dim3(256), 0, st, x, W, bias, y, z, M, N, K, act);
}
template <int MB>
static void launch_bwd_input(hipStream_t st, const float* gy, const float* z, const float* W, float* gx, float* part,
                             int M, int N, int K, int act, int KT, int NS, int rpb, const float* add, const float* z_out,
                             int act_out) {
  hipLaunchKernelGGL((skinny_bwd_input_k<MB>), dim3(KT * NS), dim3(256), 0, st, gy, z, W, gx, part, M, N, K, act, KT, NS,
                     rpb);
  if (NS > 1) {
    const int n4 = M * K / 4;
    hipLaunchKernelGGL(skinny_bwd_input_reduce_k, dim3((4 * n4 + 255) / 256), dim3(256), 0, st, part, gx, n4, NS, add, 0ll,
                       z_out, act_out);
  }
}
// one product (+ its reduction launch when NS > 1, which carries add / z_out): the kernel of M's row blocks
static void bwd_input_dispatch(hipStream_t st, const float* gy, const float* z, const float* W, float* gx, float* part, int M,
                               int N, int K, int act, int KT, int NS, int rpb, const float* add = nullptr,
                               const float* z_out = nullptr, int act_out = 0) {
  switch ((M + 15) / 16) {
    case 1: launch_bwd_input<1>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
    case 2: launch_bwd_input<2>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
    case 3: launch_bwd_input<3>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
    case 4: launch_bwd_input<4>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
    case 5:
    case 6: launch_bwd_input<6>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
    default: launch_bwd_input<8>(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out); break;
  }
}
// the products of a BiPair record (M <= 64): grid.y picks the problem
static void bwd_input_pair_dispatch(hipStream_t st, const BiPair& p, dim3 grid, int M, int N, int K, int KT, int NS, int rpb) {
  switch ((M + 15) / 16) {
    case 1: hipLaunchKernelGGL((skinny_bwd_input_pair_k<1>), grid, dim3(256), 0, st, p, M, N, K, KT, NS, rpb); break;
    case 2: hipLaunchKernelGGL((skinny_bwd_input_pair_k<2>), grid, dim3(256), 0, st, p, M, N, K, KT, NS, rpb); break;
    case 3: hipLaunchKernelGGL((skinny_bwd_input_pair_k<3>), grid, dim3(256), 0, st, p, M, N, K, KT, NS, rpb); break;
    default: hipLaunchKernelGGL((skinny_bwd_input_pair_k<4>), grid, dim3(256), 0, st, p, M, N, K, KT, NS, rpb); break;
  }
}

// ------------------------------------------------------------------ Dense backward prologue (any M)
// g = gy * act'(z) (stored when g_out != NULL) and gb[n] (+)= sum_m g[m, n] in one pass: replaces the
// sigmoid / mul / add tensor ops and the separate column-sum reduction of the library-GEMM path
// (encoder Dense layers, M = atoms).  Block = 64 columns x 16 row groups, fixed summation order.
__global__ __launch_bounds__(1024) void dense_grad_prepare_k(const float* __restrict__ gy, const float* __restrict__ z,
                                                             float* __restrict__ g_out, float* __restrict__ gb, int M,
                                                             int N, int act, int accumulate) {
  __shared__ float4 red[64][16];
  const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;          // 16 float4 column groups x 64 row groups
  const int n = blockIdx.x * 64 + 4 * c4;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n < N) {                                                     // N % 4 == 0
#pragma unroll 8
    for (int m = rg; m < M; m += 64) {
      const size_t at = (size_t)m * N + n;
      float4 g = *reinterpret_cast<const float4*>(gy + at);
      if (act) {
        const float4 zz = *reinterpret_cast<const float4*>(z + at);
        g.x *= act_bwd(zz.x, act); g.y *= act_bwd(zz.y, act); g.z *= act_bwd(zz.z, act); g.w *= act_bwd(zz.w, act);
        if (g_out) *reinterpret_cast<float4*>(g_out + at) = g;
      }
      sum.x += g.x; sum.y += g.y; sum.z += g.z; sum.w += g.w;
    }
  }
  red[rg][c4] = sum;
  __syncthreads();
  if (rg < 4 && n < N && gb) {                                     // thread (rg, c4) finishes column n + rg
    float t = 0.f;
#pragma unroll 16
    for (int k = 0; k < 64; ++k) t += reinterpret_cast<const float*>(&red[k][c4])[rg];
    gb[n + rg] = accumulate ? gb[n + rg] + t : t;
  }
}
}  // namespace cgv

extern "C" {

int cgv_skinny_max_rows(void) { return 64; }

int cgv_skinny_supported(int M, int N, int K) {
  return M >= 1 && M <= 64 && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0;
}

/* the forward alone takes any row count: a thread block owns 16 - 64 rows (blockIdx.y), cgv_skinny_linear_fwd picks how many */
int cgv_skinny_fwd_supported(int M, int N, int K) {
  return M >= 1 && (M + 15) / 16 <= 65535 && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0;
}

int cgv_skinny_linear_fwd(const float* x, const float* W, const float* bias, float* y, float* z, int M, int N, int K,
                          int act, void* stream) {
  CGV_REQUIRE(x && W && y, "null pointer");
  CGV_REQUIRE(act >= 0 && act <= cgv::CGV_ACT_MAX, "act must be 0 (identity), 1 (swish), 2 (tanh), 3 (relu), 4 / 5 (c + exp(z/2))");
  CGV_REQUIRE(cgv_skinny_fwd_supported(M, N, K), "unsupported shape (need N % 4 == 0, K % 4 == 0, at most 65535 row blocks)");
  CGV_REQUIRE(((((uintptr_t)x | (uintptr_t)W | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)z)) & 15) == 0,
              "operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((N + 15) / 16);
  // row blocks (of 16 rows) per thread block: all of them, or -- when that leaves the chip mostly idle -- fewer, in more blocks
  const int row_blocks = (M + 15) / 16;
  // (64 bead rows, 2000-atom config: 600 x 600 8.98 -> 4.65 us, 1800 x 600 9.43 -> 6.02, 600 x 1200 13.3 -> 6.1 with one
  //  row block per thread block; 5400 x 600, 338 column blocks: 14.2 -> 16.0, left alone)
  int mb = cgv::option(CGV_OPT_SKINNY_ROWS);
  if (mb <= 0 || mb > 4) mb = (long)grid.x * row_blocks <= 512 ? 1 : 4;
  if (mb > row_blocks) mb = row_blocks;
  grid.y = (row_blocks + mb - 1) / mb;
  // enough waves to fill the chip: few blocks -> split K over more waves per block
  const long blocks = (long)grid.x * grid.y;
  const int waves = blocks >= 256 ? 4 : (blocks >= 96 ? 8 : 16);
  switch (mb) {
    case 1: cgv::launch_fwd<1>(grid, waves, st, x, W, bias, y, z, M, N, K, act); break;
    case 2: cgv::launch_fwd<2>(grid, waves, st, x, W, bias, y, z, M, N, K, act); break;
    case 3: cgv::launch_fwd<3>(grid, waves, st, x, W, bias, y, z, M, N, K, act); break;
    default: cgv::launch_fwd<4>(grid, waves, st, x, W, bias, y, z, M, N, K, act); break;
  }
  return cgv::check_launch("cgv_skinny_linear_fwd");
}

/* bwd_input alone also takes 65..128 rows (row blocks 5..8): the weight rows are split over ~300 blocks whatever M is,
 * where the tile kernel has one block per 16 x 64 outputs -- 60 blocks for 96 bead rows (dipeptide batch). */
int cgv_skinny_bwd_input_supported(int M, int N, int K) {
  return M >= 1 && M <= 128 && N >= 4 && K >= 4 && (N % 4) == 0 && (K % 4) == 0;
}

size_t cgv_skinny_bwd_input_workspace_bytes(int M, int N, int K) {
  if (!cgv_skinny_bwd_input_supported(M, N, K)) return 0;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, true, &KT, &NS, &rpb);
  return NS > 1 ? sizeof(float) * (size_t)NS * M * K : 0;
}

int cgv_skinny_linear_bwd_input(const float* gy, const float* z, const float* W, float* gx, int M, int N, int K, int act,
                                void* ws, size_t ws_bytes, void* stream) {
  CGV_REQUIRE(gy && W && gx, "null pointer");
  CGV_REQUIRE(act == 0 || (act >= 1 && act <= cgv::CGV_ACT_MAX && z), "act != 0 needs the saved pre-activation z");
  CGV_REQUIRE(cgv_skinny_bwd_input_supported(M, N, K), "unsupported shape (need M <= 128, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(((((uintptr_t)gx) | ((uintptr_t)W) | ((uintptr_t)ws)) & 15) == 0, "gx, W, ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, ws != nullptr, &KT, &NS, &rpb);
  if (NS > 1) CGV_REQUIRE(ws_bytes >= cgv_skinny_bwd_input_workspace_bytes(M, N, K), "workspace too small");
  float* part = reinterpret_cast<float*>(ws);
  cgv::bwd_input_dispatch(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb);
  return cgv::check_launch("cgv_skinny_linear_bwd_input");
}

/* gx = add + (gy * act'(z)) W: the accumulation of a second gradient of the layer's input (the input also feeds the
 * message kernel / the residual: blocks.py) rides in the reduction launch of the row-split product.  Only where that
 * launch exists (more than one row slice): CGV_E_UNSUPPORTED otherwise -- the caller then adds separately. */
int cgv_skinny_linear_bwd_input_add(const float* gy, const float* z, const float* W, const float* add, float* gx, int M, int N,
                                    int K, int act, void* ws, size_t ws_bytes, void* stream) {
  CGV_REQUIRE(gy && W && gx && add && ws, "null pointer");
  CGV_REQUIRE(act == 0 || (act >= 1 && act <= cgv::CGV_ACT_MAX && z), "act != 0 needs the saved pre-activation z");
  CGV_REQUIRE(cgv_skinny_bwd_input_supported(M, N, K), "unsupported shape (need M <= 128, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(((((uintptr_t)gx) | ((uintptr_t)W) | ((uintptr_t)ws) | ((uintptr_t)add)) & 15) == 0, "gx, W, ws, add must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, true, &KT, &NS, &rpb);
  if (NS <= 1) { cgv::set_error("cgv_skinny_linear_bwd_input_add: one row slice, no reduction launch to carry the add"); return CGV_E_UNSUPPORTED; }
  CGV_REQUIRE(ws_bytes >= cgv_skinny_bwd_input_workspace_bytes(M, N, K), "workspace too small");
  float* part = reinterpret_cast<float*>(ws);
  cgv::bwd_input_dispatch(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add);
  return cgv::check_launch("cgv_skinny_linear_bwd_input_add");
}

/* gx = (add + (gy * act'(z)) W) * act_out'(z_out) (add may be NULL): the reduction launch of the row-split product also
 * multiplies by the activation derivative of the layer that produced this layer's input (cgv_tile_linear_bwd_input_out for
 * few rows x very long reductions).  CGV_E_UNSUPPORTED when the product has one row slice only. */
int cgv_skinny_linear_bwd_input_out(const float* gy, const float* z, const float* W, const float* add, float* gx, int M, int N,
                                    int K, int act, const float* z_out, int act_out, void* ws, size_t ws_bytes, void* stream) {
  CGV_REQUIRE(gy && W && gx && z_out && ws, "null pointer");
  CGV_REQUIRE(act == 0 || (act >= 1 && act <= cgv::CGV_ACT_MAX && z), "act != 0 needs the saved pre-activation z");
  CGV_REQUIRE(act_out >= 1 && act_out <= cgv::CGV_ACT_MAX, "act_out must name an activation");
  CGV_REQUIRE(cgv_skinny_bwd_input_supported(M, N, K), "unsupported shape (need M <= 128, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(((((uintptr_t)gx) | ((uintptr_t)W) | ((uintptr_t)ws) | ((uintptr_t)add) | ((uintptr_t)z_out)) & 15) == 0,
              "gx, W, ws, add, z_out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, true, &KT, &NS, &rpb);
  if (NS <= 1) { cgv::set_error("cgv_skinny_linear_bwd_input_out: one row slice, no reduction launch to carry the epilogue"); return CGV_E_UNSUPPORTED; }
  CGV_REQUIRE(ws_bytes >= cgv_skinny_bwd_input_workspace_bytes(M, N, K), "workspace too small");
  float* part = reinterpret_cast<float*>(ws);
  cgv::bwd_input_dispatch(st, gy, z, W, gx, part, M, N, K, act, KT, NS, rpb, add, z_out, act_out);
  return cgv::check_launch("cgv_skinny_linear_bwd_input_out");
}

/* Two backward-input products of ONE shape in one launch pair (+ one reduction launch): gx_j = (gy_j * act_j'(z_j)) W_j for
 * j = 0, 1 -- or, with gx1 == NULL, their SUM in gx0 (two layers that read the same input: the gradient accumulation is
 * part of the reduction).  M <= 64 rows.  ws: 2 x cgv_skinny_bwd_input_workspace_bytes(M, N, K). */
int cgv_pair_linear_bwd_input(const float* gy0, const float* gy1, const float* z0, const float* z1, const float* W0,
                              const float* W1, int act0, int act1, float* gx0, float* gx1, int M, int N, int K, void* ws,
                              size_t ws_bytes, void* stream) {
  CGV_REQUIRE(gy0 && gy1 && W0 && W1 && gx0 && ws, "null pointer");
  CGV_REQUIRE((act0 == 0 || (act0 >= 1 && act0 <= cgv::CGV_ACT_MAX && z0)) && (act1 == 0 || (act1 >= 1 && act1 <= cgv::CGV_ACT_MAX && z1)),
              "act != 0 needs the saved pre-activation z");
  CGV_REQUIRE(cgv_skinny_bwd_input_supported(M, N, K) && M <= 64, "unsupported shape (need M <= 64, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE(((((uintptr_t)gx0) | ((uintptr_t)gx1) | ((uintptr_t)W0) | ((uintptr_t)W1) | ((uintptr_t)ws)) & 15) == 0, "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, true, &KT, &NS, &rpb);
  const size_t one = sizeof(float) * (size_t)NS * M * K;
  CGV_REQUIRE(ws_bytes >= 2 * one, "workspace too small");
  float* part0 = reinterpret_cast<float*>(ws);
  float* part1 = part0 + (size_t)NS * M * K;
  // partial products always go through the workspace (also at NS == 1): the reduction launch writes / sums the outputs
  cgv::BiPair p{{gy0, gy1}, {z0, z1}, {W0, W1}, {nullptr, nullptr}, {part0, part1}, {act0, act1}};
  const dim3 grid(KT * NS, 2);
  cgv::bwd_input_pair_dispatch(st, p, grid, M, N, K, KT, NS, rpb);
  const int n4 = M * K / 4;
  if (gx1)
    hipLaunchKernelGGL(cgv::skinny_bwd_input_reduce_pair_k, dim3((4 * n4 + 255) / 256, 2), dim3(256), 0, st, part0, part1, gx0,
                       gx1, n4, NS);
  else        // one output: the 2 NS slices of both problems are adjacent in the workspace
    hipLaunchKernelGGL(cgv::skinny_bwd_input_reduce_k, dim3((4 * n4 + 255) / 256), dim3(256), 0, st, part0, gx0, n4, 2 * NS);
  return cgv::check_launch("cgv_pair_linear_bwd_input");
}

/* Up to four backward-input products of ONE shape in one launch + one reduction launch: gx_j = (gy_j * act_j'(z_j)) W_j.
 * ``group`` = 1: one output per problem (gx[0 .. n-1]); ``group`` = 2: problems 2o and 2o + 1 read the same input and
 * their products are SUMMED into gx[o] (n / 2 outputs) -- the accumulation is part of the reduction.  M <= 64 rows.
 * ws: n x cgv_skinny_bwd_input_workspace_bytes(M, N, K) (at least n x 4 M K bytes). */
int cgv_multi_linear_bwd_input(int n, int group, const float* const* gy, const float* const* z, const float* const* W,
                               const int* act, float* const* gx, int M, int N, int K, void* ws, size_t ws_bytes, void* stream) {
  CGV_REQUIRE(n >= 1 && n <= cgv::BI_MULTI_MAX && (group == 1 || group == 2) && n % group == 0, "1 .. 4 problems, group 1 or 2");
  CGV_REQUIRE(gy && W && act && gx && ws, "null pointer");
  CGV_REQUIRE(cgv_skinny_bwd_input_supported(M, N, K) && M <= 64, "unsupported shape (need M <= 64, N % 4 == 0, K % 4 == 0)");
  CGV_REQUIRE((((uintptr_t)ws) & 15) == 0, "16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  int KT, NS, rpb;
  cgv::bwd_input_plan(N, K, true, &KT, &NS, &rpb);
  const size_t one = (size_t)NS * M * K;
  CGV_REQUIRE(ws_bytes >= sizeof(float) * one * n, "workspace too small");
  cgv::BiPair p{};
  for (int j = 0; j < n; ++j) {
    CGV_REQUIRE(gy[j] && W[j] && ((((uintptr_t)W[j]) & 15) == 0), "null / unaligned operand");
    CGV_REQUIRE(act[j] == 0 || (act[j] >= 1 && act[j] <= cgv::CGV_ACT_MAX && z && z[j]), "act != 0 needs the saved pre-activation z");
    p.gy[j] = gy[j]; p.z[j] = z ? z[j] : nullptr; p.W[j] = W[j]; p.gx[j] = nullptr;
    p.part[j] = reinterpret_cast<float*>(ws) + one * j;      // partial products always go through the workspace
    p.act[j] = act[j];
  }
  const dim3 grid(KT * NS, n);
  cgv::bwd_input_pair_dispatch(st, p, grid, M, N, K, KT, NS, rpb);
  const int n4 = M * K / 4, outs = n / group;
  cgv::ReduceMulti rm{};
  for (int o = 0; o < outs; ++o) {
    CGV_REQUIRE(gx[o] && ((((uintptr_t)gx[o]) & 15) == 0), "null / unaligned output");
    rm.part[o] = reinterpret_cast<float*>(ws) + one * group * o;       // the slices of a group's problems are adjacent
    rm.gx[o] = gx[o];
  }
  hipLaunchKernelGGL(cgv::skinny_bwd_input_reduce_multi_k, dim3((4 * n4 + 255) / 256, outs), dim3(256), 0, st, rm, n4, group * NS);
  return cgv::check_launch("cgv_multi_linear_bwd_input");
}

int cgv_dense_grad_prepare(const float* gy, const float* z, float* g_out, float* gb, int M, int N, int act, int accumulate,
                           void* stream) {
  CGV_REQUIRE(gy && M >= 0 && N > 0, "bad argument");
  CGV_REQUIRE(act == 0 || (act >= 1 && act <= cgv::CGV_ACT_MAX && z), "act != 0 needs the saved pre-activation z");
  CGV_REQUIRE(gb || (act && g_out), "nothing to compute");
  CGV_REQUIRE((N % 4) == 0 && ((((uintptr_t)gy | (uintptr_t)z | (uintptr_t)g_out)) & 15) == 0, "need N % 4 == 0, 16-byte aligned");
  if (M == 0 && !gb) return 0;
  hipLaunchKernelGGL(cgv::dense_grad_prepare_k, dim3((N + 63) / 64), dim3(1024), 0, (hipStream_t)stream, gy, z, g_out, gb, M,
                     N, act, accumulate);
  return cgv::check_launch("cgv_dense_grad_prepare");
}

}  // extern "C"
