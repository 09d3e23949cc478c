// K14 ensemble check: reference-free quality of generated ensembles (see include/cgvae_hip.h).
//
// Two questions per frame of K generated samples, answered for a whole chunk of frames in one launch:
//   validity   does sample k have exactly the bond graph of the topology?  counts [B,K,4]
//   diversity  how far apart are samples k and l?                          pair_sums [B,K,K,2]  (sum of squared distances)
// No [n,n] or [K,K,n] tensor exists.  One kernel, one wave per block, grid (x, frame); x selects the block's role:
//
//   x < ktp                 PAIR role, ktp = kt (kt + 1) / 2 tile pairs (KI <= LI) of kt = ceil(K / 8) sample tiles.
//                           The 64 lanes are the 8 x 8 sample pairs (k, l) of the tile pair.  32 atoms of the 8 + 8 samples
//                           are staged in LDS per step (every coordinate is read from L2 once per tile pair, i.e. kt times
//                           instead of K times); lane (k, l) walks the staged atoms in order and adds its pair's squared
//                           distance in fp64.  One lane owns one sum and adds in atom order: no reduction, no atomics, the
//                           same bits on every run.  Tiles with KI < LI write [k,l] and [l,k]; diagonal tiles write k <= l.
//                           Sample rows are padded to 97 floats: the 8 distinct addresses of a read fall on 8 banks.
//   ktp <= x < ktp + K      BOND role, sample k = x - ktp: the lanes stride over the frame's bond list and count the
//                           topology bonds that are present (H_all, H_heavy) and the heavy-heavy bonds (Eb_heavy).
//   x >= ktp + K            TILE role, as K12: (sample k, tile pair I <= J of 64-atom tiles); the wave keeps 64 row atoms
//                           in registers, stages 64 column atoms in LDS and counts the pairs j > i with
//                           s <= thr_sq[cls_i][cls_j] (P_all, P_heavy).
//
// Validity needs no membership lookup "is (i, j) in the bond list": with unique pairs i < j the present topology bonds
// are a subset of the inferred bonds, so  missing = Eb - H  and  extra = P - H.  The BOND role adds (Eb - H, -H), the TILE
// role adds P, with integer vector atomics into the zeroed counts: exact in any order (a count may pass through a
// negative value while the launch runs).  Without a topology (bond_ptr == NULL) only the PAIR role is launched.
//
// The PAIR blocks come first in x: they are the longest (n / 32 serial steps), the dispatcher starts them first.
// Bound: launch latency for 22 .. 166 atom frames; L2 / LDS delivery of the PAIR role for K >= 64.
#include "cgv_common.h"
#include "sq_dist.h"

namespace cgv {

constexpr int EC_MAX_SAMPLES = 1024;             // K of one launch: pair_sums holds K * K * 2 doubles per frame
constexpr int EC_KT = 8;                         // samples per side of a PAIR tile
constexpr int EC_CHUNK = 32;                     // atoms staged per step of the PAIR role
constexpr int EC_ROW = 3 * EC_CHUNK + 1;         // floats per staged sample row (+1: bank spread)
constexpr int EC_PAIR_LDS = 2 * EC_KT * EC_ROW + EC_CHUNK;                     // two tiles + heavy flags
constexpr int EC_TILE_LDS = 3 * SQ_TILE + SQ_TILE + SQ_MAX_CLASSES * SQ_MAX_CLASSES;  // x y z + class words + thresholds
constexpr int EC_LDS = EC_TILE_LDS > EC_PAIR_LDS ? EC_TILE_LDS : EC_PAIR_LDS;
enum { EC_MISSING_ALL = 0, EC_EXTRA_ALL = 1, EC_MISSING_HEAVY = 2, EC_EXTRA_HEAVY = 3 };

// index of the first tile of pair p in the row-major list of pairs (I <= J) of `tiles` tiles
__device__ __forceinline__ void ec_tile_pair(int p, int tiles, int& I, int& J) {
  I = 0;
  while (I < tiles && p >= tiles - I) { p -= tiles - I; ++I; }
  J = I + p;
}

__device__ __forceinline__ void ec_pair_role(float* smem, const float* __restrict__ gf, const int* __restrict__ h, int n,
                                             int K, int k_tiles, int p, double* __restrict__ out) {
  float* tk = smem;
  float* tl = smem + EC_KT * EC_ROW;
  int* hv = reinterpret_cast<int*>(smem + 2 * EC_KT * EC_ROW);
  const int lane = threadIdx.x;
  int KI, LI;
  ec_tile_pair(p, k_tiles, KI, LI);
  if (KI >= k_tiles) return;                               // (uniform)
  const int kk = lane >> 3, ll = lane & 7;
  const int k = KI * EC_KT + kk, l = LI * EC_KT + ll;
  double all = 0.0, hvy = 0.0;
  for (int a0 = 0; a0 < n; a0 += EC_CHUNK) {
    const int cols = min(EC_CHUNK, n - a0);
    __syncthreads();                                       // the previous step's tiles have been read
    for (int idx = lane; idx < EC_KT * 3 * EC_CHUNK; idx += WAVE) {
      const int s = idx / (3 * EC_CHUNK), r = idx - s * (3 * EC_CHUNK);
      if (r < 3 * cols) {
        const int ks = KI * EC_KT + s, ls = LI * EC_KT + s;
        tk[s * EC_ROW + r] = ks < K ? gf[3 * ((size_t)ks * (size_t)n + (size_t)a0) + r] : 0.f;
        tl[s * EC_ROW + r] = ls < K ? gf[3 * ((size_t)ls * (size_t)n + (size_t)a0) + r] : 0.f;
      }
    }
    if (lane < cols) hv[lane] = h ? (h[a0 + lane] != 0 ? 1 : 0) : 0;
    __syncthreads();
    const float* a = tk + kk * EC_ROW;
    const float* b = tl + ll * EC_ROW;
    for (int t = 0; t < cols; ++t) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double dd = (double)a[3 * t + d] - (double)b[3 * t + d];
        s += dd * dd;
      }
      all += s;
      if (hv[t]) hvy += s;
    }
  }
  if (k < K && l < K && k <= l) {                          // off-diagonal tiles: k < l always
    double* o = out + 2 * ((size_t)k * (size_t)K + (size_t)l);
    o[0] = all;
    o[1] = hvy;
    if (k < l) {
      o = out + 2 * ((size_t)l * (size_t)K + (size_t)k);
      o[0] = all;
      o[1] = hvy;
    }
  }
}

__device__ __forceinline__ void ec_bond_role(const float* __restrict__ g, const int* __restrict__ c, const int* __restrict__ h,
                                             const float* __restrict__ thr_sq, int n, int n_classes, const int* __restrict__ bonds,
                                             int e0, int e1, int* __restrict__ cnt) {
  const int lane = threadIdx.x;
  int h_all = 0, h_hv = 0, eb_hv = 0;
  for (int e = e0 + lane; e < e1; e += WAVE) {
    const int i = bonds[2 * (size_t)e], j = bonds[2 * (size_t)e + 1];
    const bool ok = i >= 0 && i < j && j < n;              // the host guarantees it; a bad entry counts as a missing bond
    const int ii = ok ? i : 0, jj = ok ? j : 0;
    const int ci = min(max(c[ii], 0), n_classes - 1), cj = min(max(c[jj], 0), n_classes - 1);
    const float s = sq_dist2(g[3 * ii], g[3 * ii + 1], g[3 * ii + 2], g[3 * jj], g[3 * jj + 1], g[3 * jj + 2]);
    const bool both = h[ii] != 0 && h[jj] != 0;
    const bool present = ok && s <= thr_sq[cj * n_classes + ci];
    h_all += present ? 1 : 0;
    h_hv += (present && both) ? 1 : 0;
    eb_hv += (ok && both) ? 1 : 0;
  }
  h_all = sq_wave_sum(h_all);
  h_hv = sq_wave_sum(h_hv);
  eb_hv = sq_wave_sum(eb_hv);
  if (lane == 0) {
    const int v[4] = {(e1 - e0) - h_all, -h_all, eb_hv - h_hv, -h_hv};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (v[q] != 0) atomicAdd(cnt + q, v[q]);
  }
}

__device__ __forceinline__ void ec_tile_role(float* smem, const float* __restrict__ g, const int* __restrict__ c,
                                             const int* __restrict__ h, const float* __restrict__ thr_sq, int n, int n_classes,
                                             int n_tiles, int p, int* __restrict__ cnt) {
  float* col = smem;                                        // [3][SQ_TILE]
  int* col_cls = reinterpret_cast<int*>(smem + 3 * SQ_TILE);   // class | heavy << 16
  float* thr = smem + 4 * SQ_TILE;
  const int lane = threadIdx.x;
  int I, J;
  ec_tile_pair(p, n_tiles, I, J);
  if (I >= n_tiles || J * SQ_TILE >= n) return;             // (uniform) tile pair outside this frame
  const int j = J * SQ_TILE + lane;
  if (j < n) {
#pragma unroll
    for (int d = 0; d < 3; ++d) col[d * SQ_TILE + lane] = g[3 * j + d];
    col_cls[lane] = min(max(c[j], 0), n_classes - 1) | (h[j] != 0 ? 0x10000 : 0);
  }
  for (int t = lane; t < n_classes * n_classes; t += SQ_TILE) thr[t] = thr_sq[t];
  const int i = I * SQ_TILE + lane;
  const bool row = i < n;
  const int ii = row ? i : n - 1;
  const float gx = g[3 * ii], gy = g[3 * ii + 1], gz = g[3 * ii + 2];
  const int ci = min(max(c[ii], 0), n_classes - 1);
  const bool hi = h[ii] != 0;
  __syncthreads();
  int p_all = 0, p_hv = 0;
  const int cols = min(SQ_TILE, n - J * SQ_TILE);
  const int first = (I == J) ? lane + 1 : 0;                // diagonal tile: j > i only
#pragma unroll 4
  for (int t = 0; t < cols; ++t) {
    const int w = col_cls[t];
    // the table is symmetric: [column class][row class] puts the lanes of one read on consecutive words
    const float s_star = thr[(w & 0xffff) * n_classes + ci];
    const int bg = (row && t >= first && sq_dist2(gx, gy, gz, col[t], col[SQ_TILE + t], col[2 * SQ_TILE + t]) <= s_star) ? 1 : 0;
    p_all += bg;
    p_hv += (hi && (w >> 16)) ? bg : 0;
  }
  p_all = sq_wave_sum(p_all);
  p_hv = sq_wave_sum(p_hv);
  if (lane == 0) {
    if (p_all != 0) atomicAdd(cnt + EC_EXTRA_ALL, p_all);
    if (p_hv != 0) atomicAdd(cnt + EC_EXTRA_HEAVY, p_hv);
  }
}

// grid: x = role (see the header comment), y = frame; one wave per block.
__global__ __launch_bounds__(64) void ensemble_check_k(const float* __restrict__ gen_xyz, const int* __restrict__ frame_ptr,
                                                       const int* __restrict__ cls, const int* __restrict__ heavy,
                                                       const float* __restrict__ thr_sq, const int* __restrict__ bond_ptr,
                                                       const int* __restrict__ bonds, int n_atoms, int n_bonds, int K,
                                                       int n_classes, int n_tiles, int k_tiles, int* __restrict__ counts,
                                                       double* __restrict__ pair_sums) {
  __shared__ float smem[EC_LDS];
  const int f = blockIdx.y;
  const int beg = frame_ptr[f], end = frame_ptr[f + 1], n = end - beg;
  if (beg < 0 || n <= 0 || end > n_atoms) return;           // (uniform) an empty or malformed frame keeps its zeros
  const float* __restrict__ gf = gen_xyz + 3 * (size_t)K * (size_t)beg;   // the frame's K samples, n rows each
  int x = blockIdx.x;
  const int ktp = k_tiles * (k_tiles + 1) / 2;
  if (x < ktp) {
    ec_pair_role(smem, gf, heavy ? heavy + beg : nullptr, n, K, k_tiles, x, pair_sums + 2 * (size_t)f * (size_t)K * (size_t)K);
    return;
  }
  x -= ktp;
  const int tp = n_tiles * (n_tiles + 1) / 2;
  const int k = x < K ? x : (x - K) / tp;
  if (k >= K) return;
  const float* __restrict__ g = gf + 3 * (size_t)k * (size_t)n;
  int* __restrict__ cnt = counts + 4 * ((size_t)f * (size_t)K + (size_t)k);
  if (x < K) {
    int e0 = bond_ptr[f], e1 = bond_ptr[f + 1];
    if (e0 < 0 || e1 < e0 || e1 > n_bonds) e1 = e0;         // malformed: no bonds
    ec_bond_role(g, cls + beg, heavy + beg, thr_sq, n, n_classes, bonds, e0, e1, cnt);
  } else {
    ec_tile_role(smem, g, cls + beg, heavy + beg, thr_sq, n, n_classes, n_tiles, (x - K) % tp, cnt);
  }
}

}  // namespace cgv

extern "C" {

int cgv_ensemble_check_max_classes(void) { return cgv::SQ_MAX_CLASSES; }
int cgv_ensemble_check_max_samples(void) { return cgv::EC_MAX_SAMPLES; }

int cgv_ensemble_check(const float* gen_xyz, const int32_t* frame_ptr, const int32_t* cls, const int32_t* heavy,
                       const float* thr_sq, const int32_t* bond_ptr, const int32_t* bonds, int n_frames, int n_atoms,
                       int n_samples, int n_classes, int max_frame_atoms, int n_bonds, int32_t* counts, double* pair_sums,
                       void* stream) {
  CGV_REQUIRE(n_frames >= 0 && n_atoms >= 0 && n_samples >= 0 && n_bonds >= 0, "bad size");
  if (n_frames == 0 || n_samples == 0) return 0;
  CGV_REQUIRE(counts && pair_sums && frame_ptr, "null pointer");
  CGV_REQUIRE(n_samples <= cgv::EC_MAX_SAMPLES, "n_samples <= cgv_ensemble_check_max_samples()");
  CGV_REQUIRE(n_frames <= 65535, "at most 65535 frames per launch");
  CGV_REQUIRE(max_frame_atoms >= 0 && max_frame_atoms <= n_atoms && max_frame_atoms <= cgv::SQ_MAX_FRAME_ATOMS,
              "max_frame_atoms must be the largest frame's atom count (<= 32768)");
  CGV_REQUIRE((((uintptr_t)pair_sums) & 7) == 0, "pair_sums must be 8-byte aligned");
  const bool validity = bond_ptr != nullptr;
  if (validity) {
    CGV_REQUIRE(n_classes >= 1 && n_classes <= cgv::SQ_MAX_CLASSES, "1 <= n_classes <= cgv_ensemble_check_max_classes()");
    CGV_REQUIRE(n_bonds == 0 || bonds, "null bond list");
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t units = (size_t)n_frames * (size_t)n_samples;
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 4 * units, st);
  if (e == hipSuccess) e = hipMemsetAsync(pair_sums, 0, sizeof(double) * 2 * units * (size_t)n_samples, st);
  if (e != hipSuccess) {
    cgv::set_error("cgv_ensemble_check: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (max_frame_atoms == 0) return 0;
  CGV_REQUIRE(gen_xyz, "null pointer");
  if (validity) CGV_REQUIRE(cls && heavy && thr_sq, "a topology needs cls, heavy and thr_sq");
  const int n_tiles = (max_frame_atoms + cgv::SQ_TILE - 1) / cgv::SQ_TILE;
  const int k_tiles = (n_samples + cgv::EC_KT - 1) / cgv::EC_KT;
  const long long tp = (long long)n_tiles * (n_tiles + 1) / 2;
  const long long gx = (long long)k_tiles * (k_tiles + 1) / 2 + (validity ? (long long)n_samples * (1 + tp) : 0);
  CGV_REQUIRE(gx <= 0x7fffffffLL, "too many blocks: fewer samples or smaller frames per launch");
  hipLaunchKernelGGL(cgv::ensemble_check_k, dim3((unsigned)gx, (unsigned)n_frames), dim3(64), 0, st, gen_xyz, frame_ptr, cls,
                     heavy, thr_sq, bond_ptr, bonds, n_atoms, n_bonds, n_samples, n_classes, n_tiles, k_tiles, counts,
                     pair_sums);
  return cgv::check_launch("cgv_ensemble_check");
}

}  // extern "C"
