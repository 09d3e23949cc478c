// K17 superposed RMSD between two sets of structures: for every pair (a_i, b_j) the minimum over PROPER rotations and
// translations of the root-mean-square deviation over a selection of atoms, and the nearest neighbour of every
// structure in the other set -- what coverage (recall) and precision of a generated ensemble are made of.  See
// include/cgvae_hip.h.  Nothing in the reference computes it (its RMSDs are unaligned, sampling.py: compute_rmsd).
//
//   rmsd^2(i, j) = max(0, G_a[i] + G_b[j] - 2 lambda(i, j)) / m
// G: sum of squared centred coordinates over the selection; lambda: largest eigenvalue of the quaternion key matrix of
// M = sum_k a~_i[k]^T b~_j[k] (superpose_eig.h).  fp32 coordinates are widened on load; everything after is fp64.
//
// cgv_superpose, four launches:
//   superpose_prep_k   (once per set) one thread per structure: centroid and G over sel in ascending order, a `bad`
//                      flag for a non-finite selected coordinate (its centroid and G are stored as 0).
//   superpose_cross_k  256 threads, grid (tiles of 32 row structures, tiles of 32 column structures).  Per stage of
//                      SP_KA = 16 selected atoms the block gathers them for its 32 + 32 structures from xyz, widens,
//                      subtracts the centroid and writes three coordinate planes per side to LDS, atom major; wave w owns
//                      the 16 x 16 pairs (w >> 1, w & 1) and accumulates the nine M_ab with v_mfma_f64_16x16x4_f64 (A:
//                      plane a of 16 row structures x 4 atoms, B: plane b of 16 column structures x 4 atoms), so the
//                      nine accumulators share one result layout and a lane ends with the whole 3 x 3 of its four pairs
//                      in registers.  Atoms past m, structures past S and bad structures are staged as +0.0.  Epilogue
//                      per lane: four key matrices, SP_SWEEPS Jacobi sweeps over the four together (independent chains
//                      for the fp64 pipe), rmsd^2 into a 32 x 33 LDS tile that reuses the staging buffer (and into the
//                      dense output when asked); threads 0..31 scan their row of the tile in ascending column order,
//                      threads 32..63 their column in ascending row order (strictly smaller wins: the lowest index of
//                      equal values), and write (value, global index) partials to the workspace.
//   superpose_merge_k  one thread per row and per column: the partials in ascending tile order, then against the
//                      caller's running (value, index): the smaller value, on equal bits the lower index.
// No floating-point atomics, no order left to the scheduler: the same bits on every run, and the same minima whatever
// chunks the caller cuts the sets into.  An index of sel outside [0, n) reads atom 0 (the host wrapper refuses such a
// selection); nothing is read out of bounds.
#include <math.h>

#include "cgv_common.h"
#include "superpose_eig.h"

namespace cgv {

constexpr int SP_THREADS = 256;
constexpr int SP_TILE = 32;                   // structures of a block's row / column tile: 2 x 2 MFMA tiles, one per wave
constexpr int SP_KA = 16;                     // selected atoms of a stage: 4 MFMA steps of depth 4
constexpr int SP_LD = SP_TILE + 1;            // padded row of an LDS plane / of the value tile
constexpr int SP_MAX_STRUCTURES = 1 << 20;    // per set and launch: the grid's y extent stays below 65 536
constexpr int SP_MAX_ATOMS = 1 << 20;

typedef double sp_d4 __attribute__((ext_vector_type(4)));

static inline int sp_tiles(int s) { return (s + SP_TILE - 1) / SP_TILE; }

// byte offsets into the workspace: the doubles first (the workspace is 8-byte aligned), then the int32 arrays
struct SpLayout {
  size_t cen_a, g_a, cen_b, g_b, prow_v, pcol_v, bad_a, bad_b, prow_i, pcol_i, bytes;
};
static inline SpLayout sp_layout(int sa, int sb) {
  const size_t A = (size_t)sa, B = (size_t)sb, ncb = (size_t)sp_tiles(sb), nrb = (size_t)sp_tiles(sa);
  SpLayout L;
  size_t at = 0;
  L.cen_a = at, at += 3 * A * 8;
  L.g_a = at, at += A * 8;
  L.cen_b = at, at += 3 * B * 8;
  L.g_b = at, at += B * 8;
  L.prow_v = at, at += ncb * A * 8;
  L.pcol_v = at, at += nrb * B * 8;
  L.bad_a = at, at += A * 4;
  L.bad_b = at, at += B * 4;
  L.prow_i = at, at += ncb * A * 4;
  L.pcol_i = at, at += nrb * B * 4;
  L.bytes = (at + 7) & ~(size_t)7;
  return L;
}

__global__ __launch_bounds__(256) void superpose_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel, int S, int n,
                                                        int m, double* __restrict__ cen, double* __restrict__ G,
                                                        int* __restrict__ bad) {
  const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (s >= S) return;
  const float* base = xyz + (size_t)s * n * 3;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  bool ok = true;
  for (int k = 0; k < m; ++k) {
    const f3 p = ld3(base + 3 * (size_t)sel_atom(sel[k], n));
    ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    sx += (double)p.x, sy += (double)p.y, sz += (double)p.z;
  }
  double cx = sx / (double)m, cy = sy / (double)m, cz = sz / (double)m, g = 0.0;
  for (int k = 0; k < m; ++k) {
    const f3 p = ld3(base + 3 * (size_t)sel_atom(sel[k], n));
    const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
    g += (dx * dx + dy * dy) + dz * dz;
  }
  if (!ok) cx = cy = cz = g = 0.0;
  cen[3 * (size_t)s] = cx, cen[3 * (size_t)s + 1] = cy, cen[3 * (size_t)s + 2] = cz;
  G[s] = g;
  bad[s] = ok ? 0 : 1;
}

// grid: x = row tile, y = column tile
__global__ __launch_bounds__(SP_THREADS) void superpose_cross_k(
    const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ sel, int sa, int sb, int n, int m,
    const double* __restrict__ cen_a, const double* __restrict__ g_a, const int* __restrict__ bad_a,
    const double* __restrict__ cen_b, const double* __restrict__ g_b, const int* __restrict__ bad_b, int off_a, int off_b, int same,
    double* __restrict__ prow_v, int* __restrict__ prow_i, double* __restrict__ pcol_v, int* __restrict__ pcol_i,
    double* __restrict__ dense) {
  __shared__ double st[2][3][SP_KA][SP_LD];                  // [rows | columns][x, y, z][atom of the stage][structure] (24.75 KB)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = (int)blockIdx.x * SP_TILE, col0 = (int)blockIdx.y * SP_TILE;
  // staging: a thread owns atom slot kk of four structures, two of the row tile (u = 0, 1) and two of the column tile
  const int kk = tid & 15, s0 = tid >> 4;
  const float* base[4];
  double c[4][3];
  bool live[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool col = u >= 2;
    const int gs = (col ? col0 : row0) + s0 + 16 * (u & 1);
    live[u] = gs < (col ? sb : sa) && (col ? bad_b : bad_a)[gs < (col ? sb : sa) ? gs : 0] == 0;
    const int safe = live[u] ? gs : 0;
    base[u] = (col ? b : a) + (size_t)safe * n * 3;
    const double* cc = (col ? cen_b : cen_a) + 3 * (size_t)safe;
    c[u][0] = cc[0], c[u][1] = cc[1], c[u][2] = cc[2];
  }
  const int sr = (wave >> 1) * 16, sc = (wave & 1) * 16;     // the wave's 16 x 16 pairs
  const int ml = lane & 15, mk = lane >> 4;                  // A: row ml, depth mk; B: depth mk, column ml
  sp_d4 acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = sp_d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < m; k0 += SP_KA) {
    __syncthreads();                                         // the previous stage has been read
    const bool in = k0 + kk < m;
    const int at = in ? sel_atom(sel[k0 + kk], n) : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      double x = 0.0, y = 0.0, z = 0.0;
      if (in && live[u]) {
        const f3 p = ld3(base[u] + 3 * (size_t)at);
        x = (double)p.x - c[u][0], y = (double)p.y - c[u][1], z = (double)p.z - c[u][2];
      }
      const int side = u >> 1, sl = s0 + 16 * (u & 1);
      st[side][0][kk][sl] = x, st[side][1][kk][sl] = y, st[side][2][kk][sl] = z;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SP_KA / 4; ++s) {
      const int k = 4 * s + mk;
      double pa[3], pb[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) pa[d] = st[0][d][k][sr + ml], pb[d] = st[1][d][k][sc + ml];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[i], pb[j], acc[i][j], 0, 0, 0);
    }
  }
  // result layout of the f64 MFMA: register r of lane l is row (l >> 4) + 4 r, column l & 15
  double key[4][10];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[3 * i + j] = acc[i][j][r];
    sp_key_matrix(M, key[r]);
  }
#pragma unroll 1
  for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sp_sweep(key[r]);
  }
  __syncthreads();                                           // every wave has read its last stage: st becomes the value tile
  double (*vt)[SP_LD] = reinterpret_cast<double (*)[SP_LD]>(&st[0][0][0][0]);   // 32 x 33 doubles of the 6 x 16 x 33
  const int jl = sc + ml, j = col0 + jl;
  const bool in_j = j < sb, ok_j = in_j && bad_b[in_j ? j : 0] == 0;
  const double gb = ok_j ? g_b[j] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int il = sr + mk + 4 * r, i = row0 + il;
    const bool in_i = i < sa, ok = ok_j && in_i && bad_a[in_i ? i : 0] == 0;
    const double ga = ok ? g_a[i] : 0.0;
    const double v = fmax(0.0, ga + gb - 2.0 * sp_largest(key[r])) / (double)m;
    const bool self = same != 0 && off_a + i == off_b + j;
    vt[il][jl] = (ok && !self) ? v : (double)INFINITY;
    if (dense != nullptr && in_i && in_j) dense[(size_t)i * sb + j] = ok ? v : (double)NAN;
  }
  __syncthreads();
  if (tid < 2 * SP_TILE) {
    const bool cols = tid >= SP_TILE;
    const int t = tid & (SP_TILE - 1);
    double best = (double)INFINITY;
    int idx = -1;
#pragma unroll 4
    for (int q = 0; q < SP_TILE; ++q) {
      const double v = cols ? vt[q][t] : vt[t][q];
      if (v < best) best = v, idx = q;
    }
    if (!cols && row0 + t < sa) {
      const size_t at = (size_t)blockIdx.y * sa + (size_t)(row0 + t);
      prow_v[at] = best;
      prow_i[at] = idx < 0 ? -1 : off_b + col0 + idx;
    }
    if (cols && col0 + t < sb) {
      const size_t at = (size_t)blockIdx.x * sb + (size_t)(col0 + t);
      pcol_v[at] = best;
      pcol_i[at] = idx < 0 ? -1 : off_a + row0 + idx;
    }
  }
}

// one thread per row (e < sa) and per column (sa <= e < sa + sb)
__global__ __launch_bounds__(256) void superpose_merge_k(const double* __restrict__ prow_v, const int* __restrict__ prow_i,
                                                         const double* __restrict__ pcol_v, const int* __restrict__ pcol_i, int sa,
                                                         int sb, int ncb, int nrb, double* __restrict__ row_min,
                                                         int* __restrict__ row_arg, double* __restrict__ col_min,
                                                         int* __restrict__ col_arg) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= sa + sb) return;
  const bool cols = e >= sa;
  const int at = cols ? e - sa : e, S = cols ? sb : sa, ranges = cols ? nrb : ncb;
  const double* pv = cols ? pcol_v : prow_v;
  const int* pi = cols ? pcol_i : prow_i;
  double best = (double)INFINITY;
  int idx = -1;
  for (int r = 0; r < ranges; ++r) {                         // ascending ranges hold ascending indices
    const double v = pv[(size_t)r * S + at];
    const int i = pi[(size_t)r * S + at];
    if (i >= 0 && (idx < 0 || v < best)) best = v, idx = i;
  }
  double* out_v = (cols ? col_min : row_min) + at;
  int* out_i = (cols ? col_arg : row_arg) + at;
  const double cur = *out_v;
  const int ci = *out_i;
  if (idx >= 0 && (ci < 0 || best < cur || (best == cur && idx < ci))) *out_v = best, *out_i = idx;
}

}  // namespace cgv

extern "C" {

int cgv_superpose_max_structures(void) { return cgv::SP_MAX_STRUCTURES; }
int cgv_superpose_max_atoms(void) { return cgv::SP_MAX_ATOMS; }

size_t cgv_superpose_workspace_bytes(int sa, int sb) {
  if (sa < 0 || sb < 0 || sa > cgv::SP_MAX_STRUCTURES || sb > cgv::SP_MAX_STRUCTURES) return 0;
  return cgv::sp_layout(sa, sb).bytes;
}

int cgv_superpose(const float* a, const float* b, const int32_t* sel, int sa, int sb, int n_atoms, int m, int off_a, int off_b,
                  int same, double* row_min, int32_t* row_arg, double* col_min, int32_t* col_arg, double* dense,
                  void* workspace, size_t workspace_bytes, void* stream) {
  CGV_REQUIRE(sa >= 0 && sb >= 0 && n_atoms >= 0, "bad size");
  CGV_REQUIRE(sa <= cgv::SP_MAX_STRUCTURES && sb <= cgv::SP_MAX_STRUCTURES, "structures per set <= cgv_superpose_max_structures()");
  CGV_REQUIRE(n_atoms <= cgv::SP_MAX_ATOMS, "n_atoms <= cgv_superpose_max_atoms()");
  CGV_REQUIRE(m >= 1 && m <= n_atoms, "1 <= m <= n_atoms");
  CGV_REQUIRE(off_a >= 0 && off_b >= 0 && off_a <= INT32_MAX - sa && off_b <= INT32_MAX - sb, "offsets: global indices are int32");
  if (sa == 0 || sb == 0) return 0;
  CGV_REQUIRE(a && b && sel && row_min && row_arg && col_min && col_arg, "null pointer");
  const cgv::SpLayout L = cgv::sp_layout(sa, sb);
  CGV_REQUIRE(workspace && workspace_bytes >= L.bytes, "workspace smaller than cgv_superpose_workspace_bytes()");
  CGV_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  char* ws = (char*)workspace;
  double *cen_a = (double*)(ws + L.cen_a), *g_a = (double*)(ws + L.g_a), *cen_b = (double*)(ws + L.cen_b), *g_b = (double*)(ws + L.g_b);
  double *prow_v = (double*)(ws + L.prow_v), *pcol_v = (double*)(ws + L.pcol_v);
  int *bad_a = (int*)(ws + L.bad_a), *bad_b = (int*)(ws + L.bad_b), *prow_i = (int*)(ws + L.prow_i), *pcol_i = (int*)(ws + L.pcol_i);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cgv::superpose_prep_k, dim3((unsigned)((sa + 255) / 256)), dim3(256), 0, st, a, sel, sa, n_atoms, m, cen_a, g_a,
                     bad_a);
  hipLaunchKernelGGL(cgv::superpose_prep_k, dim3((unsigned)((sb + 255) / 256)), dim3(256), 0, st, b, sel, sb, n_atoms, m, cen_b, g_b,
                     bad_b);
  int rc = cgv::check_launch("cgv_superpose (preparation)");
  if (rc) return rc;
  const int nrb = cgv::sp_tiles(sa), ncb = cgv::sp_tiles(sb);
  hipLaunchKernelGGL(cgv::superpose_cross_k, dim3((unsigned)nrb, (unsigned)ncb), dim3(cgv::SP_THREADS), 0, st, a, b, sel, sa, sb,
                     n_atoms, m, cen_a, g_a, bad_a, cen_b, g_b, bad_b, off_a, off_b, same, prow_v, prow_i, pcol_v, pcol_i, dense);
  rc = cgv::check_launch("cgv_superpose");
  if (rc) return rc;
  hipLaunchKernelGGL(cgv::superpose_merge_k, dim3((unsigned)((sa + sb + 255) / 256)), dim3(256), 0, st, prow_v, prow_i, pcol_v, pcol_i,
                     sa, sb, ncb, nrb, row_min, row_arg, col_min, col_arg);
  return cgv::check_launch("cgv_superpose (merge)");
}

}  // extern "C"
