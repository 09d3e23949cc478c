// K26 secondary structure of an ensemble (DSSP, Kabsch & Sander 1983): for every structure the class H B E G I T S - of
// every residue of a peptide, from backbone heavy atoms alone, and over the structures how often every residue is in every
// class.  See include/cgvae_hip.h.  Nothing in the reference computes it.
//
// The CALLER's tables name the atoms: res [R,4] = N, CA, C, O of residue r in chain order, prev [R,2] = the carbonyl C' and
// O' in front of N(r) (-1, -1: the residue has no amide hydrogen and never donates), link [R] = 1 iff C(r) is bonded to
// N(r+1).  All floating point is fp32 with every operation rounded on its own (this file is compiled with
// -ffp-contract=off; sqrtf and / are the correctly rounded forms, see csrc/tica.hip), every test is written so that a NaN
// fails it, and the host restates it operation for operation: every integer this file produces is exact.
//   virtual hydrogen     w = C' - O',  l = sqrtf((wx*wx + wy*wy) + wz*wz),  H_k = N_k + w_k / l
//   hb[i][j]             C=O of i accepts from N-H of j: j has an H, j != i, j != i + 1, sq_dist2(CA_i, CA_j) < 81 and e < -0.5,
//                        e = 27.888 * (((1/rON + 1/rCH) - 1/rOH) - 1/rCN), r = sqrtf(d2); e = -9.9 when a d2 < 0.25
//   cont(a, b)           link[a .. b-1] are all 1
//   turn_n(i)            hb[i][i+n] and cont(i, i+n), n = 3, 4, 5
//   bridges (i, j)       |i-j| >= 3, i+-1 and j+-1 exist, cont(i-1, i+1), cont(j-1, j+1):
//                        par  = (hb[i-1][j] & hb[j][i+1]) | (hb[j-1][i] & hb[i][j+1])
//                        anti = (hb[i][j] & hb[j][i])     | (hb[i-1][j+1] & hb[j-1][i+1])
//                        in a ladder: the same type also at (i+1, j+1) or (i-1, j-1) (par), (i+1, j-1) or (i-1, j+1) (anti)
//   bend(i)              cont(i-2, i+2), u = CA_i - CA_{i-2}, v = CA_{i+2} - CA_i: uu > 0, vv > 0 and
//                        (dot <= 0 or dot*dot < (c2*uu)*vv), c2 = fp32(cos(70 degrees)^2)
//   classes              H: i..i+3 where turn_4(i-1) & turn_4(i);  E / B: not H, a bridge in a ladder / a bridge but none in a
//                        ladder;  G: i..i+2 where turn_3(i-1) & turn_3(i) and none of the three is H E B;  I: i..i+4 likewise
//                        for n = 5, none of the five H E B G;  T: unassigned and turn_n(i-k), 1 <= k < n;  S: unassigned and
//                        bend;  - otherwise.  Code = index into "HBEGITS-".
//
// dssp_k<GROUP>   GROUP threads own a structure, 256 / GROUP structures a block.  GROUP = 64 (R <= 64, the chignolin case):
//                 one wave per structure, the block walks the structures with a stride of the grid and keeps class_counts in
//                 LDS until it ends.  GROUP = 256 (larger R): one block per structure.  The whole assignment of a structure
//                 stays in LDS: N CA C O H of every residue; the bit matrix hb [R][W] and its transpose tb [R][W] (W words of
//                 64); the per-residue flags.  In the energy stage a lane owns a donor j and a wave an acceptor row i: the
//                 ballot of the test IS the word of hb (and of hb_bits); a set bit is ORed into tb.  Bridges and ladders are
//                 words of hb and tb ANDed after shifts by one bit -- 64 partners at a time, nothing per pair.  The class
//                 stages are separated by barriers and each reads only what an earlier stage finished.
// Sums of integers meet in atomicAdd, whose order does not matter, and everything else has one writer: two runs give the
// same bits, and nothing depends on how the caller cuts the structures into launches.
#include <math.h>

#include "cgv_common.h"
#include "sq_dist.h"

namespace cgv {

constexpr int DS_THREADS = 256;
constexpr int DS_WAVE_PATH_MAX = 64;          // residues up to which a wave owns a structure
constexpr int DS_LDS_BUDGET = 64 * 1024;      // bytes of LDS a block may ask for without an attribute
constexpr int DS_MAX_RESIDUES = 384;          // the most for which ds_slot_bytes(R, false) <= DS_LDS_BUDGET (static_assert below)
constexpr int DS_MAX_STRUCTURES = 1 << 20;    // per launch
constexpr int DS_WAVE_BLOCKS = 2048;          // grid of the wave path at most: 8 blocks on each of 256 CUs
constexpr int DS_CLASSES = 8;
constexpr float DS_BEND_C2 = 0.116977781f;    // fp32(cos(70 degrees)^2) = 0x3DEF920C (cgv_dssp_bend_c2; the host checks it)
enum { DS_H = 0, DS_B = 1, DS_E = 2, DS_G = 3, DS_I = 4, DS_T = 5, DS_S = 6, DS_LOOP = 7, DS_NONE = 255 };
enum { DS_N = 0, DS_CA = 1, DS_C = 2, DS_O = 3, DS_HY = 4, DS_ATOMS = 5 };

typedef unsigned long long u64;

// LDS of one structure: hb, tb [R][W] u64; valid [W] u64; cc [R][8] int (wave path); cnt [16] int; pos [5][R][3] float;
// seven byte flags per residue
__host__ __device__ constexpr size_t ds_slot_bytes(int R, bool accumulate) {
  const size_t W = (size_t)(R + 63) / 64;
  const size_t bytes = 16 * (size_t)R * W + 8 * W + (accumulate ? 32 * (size_t)R : 0) + 64 + 60 * (size_t)R + 7 * (size_t)R;
  return (bytes + 7) / 8 * 8;
}
static_assert(ds_slot_bytes(DS_MAX_RESIDUES, false) <= DS_LDS_BUDGET && ds_slot_bytes(DS_MAX_RESIDUES + 1, false) > DS_LDS_BUDGET,
              "DS_MAX_RESIDUES is what the LDS budget holds");
static_assert((DS_THREADS / 64) * ds_slot_bytes(DS_WAVE_PATH_MAX, true) <= DS_LDS_BUDGET, "the wave path's four structures fit");

struct DsSlot {
  u64 *hb, *tb, *valid;
  int *cc, *cnt;                                             // cnt[0..7]: n_class; cnt[8]: bad
  float* pos;
  unsigned char *has_h, *link, *turn, *bridge, *bend, *code0, *code1;
  int R, W;
};

__device__ __forceinline__ DsSlot ds_slot(unsigned char* base, int R, bool accumulate) {
  DsSlot L;
  const int W = (R + 63) / 64;
  L.R = R;
  L.W = W;
  L.hb = (u64*)base;
  L.tb = L.hb + (size_t)R * W;
  L.valid = L.tb + (size_t)R * W;
  L.cc = (int*)(L.valid + W);
  L.cnt = L.cc + (accumulate ? 8 * R : 0);
  L.pos = (float*)(L.cnt + 16);
  L.has_h = (unsigned char*)(L.pos + DS_ATOMS * 3 * R);
  L.link = L.has_h + R;
  L.turn = L.link + R;
  L.bridge = L.turn + R;
  L.bend = L.bridge + R;
  L.code0 = L.bend + R;
  L.code1 = L.code0 + R;
  return L;
}

__device__ __forceinline__ const float* ds_at(const DsSlot& L, int which, int r) { return L.pos + 3 * (which * L.R + r); }
__device__ __forceinline__ float ds_sq(const float* a, const float* b) { return sq_dist2(a[0], a[1], a[2], b[0], b[1], b[2]); }

__device__ __forceinline__ bool ds_cont(const DsSlot& L, int a, int b) {   // 0 <= a <= b <= R - 1
  for (int k = a; k < b; ++k)
    if (!L.link[k]) return false;
  return true;
}

// the words of a bit matrix, 0 outside it, and a row moved by one bit: shl's bit j is the row's bit j - 1, shr's its bit j + 1
__device__ __forceinline__ u64 ds_word(const DsSlot& L, const u64* m, int i, int w) {
  return (i < 0 || i >= L.R || w < 0 || w >= L.W) ? 0ull : m[i * L.W + w];
}
__device__ __forceinline__ u64 ds_shl(const DsSlot& L, const u64* m, int i, int w) {
  return (ds_word(L, m, i, w) << 1) | (ds_word(L, m, i, w - 1) >> 63);
}
__device__ __forceinline__ u64 ds_shr(const DsSlot& L, const u64* m, int i, int w) {
  return (ds_word(L, m, i, w) >> 1) | (ds_word(L, m, i, w + 1) << 63);
}
__device__ __forceinline__ bool ds_hb(const DsSlot& L, int i, int j) { return (L.hb[i * L.W + (j >> 6)] >> (j & 63)) & 1ull; }

// bit j of the result: residue i and residue 64 w + j form a parallel (anti == false) or antiparallel bridge
__device__ __forceinline__ u64 ds_bridge(const DsSlot& L, bool anti, int i, int w) {
  if (w < 0 || w >= L.W || i < 1 || i > L.R - 2 || !L.link[i - 1] || !L.link[i]) return 0ull;
  u64 far = ~0ull;                                           // |i - j| >= 3
  for (int j = max(i - 2, 0); j <= i + 2; ++j)
    if ((j >> 6) == w) far &= ~(1ull << (j & 63));
  const u64 b = anti ? ((ds_word(L, L.hb, i, w) & ds_word(L, L.tb, i, w)) | (ds_shr(L, L.hb, i - 1, w) & ds_shl(L, L.tb, i + 1, w)))
                     : ((ds_word(L, L.hb, i - 1, w) & ds_word(L, L.tb, i + 1, w)) | (ds_shl(L, L.tb, i, w) & ds_shr(L, L.hb, i, w)));
  return b & L.valid[w] & far;
}
// the bridges of (i, .) moved by one bit, as ds_shl / ds_shr
__device__ __forceinline__ u64 ds_bridge_shl(const DsSlot& L, bool anti, int i, int w) {
  return (ds_bridge(L, anti, i, w) << 1) | (ds_bridge(L, anti, i, w - 1) >> 63);
}
__device__ __forceinline__ u64 ds_bridge_shr(const DsSlot& L, bool anti, int i, int w) {
  return (ds_bridge(L, anti, i, w) >> 1) | (ds_bridge(L, anti, i, w + 1) << 63);
}

// C=O of i accepts from N-H of j (j has an H, j != i, j != i + 1: the caller's)
__device__ __forceinline__ bool ds_accepts(const DsSlot& L, int i, int j) {
  if (!(ds_sq(ds_at(L, DS_CA, i), ds_at(L, DS_CA, j)) < 81.0f)) return false;
  const float* O = ds_at(L, DS_O, i);
  const float* C = ds_at(L, DS_C, i);
  const float* N = ds_at(L, DS_N, j);
  const float* H = ds_at(L, DS_HY, j);
  const float on = ds_sq(O, N), ch = ds_sq(C, H), oh = ds_sq(O, H), cn = ds_sq(C, N);
  float e = -9.9f;
  if (!(on < 0.25f || ch < 0.25f || oh < 0.25f || cn < 0.25f)) {
    const float s = __fsub_rn(__fsub_rn(__fadd_rn(1.0f / sqrtf(on), 1.0f / sqrtf(ch)), 1.0f / sqrtf(oh)), 1.0f / sqrtf(cn));
    e = __fmul_rn(27.888f, s);
  }
  return e < -0.5f;
}

// GROUP threads a structure: 64 (a wave; the block walks the structures, class_counts gathered in LDS) or 256 (the block)
template <int GROUP>
__global__ __launch_bounds__(DS_THREADS) void dssp_k(const float* __restrict__ xyz, const int* __restrict__ res,
                                                     const int* __restrict__ prev, const int* __restrict__ link, int S, int n, int R,
                                                     u64* __restrict__ class_counts, int* __restrict__ n_class, int* __restrict__ bad,
                                                     unsigned char* __restrict__ codes, u64* __restrict__ hb_bits) {
  constexpr int SLOTS = DS_THREADS / GROUP, WAVES = GROUP / 64;
  constexpr bool ACC = GROUP == 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char ds_lds[];
  const int tid = threadIdx.x, slot = tid / GROUP, t = tid % GROUP, lane = tid & 63, gw = t >> 6;
  const DsSlot L = ds_slot(ds_lds + (size_t)slot * ds_slot_bytes(R, ACC), R, ACC);
  const int W = L.W;
  if (ACC)
    for (int e = t; e < 8 * R; e += GROUP) L.cc[e] = 0;
  for (int s0 = (int)blockIdx.x * SLOTS; s0 < S; s0 += (int)gridDim.x * SLOTS) {   // the same trips for the whole block
    const int s = s0 + slot;
    const bool active = s < S;
    // ---- clear
    for (int e = t; e < R * W; e += GROUP) L.tb[e] = 0ull;
    if (t < 16) L.cnt[t] = 0;
    __syncthreads();
    // ---- the table atoms and the virtual hydrogen
    const float* base = xyz + (size_t)(active ? s : 0) * n * 3;
    for (int r = t; r < R; r += GROUP) {
      bool ok = true;
      for (int a = 0; a < 4; ++a) {
        const f3 p = ld3(base + 3 * (size_t)sel_atom(res[4 * r + a], n));
        ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
        float* q = L.pos + 3 * (a * R + r);
        q[0] = p.x, q[1] = p.y, q[2] = p.z;
      }
      const int pc = prev[2 * r], po = prev[2 * r + 1];
      const bool has = pc >= 0 && po >= 0;
      float hx = 0.f, hy = 0.f, hz = 0.f;
      if (has) {
        const f3 c = ld3(base + 3 * (size_t)sel_atom(pc, n)), o = ld3(base + 3 * (size_t)sel_atom(po, n));
        ok = ok && isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(o.x) && isfinite(o.y) && isfinite(o.z);
        const float wx = __fsub_rn(c.x, o.x), wy = __fsub_rn(c.y, o.y), wz = __fsub_rn(c.z, o.z);
        const float l = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(wx, wx), __fmul_rn(wy, wy)), __fmul_rn(wz, wz)));
        const float* N = ds_at(L, DS_N, r);                  // this thread wrote it
        hx = __fadd_rn(N[0], wx / l), hy = __fadd_rn(N[1], wy / l), hz = __fadd_rn(N[2], wz / l);
      }
      float* q = L.pos + 3 * (DS_HY * R + r);
      q[0] = hx, q[1] = hy, q[2] = hz;
      L.has_h[r] = has ? 1 : 0;
      L.link[r] = (r + 1 < R && link[r] != 0) ? 1 : 0;
      if (!ok) L.cnt[8] = 1;                                 // every writer writes 1
    }
    __syncthreads();
    // ---- which partners can be in a bridge at all; the energy stage
    for (int w = t; w < W; w += GROUP) {
      u64 v = 0ull;
      for (int b = 0; b < 64; ++b) {
        const int j = 64 * w + b;
        if (j >= 1 && j <= R - 2 && L.link[j - 1] && L.link[j]) v |= 1ull << b;
      }
      L.valid[w] = v;
    }
    for (int i = gw; i < R; i += WAVES)                      // a wave owns the acceptor row, a lane the donor
      for (int w = 0; w < W; ++w) {
        const int j = 64 * w + lane;
        bool bond = false;
        if (j < R && L.has_h[j] && j != i && j != i + 1) bond = ds_accepts(L, i, j);
        const u64 word = __ballot(bond);
        if (lane == 0) L.hb[i * W + w] = word;
        if (bond) atomicOr((unsigned int*)(L.tb + j * W) + (i >> 5), 1u << (i & 31));   // little endian: bit i of the row
      }
    __syncthreads();
    const bool good = active && L.cnt[8] == 0;
    // ---- per residue: turns, bridges, bend; hb_bits leaves
    if (hb_bits != nullptr && active)
      for (int e = t; e < R * W; e += GROUP) hb_bits[(size_t)s * R * W + e] = good ? L.hb[e] : 0ull;
    for (int i = t; i < R; i += GROUP) {
      int turn = 0;
      for (int k = 3; k <= 5; ++k)
        if (i + k < R && ds_hb(L, i, i + k) && ds_cont(L, i, i + k)) turn |= 1 << (k - 3);
      L.turn[i] = (unsigned char)turn;
      int bridge = 0;                                        // 1: a bridge, 2: one of them in a ladder
      for (int w = 0; w < W; ++w) {
        const u64 p = ds_bridge(L, false, i, w), a = ds_bridge(L, true, i, w);
        if (p | a) bridge = max(bridge, 1);
        u64 lad = 0ull;
        if (p) lad |= p & (ds_bridge_shr(L, false, i + 1, w) | ds_bridge_shl(L, false, i - 1, w));
        if (a) lad |= a & (ds_bridge_shl(L, true, i + 1, w) | ds_bridge_shr(L, true, i - 1, w));
        if (lad) bridge = 2;
      }
      L.bridge[i] = (unsigned char)bridge;
      bool bend = false;
      if (i >= 2 && i + 2 < R && ds_cont(L, i - 2, i + 2)) {
        const float *a = ds_at(L, DS_CA, i - 2), *b = ds_at(L, DS_CA, i), *c = ds_at(L, DS_CA, i + 2);
        const float ux = __fsub_rn(b[0], a[0]), uy = __fsub_rn(b[1], a[1]), uz = __fsub_rn(b[2], a[2]);
        const float vx = __fsub_rn(c[0], b[0]), vy = __fsub_rn(c[1], b[1]), vz = __fsub_rn(c[2], b[2]);
        const float uu = __fadd_rn(__fadd_rn(__fmul_rn(ux, ux), __fmul_rn(uy, uy)), __fmul_rn(uz, uz));
        const float vv = __fadd_rn(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)), __fmul_rn(vz, vz));
        const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy)), __fmul_rn(uz, vz));
        bend = uu > 0.f && vv > 0.f && (dot <= 0.f || __fmul_rn(dot, dot) < __fmul_rn(__fmul_rn(DS_BEND_C2, uu), vv));
      }
      L.bend[i] = bend ? 1 : 0;
    }
    __syncthreads();
    // ---- H, then E / B
    for (int i = t; i < R; i += GROUP) {
      bool helix = false;
      for (int a = max(i - 3, 1); a <= i; ++a) helix = helix || ((L.turn[a - 1] & 2) && (L.turn[a] & 2));
      L.code0[i] = helix ? DS_H : L.bridge[i] == 2 ? DS_E : L.bridge[i] == 1 ? DS_B : DS_NONE;
    }
    __syncthreads();
    // ---- G
    for (int i = t; i < R; i += GROUP) {
      int code = L.code0[i];
      for (int a = max(i - 2, 1); a <= i && code == DS_NONE; ++a)
        if ((L.turn[a - 1] & 1) && (L.turn[a] & 1) && L.code0[a] == DS_NONE && L.code0[a + 1] == DS_NONE && L.code0[a + 2] == DS_NONE)
          code = DS_G;                                       // turn_3(a): a + 3 < R
      L.code1[i] = (unsigned char)code;
    }
    __syncthreads();
    // ---- I, T, S, loop; the outputs
    for (int i = t; i < R; i += GROUP) {
      int code = L.code1[i];
      for (int a = max(i - 4, 1); a <= i && code == DS_NONE; ++a)
        if ((L.turn[a - 1] & 4) && (L.turn[a] & 4)) {        // turn_5(a): a + 5 < R
          bool free5 = true;
          for (int k = 0; k < 5; ++k) free5 = free5 && L.code1[a + k] == DS_NONE;
          if (free5) code = DS_I;
        }
      if (code == DS_NONE)
        for (int k = 1; k < 5; ++k)                          // turn_n(i - k), 1 <= k < n: n = 3 for k < 3, 4 for k < 4, 5
          if (i - k >= 0 && (L.turn[i - k] & (k < 3 ? 7 : k < 4 ? 6 : 4))) code = DS_T;
      if (code == DS_NONE) code = L.bend[i] ? DS_S : DS_LOOP;
      if (active && codes != nullptr) codes[(size_t)s * R + i] = (unsigned char)(good ? code : DS_NONE);
      if (good) {
        atomicAdd(&L.cnt[code], 1);
        if (ACC) L.cc[8 * i + code] += 1;                    // this thread alone owns residue i of this structure
        else atomicAdd(class_counts + 8 * (size_t)i + code, 1ull);
      }
    }
    __syncthreads();
    if (active) {
      if (t < 8) n_class[8 * (size_t)s + t] = good ? L.cnt[t] : -1;
      if (t == 8) bad[s] = good ? 0 : 1;
    }
    __syncthreads();                                         // cnt has been read before the next structure clears it
  }
  if (ACC)
    for (int e = t; e < 8 * R; e += GROUP)
      if (L.cc[e] != 0) atomicAdd(class_counts + e, (u64)L.cc[e]);
}

// THE dispatch rule: a wave owns a structure up to DS_WAVE_PATH_MAX residues, a block beyond
static inline bool ds_wave_path(int R) { return R <= DS_WAVE_PATH_MAX; }

}  // namespace cgv

extern "C" {

int cgv_dssp_max_residues(void) { return cgv::DS_MAX_RESIDUES; }
int cgv_dssp_max_structures(void) { return cgv::DS_MAX_STRUCTURES; }
int cgv_dssp_wave_path_max(void) { return cgv::DS_WAVE_PATH_MAX; }
float cgv_dssp_bend_c2(void) { return cgv::DS_BEND_C2; }

int cgv_dssp_assign(const float* xyz, const int32_t* res, const int32_t* prev, const int32_t* link, int n_structures, int n_atoms,
                    int n_residues, int64_t* class_counts, int32_t* n_class, int32_t* bad, uint8_t* codes, uint64_t* hb_bits,
                    void* stream) {
  const int S = n_structures, R = n_residues;
  CGV_REQUIRE(S >= 0 && n_atoms >= 1, "bad size");
  CGV_REQUIRE(S <= cgv::DS_MAX_STRUCTURES, "structures per launch <= cgv_dssp_max_structures()");
  CGV_REQUIRE(R >= 1, "at least one residue");
  CGV_REQUIRE(R <= cgv::DS_MAX_RESIDUES, "n_residues <= cgv_dssp_max_residues()");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && res && prev && link && class_counts && n_class && bad, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (cgv::ds_wave_path(R)) {
    constexpr int SLOTS = cgv::DS_THREADS / 64;
    const int blocks = (S + SLOTS - 1) / SLOTS < cgv::DS_WAVE_BLOCKS ? (S + SLOTS - 1) / SLOTS : cgv::DS_WAVE_BLOCKS;
    hipLaunchKernelGGL(cgv::dssp_k<64>, dim3((unsigned)blocks), dim3(cgv::DS_THREADS), SLOTS * cgv::ds_slot_bytes(R, true), st, xyz,
                       res, prev, link, S, n_atoms, R, (cgv::u64*)class_counts, n_class, bad, codes, (cgv::u64*)hb_bits);
  } else {
    hipLaunchKernelGGL(cgv::dssp_k<256>, dim3((unsigned)S), dim3(cgv::DS_THREADS), cgv::ds_slot_bytes(R, false), st, xyz, res, prev,
                       link, S, n_atoms, R, (cgv::u64*)class_counts, n_class, bad, codes, (cgv::u64*)hb_bits);
  }
  return cgv::check_launch("cgv_dssp_assign");
}

}  // extern "C"
