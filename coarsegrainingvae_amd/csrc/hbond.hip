// K25 hydrogen bonds of an ensemble (Baker-Hubbard, intramolecular): how often every pair (donor hydrogen, acceptor) of a
// molecule is hydrogen bonded over S structures, per structure the number of bonds and of NATIVE bonds (pairs of a given
// set), and, when asked for, every bond of every structure as a bit.  See include/cgvae_hip.h.  Nothing in the reference
// computes it.
//
// A donor hydrogen is an H bonded to exactly one heavy atom D of a donor element, an acceptor an atom A of an acceptor
// element: the CALLER's tables don_h / don_d [nH] and acc [nA].  A pair (h, a) is excluded when A is D itself, when A is
// bonded to D, or when the caller's mask names it: the CALLER's mask.  In a structure a pair that is not excluded is
// bonded iff, in fp32 with every operation rounded on its own (this file is compiled with -ffp-contract=off),
//   d2  = sq_dist2(A, H)                       (dx*dx + dy*dy) + dz*dz of A - H, csrc/sq_dist.h
//   l2  = sq_dist2(D, H)
//   dot = (ux*vx + uy*vy) + uz*vz              u = D - H, v = A - H
//   d2 < cutoff2  and  dot < 0  and  dot*dot > (c2 * l2) * d2
// with c2 = fp32(cos(angle)^2) of the minimum D-H...A angle in [90, 180) degrees -- there cos(angle) <= 0, so the last two
// tests are cos(D-H-A) < cos(angle) without a square root or a division.  The host restates the test bit for bit, so every
// integer this file produces is exact.  A structure with a non-finite coordinate among its D, H or A atoms is bad.
//
// hbond_prep_k    one wave per structure, 4 per block: packed_dev.h's gather_structure with the index (don_h | don_d | acc)
//                 fills the packed copy [S, 2 nH + nA] float4 of the workspace (H rows, then D rows, then acceptors), what
//                 the pair kernel streams.  A bad structure gets n_hbonds = n_native = -1 and a packed row of NaN, which
//                 bonds with nothing: the pair kernel need not know of it.
// hbond_pairs_k   256 threads, grid (words of 64 acceptors, row tiles of 32 hydrogens, slices of the structure axis).  A
//                 lane owns an acceptor column, wave w the rows 8 w .. 8 w + 7 of the tile, whose 8 counters a lane keeps in
//                 registers.  HB_CHUNK structures at a time go through LDS as float4 (staged here, not by stage_chunk: a
//                 tile has three ranges of the packed row, not two): a lane's acceptor is one ds_read_b128, H and D of a
//                 row are the same address in every lane.  The wave's ballot of the predicate, ANDed with the row's word
//                 of pairs that count, IS the word of `bits`; its popcount goes to the chunk's counters (packed_dev.h:
//                 ChunkCounts), which the block adds to n_hbonds / n_native once per structure.  At the end a nonzero
//                 counter is added to pair_counts.
// Sums of integers meet in atomicAdd, whose order does not matter, and every word of `bits` has one writer: two runs give the
// same bits, and nothing depends on how the caller cuts the structures into launches.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr int HB_WAVES = 4;                  // waves of a block
constexpr int HB_RPW = 8;                    // rows of a wave: the counters a lane keeps in registers
constexpr int HB_ROWS = HB_WAVES * HB_RPW;   // rows (donor hydrogens) of a tile
constexpr int HB_COLS = 64;                  // columns (acceptors) of a tile: the lanes of a wave, one word of the masks
constexpr int HB_CHUNK = 8;                  // structures staged at once: 8 x 128 x 16 B = 16 KB of LDS
constexpr int HB_STAGE = 2 * HB_ROWS + HB_COLS;   // float4 of a staged structure: H rows, D rows, acceptors
constexpr int HB_MAX_HYDROGENS = 4096;
constexpr int HB_MAX_ACCEPTORS = 4096;
constexpr int HB_MAX_STRUCTURES = 1 << 20;   // per launch

__global__ __launch_bounds__(256) void hbond_prep_k(const float* __restrict__ xyz, const int* __restrict__ don_h,
                                                    const int* __restrict__ don_d, const int* __restrict__ acc, int S, int n,
                                                    int nH, int nA, float4* __restrict__ packed, int* __restrict__ bad,
                                                    int* __restrict__ n_hbonds, int* __restrict__ n_native) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  const int P = 2 * nH + nA;
  float4* row = packed + (size_t)s * P;
  const auto at = [=](int k) { return k < nH ? don_h[k] : k < 2 * nH ? don_d[k - nH] : acc[k - 2 * nH]; };
  const bool is_bad = !gather_structure(xyz + (size_t)s * n * 3, at, n, P, row, lane);
  if (is_bad) poison_row(row, P, lane);
  if (lane == 0) {
    bad[s] = is_bad ? 1 : 0;
    n_hbonds[s] = is_bad ? -1 : 0;
    n_native[s] = is_bad ? -1 : 0;
  }
}

// grid: x = word of acceptors, y = row tile, z = slice of the structure axis (`per` structures each, a multiple of HB_CHUNK)
__global__ __launch_bounds__(256) void hbond_pairs_k(const float4* __restrict__ packed, const unsigned long long* __restrict__ excl,
                                                     const unsigned long long* __restrict__ native, int S, int nH, int nA,
                                                     int words, int per, float cutoff2, float c2,
                                                     unsigned long long* __restrict__ pair_counts, int* __restrict__ n_hbonds,
                                                     int* __restrict__ n_native, unsigned long long* __restrict__ bits) {
  __shared__ float4 st[HB_CHUNK][HB_STAGE];
  __shared__ ChunkCounts<int, HB_CHUNK, 2> hits;             // per structure: bonds, native bonds
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int word = (int)blockIdx.x, r0 = (int)blockIdx.y * HB_ROWS, c0 = word * HB_COLS;
  const int P = 2 * nH + nA, rw = r0 + HB_RPW * wave;        // the first of this wave's rows
  // bit l of ok[u]: the pair (rw + u, c0 + l) counts -- inside the table and not excluded.  The same in every lane.
  const unsigned long long inside = nA - c0 >= 64 ? ~0ull : (1ull << (nA - c0)) - 1ull;
  unsigned long long ok[HB_RPW], nat[HB_RPW];
#pragma unroll
  for (int u = 0; u < HB_RPW; ++u) {
    ok[u] = nat[u] = 0ull;
    if (rw + u < nH) {
      ok[u] = inside & ~excl[(size_t)(rw + u) * words + word];
      if (native != nullptr) nat[u] = ok[u] & native[(size_t)(rw + u) * words + word];
    }
  }
  int cnt[HB_RPW];
#pragma unroll
  for (int u = 0; u < HB_RPW; ++u) cnt[u] = 0;
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += HB_CHUNK) {
    __syncthreads();                                         // the previous chunk has been read and its hits flushed
    for (int e = tid; e < HB_CHUNK * HB_STAGE; e += 256) {
      const int sl = e / HB_STAGE, a = e - sl * HB_STAGE;
      int at = -1;                                           // where the entry is in a packed structure; -1: nowhere
      if (a < HB_ROWS) at = r0 + a < nH ? r0 + a : -1;
      else if (a < 2 * HB_ROWS) at = r0 + a - HB_ROWS < nH ? nH + r0 + a - HB_ROWS : -1;
      else at = c0 + a - 2 * HB_ROWS < nA ? 2 * nH + c0 + a - 2 * HB_ROWS : -1;
      float4 v = make_float4(NAN, NAN, NAN, 0.f);            // past the slice or the table: bonded to nothing
      if (s0 + sl < s_end && at >= 0) v = packed[(size_t)(s0 + sl) * P + at];
      st[sl][a] = v;
    }
    hits.zero(tid);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < HB_CHUNK; ++sl) {
      if (s0 + sl >= s_end) break;                           // the same for the whole block
      const float4 a = st[sl][2 * HB_ROWS + lane];
      int nh = 0, nn = 0;
#pragma unroll
      for (int u = 0; u < HB_RPW; ++u) {
        const float4 h = st[sl][HB_RPW * wave + u], d = st[sl][HB_ROWS + HB_RPW * wave + u];
        const float vx = __fsub_rn(a.x, h.x), vy = __fsub_rn(a.y, h.y), vz = __fsub_rn(a.z, h.z);
        const float ux = __fsub_rn(d.x, h.x), uy = __fsub_rn(d.y, h.y), uz = __fsub_rn(d.z, h.z);
        const float d2 = sq_dist2(a.x, a.y, a.z, h.x, h.y, h.z), l2 = sq_dist2(d.x, d.y, d.z, h.x, h.y, h.z);
        const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy)), __fmul_rn(uz, vz));
        const bool bond = d2 < cutoff2 && dot < 0.f && __fmul_rn(dot, dot) > __fmul_rn(__fmul_rn(c2, l2), d2);
        const unsigned long long w = __ballot(bond) & ok[u];  // a padding lane or row holds NaN and is outside `ok`
        cnt[u] += (int)((w >> lane) & 1ull);
        nh += __popcll(w);
        nn += __popcll(w & nat[u]);
        if (bits != nullptr && lane == 0 && rw + u < nH) bits[((size_t)(s0 + sl) * nH + (rw + u)) * words + word] = w;
      }
      if (lane == 0) {
        if (nh != 0) hits.add(sl, 0, nh);
        if (nn != 0) hits.add(sl, 1, nn);
      }
    }
    __syncthreads();
    hits.flush(s0, s_end, tid, n_hbonds, n_native);
  }
  if (c0 + lane < nA) {
#pragma unroll
    for (int u = 0; u < HB_RPW; ++u)
      if (cnt[u] != 0) atomicAdd(pair_counts + (size_t)(rw + u) * nA + c0 + lane, (unsigned long long)cnt[u]);   // cnt != 0: rw + u < nH
  }
}

static inline size_t hb_workspace(int S, int nH, int nA) { return (size_t)S * (size_t)(2 * nH + nA) * sizeof(float4); }

}  // namespace cgv

extern "C" {

int cgv_hbond_max_structures(void) { return cgv::HB_MAX_STRUCTURES; }
int cgv_hbond_max_hydrogens(void) { return cgv::HB_MAX_HYDROGENS; }
int cgv_hbond_max_acceptors(void) { return cgv::HB_MAX_ACCEPTORS; }
int cgv_hbond_row_tile(void) { return cgv::HB_ROWS; }
int cgv_hbond_chunk(void) { return cgv::HB_CHUNK; }

size_t cgv_hbond_workspace_bytes(int n_structures, int n_hydrogens, int n_acceptors) {
  if (n_structures < 0 || n_hydrogens < 0 || n_acceptors < 0 || n_structures > cgv::HB_MAX_STRUCTURES ||
      n_hydrogens > cgv::HB_MAX_HYDROGENS || n_acceptors > cgv::HB_MAX_ACCEPTORS)
    return 0;
  return cgv::hb_workspace(n_structures, n_hydrogens, n_acceptors);
}

int cgv_hbond_counts(const float* xyz, const int32_t* don_h, const int32_t* don_d, const int32_t* acc, const uint64_t* excluded,
                     const uint64_t* native, int n_structures, int n_atoms, int n_hydrogens, int n_acceptors, float cutoff2,
                     float c2, int64_t* pair_counts, int32_t* n_hbonds, int32_t* n_native, int32_t* bad, uint64_t* bits,
                     void* workspace, size_t workspace_bytes, void* stream) {
  const int S = n_structures, nH = n_hydrogens, nA = n_acceptors;
  CGV_REQUIRE(S >= 0 && n_atoms >= 1, "bad size");
  CGV_REQUIRE(S <= cgv::HB_MAX_STRUCTURES, "structures per launch <= cgv_hbond_max_structures()");
  CGV_REQUIRE(nH >= 1 && nA >= 1, "at least one donor hydrogen and one acceptor");
  CGV_REQUIRE(nH <= cgv::HB_MAX_HYDROGENS, "n_hydrogens <= cgv_hbond_max_hydrogens()");
  CGV_REQUIRE(nA <= cgv::HB_MAX_ACCEPTORS, "n_acceptors <= cgv_hbond_max_acceptors()");
  CGV_REQUIRE(cutoff2 >= 0.f && cutoff2 <= 3.0e38f, "cutoff2 must be a finite number >= 0");
  CGV_REQUIRE(c2 >= 0.f && c2 <= 1.f, "c2 must be the squared cosine of an angle in [90, 180) degrees");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && don_h && don_d && acc && excluded && pair_counts && n_hbonds && n_native && bad, "null pointer");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::hb_workspace(S, nH, nA), "workspace smaller than cgv_hbond_workspace_bytes()");
  CGV_REQUIRE(why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::hbond_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, don_h, don_d, acc, S, n_atoms, nH, nA,
                     packed, bad, n_hbonds, n_native);
  const int rc = cgv::check_launch("cgv_hbond_counts (preparation)");
  if (rc) return rc;
  const int words = (nA + 63) / 64, tiles = (nH + cgv::HB_ROWS - 1) / cgv::HB_ROWS;
  int per;
  const int slices = cgv::struct_slices(S, words * tiles, cgv::HB_CHUNK, &per);
  hipLaunchKernelGGL(cgv::hbond_pairs_k, dim3((unsigned)words, (unsigned)tiles, (unsigned)slices), dim3(256), 0, st, packed,
                     (const unsigned long long*)excluded, (const unsigned long long*)native, S, nH, nA, words, per, cutoff2, c2,
                     (unsigned long long*)pair_counts, n_hbonds, n_native, (unsigned long long*)bits);
  return cgv::check_launch("cgv_hbond_counts");
}

}  // extern "C"
