// K31 stereochemistry of an ensemble: over S structures, how often every stereocentre is of the negative hand or flat, how
// often every torsion about a bond that does not rotate is cis, how often every bond pierces every ring, and per structure
// the number of centres of the wrong hand, of torsions in the wrong state and of pierced (ring, bond) pairs.  Everything the
// other analyses of a single structure read is a distance, which a mirror image keeps; what is here is not.  See
// include/cgvae_hip.h.  Nothing in the reference computes it (its --reflectiontest mirrors the input, it scores no output).
//
// The tables index the packed structure: sel [P] lists the atoms that the tables name, and every entry of centres, torsions,
// rings and bonds is a PLACE in sel.  In fp32 with every operation rounded on its own (this file is compiled with
// -ffp-contract=off), no fused multiply-add, no square root, no division:
//   x(u, v) = (u.y*v.z - u.z*v.y,  u.z*v.x - u.x*v.z,  u.x*v.y - u.y*v.x)          d(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z
//   centre (c, a, b, d)     V = d(a - c, x(b - c, d - c))                        negative: V < 0     flat: V == 0
//   torsion (i, j, k, l)    X = d(x(j - i, k - j), x(k - j, l - k))              cis: X > 0
//   ring v_0 .. v_{k-1}, 3 <= k <= 8 (padded with -1), against the bond (p0, p1):
//     g = (((v_0 + v_1) + v_2) + ...) * fp32(1 / k)       dir = p1 - p0       tvec = p0 - g
//     for t = 0 .. k - 1, the triangle (g, v_t, v_{t+1 mod k}):   e1 = v_t - g   e2 = v_{t+1} - g
//       pv = x(dir, e2)   det = d(e1, pv)   u' = d(tvec, pv)   q = x(tvec, e1)   v' = d(dir, q)   t' = d(e2, q)   w' = u' + v'
//       crossed:  det > 0 and u' >= 0 and v' >= 0 and w' <= det and t' >= 0 and t' <= det
//             or  det < 0 and u' <= 0 and v' <= 0 and w' >= det and t' <= 0 and t' >= det             (det == 0: not crossed)
//     pierced: at least one of the k triangles is crossed (a segment through a fan edge counts once)
// A mirror image negates V, det, u', v', t' and w' exactly and keeps X: it flips every centre and nothing else.  A NaN
// fails every comparison: a centre with a NaN V is neither negative nor flat, a torsion with a NaN X is not cis.  The host
// restates all of it in numpy.float32, so every integer this file produces is exact.  A structure with a non-finite
// coordinate among the atoms of sel is bad: bad[s] = 1, a packed row of NaN, and it enters nothing.
//
// The gather, the slices of the structure axis, the workspace check and the chunk's counters are packed_dev.h's.
// stereo_prep_k    one wave per structure, 4 per block: gather_structure fills the packed copy [S, P + R] float4 of the
//                  workspace; entry P + r is the centre g of ring r, summed from the same coordinates in table order.  bad
//                  and counts [S, 3] = 0 are written here.
// stereo_local_k   256 threads, grid (tiles of 256 centres, then tiles of 256 torsions; slices of the structure axis).  A
//                  lane owns one centre or one torsion with its four places and its counters in registers and reads its
//                  four atoms of every good structure from the packed copy.  The wave's ballot of "wrong" (against want_sign
//                  / want_cis) goes to the chunk's counters, which the block adds to counts once per structure; at the end
//                  a nonzero counter is added to neg / flat / cis.
// stereo_rings_k   256 threads, grid (tiles of 64 bonds, tiles of 16 rings, slices of the structure axis), a rectangular
//                  table like K25's: a lane owns a bond column, wave w the rings 4 w .. 4 w + 3 of the tile, whose 4 counters
//                  a lane keeps in registers.  ST_CHUNK structures at a time go through LDS as float4: 9 entries a ring (its
//                  vertices and g: the same address in every lane) and the two ends of the 64 bonds (one ds_read_b128 per
//                  lane each); where an entry comes from in a packed structure is worked out once per block.  A ring whose
//                  word of `tested` has no bit among the wave's bonds is skipped; there is NO geometric pre-filter: every
//                  tested pair gets the full fan.  The wave's ballot of `pierced`, ANDed with the tested bits, is counted
//                  per lane and by popcount into the chunk's counters.
// Sums of integers meet in atomicAdd (LDS and global), whose order does not matter: two runs give the same bits, and nothing
// depends on how the caller cuts the structures into launches or struct_slices cuts a launch into slices.
#include <math.h>

#include "packed_dev.h"

namespace cgv {

constexpr int ST_RING = 8;                   // vertices of a ring at the most: the width of the ring table
constexpr int ST_SLOT = ST_RING + 1;         // staged float4 of a ring: its vertices, then g
constexpr int ST_ITEMS = 256;                // centres or torsions of a block of the light pass: one per thread
constexpr int ST_WAVES = 4;
constexpr int ST_RPW = 4;                    // rings of a wave: the counters a lane keeps in registers
constexpr int ST_ROWS = ST_WAVES * ST_RPW;   // rings of a tile
constexpr int ST_COLS = 64;                  // bonds of a tile: the lanes of a wave, two words of `tested`
constexpr int ST_CHUNK = 8;                  // structures staged at once: 8 x 272 x 16 B = 34 KB of LDS, 4 blocks per CU
constexpr int ST_STAGE = ST_ROWS * ST_SLOT + 2 * ST_COLS;   // float4 of a staged structure
constexpr int ST_MAX_ATOMS = 32768;          // places of sel
constexpr int ST_MAX_CENTRES = 65536;
constexpr int ST_MAX_TORSIONS = 65536;
constexpr int ST_MAX_RINGS = 2048;
constexpr int ST_MAX_BONDS = 32768;          // with ST_MAX_RINGS: pierced [R, B] int32 is 256 MB there
constexpr int ST_MAX_STRUCTURES = 1 << 20;   // per launch

struct v3 { float x, y, z; };
__device__ __forceinline__ v3 sub3(const float4& a, const float4& b) { return {__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)}; }
__device__ __forceinline__ v3 cross3(const v3& u, const v3& v) {
  return {__fsub_rn(__fmul_rn(u.y, v.z), __fmul_rn(u.z, v.y)), __fsub_rn(__fmul_rn(u.z, v.x), __fmul_rn(u.x, v.z)),
          __fsub_rn(__fmul_rn(u.x, v.y), __fmul_rn(u.y, v.x))};
}
__device__ __forceinline__ float dot3(const v3& u, const v3& v) {
  return __fadd_rn(__fadd_rn(__fmul_rn(u.x, v.x), __fmul_rn(u.y, v.y)), __fmul_rn(u.z, v.z));
}
// the segment (p0, p0 + dir), tvec = p0 - g, against the triangle (g, g + e1, g + e2): the header's comparisons
__device__ __forceinline__ bool fan_crossed(const v3& dir, const v3& tvec, const v3& e1, const v3& e2) {
  const v3 pv = cross3(dir, e2);
  const float det = dot3(e1, pv), up = dot3(tvec, pv);
  const v3 q = cross3(tvec, e1);
  const float vp = dot3(dir, q), tp = dot3(e2, q), wp = __fadd_rn(up, vp);
  const bool pos = det > 0.f && up >= 0.f && vp >= 0.f && wp <= det && tp >= 0.f && tp <= det;
  const bool neg = det < 0.f && up <= 0.f && vp <= 0.f && wp >= det && tp <= 0.f && tp >= det;
  return pos || neg;
}
// the atoms of a ring's row (the entries before the first -1); 0 for fewer than 3: such a ring has no fan
__host__ __device__ __forceinline__ int ring_size(const int* __restrict__ ring) {
  int k = 0;
  while (k < ST_RING && ring[k] >= 0) ++k;
  return k >= 3 ? k : 0;
}
// fp32(1 / k): the constant that turns a ring's vertex sum into g
__device__ __forceinline__ float ring_inv(int k) {
  constexpr float inv[ST_RING + 1] = {0.f, 1.f, 1.f / 2.f, 1.f / 3.f, 1.f / 4.f, 1.f / 5.f, 1.f / 6.f, 1.f / 7.f, 1.f / 8.f};
  return inv[k];
}

// grid: 4 structures per block
__global__ __launch_bounds__(256) void stereo_prep_k(const float* __restrict__ xyz, const int* __restrict__ sel,
                                                     const int* __restrict__ rings, int S, int n, int P, int R,
                                                     float4* __restrict__ packed, int* __restrict__ bad, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (s >= S) return;                                        // whole waves leave
  const int W = P + R;
  float4* row = packed + (size_t)s * W;
  const float* base = xyz + (size_t)s * n * 3;
  const bool is_bad = !gather_structure(base, [=](int k) { return sel[k]; }, n, P, row, lane);
  for (int r = lane; r < R; r += 64) {                       // from the coordinates themselves: another lane packed them
    const int* ring = rings + (size_t)r * ST_RING;
    const int k = ring_size(ring);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int t = 0; t < k; ++t) {
      const f3 p = ld3(base + 3 * (size_t)sel_atom(sel[sel_atom(ring[t], P)], n));
      if (t == 0) gx = p.x, gy = p.y, gz = p.z;
      else gx = __fadd_rn(gx, p.x), gy = __fadd_rn(gy, p.y), gz = __fadd_rn(gz, p.z);
    }
    const float inv = ring_inv(k);
    row[P + r] = make_float4(__fmul_rn(gx, inv), __fmul_rn(gy, inv), __fmul_rn(gz, inv), 0.f);
  }
  if (is_bad) poison_row(row, W, lane);
  if (lane == 0) bad[s] = is_bad ? 1 : 0;
  if (lane < 3) counts[(size_t)s * 3 + lane] = 0;
}

// grid: x = tile of 256 centres (the first tiles_c) or of 256 torsions, z = slice of the structure axis (`per` structures
// each, a multiple of ST_CHUNK)
__global__ __launch_bounds__(256) void stereo_local_k(const float4* __restrict__ packed, const int* __restrict__ bad,
                                                      const int* __restrict__ centres, const int* __restrict__ torsions,
                                                      const int* __restrict__ want_sign, const int* __restrict__ want_cis, int S,
                                                      int W, int P, int C, int Q, int tiles_c, int per,
                                                      unsigned long long* __restrict__ neg, unsigned long long* __restrict__ flat,
                                                      unsigned long long* __restrict__ cis, int* __restrict__ counts) {
  __shared__ ChunkCounts<int, ST_CHUNK, 3> wrong;            // per structure: wrong centres, wrong torsions, (pierced pairs)
  const int tid = threadIdx.x, lane = tid & 63;
  const bool is_c = (int)blockIdx.x < tiles_c;               // the same for the whole block
  const int item = ((int)blockIdx.x - (is_c ? 0 : tiles_c)) * ST_ITEMS + tid;
  const bool live = item < (is_c ? C : Q);
  const int* want_tab = is_c ? want_sign : want_cis;
  int at[4] = {0, 0, 0, 0}, want = 0;
  if (live) {
    const int* q = (is_c ? centres : torsions) + (size_t)item * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) at[u] = sel_atom(q[u], P);
    if (want_tab != nullptr) want = want_tab[item];
  }
  int n0 = 0, n1 = 0;                                        // negative and flat, or cis: over the slice
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += ST_CHUNK) {
    __syncthreads();                                         // the previous chunk's counters have been flushed
    wrong.zero(tid);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < ST_CHUNK; ++sl) {
      if (s0 + sl >= s_end) break;                           // the same for the whole block
      if (bad[s0 + sl] != 0) continue;                       // likewise
      bool w = false;
      if (live) {
        const float4* row = packed + (size_t)(s0 + sl) * W;
        const float4 a0 = row[at[0]], a1 = row[at[1]], a2 = row[at[2]], a3 = row[at[3]];
        if (is_c) {
          const float V = dot3(sub3(a1, a0), cross3(sub3(a2, a0), sub3(a3, a0)));
          const bool ng = V < 0.f, fl = V == 0.f;
          n0 += ng ? 1 : 0, n1 += fl ? 1 : 0;
          w = want_tab != nullptr && (ng ? -1 : fl ? 0 : 1) != want;
        } else {
          const v3 b1 = sub3(a1, a0), b2 = sub3(a2, a1), b3 = sub3(a3, a2);
          const bool c = dot3(cross3(b1, b2), cross3(b2, b3)) > 0.f;
          n0 += c ? 1 : 0;
          w = want_tab != nullptr && (c ? 1 : 0) != (want != 0 ? 1 : 0);
        }
      }
      const unsigned long long m = __ballot(w);
      if (lane == 0 && m != 0ull) wrong.add(sl, is_c ? 0 : 1, __popcll(m));
    }
    __syncthreads();
    wrong.flush(s0, s_end, tid, counts);
  }
  if (live) {
    if (is_c) {
      if (n0 != 0) atomicAdd(neg + item, (unsigned long long)n0);
      if (n1 != 0) atomicAdd(flat + item, (unsigned long long)n1);
    } else if (n0 != 0) {
      atomicAdd(cis + item, (unsigned long long)n0);
    }
  }
}

// grid: x = tile of 64 bonds, y = tile of 16 rings, z = slice of the structure axis (`per` structures each, a multiple of ST_CHUNK)
__global__ __launch_bounds__(256) void stereo_rings_k(const float4* __restrict__ packed, const int* __restrict__ bad,
                                                      const int* __restrict__ rings, const int* __restrict__ bonds,
                                                      const uint32_t* __restrict__ tested, int S, int W, int P, int R, int B,
                                                      int words, int per, int* __restrict__ pierced, int* __restrict__ counts) {
  __shared__ float4 st[ST_CHUNK][ST_STAGE];
  __shared__ int where[ST_STAGE];                            // the place of a staged entry in a packed structure; -1: nowhere
  __shared__ int ksz[ST_ROWS];                               // the tile's ring sizes; 0: no ring
  __shared__ int skip[ST_CHUNK];                             // 1: bad, or past the slice
  __shared__ ChunkCounts<int, ST_CHUNK, 3> hits;             // per structure: (wrong centres, wrong torsions,) pierced pairs
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = (int)blockIdx.y * ST_ROWS, c0 = (int)blockIdx.x * ST_COLS, rw = r0 + ST_RPW * wave;
  for (int a = tid; a < ST_STAGE; a += 256) {
    int at = -1;
    if (a < ST_ROWS * ST_SLOT) {
      const int u = a / ST_SLOT, t = a - u * ST_SLOT, r = r0 + u;
      if (r < R) {
        const int k = ring_size(rings + (size_t)r * ST_RING);
        if (t == ST_RING) at = k != 0 ? P + r : -1;
        else if (t < k) at = sel_atom(rings[(size_t)r * ST_RING + t], P);
      }
    } else {
      const int e = a - ST_ROWS * ST_SLOT, c = c0 + (e & (ST_COLS - 1));
      if (c < B) at = sel_atom(bonds[2 * (size_t)c + (e >> 6)], P);
    }
    where[a] = at;
  }
  if (tid < ST_ROWS) ksz[tid] = r0 + tid < R ? ring_size(rings + (size_t)(r0 + tid) * ST_RING) : 0;
  // bit l of ok[u]: the pair (ring rw + u, bond c0 + l) is looked at -- inside the tables and tested.  The same in every lane.
  const unsigned long long inside = B - c0 >= 64 ? ~0ull : (1ull << (B - c0)) - 1ull;
  unsigned long long ok[ST_RPW];
  int cnt[ST_RPW];
#pragma unroll
  for (int u = 0; u < ST_RPW; ++u) {
    ok[u] = 0ull, cnt[u] = 0;
    if (rw + u < R) {
      const uint32_t* t = tested + (size_t)(rw + u) * words + (c0 >> 5);
      const unsigned long long lo = t[0], hi = (c0 >> 5) + 1 < words ? t[1] : 0u;
      ok[u] = inside & (lo | (hi << 32));
    }
  }
  const int s_begin = (int)blockIdx.z * per, s_end = min(S, s_begin + per);
  for (int s0 = s_begin; s0 < s_end; s0 += ST_CHUNK) {
    __syncthreads();                                         // `where` is written; the previous chunk has been read and flushed
    if (tid < ST_CHUNK) skip[tid] = s0 + tid < s_end && bad[s0 + tid] == 0 ? 0 : 1;
    for (int e = tid; e < ST_CHUNK * ST_STAGE; e += 256) {
      const int sl = e / ST_STAGE, a = e - sl * ST_STAGE, at = where[a];
      float4 v = make_float4(NAN, NAN, NAN, 0.f);            // past the slice or the tables: crosses nothing
      if (s0 + sl < s_end && at >= 0) v = packed[(size_t)(s0 + sl) * W + at];
      st[sl][a] = v;
    }
    hits.zero(tid);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < ST_CHUNK; ++sl) {
      if (skip[sl] != 0) continue;                           // the same for the whole block
      const float4 p0 = st[sl][ST_ROWS * ST_SLOT + lane], p1 = st[sl][ST_ROWS * ST_SLOT + ST_COLS + lane];
      const v3 dir = sub3(p1, p0);
      int np = 0;
#pragma unroll
      for (int u = 0; u < ST_RPW; ++u) {
        if (ok[u] == 0ull) continue;                         // the same in every lane: no pair of this ring and these bonds is tested
        const float4* ring = &st[sl][(ST_RPW * wave + u) * ST_SLOT];
        const int k = ksz[ST_RPW * wave + u];
        const float4 g = ring[ST_RING];
        const v3 tvec = sub3(p0, g);
        v3 e1 = sub3(ring[0], g);
        bool hit = false;
#pragma unroll 1
        for (int t = 0; t < k; ++t) {
          const v3 e2 = sub3(ring[t + 1 == k ? 0 : t + 1], g);
          hit = fan_crossed(dir, tvec, e1, e2) || hit;
          e1 = e2;
        }
        const unsigned long long w = __ballot(hit) & ok[u];  // a padding lane holds NaN and is outside `ok`
        cnt[u] += (int)((w >> lane) & 1ull);
        np += __popcll(w);
      }
      if (lane == 0 && np != 0) hits.add(sl, 2, np);
    }
    __syncthreads();
    hits.flush(s0, s_end, tid, counts);
  }
  if (c0 + lane < B) {
#pragma unroll
    for (int u = 0; u < ST_RPW; ++u)
      if (cnt[u] != 0) atomicAdd(pierced + (size_t)(rw + u) * B + c0 + lane, cnt[u]);      // cnt != 0: rw + u < R
  }
}

static inline bool st_sizes_ok(int S, int P, int R) {
  return S >= 0 && P >= 0 && R >= 0 && S <= ST_MAX_STRUCTURES && P <= ST_MAX_ATOMS && R <= ST_MAX_RINGS;
}
static inline size_t st_workspace(int S, int P, int R) { return (size_t)S * (size_t)(P + R) * sizeof(float4); }

}  // namespace cgv

extern "C" {

int cgv_stereo_max_structures(void) { return cgv::ST_MAX_STRUCTURES; }
int cgv_stereo_max_atoms(void) { return cgv::ST_MAX_ATOMS; }
int cgv_stereo_max_centres(void) { return cgv::ST_MAX_CENTRES; }
int cgv_stereo_max_torsions(void) { return cgv::ST_MAX_TORSIONS; }
int cgv_stereo_max_rings(void) { return cgv::ST_MAX_RINGS; }
int cgv_stereo_max_bonds(void) { return cgv::ST_MAX_BONDS; }
int cgv_stereo_max_ring(void) { return cgv::ST_RING; }
int cgv_stereo_item_tile(void) { return cgv::ST_ITEMS; }
int cgv_stereo_row_tile(void) { return cgv::ST_ROWS; }
int cgv_stereo_col_tile(void) { return cgv::ST_COLS; }
int cgv_stereo_chunk(void) { return cgv::ST_CHUNK; }

size_t cgv_stereo_workspace_bytes(int n_structures, int n_sel, int n_rings) {
  return cgv::st_sizes_ok(n_structures, n_sel, n_rings) ? cgv::st_workspace(n_structures, n_sel, n_rings) : 0;
}

int cgv_stereo_counts(const float* xyz, const int32_t* sel, const int32_t* centres, const int32_t* torsions, const int32_t* rings,
                      const int32_t* bonds, const uint32_t* tested, const int32_t* want_sign, const int32_t* want_cis,
                      int n_structures, int n_atoms, int n_sel, int n_centres, int n_torsions, int n_rings, int n_bonds,
                      int64_t* neg, int64_t* flat, int64_t* cis, int32_t* pierced, int32_t* counts, int32_t* bad, void* workspace,
                      size_t workspace_bytes, void* stream) {
  const int S = n_structures, P = n_sel, C = n_centres, Q = n_torsions, R = n_rings, B = n_bonds;
  CGV_REQUIRE(S >= 0 && n_atoms >= 0 && P >= 0 && C >= 0 && Q >= 0 && R >= 0 && B >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::ST_MAX_STRUCTURES, "structures per launch <= cgv_stereo_max_structures()");
  CGV_REQUIRE(P <= n_atoms, "n_sel <= n_atoms");
  CGV_REQUIRE(P <= cgv::ST_MAX_ATOMS, "n_sel <= cgv_stereo_max_atoms()");
  CGV_REQUIRE(C <= cgv::ST_MAX_CENTRES, "n_centres <= cgv_stereo_max_centres()");
  CGV_REQUIRE(Q <= cgv::ST_MAX_TORSIONS, "n_torsions <= cgv_stereo_max_torsions()");
  CGV_REQUIRE(R <= cgv::ST_MAX_RINGS, "n_rings <= cgv_stereo_max_rings()");
  CGV_REQUIRE(B <= cgv::ST_MAX_BONDS, "n_bonds <= cgv_stereo_max_bonds()");
  CGV_REQUIRE(P >= 1 || (C == 0 && Q == 0 && R == 0 && B == 0), "tables need at least one selected atom");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && counts && bad && (P == 0 || sel), "null pointer");
  CGV_REQUIRE((C == 0 || (centres && neg && flat)) && (Q == 0 || (torsions && cis)), "null pointer");
  CGV_REQUIRE((R == 0 || rings) && (B == 0 || bonds) && (R == 0 || B == 0 || (tested && pierced)), "null pointer");
  const char* why = cgv::workspace_why(workspace, workspace_bytes, cgv::st_workspace(S, P, R), "workspace smaller than cgv_stereo_workspace_bytes()");
  CGV_REQUIRE(P + R == 0 || why == nullptr, why);
  hipStream_t st = (hipStream_t)stream;
  float4* packed = (float4*)workspace;
  hipLaunchKernelGGL(cgv::stereo_prep_k, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, xyz, sel, rings, S, n_atoms, P, R, packed, bad,
                     counts);
  int rc = cgv::check_launch("cgv_stereo_counts (preparation)");
  if (rc) return rc;
  int per;
  if (C + Q > 0) {
    const int tiles_c = (C + cgv::ST_ITEMS - 1) / cgv::ST_ITEMS, tiles_q = (Q + cgv::ST_ITEMS - 1) / cgv::ST_ITEMS;
    const int slices = cgv::struct_slices(S, tiles_c + tiles_q, cgv::ST_CHUNK, &per);
    hipLaunchKernelGGL(cgv::stereo_local_k, dim3((unsigned)(tiles_c + tiles_q), 1u, (unsigned)slices), dim3(256), 0, st,
                       (const float4*)packed, (const int*)bad, centres, torsions, want_sign, want_cis, S, P + R, P, C, Q, tiles_c, per,
                       (unsigned long long*)neg, (unsigned long long*)flat, (unsigned long long*)cis, counts);
    rc = cgv::check_launch("cgv_stereo_counts (centres and torsions)");
    if (rc) return rc;
  }
  if (R > 0 && B > 0) {
    const int cols = (B + cgv::ST_COLS - 1) / cgv::ST_COLS, rows = (R + cgv::ST_ROWS - 1) / cgv::ST_ROWS;
    const int slices = cgv::struct_slices(S, cols * rows, cgv::ST_CHUNK, &per);
    hipLaunchKernelGGL(cgv::stereo_rings_k, dim3((unsigned)cols, (unsigned)rows, (unsigned)slices), dim3(256), 0, st,
                       (const float4*)packed, (const int*)bad, rings, bonds, tested, S, P + R, P, R, B, (B + 31) / 32, per, pierced, counts);
    rc = cgv::check_launch("cgv_stereo_counts (rings)");
  }
  return rc;
}

}  // extern "C"
