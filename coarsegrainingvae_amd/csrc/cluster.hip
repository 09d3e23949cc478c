// K24 clustering of an ensemble by superposed RMSD (Daura et al., "GROMOS"; the default of `gmx cluster -method gromos`):
// the dense squared RMSDs of K17 (cgv_superpose, `dense`) become a bit-packed neighbour matrix, and the greedy loop --
// take the structure with most neighbours, remove it and them, repeat -- runs on the device.  See include/cgvae_hip.h.
// Nothing in the reference computes it.  Everything here is integer and ordered: two calls give the same bits.
//
// THE GRAPH.  c2 = double(cutoff)^2, computed by the caller.  For p < q, adj(p, q) = adj(q, p) = (d2(p, q) <= c2) with
// d2(p, q) the value K17 wrote for row p, column q: only the UPPER triangle decides (the transposed pair may differ in its
// last bits, and the loop below needs a symmetric graph).  adj(p, p) = (d2(p, p) == d2(p, p)): a structure is good iff its
// diagonal is not NaN.  NaN compares false, so a bad structure has an empty row and an empty column.
// bits [S, W] uint64, W = ceil(S / 64): bit (q & 63) of word q >> 6 of row p is adj(p, q); bits at columns >= S are 0.
//
// cluster_pack_k   grid (column tiles, row tiles) x 256 threads, one 64 x 64 tile of one dense rectangle [sa, sb] of the
//                  chunk pair (off_a <= off_b, multiples of 64).  A wave reads 64 consecutive doubles of a row, ballots the
//                  comparison, lane 0 writes the word of row off_a + i and keeps it in LDS: the tile as 64 words.  The
//                  mirrored word of row off_b + j is bit j of the 64 staged words, balloted again -- reads of `dense` stay
//                  coalesced, and the lower triangle never reads a transposed double.  In the diagonal chunk the tiles
//                  below the diagonal leave at once, and the diagonal tile takes T[min(i, j)][max(i, j)] from the staged
//                  words.  Every word of `bits` has exactly one owner: no atomics, no word written twice.
// cluster_gromos_k one workgroup of 1024 threads; all loop state lives in LDS: `alive` (S bits), `members` (S bits),
//                  count[i] = popcount(row_i & alive) (int32; INT_MIN for a structure that is not alive).  An iteration:
//                  (1) the centre c = the alive structure of largest count, lowest index on ties -- one 64-bit key
//                  (count, ~index) per thread, a wave reduction and 16 partials; (2) members = row_c & alive, plus c
//                  whatever its diagonal bit says; label, centre, size are written and the members leave `alive`;
//                  (3) for every removed r a wave walks row_r & alive 64 words at a time and lane b decrements
//                  count[64 w + b] for the set bits of word w with an integer LDS atomic (consecutive addresses) -- exact
//                  because the matrix is symmetric; no row is ever recounted.  The loop is a `for` of at most S
//                  iterations that leaves when nothing is alive, and an iteration removes at least its centre: a
//                  malformed matrix gives wrong clusters, never a hang.  Once the largest count is 1 and every alive
//                  structure has its diagonal bit, what is left are singletons in ascending order: one pass assigns them.
#include <limits.h>

#include "cgv_common.h"

namespace cgv {

constexpr int CL_THREADS = 1024;
constexpr int CL_WAVES = CL_THREADS / WAVE;
constexpr size_t CL_LDS_CU = 160 * 1024;     // the LDS of a CU, all of which one workgroup may take

// dynamic LDS of cluster_gromos_k, in this order: alive [W] u64 | members [W] u64 | partial keys [CL_WAVES] u64 |
// count [64 W] i32 | n_alive, size of the cluster, "an alive structure lacks its diagonal bit", spare: 4 i32
__host__ __device__ constexpr size_t cl_lds_bytes(long long S) {
  return (size_t)((S + 63) / 64) * (8 + 8 + 64 * 4) + CL_WAVES * 8 + 4 * 4;
}
// what the LDS holds: the largest power of two whose state fits (int32 counts, two masks, the reduction scratch)
constexpr int cl_max_structures() {
  long long s = 64;
  while (cl_lds_bytes(2 * s) <= CL_LDS_CU) s *= 2;
  return (int)s;
}
constexpr int CL_MAX_STRUCTURES = cl_max_structures();
static_assert(CL_MAX_STRUCTURES == 32768, "128 KiB of counts, 8 KiB of masks and the scratch are what fits 160 KiB");

__host__ __device__ constexpr size_t cl_bits_bytes(long long S) { return (size_t)S * (size_t)((S + 63) / 64) * 8; }

// ----------------------------------------------------------------------------------------------------------- pack
__global__ __launch_bounds__(256) void cluster_pack_k(const double* __restrict__ dense, int sa, int sb, int off_a, int off_b,
                                                      int W, double c2, unsigned long long* __restrict__ bits) {
  __shared__ unsigned long long tile[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jw = blockIdx.x, iw = blockIdx.y;
  const bool diag_chunk = off_a == off_b;
  if (diag_chunk && iw > jw) return;                          // the whole block: its words are the mirror of tile (jw, iw)
  const bool diag_tile = diag_chunk && iw == jw;
  const int j = jw * 64 + lane;
  for (int r = wave; r < 64; r += 4) {
    const int i = iw * 64 + r;
    bool in = false;
    if (i < sa && j < sb) {
      const double d = dense[(size_t)i * sb + j];
      in = (diag_tile && lane == r) ? d == d : d <= c2;       // NaN compares false
    }
    const unsigned long long word = __ballot(in);
    if (lane == 0) {
      tile[r] = word;
      if (!diag_tile && i < sa) bits[(size_t)(off_a + i) * W + (off_b >> 6) + jw] = word;
    }
  }
  __syncthreads();
  const unsigned long long mine = tile[lane];                 // the staged word of row `lane` of the tile
  for (int r = wave; r < 64; r += 4) {
    if (diag_tile) {                                          // row r: columns above r from its own word, below from theirs
      const unsigned long long own = tile[r];
      const bool in = lane >= r ? ((own >> lane) & 1ull) != 0 : ((mine >> r) & 1ull) != 0;
      const unsigned long long word = __ballot(in);
      if (lane == 0 && iw * 64 + r < sa) bits[(size_t)(off_a + iw * 64 + r) * W + (off_a >> 6) + iw] = word;
    } else {                                                  // the mirror: row off_b + column r of the tile
      const unsigned long long word = __ballot(((mine >> r) & 1ull) != 0);
      if (lane == 0 && jw * 64 + r < sb) bits[(size_t)(off_b + jw * 64 + r) * W + (off_a >> 6) + iw] = word;
    }
  }
}

// --------------------------------------------------------------------------------------------------------- gromos
extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];

__device__ __forceinline__ unsigned long long cl_key(int count, int index) {   // larger count first, then the lower index
  return ((unsigned long long)((unsigned)count ^ 0x80000000u) << 32) | (unsigned long long)(0xffffffffu - (unsigned)index);
}

__global__ __launch_bounds__(CL_THREADS) void cluster_gromos_k(const unsigned long long* __restrict__ bits,
                                                               const unsigned long long* __restrict__ good, int S, int W,
                                                               int* __restrict__ label, int* __restrict__ centre,
                                                               int* __restrict__ size, int* __restrict__ n_clusters) {
  unsigned long long* alive = reinterpret_cast<unsigned long long*>(cl_smem);
  unsigned long long* members = alive + W;
  unsigned long long* part = members + W;
  int* count = reinterpret_cast<int*>(part + CL_WAVES);
  int* misc = count + 64 * W;                                 // [0] n_alive  [1] size of this cluster  [2] diagonal missing
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if (tid < 4) misc[tid] = 0;
  for (int i = tid; i < S; i += CL_THREADS) label[i] = -1, centre[i] = -1, size[i] = 0;
  __syncthreads();
  // alive = the good structures (the caller's mask, else the diagonal); a wave's 64 structures are one word
  for (int i0 = wave * 64; i0 < 64 * W; i0 += CL_THREADS) {
    const int i = i0 + lane;
    const bool dg = i < S && ((bits[(size_t)i * W + (i >> 6)] >> (i & 63)) & 1ull) != 0;
    const bool ok = good == nullptr ? dg : (i < S && ((good[i >> 6] >> (i & 63)) & 1ull) != 0);
    const unsigned long long word = __ballot(ok), lacks = __ballot(ok && !dg);
    if (lane == 0) {
      alive[i0 >> 6] = word;
      members[i0 >> 6] = 0ull;
      if (word != 0ull) atomicAdd(&misc[0], __popcll(word));
      if (lacks != 0ull) atomicOr(&misc[2], 1);
    }
  }
  __syncthreads();
  // count[r] = popcount(row_r & alive), a wave per row
  for (int r = wave; r < 64 * W; r += CL_WAVES) {
    const bool is_alive = r < S && ((alive[r >> 6] >> (r & 63)) & 1ull) != 0;   // uniform in the wave
    int c = 0;
    if (is_alive) {
#pragma unroll 4
      for (int w = lane; w < W; w += 64) c += __popcll(bits[(size_t)r * W + w] & alive[w]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    }
    if (lane == 0) count[r] = is_alive ? c : INT_MIN;
  }
  __syncthreads();
  int n_alive = misc[0];
  const bool all_diagonal = misc[2] == 0;
  int k = 0;

  for (int it = 0; it < S; ++it) {                            // at most S iterations: each removes at least its centre
    if (n_alive <= 0) break;                                  // uniform
    // (1) the centre
    unsigned long long best = 0ull;                           // below every key of an alive structure
    for (int i = tid; i < S; i += CL_THREADS) {
      const unsigned long long key = cl_key(count[i], i);
      best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long other = __shfl_xor(best, off);
      best = other > best ? other : best;
    }
    if (lane == 0) part[wave] = best;
    if (tid == 0) misc[1] = 0;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < CL_WAVES; ++v) best = part[v] > best ? part[v] : best;
    const int c = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
    const int most = (int)((unsigned)(best >> 32) ^ 0x80000000u);
    if (most == INT_MIN || c < 0 || c >= S) break;            // cannot happen while n_alive > 0; never index with it

    if (most <= 1 && all_diagonal) {
      // every alive structure has only itself left: singletons in ascending order, cluster k + its rank among the alive
      for (int w = tid; w < W; w += CL_THREADS) {
        unsigned long long word = alive[w];
        if (word == 0ull) continue;
        int at = k;
        for (int v = 0; v < w; ++v) at += __popcll(alive[v]);
        while (word != 0ull) {
          const int i = w * 64 + __builtin_ctzll(word);
          word &= word - 1ull;
          if (at < S) label[i] = at, centre[at] = i, size[at] = 1;
          ++at;
        }
      }
      k += n_alive;
      n_alive = 0;
      break;                                                  // uniform: `most` and the flag are the same in every thread
    }

    // (2) its members leave
    int mine = 0;
    for (int w = tid; w < W; w += CL_THREADS) {
      const unsigned long long live = alive[w];
      unsigned long long word = bits[(size_t)c * W + w] & live;
      if (w == (c >> 6)) word |= 1ull << (c & 63);            // c is alive, whatever its diagonal bit says
      members[w] = word;
      alive[w] = live & ~word;
      mine += __popcll(word);
      while (word != 0ull) {
        const int i = w * 64 + __builtin_ctzll(word);
        word &= word - 1ull;
        label[i] = k;
        count[i] = INT_MIN;
      }
    }
    if (W > 64 || wave == 0) {                                // waves that own no word have nothing to add
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
      if (lane == 0 && mine != 0) atomicAdd(&misc[1], mine);
    }
    __syncthreads();
    const int removed = misc[1];
    if (tid == 0) centre[k] = c, size[k] = removed;
    n_alive -= removed;
    ++k;

    // (3) the counts of the neighbours that stay, one removed structure per wave in turn
    if (n_alive > 0) {
      int turn = 0;                                           // the same in every thread: all read the same masks
      for (int m0 = 0; m0 < W; m0 += 64) {
        const unsigned long long mw = m0 + lane < W ? members[m0 + lane] : 0ull;
        unsigned long long some = __ballot(mw != 0ull);
        while (some != 0ull) {
          const int t = __builtin_ctzll(some);
          some &= some - 1ull;
          unsigned long long rows = __shfl(mw, t);
          while (rows != 0ull) {
            const int r = (m0 + t) * 64 + __builtin_ctzll(rows);
            rows &= rows - 1ull;
            if ((turn++ & (CL_WAVES - 1)) != wave) continue;
            for (int w0 = 0; w0 < W; w0 += 64) {
              const int w = w0 + lane;
              const unsigned long long word = w < W ? bits[(size_t)r * W + w] & alive[w] : 0ull;
              unsigned long long any = __ballot(word != 0ull);
              while (any != 0ull) {
                const int u = __builtin_ctzll(any);
                any &= any - 1ull;
                const unsigned long long nb = __shfl(word, u);
                if (((nb >> lane) & 1ull) != 0) atomicSub(&count[(w0 + u) * 64 + lane], 1);
              }
            }
          }
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) *n_clusters = k;
}

}  // namespace cgv

extern "C" {

int cgv_cluster_max_structures(void) { return cgv::CL_MAX_STRUCTURES; }

size_t cgv_cluster_workspace_bytes(int n_structures, int chunk) {
  if (n_structures < 0 || chunk < 1 || n_structures > cgv::CL_MAX_STRUCTURES || chunk > cgv::CL_MAX_STRUCTURES) return 0;
  const size_t side = (size_t)((chunk + 63) & ~63);
  return cgv::cl_bits_bytes(n_structures) + side * side * sizeof(double);
}

int cgv_cluster_pack(const double* dense, int sa, int sb, int off_a, int off_b, int n_structures, double c2, uint64_t* bits,
                     void* stream) {
  const int S = n_structures;
  CGV_REQUIRE(S >= 0 && S <= cgv::CL_MAX_STRUCTURES, "0 <= n_structures <= cgv_cluster_max_structures()");
  CGV_REQUIRE(sa >= 0 && sb >= 0 && off_a >= 0 && off_b >= 0, "bad size");
  CGV_REQUIRE((off_a & 63) == 0 && (off_b & 63) == 0, "chunk offsets must be multiples of 64");
  CGV_REQUIRE(off_a <= off_b, "off_a <= off_b: the upper triangle decides");
  CGV_REQUIRE(off_a <= S - sa && off_b <= S - sb, "a chunk ends beyond n_structures");
  CGV_REQUIRE(off_a == off_b ? sa == sb : off_a + sa <= off_b, "the chunks must be the same one or apart");
  CGV_REQUIRE(((sa & 63) == 0 || off_a + sa == S) && ((sb & 63) == 0 || off_b + sb == S),
              "only the last chunk may be no multiple of 64");
  CGV_REQUIRE(!(c2 != c2), "c2 is NaN");
  if (sa == 0 || sb == 0) return 0;
  CGV_REQUIRE(dense && bits, "null pointer");
  const int W = (S + 63) / 64;
  hipLaunchKernelGGL(cgv::cluster_pack_k, dim3((unsigned)((sb + 63) / 64), (unsigned)((sa + 63) / 64)), dim3(256), 0,
                     (hipStream_t)stream, dense, sa, sb, off_a, off_b, W, c2, (unsigned long long*)bits);
  return cgv::check_launch("cgv_cluster_pack");
}

int cgv_cluster_gromos(const uint64_t* bits, const uint64_t* good, int n_structures, int32_t* label, int32_t* centre,
                       int32_t* size, int32_t* n_clusters, void* stream) {
  const int S = n_structures;
  CGV_REQUIRE(S >= 0 && S <= cgv::CL_MAX_STRUCTURES, "0 <= n_structures <= cgv_cluster_max_structures()");
  CGV_REQUIRE(n_clusters, "null pointer");
  CGV_REQUIRE(S == 0 || (bits && label && centre && size), "null pointer");
  const int W = (S + 63) / 64;
  const size_t lds = cgv::cl_lds_bytes(S);
  static bool attr_done = false;                              // the largest size once: 139 408 of the CU's 163 840 bytes
  if (!attr_done) {
    const size_t most = cgv::cl_lds_bytes(cgv::CL_MAX_STRUCTURES);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cgv::cluster_gromos_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) { cgv::set_error("hipFuncSetAttribute(%zu bytes of LDS): %s", most, hipGetErrorString(e)); return (int)e; }
    attr_done = true;
  }
  hipLaunchKernelGGL(cgv::cluster_gromos_k, dim3(1), dim3(cgv::CL_THREADS), lds, (hipStream_t)stream,
                     (const unsigned long long*)bits, (const unsigned long long*)good, S, W, label, centre, size, n_clusters);
  return cgv::check_launch("cgv_cluster_gromos");
}

}  // extern "C"
