// K15 internal-coordinate histograms: the numbers behind the reference's Ramachandran maps and bond-length plots
// (see include/cgvae_hip.h).
//
// S structures of one molecule go in; per feature (bond length, angle, proper torsion) a histogram comes out, and per
// pair of torsions a joint histogram.  No [S, features] tensor exists.  One kernel, 256 threads per block,
// grid (x, y):
//   x < n_ftiles    FEATURE role: the block owns `ftile` consecutive features, ftile = cgv_internal_hist_feature_tile()
//                   = min(256, IH_HIST_WORDS / (n_bins + 3)): their histograms fill the block's LDS histogram.
//   x >= n_ftiles   PAIR role: the block owns `ptile` consecutive pairs, ptile = cgv_internal_hist_pair_tile()
//                   = min(64, IH_HIST_WORDS / n_bins2^2); both torsions of a pair are computed by the lane that bins it.
//   y               the block's range of structures, s_per_block of them (the host sizes the ranges so that the grid has
//                   about four blocks per CU; the counts do not depend on the split).
// A block walks its range in stages of `stage` = IH_XYZ_WORDS / (3 n) structures: the stage's coordinates are copied to
// LDS once with coalesced loads, then the threads run over the (structure, feature) items of the stage, adjacent lanes on
// adjacent features of one structure -- their LDS atomics go to different histogram rows.  Structures of more than
// IH_STAGED_ATOMS atoms do not fit a stage: the DIRECT instance of the kernel gathers the 2 .. 4 atoms of an item from
// global memory instead (same arithmetic, same results).
//
// fp32 coordinates are widened on use; everything from there to the bin index is fp64 in the operation order of the
// header comment (this file is built without FMA contraction), so that a host restatement of the same formulas lands in
// the same bin whenever the value is not within rounding of a bin edge.  Counts are integers: LDS integer atomics, then
// one integer vector atomic per non-zero LDS slot into the caller's buffers -- exact in any order, the same bits on
// every run.  Feature records are validated in the kernel: an atom index outside [0, n), an unknown kind or a non-finite
// coordinate counts as invalid and reads nothing out of bounds.
// Bound: launch latency up to a few thousand dipeptide structures; beyond that the fp64 atan2 / sqrt of the items
// (a few hundred fp64 operations each), not the coordinate traffic: every coordinate is read from L2 once per tile.
#include "cgv_common.h"

namespace cgv {

constexpr int IH_THREADS = 256;
constexpr int IH_HIST_WORDS = 8192;              // int32 slots of a block's LDS histogram (32 KB)
constexpr int IH_XYZ_WORDS = 6144;               // floats of a stage's coordinates (24 KB)
constexpr int IH_STAGED_ATOMS = IH_XYZ_WORDS / 3;   // 2048: the largest structure a stage holds
constexpr int IH_MAX_FTILE = 256;                // features of a tile (their records live in LDS)
constexpr int IH_MAX_PTILE = 64;                 // pairs of a tile: 2 * 64 torsion records
constexpr int IH_RECORDS = IH_MAX_FTILE > 2 * IH_MAX_PTILE ? IH_MAX_FTILE : 2 * IH_MAX_PTILE;
constexpr int IH_MAX_BINS = 1024;
constexpr int IH_MAX_BINS2 = 64;
constexpr int IH_MAX_FEATURES = 1 << 20;
constexpr int IH_MAX_PAIRS = 1 << 16;
constexpr int IH_MAX_ATOMS = 1 << 20;
constexpr int IH_TARGET_BLOCKS = 1024;           // four per CU
constexpr double IH_PI = 3.14159265358979323846;
enum { IH_BOND = 2, IH_ANGLE = 3, IH_TORSION = 4 };

__host__ __device__ constexpr int ih_feature_tile(int n_bins) {
  return IH_HIST_WORDS / (n_bins + 3) < IH_MAX_FTILE ? IH_HIST_WORDS / (n_bins + 3) : IH_MAX_FTILE;
}
__host__ __device__ constexpr int ih_pair_tile(int n_bins2) {
  return IH_HIST_WORDS / (n_bins2 * n_bins2) < IH_MAX_PTILE ? IH_HIST_WORDS / (n_bins2 * n_bins2) : IH_MAX_PTILE;
}

struct d3 {
  double x, y, z;
};
__device__ __forceinline__ d3 ih_sub(const d3& a, const d3& b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double ih_dot(const d3& a, const d3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 ih_cross(const d3& a, const d3& b) {
  return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// The value of one feature of one structure (`base`: the structure's [n,3] coordinates, LDS or global).
// false: invalid (unknown kind, atom index outside the structure, non-finite coordinate or value).
__device__ __forceinline__ bool ih_value(const float* base, int n, const int* rec, int kind, double& val) {
  if (kind < IH_BOND || kind > IH_TORSION) return false;
  d3 p[4];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a < kind) {
      const int i = rec[a];
      const bool in = i >= 0 && i < n;
      const float* q = base + 3 * (size_t)(in ? i : 0);
      const float x = q[0], y = q[1], z = q[2];
      ok = ok && in && isfinite(x) && isfinite(y) && isfinite(z);
      p[a] = d3{(double)x, (double)y, (double)z};
    }
  }
  if (!ok) return false;
  if (kind == IH_BOND) {
    const d3 d = ih_sub(p[0], p[1]);
    val = sqrt(ih_dot(d, d));
  } else if (kind == IH_ANGLE) {
    const d3 u = ih_sub(p[0], p[1]), v = ih_sub(p[2], p[1]);
    const d3 c = ih_cross(u, v);
    val = atan2(sqrt(ih_dot(c, c)), ih_dot(u, v));
  } else {
    const d3 b1 = ih_sub(p[1], p[0]), b2 = ih_sub(p[2], p[1]), b3 = ih_sub(p[3], p[2]);
    const d3 c23 = ih_cross(b2, b3), c12 = ih_cross(b1, b2);
    val = atan2(sqrt(ih_dot(b2, b2)) * ih_dot(b1, c23), ih_dot(c12, c23));
  }
  return isfinite(val);
}

// periodic bin of a torsion in [-pi, pi]: exactly pi (and anything rounding puts past the last bin) is bin 0
__device__ __forceinline__ int ih_torsion_bin(double val, int nb) {
  const double t = floor((val - (-IH_PI)) * (double)nb / (IH_PI - (-IH_PI)));
  const int b = (int)t;
  return (b < 0 || b >= nb) ? 0 : b;
}

// slot of a feature's row [under, n_bins bins, over, invalid]
__device__ __forceinline__ int ih_slot(const float* base, int n, const int* rec, int kind, int nb, double lo, double hi) {
  double val;
  if (!ih_value(base, n, rec, kind, val)) return nb + 2;
  if (kind == IH_TORSION) return 1 + ih_torsion_bin(val, nb);
  if (kind == IH_ANGLE) {
    const int b = (int)floor((val - 0.0) * (double)nb / (IH_PI - 0.0));
    return 1 + (b >= nb ? nb - 1 : (b < 0 ? 0 : b));          // [0, pi], pi in the last bin
  }
  if (val < lo) return 0;
  if (val >= hi) return nb + 1;
  const int b = (int)floor((val - lo) * (double)nb / (hi - lo));
  return 1 + (b >= nb ? nb - 1 : (b < 0 ? 0 : b));            // lo <= val < hi: rounding alone could leave [0, nb)
}

// grid: x = tile (feature tiles, then pair tiles), y = range of structures.
template <bool STAGED>
__global__ __launch_bounds__(IH_THREADS) void internal_hist_k(const float* __restrict__ xyz, const int* __restrict__ feat,
                                                              const int* __restrict__ kind, const int* __restrict__ pairs, int S,
                                                              int n, int Nf, int Np, int nb, int nb2, double lo, double hi,
                                                              int n_ftiles, int s_per_block, int stage,
                                                              int* __restrict__ counts, int* __restrict__ pair_counts) {
  __shared__ int hist[IH_HIST_WORDS];
  __shared__ float xs[STAGED ? IH_XYZ_WORDS : 1];
  __shared__ int recs[4 * IH_RECORDS];
  __shared__ int kinds[IH_RECORDS];
  const int tid = threadIdx.x;
  const bool pair_role = (int)blockIdx.x >= n_ftiles;
  int first, items, words;                                   // (uniform) the tile
  if (!pair_role) {
    const int ft = ih_feature_tile(nb);
    first = (int)blockIdx.x * ft;
    items = min(ft, Nf - first);
    words = items * (nb + 3);
    for (int i = tid; i < items; i += IH_THREADS) {
#pragma unroll
      for (int a = 0; a < 4; ++a) recs[4 * i + a] = feat[4 * (size_t)(first + i) + a];
      kinds[i] = kind[first + i];
    }
  } else {
    const int pt = ih_pair_tile(nb2);
    first = ((int)blockIdx.x - n_ftiles) * pt;
    items = min(pt, Np - first);
    words = items * nb2 * nb2;
    for (int i = tid; i < 2 * items; i += IH_THREADS) {
      const int f = pairs[2 * (size_t)first + i];
      const bool in = f >= 0 && f < Nf;
#pragma unroll
      for (int a = 0; a < 4; ++a) recs[4 * i + a] = in ? feat[4 * (size_t)f + a] : -1;
      kinds[i] = in ? kind[f] : 0;                            // a pair of anything but two torsions counts nothing
    }
  }
  for (int w = tid; w < words; w += IH_THREADS) hist[w] = 0;
  __syncthreads();
  const int s_begin = (int)blockIdx.y * s_per_block;
  const int s_end = s_begin + min(s_per_block, S - s_begin);  // s_begin < S (the host's grid)
  const size_t per = 3 * (size_t)n;
  for (int s0 = s_begin; s0 < s_end; s0 += stage) {
    const int ns = min(stage, s_end - s0);
    if (STAGED) {
      __syncthreads();                                       // the previous stage has been read
      const float* __restrict__ src = xyz + per * (size_t)s0;
      const int total = ns * 3 * n;                          // <= IH_XYZ_WORDS
      for (int w = tid; w < total; w += IH_THREADS) xs[w] = src[w];
      __syncthreads();
    }
    const int work = ns * items;                             // stage <= 2048, items <= 256
    for (int it = tid; it < work; it += IH_THREADS) {
      const int sl = it / items, i = it - sl * items;
      const float* base = STAGED ? xs + 3 * n * sl : xyz + per * (size_t)(s0 + sl);
      if (!pair_role) {
        atomicAdd(&hist[i * (nb + 3) + ih_slot(base, n, recs + 4 * i, kinds[i], nb, lo, hi)], 1);
      } else if (kinds[2 * i] == IH_TORSION && kinds[2 * i + 1] == IH_TORSION) {
        double va, vb;
        const bool oka = ih_value(base, n, recs + 8 * i, IH_TORSION, va);
        const bool okb = ih_value(base, n, recs + 8 * i + 4, IH_TORSION, vb);
        if (oka && okb) atomicAdd(&hist[(i * nb2 + ih_torsion_bin(va, nb2)) * nb2 + ih_torsion_bin(vb, nb2)], 1);
      }
    }
  }
  __syncthreads();
  // the tile's rows are consecutive in the output, as they are in the LDS histogram
  int* __restrict__ out = pair_role ? pair_counts + (size_t)first * (size_t)(nb2 * nb2) : counts + (size_t)first * (size_t)(nb + 3);
  for (int w = tid; w < words; w += IH_THREADS) {
    const int c = hist[w];
    if (c != 0) atomicAdd(out + w, c);
  }
}

}  // namespace cgv

extern "C" {

int cgv_internal_hist_max_features(void) { return cgv::IH_MAX_FEATURES; }
int cgv_internal_hist_max_pairs(void) { return cgv::IH_MAX_PAIRS; }
int cgv_internal_hist_max_bins(void) { return cgv::IH_MAX_BINS; }
int cgv_internal_hist_max_bins2(void) { return cgv::IH_MAX_BINS2; }
int cgv_internal_hist_max_atoms(void) { return cgv::IH_MAX_ATOMS; }
int cgv_internal_hist_max_staged_atoms(void) { return cgv::IH_STAGED_ATOMS; }
int cgv_internal_hist_feature_tile(int n_bins) {
  return (n_bins >= 1 && n_bins <= cgv::IH_MAX_BINS) ? cgv::ih_feature_tile(n_bins) : 0;
}
int cgv_internal_hist_pair_tile(int n_bins2) {
  return (n_bins2 >= 1 && n_bins2 <= cgv::IH_MAX_BINS2) ? cgv::ih_pair_tile(n_bins2) : 0;
}

int cgv_internal_hist(const float* xyz, const int32_t* feat, const int32_t* kind, const int32_t* pairs, int n_structures,
                      int n_atoms, int n_features, int n_pairs, int n_bins, int n_bins2, double bond_lo, double bond_hi,
                      int32_t* counts, int32_t* pair_counts, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && n_features >= 0 && n_pairs >= 0, "bad size");
  CGV_REQUIRE(n_features <= cgv::IH_MAX_FEATURES, "n_features <= cgv_internal_hist_max_features()");
  CGV_REQUIRE(n_pairs <= cgv::IH_MAX_PAIRS, "n_pairs <= cgv_internal_hist_max_pairs()");
  CGV_REQUIRE(n_atoms <= cgv::IH_MAX_ATOMS, "n_atoms <= cgv_internal_hist_max_atoms()");
  CGV_REQUIRE(n_bins >= 1 && n_bins <= cgv::IH_MAX_BINS, "1 <= n_bins <= cgv_internal_hist_max_bins()");
  CGV_REQUIRE(n_pairs == 0 || (n_bins2 >= 1 && n_bins2 <= cgv::IH_MAX_BINS2), "1 <= n_bins2 <= cgv_internal_hist_max_bins2()");
  CGV_REQUIRE(bond_lo < bond_hi && bond_hi - bond_lo < 1e300 && bond_lo > -1e300, "bond range must be finite with lo < hi");
  CGV_REQUIRE(n_pairs == 0 || n_features > 0, "pairs name features: the feature table is empty");
  if (n_structures == 0 || n_atoms == 0 || (n_features == 0 && n_pairs == 0)) return 0;
  CGV_REQUIRE(xyz && feat && kind && counts, "null pointer");
  CGV_REQUIRE(n_pairs == 0 || (pairs && pair_counts), "null pair table or pair_counts");
  const int ft = cgv::ih_feature_tile(n_bins);
  const int n_ftiles = (n_features + ft - 1) / ft;
  const int n_ptiles = n_pairs ? (n_pairs + cgv::ih_pair_tile(n_bins2) - 1) / cgv::ih_pair_tile(n_bins2) : 0;
  const int tiles = n_ftiles + n_ptiles;
  const bool staged = n_atoms <= cgv::IH_STAGED_ATOMS;
  // a stage of the direct kernel is only the unit its ranges are cut in and its item loop runs over
  const int stage = staged ? cgv::IH_XYZ_WORDS / (3 * n_atoms) : 64;
  long long ranges = (cgv::IH_TARGET_BLOCKS + tiles - 1) / tiles;
  const long long stages = ((long long)n_structures + stage - 1) / stage;
  if (ranges > stages) ranges = stages;
  if (ranges > 65535) ranges = 65535;
  if (ranges < 1) ranges = 1;
  long long spb = ((stages + ranges - 1) / ranges) * stage;   // whole stages per block
  if (spb > n_structures) spb = n_structures;
  const unsigned gy = (unsigned)(((long long)n_structures + spb - 1) / spb);
  hipStream_t st = (hipStream_t)stream;
  if (staged)
    hipLaunchKernelGGL(cgv::internal_hist_k<true>, dim3((unsigned)tiles, gy), dim3(cgv::IH_THREADS), 0, st, xyz, feat, kind, pairs,
                       n_structures, n_atoms, n_features, n_pairs, n_bins, n_bins2, bond_lo, bond_hi, n_ftiles, (int)spb, stage,
                       counts, pair_counts);
  else
    hipLaunchKernelGGL(cgv::internal_hist_k<false>, dim3((unsigned)tiles, gy), dim3(cgv::IH_THREADS), 0, st, xyz, feat, kind, pairs,
                       n_structures, n_atoms, n_features, n_pairs, n_bins, n_bins2, bond_lo, bond_hi, n_ftiles, (int)spb, stage,
                       counts, pair_counts);
  return cgv::check_launch("cgv_internal_hist");
}

}  // extern "C"

// ----------------------------------------------------------------------------- the values themselves (cgv_internal_values)
// What K15 bins, written out: values [S, Nf] fp64 through the same ih_value, one thread per (structure, feature) item,
// adjacent lanes on adjacent features of one structure, the 2 .. 4 atoms gathered from global memory.  An invalid item is
// NaN and counts once in n_invalid (an integer atomic per wave that has any: exact in any order).  Bound: as K15, the
// fp64 atan2 / sqrt of the items.
namespace cgv {

constexpr long long IV_MAX_ITEMS = 1ll << 36;            // structures x features of a launch

__global__ __launch_bounds__(IH_THREADS) void internal_values_k(const float* __restrict__ xyz, const int* __restrict__ feat,
                                                                const int* __restrict__ kind, long long items, int n, int Nf,
                                                                double* __restrict__ values, int* __restrict__ n_invalid) {
  const long long it = (long long)blockIdx.x * IH_THREADS + threadIdx.x;
  bool invalid = false;
  if (it < items) {
    const long long s = it / Nf;
    const int f = (int)(it - s * Nf);
    int rec[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) rec[a] = feat[4 * (size_t)f + a];
    double val;
    invalid = !ih_value(xyz + 3 * (size_t)n * (size_t)s, n, rec, kind[f], val);
    values[it] = invalid ? (double)NAN : val;
  }
  const unsigned long long any = __ballot(invalid);
  if (any != 0ull && (threadIdx.x & 63) == 0) atomicAdd(n_invalid, (int)__popcll(any));
}

}  // namespace cgv

extern "C" {

int cgv_internal_values(const float* xyz, const int32_t* feat, const int32_t* kind, int n_structures, int n_atoms, int n_features,
                        double* values, int32_t* n_invalid, void* stream) {
  CGV_REQUIRE(n_structures >= 0 && n_atoms >= 0 && n_features >= 0, "bad size");
  CGV_REQUIRE(n_features <= cgv::IH_MAX_FEATURES, "n_features <= cgv_internal_hist_max_features()");
  CGV_REQUIRE(n_atoms <= cgv::IH_MAX_ATOMS, "n_atoms <= cgv_internal_hist_max_atoms()");
  const long long items = (long long)n_structures * n_features;
  CGV_REQUIRE(items <= cgv::IV_MAX_ITEMS, "n_structures * n_features <= 2^36 per launch");
  if (items == 0) return 0;
  CGV_REQUIRE(feat && kind && values && n_invalid, "null pointer");
  CGV_REQUIRE(n_atoms >= 1 && xyz, "features of a structure without atoms (ih_value reads atom 0 of it)");
  const unsigned blocks = (unsigned)((items + cgv::IH_THREADS - 1) / cgv::IH_THREADS);
  hipLaunchKernelGGL(cgv::internal_values_k, dim3(blocks), dim3(cgv::IH_THREADS), 0, (hipStream_t)stream, xyz, feat, kind, items,
                     n_atoms, n_features, values, n_invalid);
  return cgv::check_launch("cgv_internal_values");
}

}  // extern "C"
