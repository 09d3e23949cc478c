// K32 restrained geometry relaxation of an ensemble: every structure is moved, for `steps` damped Jacobi steps, towards the
// data's bond lengths and 1-3 distances (a restraint table) and out of its steric clashes (K28's predicate), while a weak
// spring holds every atom at its anchor.  The first kernel here that CHANGES a structure.  See include/cgvae_hip.h and
// relax.py, whose docstring is the definition; nothing in the reference computes it.
//
// In fp32 with every operation rounded on its own (this file is compiled with -ffp-contract=off; sqrtf and / are the correctly
// rounded forms, see csrc/tica.hip), one step for atom i from the positions x of the PREVIOUS step, a its anchor, r the radii:
//   g = k_pos * (x_i - a_i)                                                               per component
//   for the atom's restraints e in table order (partner j, d0, w):
//     D = x_i - x_j    q = (D.x*D.x + D.y*D.y) + D.z*D.z                                  csrc/sq_dist.h
//     if q > 0:  d = sqrtf(q)   s = (w * (d - d0)) / d          g = g + s * D
//   for j = 0 .. n - 1 ascending, j != i, not excl[i][j]:
//     c = (r_i + r_j) - tol    D, q as above
//     if c > 0 and q < c * c and q > 0:  d = sqrtf(q)   s = (k_rep * (d - c)) / d   g = g + s * D   nc += 1
//   h = (k_pos + 2 * W_i) + (2 * k_rep) * float(nc)
//   if h > 0:  f = damp / h   delta = (-f) * g   m = (delta.x^2 + delta.y^2) + delta.z^2
//              if m > cap * cap:  delta = delta * (cap / sqrtf(m))
//   else delta = 0
//   x_i' = x_i + delta
// Every comparison is strict and false for a NaN.  Before the first step and after the last, atom i adds in fp64, in this order,
//   (0.5 * k_pos) * p            p = sq_dist2(x_i, a_i) in fp32, widened;  disp2 = the largest p
//   (0.25 * w) * (t * t)         t = fp32(sqrtf(q) - d0), widened: every restraint of the atom, q = 0 included
//   (0.25 * k_rep) * (t * t)     t = fp32(sqrtf(q) - c): every j with c > 0 and q < c * c, q = 0 included -- K28's clash, counted
// to partial[i mod 256] (the atoms of a partial in ascending order); the 256 partials meet in four fixed wave trees
// (sq_wave_sum) W_0 .. W_3 over partials 0..63, 64..127, ..., and E = ((W_0 + W_1) + W_2) + W_3.  The clashing ordered pairs
// are summed as integers and halved.  Neither depends on how many threads a structure has.
//
// relax_k<T>   256 threads; a structure has T of them (64, 128 or 256: 4, 2 or 1 structures per block, chosen from n on the
//              host), thread t the atoms t, t + T, ...  Both position buffers (float4: x, y, z, r), the anchor and with them the
//              radii stay in LDS for all steps: 44 bytes an atom; the CSR table, W and the mask are read through the cache.
//              The j loop is the same in every lane, so x_j is one broadcast ds_read_b128.  One barrier per step.  A thread
//              owns 256 / T partials.  A structure with a non-finite coordinate (or anchor) is bad: copied through, outputs 0.
#include <math.h>

#include "packed_dev.h"
#include "sq_dist.h"

namespace cgv {

constexpr size_t RX_LDS_CU = 160 * 1024;     // the LDS of a CU, all of which one workgroup may take
constexpr size_t RX_LDS_STATIC = 1024;       // left to the static arrays below
constexpr int RX_MAX_STRUCTURES = 1 << 20;   // per launch
constexpr int RX_MAX_STEPS = 1 << 20;

// floats of one structure in LDS: two position buffers [n] float4, then the anchor [n, 3] padded to a whole float4
__host__ __device__ constexpr size_t rx_floats(int n) { return (size_t)8 * n + (((size_t)3 * n + 3) & ~(size_t)3); }
constexpr size_t rx_lds_bytes(int n, int per_block) { return rx_floats(n) * sizeof(float) * per_block; }
constexpr int rx_max_atoms() {
  int n = (int)((RX_LDS_CU - RX_LDS_STATIC) / 44);
  while (rx_lds_bytes(n, 1) > RX_LDS_CU - RX_LDS_STATIC) --n;
  return n;
}
constexpr int RX_MAX_ATOMS = rx_max_atoms();
static_assert(RX_MAX_ATOMS == 3700, "44 bytes an atom in 159 KB");
// threads of a structure: a wave for up to 64 atoms, two for up to 128, else the block
static inline int rx_threads(int n) { return n <= 64 ? 64 : n <= 128 ? 128 : 256; }

struct RxArgs {
  const float* xyz; const float* anchor;
  const int* row_ptr; const int* partner; const float* d0; const float* w; const float* wsum;
  const float* radii; const uint32_t* excl;
  int S, n, E, words, steps;
  float k_pos, k_rep, tol, damp, cap;
  float* xyz_out; int* clashes; double* energy; float* disp2; int* bad;
};

__device__ __forceinline__ int rx_entry(int e, int E) { return e < 0 ? 0 : e > E ? E : e; }
// bit u: column 32 * wd + u is a pair of atom i's clash loop -- inside the structure, not i, not excluded
__device__ __forceinline__ uint32_t rx_word(const RxArgs& a, int i, int wd) {
  uint32_t ok = word_inside(32 * wd, a.n) & ~a.excl[(size_t)i * a.words + wd];
  if ((i >> 5) == wd) ok &= ~(1u << (i & 31));
  return ok;
}

// x_i' of the header
__device__ __forceinline__ float4 rx_step(const RxArgs& a, const float4* __restrict__ cur, const float* __restrict__ anc, int i,
                                          float two_krep, float cap2) {
  const float4 xi = cur[i];
  float gx = a.k_pos * (xi.x - anc[3 * i]), gy = a.k_pos * (xi.y - anc[3 * i + 1]), gz = a.k_pos * (xi.z - anc[3 * i + 2]);
  const int e1 = rx_entry(a.row_ptr[i + 1], a.E);
  for (int e = rx_entry(a.row_ptr[i], a.E); e < e1; ++e) {
    const float4 xj = cur[sel_atom(a.partner[e], a.n)];
    const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
    const float q = sq_dist2(xi.x, xi.y, xi.z, xj.x, xj.y, xj.z);
    if (q > 0.f) {
      const float d = sqrtf(q);
      const float s = (a.w[e] * (d - a.d0[e])) / d;
      gx = gx + s * dx, gy = gy + s * dy, gz = gz + s * dz;
    }
  }
  int nc = 0;
  for (int wd = 0; wd < a.words; ++wd) {
    const uint32_t ok = rx_word(a, i, wd);
    const int j0 = 32 * wd, cnt = min(32, a.n - j0);
    for (int u = 0; u < cnt; ++u) {
      const float4 xj = cur[j0 + u];                         // the same address in every lane
      const float c = (xi.w + xj.w) - a.tol;
      const float q = sq_dist2(xi.x, xi.y, xi.z, xj.x, xj.y, xj.z);
      if (((ok >> u) & 1u) != 0u && c > 0.f && q < c * c && q > 0.f) {
        const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        const float d = sqrtf(q);
        const float s = (a.k_rep * (d - c)) / d;
        gx = gx + s * dx, gy = gy + s * dy, gz = gz + s * dz;
        ++nc;
      }
    }
  }
  const float h = (a.k_pos + 2.f * a.wsum[i]) + two_krep * (float)nc;
  float dx = 0.f, dy = 0.f, dz = 0.f;
  if (h > 0.f) {
    const float f = -(a.damp / h);
    dx = f * gx, dy = f * gy, dz = f * gz;
    const float m = (dx * dx + dy * dy) + dz * dz;
    if (m > cap2) {
      const float sc = a.cap / sqrtf(m);
      dx = dx * sc, dy = dy * sc, dz = dz * sc;
    }
  }
  return make_float4(xi.x + dx, xi.y + dy, xi.z + dz, xi.w);
}

// atom i's energy terms added to `e` in the header's order, its clashing partners to `nc`, its squared displacement to `dm`
__device__ __forceinline__ void rx_measure(const RxArgs& a, const float4* __restrict__ cur, const float* __restrict__ anc, int i,
                                           double& e, int& nc, float& dm) {
  const float4 xi = cur[i];
  const float p = sq_dist2(xi.x, xi.y, xi.z, anc[3 * i], anc[3 * i + 1], anc[3 * i + 2]);
  e = e + (0.5 * (double)a.k_pos) * (double)p;
  dm = p > dm ? p : dm;
  const int e1 = rx_entry(a.row_ptr[i + 1], a.E);
  for (int k = rx_entry(a.row_ptr[i], a.E); k < e1; ++k) {
    const float4 xj = cur[sel_atom(a.partner[k], a.n)];
    const float t = sqrtf(sq_dist2(xi.x, xi.y, xi.z, xj.x, xj.y, xj.z)) - a.d0[k];
    e = e + (0.25 * (double)a.w[k]) * ((double)t * (double)t);
  }
  for (int wd = 0; wd < a.words; ++wd) {
    const uint32_t ok = rx_word(a, i, wd);
    const int j0 = 32 * wd, cnt = min(32, a.n - j0);
    for (int u = 0; u < cnt; ++u) {
      const float4 xj = cur[j0 + u];
      const float c = (xi.w + xj.w) - a.tol;
      const float q = sq_dist2(xi.x, xi.y, xi.z, xj.x, xj.y, xj.z);
      if (((ok >> u) & 1u) != 0u && c > 0.f && q < c * c) {
        const float t = sqrtf(q) - c;
        e = e + (0.25 * (double)a.k_rep) * ((double)t * (double)t);
        ++nc;
      }
    }
  }
}

// grid: 256 / T structures per block; dynamic LDS: rx_lds_bytes(n, 256 / T)
template <int T>
__global__ __launch_bounds__(256) void relax_k(const RxArgs a) {
  constexpr int G = 256 / T, A = 256 / T, WPS = T / 64;      // structures of a block, partials of a thread, waves of a structure
  extern __shared__ __attribute__((aligned(16))) float rx_lds[];
  __shared__ double wpart[G][4];                             // the four wave trees of a structure's energy
  __shared__ float wmax[G][WPS];
  __shared__ int ccount[G], isbad[G];
  const int tid = threadIdx.x, g = tid / T, lt = tid % T, lane = tid & 63, wig = lt >> 6;
  const int s = (int)blockIdx.x * G + g, n = a.n;
  const bool live = s < a.S;
  float4* bufA = reinterpret_cast<float4*>(rx_lds + (size_t)g * rx_floats(n));
  float4* bufB = bufA + n;
  float* anc = reinterpret_cast<float*>(bufB + n);
  if (tid < G) ccount[tid] = 0, isbad[tid] = 0;
  __syncthreads();
  const float* in = a.xyz + (size_t)(live ? s : 0) * n * 3;
  if (live) {
    const float* an = a.anchor + (size_t)s * n * 3;
    bool ok = true;
    for (int i = lt; i < n; i += T) {
      const f3 p = ld3(in + 3 * (size_t)i), q = ld3(an + 3 * (size_t)i);
      const float r = a.radii[i];
      ok = ok && isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
      bufA[i] = make_float4(p.x, p.y, p.z, r);
      bufB[i] = make_float4(p.x, p.y, p.z, r);
      anc[3 * i] = q.x, anc[3 * i + 1] = q.y, anc[3 * i + 2] = q.z;
    }
    if (!ok) isbad[g] = 1;                                   // every writer writes 1
  }
  __syncthreads();
  const bool good = live && isbad[g] == 0;
  const float two_krep = 2.f * a.k_rep, cap2 = a.cap * a.cap;
  float4 *cur = bufA, *nxt = bufB;
  double e_before = 0.0;
  int c_before = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      if (a.steps == 0) break;                               // the same for the whole grid
      for (int step = 0; step < a.steps; ++step) {
        if (good)
          for (int i = lt; i < n; i += T) nxt[i] = rx_step(a, cur, anc, i, two_krep, cap2);
        __syncthreads();
        float4* t = cur; cur = nxt; nxt = t;
      }
    }
    double acc[A];
#pragma unroll
    for (int k = 0; k < A; ++k) acc[k] = 0.0;
    int nc = 0;
    float dm = 0.f;
    if (good) {
      int k = 0;                                             // atom lt + T * j belongs to partial lt + T * (j mod A)
      for (int i = lt; i < n; i += T) {
#pragma unroll
        for (int u = 0; u < A; ++u)
          if (u == k) rx_measure(a, cur, anc, i, acc[u], nc, dm);
        k = k + 1 == A ? 0 : k + 1;
      }
    }
#pragma unroll
    for (int k = 0; k < A; ++k) {
      const double v = sq_wave_sum(acc[k]);
      if (lane == 0) wpart[g][wig + WPS * k] = v;
    }
    nc = sq_wave_sum(nc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float o = __shfl_down(dm, d);
      dm = o > dm ? o : dm;
    }
    if (lane == 0) {
      if (nc != 0) atomicAdd(&ccount[g], nc);
      wmax[g][wig] = dm;
    }
    __syncthreads();
    if (lt == 0 && good) {
      const double E = ((wpart[g][0] + wpart[g][1]) + wpart[g][2]) + wpart[g][3];
      const int c = ccount[g] / 2;
      float m = wmax[g][0];
#pragma unroll
      for (int k = 1; k < WPS; ++k) m = wmax[g][k] > m ? wmax[g][k] : m;
      if (pass == 0) e_before = E, c_before = c;
      if (pass == 1 || a.steps == 0) {
        a.energy[2 * (size_t)s] = e_before, a.energy[2 * (size_t)s + 1] = E;
        a.clashes[2 * (size_t)s] = c_before, a.clashes[2 * (size_t)s + 1] = c;
        a.disp2[s] = m;
        a.bad[s] = 0;
      }
      ccount[g] = 0;
    }
    __syncthreads();
  }
  if (!live) return;
  float* out = a.xyz_out + (size_t)s * n * 3;
  if (good) {
    for (int i = lt; i < n; i += T) st3(out + 3 * (size_t)i, cur[i].x, cur[i].y, cur[i].z);
  } else {
    for (int i = lt; i < n; i += T) {
      const f3 p = ld3(in + 3 * (size_t)i);
      st3(out + 3 * (size_t)i, p.x, p.y, p.z);
    }
    if (lt == 0) {
      a.energy[2 * (size_t)s] = 0.0, a.energy[2 * (size_t)s + 1] = 0.0;
      a.clashes[2 * (size_t)s] = 0, a.clashes[2 * (size_t)s + 1] = 0;
      a.disp2[s] = 0.f;
      a.bad[s] = 1;
    }
  }
}

static inline bool rx_length(float v) { return v >= 0.f && v <= 3.0e38f; }   // a finite number >= 0; false for a NaN

template <int T>
static int rx_launch(const RxArgs& a, hipStream_t st) {
  static bool attr_done = false;                             // the largest size once
  if (!attr_done) {
    const size_t most = RX_LDS_CU - RX_LDS_STATIC;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(relax_k<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu bytes of LDS): %s", most, hipGetErrorString(e)); return (int)e; }
    attr_done = true;
  }
  constexpr int G = 256 / T;
  hipLaunchKernelGGL(relax_k<T>, dim3((unsigned)((a.S + G - 1) / G)), dim3(256), rx_lds_bytes(a.n, G), st, a);
  return check_launch("cgv_relax");
}

}  // namespace cgv

extern "C" {

int cgv_relax_max_atoms(void) { return cgv::RX_MAX_ATOMS; }
int cgv_relax_max_structures(void) { return cgv::RX_MAX_STRUCTURES; }
int cgv_relax_max_steps(void) { return cgv::RX_MAX_STEPS; }
int cgv_relax_pack(int n_atoms) { return n_atoms >= 1 && n_atoms <= cgv::RX_MAX_ATOMS ? 256 / cgv::rx_threads(n_atoms) : 0; }

int cgv_relax(const float* xyz, const float* anchor, const int32_t* row_ptr, const int32_t* partner, const float* d0, const float* w,
              const float* wsum, const float* radii, const uint32_t* excl, int n_structures, int n_atoms, int n_entries, float k_pos,
              float k_rep, float tol, float damp, float cap, int steps, float* xyz_out, int32_t* clashes, double* energy,
              float* disp2, int32_t* bad, void* stream) {
  const int S = n_structures, n = n_atoms;
  CGV_REQUIRE(S >= 0 && n >= 1 && n_entries >= 0, "bad size");
  CGV_REQUIRE(S <= cgv::RX_MAX_STRUCTURES, "structures per launch <= cgv_relax_max_structures()");
  CGV_REQUIRE(n <= cgv::RX_MAX_ATOMS, "n_atoms <= cgv_relax_max_atoms()");
  CGV_REQUIRE(steps >= 0 && steps <= cgv::RX_MAX_STEPS, "0 <= steps <= cgv_relax_max_steps()");
  CGV_REQUIRE(cgv::rx_length(k_pos) && cgv::rx_length(k_rep) && cgv::rx_length(tol) && cgv::rx_length(damp),
              "k_pos, k_rep, tol and damp must be finite numbers >= 0");
  CGV_REQUIRE(cap > 0.f && cap <= 3.0e38f, "cap must be a finite length > 0");
  if (S == 0) return 0;
  CGV_REQUIRE(xyz && anchor && row_ptr && wsum && radii && excl && xyz_out && clashes && energy && disp2 && bad, "null pointer");
  CGV_REQUIRE(n_entries == 0 || (partner && d0 && w), "null pointer");
  const cgv::RxArgs a{xyz, anchor, row_ptr, partner, d0, w, wsum, radii, excl, S, n, n_entries, (n + 31) / 32, steps,
                      k_pos, k_rep, tol, damp, cap, xyz_out, clashes, energy, disp2, bad};
  hipStream_t st = (hipStream_t)stream;
  switch (cgv::rx_threads(n)) {
    case 64: return cgv::rx_launch<64>(a, st);
    case 128: return cgv::rx_launch<128>(a, st);
    default: return cgv::rx_launch<256>(a, st);
  }
}

}  // extern "C"
