// K13  the coarse-graining map learner (`-cg_method cgae`): many optimiser steps of the reference's auto-encoder per launch.
//
// Reference: CoarseGrainingVAE/cgae.py:8-33 (parameters assign_map W [n,K], decode D [K,n]; forward) and the loop of
// learn_map, CoarseGrainingVAE/datasets.py:204-249 (losses 225-231, torch.optim.Adam(lr) 205 / 237-239, result
// assign_map.argmax(-1) 249).  One step, X_b [n,3] = frame b of the batch minus its mean over atoms (centred once by the
// caller; datasets.py:222-223 and cgae.py:24-25 centre it again, a no-op):
//   M = softmax(W + g) over beads, g = -log(E), E ~ Exp(1)      F.gumbel_softmax(assign_map, dim=-1), cgae.py:27.
//        The temperature is 1: learn_map decrements a `tau` (datasets.py:208, 243-244) and hands it to forward, which never
//        passes it on to gumbel_softmax.  That is kept: there is no temperature argument here.
//   s_k = sum_i M[i,k], M_norm = M / s                            cgae.py:28
//   cg_b = M_norm^T X_b, recon_b = D^T cg_b, lift_b = M cg_b      cgae.py:30-31, datasets.py:226-227
//   loss_recon = mean over B n 3 of (X - recon)^2                 datasets.py:230
//   loss_reg   = mean over B n of sum_xyz (X - lift)^2            datasets.py:229
//   loss = loss_recon + reg_weight loss_reg, backward through all of it, Adam (bias correction, no weight decay).
//
// Backward, with e1 = -2 (X - recon) / (B n 3) and e2 = -2 reg_weight (X - lift) / (B n):
//   dD[k,i]   = sum_{b,j} cg[b,k,j] e1[b,i,j]                     dMl[i,k] = sum_{b,j} cg[b,k,j] e2[b,i,j]
//   dcg[b,k,j] = sum_i D[k,i] e1[b,i,j] + M[i,k] e2[b,i,j]        dMn[i,k] = sum_{b,j} X[b,i,j] dcg[b,k,j]
//   normalisation: dM[i,k] = dMl[i,k] + (dMn[i,k] - t_k) / s_k with t_k = sum_i dMn[i,k] M_norm[i,k]
//                                                                          = sum_{b,j} dcg[b,k,j] cg[b,k,j]   (no reduction over atoms)
//   softmax: dW[i,k] = M[i,k] (dM[i,k] - sum_k' dM[i,k'] M[i,k'])
//
// The step is six phases of independent work items (a row, a (frame, bead, axis) triple, a (frame, atom) pair, an element);
// every sum runs inside one item in a fixed order, and the only cross-item reduction -- the two loss sums -- goes through
// per-wave partials that one thread adds in wave order.  The same phase functions serve two forms:
//   resident  one workgroup of 512 threads holds W, D, the four Adam moment arrays, M and the two gradient arrays in LDS and
//             runs `steps` steps in one launch with workgroup barriers between the phases (no grid-wide wait of any kind: a
//             single workgroup cannot wait for another).  e1 / e2 ([B,n,3] each, too large for LDS beside the state at 166
//             atoms) live in a caller workspace that stays in the L2.
//   streamed  state in global memory, the phases as six launches per step over the whole chip, issued by one host loop.
// Results of the same form, inputs and seed are bit identical; the two forms agree to rounding (the loss partials of the
// streamed form are cut at other item boundaries).
//
// Noise: Philox4x32-10 (Salmon et al., SC'11), key = seed, counter = (atom, bead quad, step low, step high): stateless, so a
// launch of 10 steps and ten launches of one draw the same numbers and no noise tensor exists.  A word's top 23 bits b
// give u = (b + 0.5) / 2^23, exact in fp32 and inside the OPEN interval; g = -log(-log(u)) is evaluated in fp64 and rounded
// once, so that a host restatement in fp64 reproduces the bits (tests/cgae_restatement.py).
// The schedule rule, Adam, the loss partials and the host checks are steploop_dev.h's, shared with K19.
#include <algorithm>

#include "steploop_dev.h"

namespace cgv {
namespace cgae {

using namespace steploop;                // NT, NW, LDS_LIMIT, Step, step_of, Adam, wave_partial, the host checks

constexpr int MAX_BLOCKS = 1024;         // streamed form: cap of a phase's grid (items are strided over it)

struct Params {
  float *W, *D, *mW, *vW, *mD, *vD;      // [n,K] [K,n] and the moments of each
  float *M, *dD, *dM;                    // [n,K] [K,n] [n,K]
  float *cg, *dcg;                       // [B,K,3]
  float *csum;                           // [K]
  double *part;                          // [nparts,2] loss partials (summed in double), one pair per wave of the residual phase
  float *e1, *e2;                        // [B,n,3]
  const float* frames;                   // [n_frames,n,3] centred
  const int* order;                      // frame order of every step of the schedule
  const float* noise;                    // optional explicit noise [steps,n,K] of THIS call's steps
  float* loss_log;                       // [steps,2] of this call
  float* probe;                          // optional: M [n,K], dW [n,K], dD [K,n], cg [B,K,3] of this call's last step
  int n, K, batch, n_train, n_frames, nparts;
  float reg_weight;
  double lr, beta1, beta2, eps;
  unsigned seed_lo, seed_hi;
};

struct Ctx {
  int tid, nthreads;
};

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
}

// the four noise values of (atom i, bead quad q) of one step
__device__ __forceinline__ void gumbel_quad(unsigned seed_lo, unsigned seed_hi, long long step, int i, int q, float (&g)[4]) {
  unsigned c[4] = {(unsigned)i, (unsigned)q, (unsigned)step, (unsigned)((unsigned long long)step >> 32)};
  unsigned k0 = seed_lo, k1 = seed_hi;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double u = ((double)(c[t] >> 9) + 0.5) * (1.0 / 8388608.0);
    g[t] = (float)(-log(-log(u)));
  }
}

__device__ __forceinline__ const float* frame_of(const Params& P, const Step& st, int b) {
  return steploop::frame_of(P.frames, P.order, P.n_frames, P.n, st, b);
}

// ---- phase 1: M = softmax(W + g), one row per item
__device__ __forceinline__ void ph_softmax(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K;
  for (int i = c.tid; i < P.n; i += c.nthreads) {
    float* m = P.M + (size_t)i * K;
    const float* w = P.W + (size_t)i * K;
    float mx = -INFINITY;
    if (P.noise) {
      const float* g = P.noise + ((size_t)st.local * P.n + i) * K;
      for (int k = 0; k < K; ++k) { const float a = w[k] + g[k]; m[k] = a; mx = fmaxf(mx, a); }
    } else {
      for (int q = 0; 4 * q < K; ++q) {
        float g[4];
        gumbel_quad(P.seed_lo, P.seed_hi, st.step, i, q, g);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (4 * q + t < K) { const float a = w[4 * q + t] + g[t]; m[4 * q + t] = a; mx = fmaxf(mx, a); }
      }
    }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) { const float e = expf(m[k] - mx); m[k] = e; sum += e; }
    for (int k = 0; k < K; ++k) m[k] = m[k] / sum;
  }
}

// ---- phase 2: cg[b,k,j] = sum_i M[i,k] X[b,i,j] / s_k; the item sums s_k itself (same order in every item)
__device__ __forceinline__ void ph_cg(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n, items = st.cnt * K * 3;
  for (int it = c.tid; it < items; it += c.nthreads) {
    const int b = it / (3 * K), r = it - b * 3 * K, k = r / 3, j = r - 3 * k;
    const float* x = frame_of(P, st, b);
    float acc = 0.f, s = 0.f;
    for (int i = 0; i < n; ++i) {
      const float m = P.M[(size_t)i * K + k];
      s += m;
      acc = fmaf(m, x[3 * i + j], acc);
    }
    P.cg[it] = acc / s;
    if (b == 0 && j == 0) P.csum[k] = s;
  }
}

// ---- phase 3: residuals of a (frame, atom) pair, their squares into the wave's loss partial, e1 / e2 to the workspace
__device__ __forceinline__ void ph_resid(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n, items = st.cnt * n;
  const float s1 = -2.0f / ((float)st.cnt * (float)n * 3.0f), s2 = -2.0f * P.reg_weight / ((float)st.cnt * (float)n);
  double a1 = 0.0, a2 = 0.0;
  for (int it = c.tid; it < items; it += c.nthreads) {
    const int b = it / n, i = it - b * n;
    const float* x = frame_of(P, st, b) + 3 * i;
    const float* cg = P.cg + (size_t)b * K * 3;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, l0 = 0.f, l1 = 0.f, l2 = 0.f;
    for (int k = 0; k < K; ++k) {
      const float d = P.D[(size_t)k * n + i], m = P.M[(size_t)i * K + k];
      const float c0 = cg[3 * k], c1 = cg[3 * k + 1], c2 = cg[3 * k + 2];
      r0 = fmaf(d, c0, r0); r1 = fmaf(d, c1, r1); r2 = fmaf(d, c2, r2);
      l0 = fmaf(m, c0, l0); l1 = fmaf(m, c1, l1); l2 = fmaf(m, c2, l2);
    }
    r0 = x[0] - r0; r1 = x[1] - r1; r2 = x[2] - r2;
    l0 = x[0] - l0; l1 = x[1] - l1; l2 = x[2] - l2;
    a1 += (double)(r0 * r0 + r1 * r1 + r2 * r2);
    a2 += (double)(l0 * l0 + l1 * l1 + l2 * l2);
    st3(P.e1 + (size_t)it * 3, s1 * r0, s1 * r1, s1 * r2);
    st3(P.e2 + (size_t)it * 3, s2 * l0, s2 * l1, s2 * l2);
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {                          // steploop's wave_partial, both sums side by side
    a1 += __shfl_xor(a1, o, WAVE);
    a2 += __shfl_xor(a2, o, WAVE);
  }
  if ((c.tid & (WAVE - 1)) == 0) {
    const int w = c.tid / WAVE;
    if (w < P.nparts) { P.part[2 * w] = a1; P.part[2 * w + 1] = a2; }   // streamed: blocks x NW slots
  }
}

// ---- phase 4a: dD[k,i] and the lift part of dM[i,k], one element per item
__device__ __forceinline__ void ph_grads(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n, items = n * K;
  for (int it = c.tid; it < items; it += c.nthreads) {
    const int i = it / K, k = it - i * K;
    float dd = 0.f, dm = 0.f;
    for (int b = 0; b < st.cnt; ++b) {
      const float* cg = P.cg + ((size_t)b * K + k) * 3;
      const f3 u = ld3(P.e1 + ((size_t)b * n + i) * 3), v = ld3(P.e2 + ((size_t)b * n + i) * 3);
      dd = fmaf(cg[0], u.x, dd); dd = fmaf(cg[1], u.y, dd); dd = fmaf(cg[2], u.z, dd);
      dm = fmaf(cg[0], v.x, dm); dm = fmaf(cg[1], v.y, dm); dm = fmaf(cg[2], v.z, dm);
    }
    P.dD[(size_t)k * n + i] = dd;
    P.dM[it] = dm;
  }
}

// ---- phase 4b (independent of 4a): dcg[b,k,j] = sum_i D[k,i] e1[b,i,j] + M[i,k] e2[b,i,j]
__device__ __forceinline__ void ph_dcg(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n, items = st.cnt * K * 3;
  for (int it = c.tid; it < items; it += c.nthreads) {
    const int b = it / (3 * K), r = it - b * 3 * K, k = r / 3, j = r - 3 * k;
    const float* u = P.e1 + (size_t)b * n * 3 + j;
    const float* v = P.e2 + (size_t)b * n * 3 + j;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
      acc = fmaf(P.D[(size_t)k * n + i], u[3 * i], acc);
      acc = fmaf(P.M[(size_t)i * K + k], v[3 * i], acc);
    }
    P.dcg[it] = acc;
  }
}

// ---- phase 5: dM[i,k] += (dMn[i,k] - t_k) / s_k
__device__ __forceinline__ void ph_dm(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n, items = n * K;
  for (int it = c.tid; it < items; it += c.nthreads) {
    const int i = it / K, k = it - i * K;
    float acc = 0.f, t = 0.f;
    for (int b = 0; b < st.cnt; ++b) {
      const float* x = frame_of(P, st, b) + 3 * i;
      const float* dc = P.dcg + ((size_t)b * K + k) * 3;
      const float* cg = P.cg + ((size_t)b * K + k) * 3;
      acc = fmaf(x[0], dc[0], acc); acc = fmaf(x[1], dc[1], acc); acc = fmaf(x[2], dc[2], acc);
      t = fmaf(dc[0], cg[0], t); t = fmaf(dc[1], cg[1], t); t = fmaf(dc[2], cg[2], t);
    }
    P.dM[it] += (acc - t) / P.csum[k];
  }
}

// ---- phase 6: softmax backward + Adam on W (a row per item), Adam on D (an element per item), the step's losses
__device__ __forceinline__ void ph_update(const Params& P, const Ctx& c, const Step& st) {
  const int K = P.K, n = P.n;
  const Adam a = adam_of(P.lr, P.beta1, P.beta2, P.eps, st.step);
  const bool probe = P.probe && st.last;
  for (int i = c.tid; i < n; i += c.nthreads) {
    const float* m = P.M + (size_t)i * K;
    const float* dm = P.dM + (size_t)i * K;
    float dot = 0.f;
    for (int k = 0; k < K; ++k) dot = fmaf(dm[k], m[k], dot);
    for (int k = 0; k < K; ++k) {
      const size_t e = (size_t)i * K + k;
      const float g = m[k] * (dm[k] - dot);
      if (probe) { P.probe[e] = m[k]; P.probe[(size_t)n * K + e] = g; }
      adam_elem(a, P.W[e], g, P.mW[e], P.vW[e]);
    }
  }
  for (int e = c.tid; e < n * K; e += c.nthreads) {
    const float g = P.dD[e];
    if (probe) P.probe[(size_t)2 * n * K + e] = g;
    adam_elem(a, P.D[e], g, P.mD[e], P.vD[e]);
  }
  if (probe)
    for (int e = c.tid; e < st.cnt * K * 3; e += c.nthreads) P.probe[(size_t)3 * n * K + e] = P.cg[e];
  if (c.tid == 0) {
    double s1, s2;
    partial_sums(P.part, P.nparts, s1, s2);
    const float2 out = make_float2((float)(s1 / ((double)st.cnt * n * 3.0)), (float)(s2 / ((double)st.cnt * n)));
    *reinterpret_cast<float2*>(P.loss_log + 2 * (size_t)st.local) = out;
  }
}

__host__ __device__ inline size_t resident_lds_floats(int n, int K, int batch) {
  return (size_t)9 * n * K + (size_t)6 * batch * K + K + 4 * NW;
}

__global__ __launch_bounds__(NT) void cgae_resident_k(Params G, long long step0, int steps) {
  extern __shared__ float lds[];
  const int nk = G.n * G.K, bk3 = G.batch * G.K * 3;
  Params P = G;
  P.part = reinterpret_cast<double*>(lds);                         // first: 8-byte aligned
  float* p = lds + 4 * NW;
  P.W = p; p += nk; P.D = p; p += nk; P.mW = p; p += nk; P.vW = p; p += nk; P.mD = p; p += nk; P.vD = p; p += nk;
  P.M = p; p += nk; P.dD = p; p += nk; P.dM = p; p += nk;
  P.cg = p; p += bk3; P.dcg = p; p += bk3; P.csum = p;
  P.nparts = NW;
  const Ctx c{(int)threadIdx.x, NT};
  for (int e = threadIdx.x; e < nk; e += NT) {
    P.W[e] = G.W[e]; P.D[e] = G.D[e]; P.mW[e] = G.mW[e]; P.vW[e] = G.vW[e]; P.mD[e] = G.mD[e]; P.vD[e] = G.vD[e];
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const Step st = step_of(G.n_train, G.batch, step0 + s, s, s == steps - 1);
    ph_softmax(P, c, st);
    __syncthreads();
    ph_cg(P, c, st);
    __syncthreads();
    ph_resid(P, c, st);
    __syncthreads();                                               // e1 / e2 in global memory: the barrier orders them for the workgroup
    ph_grads(P, c, st);
    ph_dcg(P, c, st);
    __syncthreads();
    ph_dm(P, c, st);
    __syncthreads();
    ph_update(P, c, st);
    __syncthreads();
  }
  for (int e = threadIdx.x; e < nk; e += NT) {
    G.W[e] = P.W[e]; G.D[e] = P.D[e]; G.mW[e] = P.mW[e]; G.vW[e] = P.vW[e]; G.mD[e] = P.mD[e]; G.vD[e] = P.vD[e];
  }
}

template <int PH>
__global__ __launch_bounds__(NT) void cgae_stream_k(Params P, Step st) {
  const Ctx c{(int)(blockIdx.x * NT + threadIdx.x), (int)(gridDim.x * NT)};
  if (PH == 0) ph_softmax(P, c, st);
  if (PH == 1) ph_cg(P, c, st);
  if (PH == 2) ph_resid(P, c, st);
  if (PH == 3) { ph_grads(P, c, st); ph_dcg(P, c, st); }
  if (PH == 4) ph_dm(P, c, st);
  if (PH == 5) ph_update(P, c, st);
}

__global__ __launch_bounds__(256) void cgae_noise_k(unsigned seed_lo, unsigned seed_hi, long long step0, int steps, int n, int K,
                                                    float* __restrict__ out) {
  const int quads = (K + 3) / 4;
  const long long items = (long long)steps * n * quads;
  for (long long it = blockIdx.x * 256ll + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
    const int q = (int)(it % quads), i = (int)((it / quads) % n), s = (int)(it / ((long long)quads * n));
    float g[4];
    gumbel_quad(seed_lo, seed_hi, step0 + s, i, q, g);
    for (int t = 0; t < 4; ++t)
      if (4 * q + t < K) out[((size_t)s * n + i) * K + 4 * q + t] = g[t];
  }
}

inline int blocks_for(long long items) { return (int)std::min<long long>(MAX_BLOCKS, std::max<long long>(1, (items + NT - 1) / NT)); }

struct Workspace {                       // byte offsets into the caller's workspace; the streamed form's arrays follow e1 / e2
  size_t e1, e2, M, dD, dM, cg, dcg, csum, part, bytes;
};
inline Workspace cgae_workspace(int n, int K, int batch, int form) {
  const size_t e = (size_t)batch * n * 3 * sizeof(float), nk = (size_t)n * K * sizeof(float), c = (size_t)batch * K * 3 * sizeof(float);
  Workspace L{};
  Carve w;
  L.e1 = w.take(e); L.e2 = w.take(e);
  if (form != CGV_CGAE_RESIDENT) {
    L.M = w.take(nk); L.dD = w.take(nk); L.dM = w.take(nk); L.cg = w.take(c); L.dcg = w.take(c);
    L.csum = w.take((size_t)K * sizeof(float)); L.part = w.take((size_t)2 * MAX_BLOCKS * NW * sizeof(double));
  }
  L.bytes = w.at;
  return L;
}

}  // namespace cgae
}  // namespace cgv

extern "C" {

using namespace cgv::cgae;

/* 1 when n atoms x K beads with batches of `batch` frames fit the resident form (everything in one workgroup's LDS). */
int cgv_cgae_resident_fits(int n, int K, int batch) {
  if (n <= 0 || K <= 0 || batch <= 0) return 0;
  return resident_lds_floats(n, K, batch) * sizeof(float) <= LDS_LIMIT ? 1 : 0;
}

size_t cgv_cgae_workspace_bytes(int n, int K, int batch, int form) {
  if (n <= 0 || K <= 0 || batch <= 0) return 0;
  return cgae_workspace(n, K, batch, form).bytes;
}

int cgv_cgae_steps(int form, float* W, float* D, float* mW, float* vW, float* mD, float* vD, const float* frames,
                   int n_frames, const int32_t* order, int64_t order_len, int n_train, int batch, int n, int K,
                   int64_t step0, int steps, float reg_weight, double lr, double beta1, double beta2, double eps,
                   uint64_t seed, const float* noise, float* loss_log, float* probe, void* workspace,
                   size_t workspace_bytes, void* stream) {
  CGV_REQUIRE(form == CGV_CGAE_RESIDENT || form == CGV_CGAE_STREAMED, "form must be CGV_CGAE_RESIDENT or CGV_CGAE_STREAMED");
  CGV_REQUIRE(n > 0 && K > 0 && batch > 0 && n_train > 0 && n_frames > 0 && steps >= 0 && step0 >= 0, "bad size");
  CGV_REQUIRE((int64_t)n * K < (1ll << 24) && (int64_t)batch * n < (1ll << 24) && (int64_t)batch * K < (1ll << 24), "problem too large");
  if (steps == 0) return 0;
  CGV_REQUIRE(W && D && mW && vW && mD && vD && frames && order && loss_log && workspace, "null pointer");
  if (int rc = schedule_check(__func__, order_len, n_train, batch, step0, steps)) return rc;
  const Workspace L = cgae_workspace(n, K, batch, form);
  if (int rc = workspace_check(__func__, workspace_bytes, L.bytes)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Params P{};
  P.W = W; P.D = D; P.mW = mW; P.vW = vW; P.mD = mD; P.vD = vD;
  P.frames = frames; P.order = order; P.noise = noise; P.loss_log = loss_log; P.probe = probe;
  P.n = n; P.K = K; P.batch = batch; P.n_train = n_train; P.n_frames = n_frames;
  P.reg_weight = reg_weight; P.lr = lr; P.beta1 = beta1; P.beta2 = beta2; P.eps = eps;
  P.seed_lo = (unsigned)seed; P.seed_hi = (unsigned)(seed >> 32);
  char* ws = (char*)workspace;
  P.e1 = (float*)(ws + L.e1); P.e2 = (float*)(ws + L.e2);
  if (form == CGV_CGAE_RESIDENT) {
    if (!cgv_cgae_resident_fits(n, K, batch)) return resident_refusal(__func__, n, K, batch);
    const size_t lds = resident_lds_floats(n, K, batch) * sizeof(float);
    if (int rc = allow_lds(cgae_resident_k, lds, __func__)) return rc;
    hipLaunchKernelGGL(cgae_resident_k, dim3(1), dim3(NT), lds, s, P, (long long)step0, steps);
    return cgv::check_launch("cgv_cgae_steps");
  }
  P.M = (float*)(ws + L.M); P.dD = (float*)(ws + L.dD); P.dM = (float*)(ws + L.dM);
  P.cg = (float*)(ws + L.cg); P.dcg = (float*)(ws + L.dcg); P.csum = (float*)(ws + L.csum); P.part = (double*)(ws + L.part);
  const long long nk = (long long)n * K;
  for (int i = 0; i < steps; ++i) {
    const Step st = step_of(n_train, batch, step0 + i, i, i == steps - 1);
    const long long bk3 = (long long)st.cnt * K * 3, bn = (long long)st.cnt * n;
    P.nparts = blocks_for(bn) * NW;
    hipLaunchKernelGGL(cgae_stream_k<0>, dim3(blocks_for(n)), dim3(NT), 0, s, P, st);
    hipLaunchKernelGGL(cgae_stream_k<1>, dim3(blocks_for(bk3)), dim3(NT), 0, s, P, st);
    hipLaunchKernelGGL(cgae_stream_k<2>, dim3(blocks_for(bn)), dim3(NT), 0, s, P, st);
    hipLaunchKernelGGL(cgae_stream_k<3>, dim3(blocks_for(std::max(nk, bk3))), dim3(NT), 0, s, P, st);
    hipLaunchKernelGGL(cgae_stream_k<4>, dim3(blocks_for(nk)), dim3(NT), 0, s, P, st);
    hipLaunchKernelGGL(cgae_stream_k<5>, dim3(blocks_for(nk)), dim3(NT), 0, s, P, st);
    const int rc = cgv::check_launch("cgv_cgae_steps (streamed)");
    if (rc) return rc;
  }
  return 0;
}

int cgv_cgae_noise(uint64_t seed, int64_t step0, int steps, int n, int K, float* out, void* stream) {
  CGV_REQUIRE(steps >= 0 && n > 0 && K > 0 && step0 >= 0 && (int64_t)steps * n * K < (1ll << 31), "bad size");
  if (steps == 0) return 0;
  CGV_REQUIRE(out, "null pointer");
  const long long items = (long long)steps * n * ((K + 3) / 4);
  hipLaunchKernelGGL(cgae_noise_k, dim3((int)std::min<long long>(1024, (items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (unsigned)seed, (unsigned)(seed >> 32), (long long)step0, steps, n, K, out);
  return cgv::check_launch("cgv_cgae_noise");
}

}  // extern "C"
