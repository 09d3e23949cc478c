// K19  the baseline models of the comparison tables (`run_baseline -model linear | equilinear | mlp`).
//
// Reference: CoarseGrainingVAE/baseline.py:8-36 (Baseline), 387-443 (EquiLinear), 109-147 (MLP) under the fixed pooler
// CGpool (diffpoolvae.py:105-195 with assign_idx, tau = 0, gumbel = True: M[a, m(a)] = 1, M_norm = M / colsum(M),
// cg = M_norm^T xyz) and the loop of scripts/run_baseline.py:86-92, 121-176 (losses, torch.optim.Adam).
//
// Both linear models are ONE matrix P over feature vectors U [b, C, 3] of the bead means:  dx[b,a,:] = sum_c P(a,c) U[b,c,:]
//   linear      C = K        U[b,c] = cg[b,c] - mean_atoms(xyz[b])            recon = dx, target xyz - mean_atoms(xyz)
//               P(a,c) = B[c,a]   (B [K,n]: element at c * n + a)
//   equilinear  C = K knn    U[b, i knn + (c-1)] = cg[b,c] - cg[b,i], c = 1..knn   (c is a BEAD INDEX: the reference sorts the
//               bead distances and then takes nonzero() of the sorted VALUES, so the second index of a pair is the rank
//               position 1..knn, used as a bead id; nothing depends on the sort.  Kept: the paper's numbers came from it.)
//               off[b,k] = mean_{a in bead k} dx[b,a]     recon[b,a] = cg[b,m(a)] - off[b,m(a)] + dx[b,a], target xyz
//               P(a,c) = B[a,c]   (B [n, K knn]: element at a * C + c)
//   loss_recon = mean over b n 3 of (recon - target)^2
//   loss_dist  = mean over (b, e) of (|recon_i - recon_j| - |x_i - x_j|)^2 over the hyperedges e = (i, j) of the molecule
//   loss = loss_recon + gamma loss_dist;  G = dloss / drecon:
//     G[b,a] = 2 (recon - target) / (b n 3) + sum_{e at a} w[b,e] (recon_a - recon_other),  w = 2 gamma (dr - dx) / (b E dr)
//   equilinear: H[b,a] = G[b,a] - mean_{a' in bead m(a)} G[b,a']  (the recentring's backward; cg does not depend on P)
//   dP(a,c) = sum_{b,j} H[b,a,j] U[b,c,j]  (linear: H = G), then torch.optim.Adam (bias correction, no weight decay).
// Two deliberate deviations (include/cgvae_hip.h): a hyperedge whose reconstructed length is exactly 0 contributes 0 to the
// gradient (reference: NaN), and an empty hyperedge list gives loss_dist = 0 (reference: NaN).
//
// The trainer is eight phases of independent work items; every sum runs inside one item in a fixed order and the two loss
// sums go through per-wave partials that one thread adds in wave order.  Everything between the fp32 inputs (frames, P) and
// the fp32 results (loss log, probe, the gradient handed to Adam) is held and summed in double and rounded once: the
// features are differences of bead means of coordinates of order 10 A, the residual a difference of two such numbers, and
// Adam turns a gradient's relative error into a step of the size of lr, so fp32 intermediates cost digits that the step
// parity against fp64 asks for.  The arrays are small and one workgroup is latency bound; Adam itself stays in fp32 as
// torch.optim.Adam runs it.  One workgroup of 512 threads runs `steps`
// steps with workgroup barriers between the phases.  The hyperedge gradient is gathered per atom over an incidence list
// (rows sorted by edge id, built once per launch), never scattered: no floating-point atomic anywhere.
//   resident  P and both Adam moments, the bead means, U and the bead offsets in LDS
//   global    the same loop on the caller's P / moments in place and the small arrays in the workspace
// recon, G ([b,n,3] each) and w ([b,E]), doubles, live in the workspace in both forms.  Same template, same arithmetic (this file is
// compiled without fp contraction, every fused multiply-add is written out): the two forms give the same bits.
// The schedule rule, Adam, the loss partials and the host checks are steploop_dev.h's, shared with K13.
#include <algorithm>

#include "steploop_dev.h"

namespace cgv {
namespace baseline {

using namespace steploop;                 // NT, NW, LDS_LIMIT, Step, step_of, Adam, wave_partial, the host checks

constexpr int LOSS_NT = 256;
constexpr long long CAP = 1ll << 24;      // n C, batch n, batch C, batch E and 2 E stay below this (header)

struct Params {
  float *P, *mP, *vP;                    // element (a, c) at a * sa + c * sc
  double* cg;                            // [batch, K + 1, 3]; row K: the frame's mean over atoms
  double* U;                             // [batch, C, 3]
  double* off;                           // [batch, K, 3] bead means of dx, later of G
  double* part;                          // [NW, 2] loss partials
  double *R, *G;                         // [batch, n, 3] recon, dloss / drecon
  double* coef;                          // [batch, E] w
  int *rowptr, *cursor, *nbr, *eid;      // incidence list of the hyperedges: [n + 1] [n] [2E] [2E]
  const float* frames;                   // [n_frames, n, 3]
  const int *order, *map, *bsize, *edges;
  float *loss_log, *probe;
  int kind, n, K, knn, C, sa, sc, batch, n_train, n_frames, E, fwd_only;
  float gamma;
  double lr, beta1, beta2, eps;
};

__device__ __forceinline__ const float* frame_of(const Params& P, const Step& st, int b) {
  return steploop::frame_of(P.frames, P.order, P.n_frames, P.n, st, b);
}
__device__ __forceinline__ int bead_of(const Params& P, int a) { return min(max(P.map[a], 0), P.K - 1); }
__device__ __forceinline__ int atom_of(int i, int n) { return min(max(i, 0), n - 1); }

// ---- once per launch: the incidence list.  Integer atomics hand out the slots, an insertion sort by edge id per row then
// makes the order (and with it every gradient sum) independent of who came first.  Self pairs contribute nothing and are left out.
__device__ void build_incidence(const Params& P, int tid) {
  const int n = P.n, E = P.E;
  for (int a = tid; a <= n; a += NT) P.rowptr[a] = 0;
  __syncthreads();
  for (int e = tid; e < E; e += NT) {
    const int i = atom_of(P.edges[2 * e], n), j = atom_of(P.edges[2 * e + 1], n);
    if (i != j) { atomicAdd(P.rowptr + i + 1, 1); atomicAdd(P.rowptr + j + 1, 1); }
  }
  __syncthreads();
  if (tid == 0)
    for (int a = 0; a < n; ++a) P.rowptr[a + 1] += P.rowptr[a];
  __syncthreads();
  for (int a = tid; a < n; a += NT) P.cursor[a] = P.rowptr[a];
  __syncthreads();
  for (int e = tid; e < E; e += NT) {
    const int i = atom_of(P.edges[2 * e], n), j = atom_of(P.edges[2 * e + 1], n);
    if (i != j) {
      const int s = atomicAdd(P.cursor + i, 1), t = atomicAdd(P.cursor + j, 1);
      P.eid[s] = e; P.nbr[s] = j;
      P.eid[t] = e; P.nbr[t] = i;
    }
  }
  __syncthreads();
  for (int a = tid; a < n; a += NT) {
    const int lo = P.rowptr[a], hi = P.rowptr[a + 1];
    for (int s = lo + 1; s < hi; ++s) {
      const int e = P.eid[s], o = P.nbr[s];
      int t = s - 1;
      while (t >= lo && P.eid[t] > e) { P.eid[t + 1] = P.eid[t]; P.nbr[t + 1] = P.nbr[t]; --t; }
      P.eid[t + 1] = e; P.nbr[t + 1] = o;
    }
  }
  __syncthreads();
}

// ---- phase 1: bead means (and the mean over all atoms as row K)
__device__ __forceinline__ void ph_cg(const Params& P, int tid, const Step& st) {
  const int K1 = P.K + 1, n = P.n, items = st.cnt * K1 * 3;
  for (int it = tid; it < items; it += NT) {
    const int b = it / (3 * K1), r = it - b * 3 * K1, k = r / 3, j = r - 3 * k;
    const float* x = frame_of(P, st, b);
    double acc = 0.0;
    for (int i = 0; i < n; ++i)
      if (k == P.K || bead_of(P, i) == k) acc += (double)x[3 * i + j];
    P.cg[((size_t)b * K1 + k) * 3 + j] = acc / (k == P.K ? (double)n : (double)P.bsize[k]);
  }
}

// ---- phase 2: the feature vectors
__device__ __forceinline__ void ph_features(const Params& P, int tid, const Step& st) {
  const int K1 = P.K + 1, C = P.C, items = st.cnt * C * 3;
  for (int it = tid; it < items; it += NT) {
    const int b = it / (3 * C), r = it - b * 3 * C, c = r / 3, j = r - 3 * c;
    const double* cg = P.cg + (size_t)b * K1 * 3;
    if (P.kind == CGV_BASELINE_LINEAR) {
      P.U[it] = cg[3 * c + j] - cg[3 * P.K + j];
    } else {
      const int i = c / P.knn, cc = c - i * P.knn + 1;
      P.U[it] = cg[3 * cc + j] - cg[3 * i + j];
    }
  }
}

// ---- phase 3: dx = P U, one (frame, atom) pair per item
__device__ __forceinline__ void ph_dx(const Params& P, int tid, const Step& st) {
  const int n = P.n, C = P.C, items = st.cnt * n;
  for (int it = tid; it < items; it += NT) {
    const int b = it / n, a = it - b * n;
    const double* u = P.U + (size_t)b * C * 3;
    const float* p = P.P + (size_t)a * P.sa;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    for (int c = 0; c < C; ++c) {
      const double w = (double)p[(size_t)c * P.sc];
      d0 = fma(w, u[3 * c], d0); d1 = fma(w, u[3 * c + 1], d1); d2 = fma(w, u[3 * c + 2], d2);
    }
    double* r = P.R + (size_t)it * 3;
    r[0] = d0; r[1] = d1; r[2] = d2;
  }
}

// ---- phases 3b / 7: bead means of a [b, n, 3] array
__device__ __forceinline__ void ph_bead_mean(const Params& P, int tid, const Step& st, const double* src) {
  const int K = P.K, n = P.n, items = st.cnt * K * 3;
  for (int it = tid; it < items; it += NT) {
    const int b = it / (3 * K), r = it - b * 3 * K, k = r / 3, j = r - 3 * k;
    const double* s = src + (size_t)b * n * 3 + j;
    double acc = 0.0;
    for (int i = 0; i < n; ++i)
      if (bead_of(P, i) == k) acc += s[3 * i];
    P.off[it] = acc / (double)P.bsize[k];
  }
}

// ---- phase 4: recon, the residual, its square into the wave's partial, the recon part of G
__device__ __forceinline__ void ph_resid(const Params& P, int tid, const Step& st) {
  const int n = P.n, K1 = P.K + 1, items = st.cnt * n;
  const double s1 = 2.0 / ((double)st.cnt * (double)n * 3.0);
  const bool probe = P.probe && st.last;
  double a1 = 0.0;
  for (int it = tid; it < items; it += NT) {
    const int b = it / n, a = it - b * n;
    const float* x = frame_of(P, st, b) + 3 * a;
    const double* cg = P.cg + (size_t)b * K1 * 3;
    double* r = P.R + (size_t)it * 3;
    double* g = P.G + (size_t)it * 3;
    double d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double t = (double)x[j], v = r[j];
      if (P.kind == CGV_BASELINE_LINEAR) {
        t -= cg[3 * P.K + j];
      } else {
        const int k = bead_of(P, a);
        v = (cg[3 * k + j] - P.off[((size_t)b * P.K + k) * 3 + j]) + v;
        r[j] = v;
      }
      d[j] = v - t;
      g[j] = s1 * d[j];
      if (probe) P.probe[(size_t)it * 3 + j] = (float)v;
    }
    a1 += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  }
  wave_partial(P.part, NW, tid, 0, a1);
}

// ---- phase 5: the hyperedges of every frame: loss partial and w
__device__ __forceinline__ void ph_edges(const Params& P, int tid, const Step& st) {
  const int n = P.n, E = P.E, items = st.cnt * E;
  const double s2 = E > 0 ? 2.0 * (double)P.gamma / ((double)st.cnt * (double)E) : 0.0;
  double a2 = 0.0;
  for (int it = tid; it < items; it += NT) {
    const int b = it / E, e = it - b * E;
    const int i = atom_of(P.edges[2 * e], n), j = atom_of(P.edges[2 * e + 1], n);
    const float* x = frame_of(P, st, b);
    const double* r = P.R + (size_t)b * n * 3;
    double rr = 0.0, xx = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double g = r[3 * i + q] - r[3 * j + q], h = (double)x[3 * i + q] - (double)x[3 * j + q];
      rr += g * g; xx += h * h;
    }
    const double dr = sqrt(rr), diff = dr - sqrt(xx);
    a2 += diff * diff;
    if (!P.fwd_only) P.coef[(size_t)b * E + e] = dr > 0.0 ? s2 * diff / dr : 0.0;   // a coincident pair: 0, not NaN
  }
  wave_partial(P.part, NW, tid, 1, a2);
}

// ---- phase 6: G += the hyperedge part, gathered over the atom's incidence row in edge order
__device__ __forceinline__ void ph_gather(const Params& P, int tid, const Step& st) {
  const int n = P.n, E = P.E, items = st.cnt * n;
  for (int it = tid; it < items; it += NT) {
    const int b = it / n, a = it - b * n;
    const double* r = P.R + (size_t)b * n * 3;
    const double* w = P.coef + (size_t)b * E;
    double* g = P.G + (size_t)it * 3;
    const double r0 = r[3 * a], r1 = r[3 * a + 1], r2 = r[3 * a + 2];
    double g0 = g[0], g1 = g[1], g2 = g[2];
    for (int s = P.rowptr[a]; s < P.rowptr[a + 1]; ++s) {
      const double c = w[P.eid[s]];
      const double* ro = r + 3 * P.nbr[s];
      g0 = fma(c, r0 - ro[0], g0); g1 = fma(c, r1 - ro[1], g1); g2 = fma(c, r2 - ro[2], g2);
    }
    g[0] = g0; g[1] = g1; g[2] = g2;
  }
}

// ---- phase 8: dP(a,c) and Adam, one element per item (the gradient arrives rounded to fp32, as torch's does)
__device__ __forceinline__ void ph_update(const Params& P, int tid, const Step& st) {
  const int n = P.n, C = P.C, K = P.K, items = n * C;
  const Adam ad = adam_of(P.lr, P.beta1, P.beta2, P.eps, st.step);
  const bool probe = P.probe && st.last;
  const bool equi = P.kind != CGV_BASELINE_LINEAR;
  for (int it = tid; it < items; it += NT) {
    const int a = it / C, c = it - a * C, k = bead_of(P, a);
    double acc = 0.0;
    for (int b = 0; b < st.cnt; ++b) {
      const double* h = P.G + ((size_t)b * n + a) * 3;
      const double* u = P.U + ((size_t)b * C + c) * 3;
      double h0 = h[0], h1 = h[1], h2 = h[2];
      if (equi) {
        const double* m = P.off + ((size_t)b * K + k) * 3;
        h0 -= m[0]; h1 -= m[1]; h2 -= m[2];
      }
      acc = fma(h0, u[0], acc); acc = fma(h1, u[1], acc); acc = fma(h2, u[2], acc);
    }
    const float g = (float)acc;
    const size_t e = (size_t)a * P.sa + (size_t)c * P.sc;
    if (probe) P.probe[(size_t)P.batch * n * 3 + e] = g;
    adam_elem(ad, P.P[e], g, P.mP[e], P.vP[e]);
  }
}

__device__ __forceinline__ void ph_losses(const Params& P, int tid, const Step& st) {
  if (tid == 0) {
    double s1, s2;
    partial_sums(P.part, NW, s1, s2);
    const double e = (double)st.cnt * (double)P.E;
    P.loss_log[2 * (size_t)st.local] = (float)(s1 / ((double)st.cnt * P.n * 3.0));
    P.loss_log[2 * (size_t)st.local + 1] = P.E > 0 ? (float)(s2 / e) : 0.f;          // no hyperedges: 0, not NaN
  }
}

__host__ __device__ inline size_t resident_lds_floats(int n, int C, int batch) {
  // P, m, v (floats); bead means + frame mean, U, bead offsets sized for K <= C and the loss partials (doubles: 2 floats each)
  return (size_t)3 * n * C + (size_t)6 * batch * (3 * (size_t)C + 1) + 4 * NW;
}

template <bool RESIDENT>
__global__ __launch_bounds__(NT) void baseline_steps_k(Params G, long long step0, int steps) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nc = G.n * G.C;
  Params P = G;
  if (RESIDENT) {
    double* d = lds;                                               // the doubles first: 8-byte aligned
    P.part = d; d += 2 * NW;
    P.cg = d; d += (size_t)3 * G.batch * (G.C + 1); P.U = d; d += (size_t)3 * G.batch * G.C; P.off = d; d += (size_t)3 * G.batch * G.C;
    float* p = reinterpret_cast<float*>(d);
    P.P = p; p += nc; P.mP = p; p += nc; P.vP = p;
    P.sa = G.sa; P.sc = G.sc;
    for (int e = tid; e < nc; e += NT) {
      P.P[e] = G.P[e];
      if (!G.fwd_only) { P.mP[e] = G.mP[e]; P.vP[e] = G.vP[e]; }
    }
  }
  if (!G.fwd_only) build_incidence(P, tid);
  __syncthreads();
  const bool equi = G.kind != CGV_BASELINE_LINEAR;
  for (int s = 0; s < steps; ++s) {
    const Step st = step_of(G.n_train, G.batch, step0 + s, s, s == steps - 1);
    ph_cg(P, tid, st);
    __syncthreads();
    ph_features(P, tid, st);
    __syncthreads();
    ph_dx(P, tid, st);
    __syncthreads();                                               // recon / G / w in global memory: the barrier orders them for the workgroup
    if (equi) {
      ph_bead_mean(P, tid, st, P.R);
      __syncthreads();
    }
    ph_resid(P, tid, st);
    __syncthreads();
    ph_edges(P, tid, st);
    __syncthreads();
    ph_losses(P, tid, st);
    if (!G.fwd_only) {
      ph_gather(P, tid, st);
      __syncthreads();
      if (equi) {
        ph_bead_mean(P, tid, st, P.G);
        __syncthreads();
      }
      ph_update(P, tid, st);
    }
    __syncthreads();
  }
  if (RESIDENT && !G.fwd_only)
    for (int e = tid; e < nc; e += NT) { G.P[e] = P.P[e]; G.mP[e] = P.mP[e]; G.vP[e] = P.vP[e]; }
}

// ---- the loss of a reconstruction that some other model made (the MLP): one block per frame.  The atom's hyperedge
// gradient is gathered by scanning the edge list in order; the blocks' loss partials meet at a self-resetting ticket and the
// last block adds them in frame order.
__global__ __launch_bounds__(LOSS_NT) void baseline_loss_k(const float* __restrict__ recon, const float* __restrict__ xyz,
                                                           const int* __restrict__ edges, int n, int E, float gamma,
                                                           float* __restrict__ losses, float* __restrict__ grad,
                                                           unsigned* ticket, double* partial, float* __restrict__ coef) {
  const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
  const float* r = recon + (size_t)b * n * 3;
  const float* x = xyz + (size_t)b * n * 3;
  float* g = grad + (size_t)b * n * 3;
  float* w = coef + (size_t)b * E;
  const float s1 = 2.0f / ((float)B * (float)n * 3.0f), s2 = E > 0 ? 2.0f * gamma / ((float)B * (float)E) : 0.f;
  double a1 = 0.0, a2 = 0.0;
  for (int e = tid; e < E; e += LOSS_NT) {
    const int i = atom_of(edges[2 * e], n), j = atom_of(edges[2 * e + 1], n);
    const f3 ri = ld3(r + 3 * i), rj = ld3(r + 3 * j), xi = ld3(x + 3 * i), xj = ld3(x + 3 * j);
    const float g0 = ri.x - rj.x, g1 = ri.y - rj.y, g2 = ri.z - rj.z;
    const float h0 = xi.x - xj.x, h1 = xi.y - xj.y, h2 = xi.z - xj.z;
    const float dr = sqrtf(g0 * g0 + g1 * g1 + g2 * g2), dx = sqrtf(h0 * h0 + h1 * h1 + h2 * h2);
    const float diff = dr - dx;
    a2 += (double)(diff * diff);
    w[e] = (dr > 0.f && i != j) ? s2 * diff / dr : 0.f;
  }
  __syncthreads();                                                 // w of this frame: written and read by this block only
  for (int a = tid; a < n; a += LOSS_NT) {
    const f3 ra = ld3(r + 3 * a), xa = ld3(x + 3 * a);
    const float d0 = ra.x - xa.x, d1 = ra.y - xa.y, d2 = ra.z - xa.z;
    a1 += (double)(d0 * d0 + d1 * d1 + d2 * d2);
    float o0 = s1 * d0, o1 = s1 * d1, o2 = s1 * d2;
    for (int e = 0; e < E; ++e) {
      const int i = atom_of(edges[2 * e], n), j = atom_of(edges[2 * e + 1], n);
      if ((i == a) != (j == a)) {
        const f3 ro = ld3(r + 3 * (i == a ? j : i));
        const float c = w[e];
        o0 = fmaf(c, ra.x - ro.x, o0); o1 = fmaf(c, ra.y - ro.y, o1); o2 = fmaf(c, ra.z - ro.z, o2);
      }
    }
    st3(g + 3 * a, o0, o1, o2);
  }
  __shared__ double wsum[2 * (LOSS_NT / WAVE)];
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) { a1 += __shfl_xor(a1, o, WAVE); a2 += __shfl_xor(a2, o, WAVE); }
  if ((tid & (WAVE - 1)) == 0) { wsum[2 * (tid / WAVE)] = a1; wsum[2 * (tid / WAVE) + 1] = a2; }
  __syncthreads();
  if (tid != 0) return;
  double t1 = 0.0, t2 = 0.0;
  for (int k = 0; k < LOSS_NT / WAVE; ++k) { t1 += wsum[2 * k]; t2 += wsum[2 * k + 1]; }
  __hip_atomic_store(partial + 2 * b, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(partial + 2 * b + 1, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  if (atomicInc(ticket, (unsigned)B - 1u) != (unsigned)B - 1u) return;   // wraps to zero at the last arrival: no reset needed
  __threadfence();
  t1 = 0.0; t2 = 0.0;
  for (int k = 0; k < B; ++k) {                                    // frame order
    t1 += __hip_atomic_load(partial + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t2 += __hip_atomic_load(partial + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  losses[0] = (float)(t1 / ((double)B * n * 3.0));
  losses[1] = E > 0 ? (float)(t2 / ((double)B * (double)E)) : 0.f;
}

inline int feature_count(int kind, int K, int knn) { return kind == CGV_BASELINE_LINEAR ? K : K * knn; }

inline bool sizes_ok(int kind, int n, int K, int knn, int batch, int E) {
  if (kind != CGV_BASELINE_LINEAR && kind != CGV_BASELINE_EQUILINEAR) return false;
  if (n <= 0 || K <= 0 || batch <= 0 || E < 0 || K > n) return false;
  if (kind == CGV_BASELINE_EQUILINEAR && (knn < 1 || knn > K - 1)) return false;
  const long long C = (long long)K * (kind == CGV_BASELINE_LINEAR ? 1 : knn);
  return C < CAP && (long long)n * C < CAP && (long long)batch * n < CAP && (long long)batch * C < CAP &&
         (long long)batch * E < CAP && 2ll * E < CAP;
}

struct Workspace {                       // byte offsets into the caller's workspace; the global form's arrays follow eid
  size_t R, G, coef, rowptr, cursor, nbr, eid, cg, U, off, part, bytes;
};
inline Workspace baseline_workspace(int n, int K, int C, int batch, int E, int form) {
  const size_t r = (size_t)batch * n * 3 * sizeof(double), e = (size_t)2 * std::max(E, 1) * sizeof(int);
  Workspace L{};
  Carve w;
  L.R = w.take(r); L.G = w.take(r);
  L.coef = w.take((size_t)batch * std::max(E, 1) * sizeof(double));
  L.rowptr = w.take((size_t)(n + 1) * sizeof(int)); L.cursor = w.take((size_t)n * sizeof(int));
  L.nbr = w.take(e); L.eid = w.take(e);
  if (form != CGV_BASELINE_RESIDENT) {
    L.cg = w.take((size_t)batch * (K + 1) * 3 * sizeof(double));
    L.U = w.take((size_t)batch * C * 3 * sizeof(double));
    L.off = w.take((size_t)batch * K * 3 * sizeof(double));
    L.part = w.take((size_t)2 * NW * sizeof(double));
  }
  L.bytes = w.at;
  return L;
}

}  // namespace baseline
}  // namespace cgv

extern "C" {

using namespace cgv::baseline;

int cgv_baseline_resident_fits(int kind, int n_atoms, int C, int batch) {
  if ((kind != CGV_BASELINE_LINEAR && kind != CGV_BASELINE_EQUILINEAR) || n_atoms <= 0 || C <= 0 || batch <= 0) return 0;
  if ((long long)n_atoms * C >= CAP || (long long)batch * C >= CAP) return 0;
  return resident_lds_floats(n_atoms, C, batch) * sizeof(float) <= LDS_LIMIT ? 1 : 0;
}

size_t cgv_baseline_workspace_bytes(int kind, int n, int K, int knn, int batch, int E, int form) {
  if (!sizes_ok(kind, n, K, knn, batch, E)) return 0;
  return baseline_workspace(n, K, feature_count(kind, K, knn), batch, E, form).bytes;
}

int cgv_baseline_steps(int kind, int form, int mode, float* B, float* mB, float* vB, const float* frames, int n_frames,
                       const int32_t* order, int64_t order_len, int n_train, int batch, int n, int K, int knn,
                       const int32_t* mapping, const int32_t* bead_sizes, const int32_t* edges, int E, int64_t step0,
                       int steps, float gamma, double lr, double beta1, double beta2, double eps, float* loss_log,
                       float* probe, void* workspace, size_t workspace_bytes, void* stream) {
  CGV_REQUIRE(form == CGV_BASELINE_RESIDENT || form == CGV_BASELINE_GLOBAL, "form must be CGV_BASELINE_RESIDENT or CGV_BASELINE_GLOBAL");
  CGV_REQUIRE(mode == CGV_BASELINE_TRAIN || mode == CGV_BASELINE_FORWARD, "mode must be CGV_BASELINE_TRAIN or CGV_BASELINE_FORWARD");
  CGV_REQUIRE(n_train > 0 && n_frames > 0 && steps >= 0 && step0 >= 0, "bad size");
  CGV_REQUIRE(sizes_ok(kind, n, K, knn, batch, E), "bad kind, or a size beyond the cap (n C, batch n, batch C, batch E, 2 E < 2^24; knn <= K - 1)");
  if (steps == 0) return 0;
  CGV_REQUIRE(B && frames && order && mapping && bead_sizes && loss_log && workspace && (E == 0 || edges), "null pointer");
  CGV_REQUIRE(mode == CGV_BASELINE_FORWARD || (mB && vB), "training needs both Adam moment arrays");
  if (int rc = schedule_check(__func__, order_len, n_train, batch, step0, steps)) return rc;
  const int C = feature_count(kind, K, knn);
  const Workspace L = baseline_workspace(n, K, C, batch, E, form);
  if (int rc = workspace_check(__func__, workspace_bytes, L.bytes)) return rc;
  Params P{};
  P.P = B; P.mP = mB; P.vP = vB;
  P.frames = frames; P.order = order; P.map = mapping; P.bsize = bead_sizes; P.edges = edges;
  P.loss_log = loss_log; P.probe = probe;
  P.kind = kind; P.n = n; P.K = K; P.knn = knn; P.C = C; P.batch = batch; P.n_train = n_train; P.n_frames = n_frames; P.E = E;
  P.sa = kind == CGV_BASELINE_LINEAR ? 1 : C;
  P.sc = kind == CGV_BASELINE_LINEAR ? n : 1;
  P.fwd_only = mode == CGV_BASELINE_FORWARD;
  P.gamma = gamma; P.lr = lr; P.beta1 = beta1; P.beta2 = beta2; P.eps = eps;
  char* ws = (char*)workspace;
  P.R = (double*)(ws + L.R); P.G = (double*)(ws + L.G); P.coef = (double*)(ws + L.coef);
  P.rowptr = (int*)(ws + L.rowptr); P.cursor = (int*)(ws + L.cursor); P.nbr = (int*)(ws + L.nbr); P.eid = (int*)(ws + L.eid);
  hipStream_t s = (hipStream_t)stream;
  if (form == CGV_BASELINE_RESIDENT) {
    if (!cgv_baseline_resident_fits(kind, n, C, batch)) return resident_refusal(__func__, n, C, batch);
    const size_t lds = resident_lds_floats(n, C, batch) * sizeof(float);
    if (int rc = allow_lds(baseline_steps_k<true>, lds, __func__)) return rc;
    hipLaunchKernelGGL(baseline_steps_k<true>, dim3(1), dim3(NT), lds, s, P, (long long)step0, steps);
    return cgv::check_launch("cgv_baseline_steps");
  }
  P.cg = (double*)(ws + L.cg); P.U = (double*)(ws + L.U); P.off = (double*)(ws + L.off); P.part = (double*)(ws + L.part);
  hipLaunchKernelGGL(baseline_steps_k<false>, dim3(1), dim3(NT), 0, s, P, (long long)step0, steps);
  return cgv::check_launch("cgv_baseline_steps (global)");
}

size_t cgv_baseline_loss_workspace_bytes(int b, int n, int E) {
  if (b <= 0 || n <= 0 || E < 0) return 0;
  return 256 + cgv::align256((size_t)2 * b * sizeof(double)) + cgv::align256((size_t)b * std::max(E, 1) * sizeof(float));
}

int cgv_baseline_loss(const float* xyz_recon, const float* xyz, const int32_t* edges, int b, int n, int E, float gamma,
                      float* losses, float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  CGV_REQUIRE(b > 0 && b <= 65535 && n > 0 && E >= 0, "bad size");
  CGV_REQUIRE((long long)b * n < CAP && (long long)b * E < CAP && (long long)n * E < (1ll << 28), "problem beyond the cap (b n, b E < 2^24; n E < 2^28)");
  CGV_REQUIRE(xyz_recon && xyz && losses && grad && workspace && (E == 0 || edges), "null pointer");
  if (int rc = workspace_check(__func__, workspace_bytes, cgv_baseline_loss_workspace_bytes(b, n, E))) return rc;
  char* ws = (char*)workspace;
  unsigned* ticket = (unsigned*)ws; ws += 256;
  double* partial = (double*)ws; ws += cgv::align256((size_t)2 * b * sizeof(double));
  hipLaunchKernelGGL(baseline_loss_k, dim3(b), dim3(LOSS_NT), 0, (hipStream_t)stream, xyz_recon, xyz, edges, n, E, gamma, losses,
                     grad, ticket, partial, (float*)ws);
  return cgv::check_launch("cgv_baseline_loss");
}

}  // extern "C"
