// The step loop that the "many optimiser steps per launch" trainers share: K13 (cgae.hip) and K19 (baseline.hip).
// newman.hip takes the LDS raise alone.  Everything is inline, so each translation unit compiles these expressions under
// its own -ffp-contract setting (build.py: SOURCE_FLAGS): no FP_CONTRACT pragma and no explicit fmaf may appear here.
//
// Schedule.  `order` holds whole epochs of n_train entries, uploaded once.  An epoch is ceil(n_train / batch) steps; step
//   s takes `batch` consecutive entries of its epoch's row and the last, partial batch of a row is kept.  A launch runs
//   steps step0 .. step0 + steps, so one launch of ten steps and ten launches of one walk the same batches.
// Adam.  torch.optim.Adam in its single-tensor form (bias correction, no weight decay): the scalars in double as the host
//   computes them, the element in fp32; the step count is the schedule position + 1.  This is NOT the AdamStep of
//   cgv_common.h (the training step's fused optimiser), which clips and is written with fmaf.
// Loss partials.  The only cross-item reduction of a step: a fixed shuffle tree inside the wave, lane 0 stores the wave's
//   slot of a pair of doubles, one thread adds the slots in wave order.
#pragma once
#include "cgv_common.h"

namespace cgv {
namespace steploop {

constexpr int NT = 512;                  // threads of a resident workgroup and of every streamed block
constexpr int NW = NT / WAVE;
constexpr size_t LDS_LIMIT = 160 * 1024; // one workgroup may hold all of a CU's LDS

struct Step {
  long long step;                        // index in the whole schedule (Adam's step count is step + 1)
  int local;                             // index within this call
  int off, cnt;                          // the batch: order[off .. off + cnt)
  int last;                              // last step of this call (the probe is written then)
};

__host__ __device__ inline Step step_of(int n_train, int batch, long long step, int local, int last) {
  const int spe = (n_train + batch - 1) / batch;
  const long long epoch = step / spe;
  const int si = (int)(step % spe);
  Step st;
  st.step = step; st.local = local; st.last = last;
  st.off = (int)(epoch * n_train) + si * batch;                    // the host checked that the table fits an int
  st.cnt = min(batch, n_train - si * batch);                       // the last, partial batch of an epoch is kept
  return st;
}

__device__ __forceinline__ const float* frame_of(const float* frames, const int* order, int n_frames, int n, const Step& st, int b) {
  const int f = min(max(order[st.off + b], 0), n_frames - 1);      // a bad table entry must not become a wild read
  return frames + (size_t)f * n * 3;
}

struct Adam {
  float w1, b2, w2, neg_step, bc2_sqrt, eps;
};
__device__ __forceinline__ Adam adam_of(double lr, double beta1, double beta2, double eps, long long step) {
  const double t = (double)(step + 1);
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  Adam a;
  a.w1 = (float)(1.0 - beta1); a.b2 = (float)beta2; a.w2 = (float)(1.0 - beta2);
  a.neg_step = (float)(-(lr / bc1)); a.bc2_sqrt = (float)sqrt(bc2); a.eps = (float)eps;
  return a;
}
__device__ __forceinline__ void adam_elem(const Adam& a, float& p, float g, float& m, float& v) {
  m = m + a.w1 * (g - m);                                          // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.b2 + a.w2 * g * g;                                     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p + a.neg_step * (m / denom);                                // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// part [nparts, 2]: wave tid / WAVE stores its sum of `a` in `slot` (0 or 1) of its pair; a wave beyond nparts stores none.
// K13's ph_resid keeps its own copy that reduces both sums side by side: through this one it compiled to other registers.
__device__ __forceinline__ void wave_partial(double* part, int nparts, int tid, int slot, double a) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);   // fixed tree inside the wave
  const int w = tid / WAVE;
  if ((tid & (WAVE - 1)) == 0 && w < nparts) part[2 * w + slot] = a;
}
__device__ __forceinline__ void partial_sums(const double* part, int nparts, double& s1, double& s2) {   // one thread
  s1 = 0.0; s2 = 0.0;
  for (int w = 0; w < nparts; ++w) { s1 += part[2 * w]; s2 += part[2 * w + 1]; }                        // wave order
}

// ---- host only: the checks every step-loop entry point makes.  `who` is the entry point (CGV_REQUIRE prints __func__).
inline int bad_arg(const char* who, const char* msg) { return set_error("%s: %s", who, msg), CGV_E_BADARG; }
inline int schedule_check(const char* who, int64_t order_len, int n_train, int batch, int64_t step0, int steps) {
  if (!(order_len > 0 && order_len < (1ll << 31) && order_len % n_train == 0))
    return bad_arg(who, "order table must hold whole epochs of n_train entries");
  const int64_t spe = (n_train + batch - 1) / batch;
  return step0 + steps <= (order_len / n_train) * spe ? 0 : bad_arg(who, "steps run past the end of the order table");
}
inline int workspace_check(const char* who, size_t have, size_t need) {
  if (have >= need) return 0;
  set_error("%s: workspace of %zu bytes, need %zu", who, have, need);
  return CGV_E_WORKSPACE;
}
inline int resident_refusal(const char* who, int rows, int cols, int batch) {
  set_error("%s: %d x %d with batches of %d does not fit the resident form", who, rows, cols, batch);
  return CGV_E_UNSUPPORTED;
}
template <typename K>
inline int allow_lds(K kernel, size_t bytes, const char* who) {   // dynamic LDS above 64 KB has to be asked for
  if (bytes <= 64 * 1024) return 0;
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) return 0;
  set_error("%s: %zu bytes of LDS refused: %s", who, bytes, hipGetErrorString(e));
  return (int)e;
}

// A kernel's ONE workspace layout (size query and pointer carve both read it) takes its arrays in order, 256-byte aligned.
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += align256(bytes); return o; }
};

}  // namespace steploop
}  // namespace cgv
