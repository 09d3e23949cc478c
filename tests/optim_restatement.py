"""csrc/optim.hip restated in plain fp64 torch: the decision pass (global norm, skip rule, clip coefficient, step counter,
bias corrections), the Adam element update (``adam_elem``, csrc/cgv_common.h) and the SGD update -- and the error bounds
the fp32 kernels are held to (tests/test_optim_gpu.py; tests/test_optim_cpu.py pins this file to torch.optim).

Everything runs on fp64 copies of the kernels' fp32 inputs, on whatever device those copies live.  The scalars enter
as the fp32 values the C ABI receives (``f32``): ``BETA1 = float(np.float32(0.9))``, ``BETA2 = float(np.float32(0.999))``.
That matters for ``v``: ``1 - 0.999f`` differs from the double ``0.001`` by -1.29e-5 relative, two hundred times the
rounding of the whole update; a reference with the double betas would need a tolerance that hides the arithmetic.

No GPU, no library call: importable anywhere."""
import math

import numpy as np
import torch

ST_STEP, ST_NORM, ST_CLIP, ST_BC1, ST_BC2SQRT, ST_SKIP, ST_NSKIPPED = range(7)      # csrc/cgv_common.h
STATE_FLOATS = 8
U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest): |fl(x) - x| <= U |x|
TINY = 2.0 ** -149                   # the smallest fp32 step (results that underflow)
SLACK = 1.0 + 2.0 ** -10             # the terms of second order in U that the first-order counts below leave out


def f32(x):
    """The double a float argument of the C ABI carries."""
    return float(np.float32(x))


BETA1, BETA2 = f32(0.9), f32(0.999)
LR, EPS = f32(1e-3), f32(1e-8)

# wrong formulas (tests/test_optim_cpu.py only: the comparison with torch must be able to see each of them)
WRONG_EPS_INSIDE_SQRT, WRONG_BIAS_STEP_MINUS_1, WRONG_CLIP_WITHOUT_1E6 = "eps_inside_sqrt", "bias_step_minus_1", "clip_without_1e-6"


def new_state():
    return [0.0] * STATE_FLOATS


def decide(g, extra, grad_scale, max_norm, beta1, beta2, loss, threshold, state, wrong=None):
    """optim_finalize / the last block of sumsq_decide_k.  ``g``: fp64 tensor (any shape, may be empty); ``extra``: fp64
    tensor of further squared norms or None; ``loss``: a float or None (no skip rule); ``state``: sequence of 8 floats.
    Returns the new state (a list of Python floats, i. e. doubles)."""
    st = [float(x) for x in state]
    total = float((g * g).sum()) if g.numel() else 0.0
    if extra is not None and extra.numel():
        total += float(extra.sum())
    norm = math.sqrt(total) * abs(grad_scale)        # (NaN stays NaN, inf stays inf)
    skip = loss is not None and (loss >= threshold or loss != loss)
    st[ST_NORM] = norm
    st[ST_SKIP] = 1.0 if skip else 0.0
    if skip:
        st[ST_NSKIPPED] += 1.0
        return st
    coef = max_norm / (norm + (0.0 if wrong == WRONG_CLIP_WITHOUT_1E6 else 1e-6))
    if coef > 1.0:                                   # (false for a NaN coefficient: it stays NaN, as in the kernel)
        coef = 1.0
    st[ST_CLIP] = coef * grad_scale
    step = st[ST_STEP] + 1.0
    st[ST_STEP] = step
    k = step - 1.0 if wrong == WRONG_BIAS_STEP_MINUS_1 else step
    st[ST_BC1] = 1.0 - beta1 ** k
    st[ST_BC2SQRT] = math.sqrt(1.0 - beta2 ** k)
    return st


def adam(p, g, m, v, lr, beta1, beta2, eps, state, wrong=None):
    """adam_update: new (p, m, v) as fp64 tensors; the inputs are left alone.  A no-op on a skip."""
    if state[ST_SKIP] != 0.0:
        return p.clone(), m.clone(), v.clone()
    gc = g * state[ST_CLIP]
    m = m + (1.0 - beta1) * (gc - m)
    v = beta2 * v + (1.0 - beta2) * gc * gc
    if wrong == WRONG_EPS_INSIDE_SQRT:
        denom = (v / state[ST_BC2SQRT] ** 2 + eps).sqrt()
    else:
        denom = v.sqrt() / state[ST_BC2SQRT] + eps
    p = p - _div(lr, state[ST_BC1]) * m / denom
    return p, m, v


def sgd(p, g, lr, state):
    """sgd_update: the new p.  A no-op on a skip."""
    if state[ST_SKIP] != 0.0:
        return p.clone()
    return p - lr * state[ST_CLIP] * g


def _div(a, b):
    """a / b with IEEE results for b == 0 (a wrong bias correction at step 1 divides by zero)."""
    return math.copysign(math.inf, a) if b == 0.0 else a / b


# ----------------------------------------------------------------------------------------------------------------------
# Inputs shared by the GPU test and by the wrong-formula controls of the CPU test (same recipe, each on its device)

CLIP_CASES = {
    # name: (scale g to this norm or None, max_norm or None for 10 x the norm, grad_scale)
    "active": (None, f32(0.01), 1.0),             # unit-variance g: the norm is far above max_norm
    "active-scaled": (None, f32(0.01), 0.25),
    "inactive": (None, None, 1.0),                # max_norm at 10 x the norm: coefficient exactly 1
    "inactive-scaled": (None, None, 0.25),
    "edge": (1.05e-4, f32(1e-4), 1.0),            # ||g|| just above max_norm = 1e-4: the + 1e-6 is 1 % of the coefficient
}


def gradient(n, gen, device, case, extra=None):
    """fp32 gradient of a clip case and the case's (max_norm, grad_scale).  ``extra``: fp64 squared norms that count
    towards the norm the case is about."""
    to_norm, max_norm, grad_scale = CLIP_CASES[case]
    g = torch.randn(n, device=device, generator=gen)
    rest = float(extra.sum()) if extra is not None else 0.0
    if to_norm is not None:
        g = g * (math.sqrt(max(to_norm ** 2 - rest, 0.0)) / float(g.double().norm()))
    if max_norm is None:
        max_norm = f32(10.0 * math.sqrt(float((g.double() ** 2).sum()) + rest) * abs(grad_scale))
    return g, max_norm, grad_scale


def adam_inputs(n, gen, device, fresh=False):
    """fp32 p, m, v: p ~ N(0, 1), m ~ 0.1 N(0, 1), v = 0.01 (0.1 + U(0, 1)) (away from 0: m / sqrt(v) stays conditioned);
    ``fresh``: m = v = 0, the optimiser's real first step."""
    p = torch.randn(n, device=device, generator=gen)
    m = 0.1 * torch.randn(n, device=device, generator=gen)
    v = 0.01 * (0.1 + torch.rand(n, device=device, generator=gen))
    if fresh:
        m.zero_()
        v.zero_()
    return p, m, v


# ----------------------------------------------------------------------------------------------------------------------
# Error bounds of the fp32 kernels against this file, from their operation counts (first order in U, times SLACK)

NORM_BLOCKS_MAX, NORM_F4_PER_BLOCK = 2048, 1024          # cgv_optim_prepare_extra's grid rule


def norm_blocks(n):
    want = ((n >> 2) + NORM_F4_PER_BLOCK - 1) // NORM_F4_PER_BLOCK
    return min(max(want, 1), NORM_BLOCKS_MAX)


def norm_roundings(n):
    """Roundings on one element's way into a block's fp32 partial sum: a thread makes ceil(n4 / (blocks x 256)) trips of
    4 squares (<= 4 below the 2048-block cap: 16 squares), plus one tail square in block 0; two roundings per link of
    the fma chain at worst (the square, the add -- an fma makes one); 6 shuffle levels; 2 adds of the block's four wave
    sums."""
    n4 = n >> 2
    trips = -(-n4 // (norm_blocks(n) * 256))
    squares = 4 * trips + 1
    return 2 * squares + 6 + 2


def norm_rel_bound(n, n_extra=0):
    """|ST_NORM - norm| <= this x norm.  All summands are non-negative, so a partial sum of k roundings is off by at most
    k U relative, and so is their sum; the partials and the extras are then summed in double (2^-53 per add, counted
    linearly, as is this file's own fp64 sum over n); the square root halves the relative error; then the cast to fp32
    and the product with |grad_scale|, one rounding each."""
    fp64_sums = (norm_blocks(n) + n_extra + 8 + n) * 2.0 ** -53
    return SLACK * (0.5 * (norm_roundings(n) * U + fp64_sums) + 2 * U)


def clip_rel_bound(n, n_extra=0):
    """|ST_CLIP - clip| <= this x |clip|: the norm's error (the positive 1e-6 only dilutes it), and one rounding each for
    the add, the constant 1e-6f itself, the divide and the product with grad_scale."""
    return norm_rel_bound(n, n_extra) + SLACK * 4 * U


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def adam_bounds(p, g, m, v, lr, beta1, beta2, eps, state, e_clip):
    """Per-element bounds (bp, bm, bv) on |kernel - adam(...)| for ONE step from fp32 p, g, m, v (given as fp64 copies),
    with ``state`` the exact state of decide() and ``e_clip`` the relative error allowed on the kernel's ST_CLIP.
    Roundings of adam_elem (U each; sqrtf and the divide are correctly rounded, -ffast-math is not used):
      gc = g * clip                      1, plus e_clip
      m' = fma(1 - b1, gc - m, m)        1 on gc - m, 1 on m'  (1 - b1 is exact in fp32: Sterbenz)
      v' = fma(1 - b2, gc * gc, b2 * v)  gc * gc: 2 (1 + e_clip) + 1;  b2 * v: 1;  v': 1  -- every term non-negative
      denom = sqrtf(v') * inv_bc2 + eps  half of v's relative error, sqrtf 1, inv_bc2 2 (ST_BC2SQRT's cast, 1 / x),
                                         the product 1, the add 1: 5 + e_v / 2
      upd = step_size * (m' / denom)     divide 1, product 1, step_size 2 (ST_BC1's cast, lr / x): with denom's 9 + e_v / 2,
                                         plus m's absolute error carried through step_size / denom
      p' = p - upd                       1 on p'
    That is 12 roundings on the update with e_v's own 3 for the worst element, plus one on p."""
    if state[ST_SKIP] != 0.0:
        z = torch.zeros_like(p)
        return z, z, z
    pr, mr, vr = adam(p, g, m, v, lr, beta1, beta2, eps, state)
    c1, c2 = 1.0 - beta1, 1.0 - beta2
    gc = g * state[ST_CLIP]
    bm = SLACK * (U * mr.abs() + c1 * (U * (gc - m).abs() + (U + e_clip) * gc.abs())) + TINY
    bv = SLACK * (U * vr + c2 * gc * gc * (3 * U + 2 * e_clip) + U * beta2 * v) + TINY
    e_v = bv / vr.clamp_min(1e-300)
    denom = vr.sqrt() / state[ST_BC2SQRT] + eps
    step_size = lr / state[ST_BC1]
    upd = step_size * mr / denom
    bp = SLACK * (U * pr.abs() + upd.abs() * (9 * U + 0.5 * e_v) + step_size * bm / denom) + TINY
    return bp, bm, bv


def sgd_bound(p, g, lr, state, e_clip):
    """One fma: U (|p| + |lr clip g|), plus the error allowed on ST_CLIP.  (The kernel rounds lr * clip once before the
    fma; clip_rel_bound counts the constant 1e-6f as a whole rounding where it weighs 1e-6 / (norm + 1e-6) of one, which
    pays for that product wherever the norm is well above 1e-6 -- the clip cases SGD is tested on.)"""
    if state[ST_SKIP] != 0.0:
        return torch.zeros_like(p)
    sg = (lr * state[ST_CLIP] * g).abs()
    return U * (p.abs() + sg) + e_clip * sg + TINY
