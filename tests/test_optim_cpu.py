"""tests/optim_restatement.py pinned to the semantics csrc/optim.hip replaces (scripts/utils.py:145-157): the skip rule,
torch.nn.utils.clip_grad_norm_ and torch.optim.Adam / SGD, all in fp64 with the fp32-rounded scalars of the C ABI -- so
that tests/test_optim_gpu.py compares the kernels with the right thing.  Also pinned: what torch does with a NaN or an
inf in the gradient, and that the comparison would see a wrong formula at ten times the GPU test's bounds or more."""
import math

import pytest
import torch

import optim_restatement as R

N = 4099                             # one float4 block of the norm pass plus a tail: a size the GPU test uses
THRESHOLD = 2.0


class TorchLoop:
    """The reference loop (ReferenceLoop of tests/test_skip_rule.py) on one flat fp64 parameter: a loss >= threshold or
    NaN skips the step; else clip_grad_norm_(max_norm) on the scaled gradient, then the optimiser's step."""

    def __init__(self, p, m, v, lr, eps, optimizer, step=0):
        self.p = torch.nn.Parameter(p.clone())
        self.skipped = 0
        if optimizer == "adam":
            self.opt = torch.optim.Adam([self.p], lr=lr, betas=(R.BETA1, R.BETA2), eps=eps)
            self.opt.state[self.p] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        else:
            self.opt = torch.optim.SGD([self.p], lr=lr)

    def step(self, g, max_norm, grad_scale, loss=None):
        if loss is not None and (loss >= THRESHOLD or loss != loss):
            self.skipped += 1
            return None
        self.p.grad = g * grad_scale
        norm = torch.nn.utils.clip_grad_norm_([self.p], max_norm)
        self.opt.step()
        return float(norm)

    def tensors(self):
        st = self.opt.state.get(self.p, {})
        return self.p.detach(), st.get("exp_avg"), st.get("exp_avg_sq")


def _close(got, want, what):
    """fp64 rounding: 1e-12 relative per element, plus a hundred roundings of the tensor's largest entry for the elements
    that cancel (m' = m + 0.1 (g - m) near zero)."""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    ok = torch.isfinite(want)
    assert torch.equal(got[~ok & ~torch.isnan(want)], want[~ok & ~torch.isnan(want)]), what
    if not bool(ok.any()):
        return
    err = (got[ok] - want[ok]).abs()
    bound = 1e-12 * want[ok].abs() + 1e-14 * want[ok].abs().max()
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


def _inputs(case, fresh=False, seed=0, n=N):
    gen = torch.Generator().manual_seed(seed)
    p, m, v = (x.double() for x in R.adam_inputs(n, gen, "cpu", fresh))
    grads = [R.gradient(n, gen, "cpu", case) for _ in range(3)]
    return p, m, v, [(g.double(), mx, gs) for g, mx, gs in grads]


@pytest.mark.parametrize("fresh", [False, True], ids=["moments", "fresh"])
@pytest.mark.parametrize("case", list(R.CLIP_CASES))
def test_adam_restatement_matches_torch(case, fresh):
    """Three steps of clip + Adam, clip active, inactive and at the edge, with and without a gradient scale."""
    p, m, v, grads = _inputs(case, fresh)
    ref = TorchLoop(p, m, v, R.LR, R.EPS, "adam")
    state = R.new_state()
    for k, (g, max_norm, gs) in enumerate(grads):
        norm = ref.step(g, max_norm, gs)
        state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, state)
        p, m, v = R.adam(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, state)
        assert abs(state[R.ST_NORM] - norm) <= 1e-12 * norm and state[R.ST_STEP] == k + 1
        active = state[R.ST_CLIP] != gs
        assert active == (not case.startswith("inactive")), (case, state)
        for got, want, what in zip((p, m, v), ref.tensors(), "pmv"):
            _close(got, want, (case, k, what))


LOSSES = [0.5, 1.999, 2.0, 1.0, float("nan"), float("inf"), 0.1]        # step, step, skip (>=), step, skip, skip, step


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_sequence_with_skipped_steps_matches_torch(optimizer):
    """A skipped step changes ST_NORM, ST_SKIP and ST_NSKIPPED only: the step counter and with it every later bias
    correction stay where the reference loop has them."""
    gen = torch.Generator().manual_seed(1)
    p, m, v = (x.double() for x in R.adam_inputs(N, gen, "cpu"))
    lr = R.LR if optimizer == "adam" else R.f32(0.05)
    ref = TorchLoop(p, m, v, lr, R.EPS, optimizer)
    state, steps = R.new_state(), 0
    for k, loss in enumerate(LOSSES):
        g, max_norm, gs = R.gradient(N, gen, "cpu", "active-scaled" if k % 2 else "inactive")
        g = g.double()
        before = list(state)
        skipped = ref.step(g, max_norm, gs, loss) is None
        state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, loss, THRESHOLD, state)
        assert (state[R.ST_SKIP] == 1.0) == skipped
        if skipped:
            changed = {i for i in range(R.STATE_FLOATS) if state[i] != before[i]}
            assert changed <= {R.ST_NORM, R.ST_SKIP, R.ST_NSKIPPED}
            assert state[R.ST_NSKIPPED] == before[R.ST_NSKIPPED] + 1
            assert state[R.ST_NORM] == math.sqrt(float((g * g).sum())) * abs(gs)
        else:
            steps += 1
        assert state[R.ST_STEP] == steps
        if optimizer == "adam":
            p2, m2, v2 = R.adam(p, g, m, v, lr, R.BETA1, R.BETA2, R.EPS, state)
            if skipped:
                assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)
            p, m, v = p2, m2, v2
            for got, want, what in zip((p, m, v), ref.tensors(), "pmv"):
                _close(got, want, (k, what))
        else:
            p2 = R.sgd(p, g, lr, state)
            if skipped:
                assert torch.equal(p2, p)
            p = p2
            _close(p, ref.tensors()[0], k)
    assert ref.skipped == 3 and state[R.ST_NSKIPPED] == 3 and steps == 4


@pytest.mark.parametrize("case", list(R.CLIP_CASES))
def test_sgd_restatement_matches_torch(case):
    p, _m, _v, grads = _inputs(case, seed=2)
    lr = R.f32(0.05)
    ref = TorchLoop(p, None, None, lr, R.EPS, "sgd")
    state = R.new_state()
    for k, (g, max_norm, gs) in enumerate(grads):
        ref.step(g, max_norm, gs)
        state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, state)
        p = R.sgd(p, g, lr, state)
        _close(p, ref.tensors()[0], (case, k))


def test_extra_sums_enter_the_norm():
    """``extra`` holds squared norms of gradients that live nowhere in g: the norm is that of the concatenation."""
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(N, generator=gen).double()
    rest = [torch.randn(k, generator=gen).double() for k in (5, 70, 300)]
    extra = torch.stack([(r * r).sum() for r in rest])
    st = R.decide(g, extra, -0.25, 0.01, R.BETA1, R.BETA2, None, 0.0, R.new_state())
    want = 0.25 * float(torch.cat([g] + rest).norm())
    assert abs(st[R.ST_NORM] - want) <= 1e-12 * want
    assert abs(st[R.ST_CLIP] - (-0.25) * 0.01 / (want + 1e-6)) <= 1e-12 * abs(st[R.ST_CLIP])
    empty = R.decide(g[:0], extra, 1.0, 0.01, R.BETA1, R.BETA2, None, 0.0, R.new_state())
    assert abs(empty[R.ST_NORM] - math.sqrt(float(extra.sum()))) <= 1e-12 * empty[R.ST_NORM]


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_non_finite_gradient_as_in_torch(optimizer, bad):
    """One NaN in g: the norm, the coefficient and with them every element of g, m, v and p are NaN.  One +inf: the norm
    is inf, the coefficient 0; the clipped gradient is NaN at that element (inf x 0) and 0 elsewhere."""
    p, m, v, grads = _inputs("active", seed=4)
    g, max_norm, gs = grads[0]
    j = N - 1                                                       # (the scalar tail of the kernels)
    g[j] = float(bad)
    lr = R.LR if optimizer == "adam" else R.f32(0.05)
    ref = TorchLoop(p, m, v, lr, R.EPS, optimizer)
    norm = ref.step(g, max_norm, gs)
    clipped = ref.p.grad
    state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, R.new_state())
    if bad == "nan":
        assert norm != norm and state[R.ST_NORM] != state[R.ST_NORM] and state[R.ST_CLIP] != state[R.ST_CLIP]
        assert bool(torch.isnan(clipped).all())
    else:
        assert norm == math.inf and state[R.ST_NORM] == math.inf and state[R.ST_CLIP] == 0.0
        only = torch.zeros(N, dtype=torch.bool)
        only[j] = True
        assert torch.equal(torch.isnan(clipped), only) and bool((clipped[~only] == 0).all())
    assert state[R.ST_SKIP] == 0.0 and state[R.ST_STEP] == 1.0
    if optimizer == "adam":
        got = R.adam(p, g, m, v, lr, R.BETA1, R.BETA2, R.EPS, state)
        zero = R.adam(p, torch.zeros_like(g), m, v, lr, R.BETA1, R.BETA2, R.EPS, state)
    else:
        got = (R.sgd(p, g, lr, state),)
        zero = (R.sgd(p, torch.zeros_like(g), lr, state),)
    for a, b, z, what in zip(got, ref.tensors(), zero, "pmv"):
        _close(a, b, (bad, what))
        if bad == "nan":
            assert bool(torch.isnan(a).all()), what
        else:
            assert bool(torch.isnan(a[j])) and torch.equal(a[:j], z[:j]), what      # elsewhere: a step on a zero gradient


# ----------------------------------------------------------------------------------------------------------------------
# Wrong-formula controls: each must miss torch by >= 10 x the GPU test's bound, on the inputs the GPU test uses

CONTROLS = [
    # wrong formula, clip case, fresh optimiser
    (R.WRONG_EPS_INSIDE_SQRT, "active", True),          # v of the size of the clipped g^2: eps is not small beside sqrt(v)
    (R.WRONG_BIAS_STEP_MINUS_1, "active", False),       # moderate v, lr 1e-3: the update scales with the corrections
    (R.WRONG_CLIP_WITHOUT_1E6, "edge", False),          # ||g|| = 1.05e-4, max_norm 1e-4: the 1e-6 is 1 % of the coefficient
]


@pytest.mark.parametrize("wrong,case,fresh", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_the_torch_comparison_sees_a_wrong_formula(wrong, case, fresh):
    """Step by step from fp32-rounded state, as the GPU test compares: the right restatement equals torch's step, the
    wrong one misses it by at least 10 x the bound the kernels are held to (a non-finite result counts as a miss)."""
    p, m, v, grads = _inputs(case, fresh, seed=5)
    e_clip = R.clip_rel_bound(N)
    state = wrong_state = R.new_state()
    for k, (g, max_norm, gs) in enumerate(grads):
        ref = TorchLoop(p, m, v, R.LR, R.EPS, "adam", step=k)
        ref.step(g, max_norm, gs)
        want = ref.tensors()
        state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, state)
        wrong_state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, wrong_state, wrong=wrong)
        right = R.adam(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, state)
        off = R.adam(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, wrong_state, wrong=wrong)
        bounds = R.adam_bounds(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, state, e_clip)
        worst = 0.0
        for a, w, b, bound, what in zip(right, off, want, bounds, "pmv"):
            _close(a, b, (wrong, k, what))
            ratio = torch.nan_to_num((w - b).abs() / bound, nan=math.inf)
            worst = max(worst, float(ratio.max()))
        if wrong == R.WRONG_CLIP_WITHOUT_1E6:
            miss = abs(wrong_state[R.ST_CLIP] - state[R.ST_CLIP]) / (e_clip * abs(state[R.ST_CLIP]))
            assert miss >= 10.0, (k, miss)
        if wrong == R.WRONG_BIAS_STEP_MINUS_1:
            for i in (R.ST_BC1, R.ST_BC2SQRT):
                assert abs(wrong_state[i] - state[i]) >= 10.0 * R.ulp32(state[i]), (k, i)
        assert worst >= 10.0, (wrong, k, worst)
        print(f"{wrong} step {k + 1}: {worst:.3g} x the bound")
        p, m, v = (x.float().double() for x in right)                  # the kernels hand fp32 state to the next step


def test_v_bound_is_well_under_the_old_tolerance():
    """With the fp32 betas in the reference, v's bound is a small multiple of U: far below the rtol 2e-5 that a reference
    with the double 0.999 needs (1 - 0.999f is off by -1.29e-5 relative)."""
    assert abs((1.0 - R.BETA2) / 0.001 - 1.0 + 1.29e-5) < 1e-7
    p, m, v, grads = _inputs("active", seed=6)
    g, max_norm, gs = grads[0]
    state = R.decide(g, None, gs, max_norm, R.BETA1, R.BETA2, None, 0.0, R.new_state())
    _bp, _bm, bv = R.adam_bounds(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, state, R.clip_rel_bound(N))
    vr = R.adam(p, g, m, v, R.LR, R.BETA1, R.BETA2, R.EPS, state)[2]
    assert float((bv / vr).max()) < 2e-5 / 10


def test_bounds_follow_the_grid_rule():
    """16 squares per thread (+ the tail) below the 2048-block cap; above it the trips grow with n."""
    assert R.norm_blocks(1) == 1 and R.norm_blocks(4096) == 1 and R.norm_blocks(4100) == 2
    assert R.norm_blocks(8_388_608) == 2048 and R.norm_blocks(40_000_003) == 2048
    assert R.norm_roundings(3) == 2 * 1 + 8 and R.norm_roundings(8_388_608) == 2 * 17 + 8
    assert R.norm_roundings(40_000_003) == 2 * (4 * 20 + 1) + 8
    assert R.norm_rel_bound(40_000_003) < 6e-6 and R.norm_rel_bound(4099) < 1.5e-6
