"""csrc/optim.hip called directly: the norm pass and the decision pass (two launches, or one with option
``optim_one_launch``), the flat Adam pass and the SGD pass, against tests/optim_restatement.py in fp64 -- at the sizes
where their loops change shape, with bounds derived from their operation counts (optim_restatement: norm_rel_bound,
clip_rel_bound, adam_bounds, sgd_bound; tests/test_optim_cpu.py pins that file to torch.optim).  The rank-update Adam
epilogues, which read the same state, are in tests/test_hip_parity.py and tests/test_dp_exchange.py."""
import pytest
import torch

import optim_restatement as R
from coarsegrainingvae_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

BIG = 40_000_003      # above both grid caps (norm: n > 8,388,608; Adam: n > 33,554,432): n4 = 10,000,000 against Adam's stride
#                       of 4,194,304 -- one double step, then the single step for some threads and nothing for the rest; the
#                       norm's threads make 20 trips.  Runs once per test that needs it.
SMALL = [
    1, 2, 3,          # n4 = 0: only block 0's scalar tail runs
    4, 5, 7,          # one float4, plus tails of 1 and 3
    2044,             # n4 = 511: Adam's thread 255 takes the single-step branch `if (i < n4)`, the rest one double step
    2048,             # n4 = 512: every Adam thread in one double step, nothing in the tail
    2052,             # n4 = 513: 2 Adam blocks (stride 512), only i = 0 takes the double step
    2055,             # ... and a scalar tail of 3
    4092,             # n4 = 1023: one norm block, its last thread one trip short
    4096,             # n4 = 1024: one full norm block (4 trips per thread)
    4100,             # n4 = 1025: a second norm block with one float4
    4099,             # one full norm block and a scalar tail of 3
    1_000_003,        # many blocks (norm 977, Adam 1954), n & 3 = 3
]
N_MODE = [(n, md) for n in SMALL for md in (0, 1)] + [(BIG, 0)]
N_MODE_IDS = [f"{n}-{'one' if md else 'two'}-launch" for n, md in N_MODE]
CHUNK = 1 << 22       # the fp64 reference of the element passes runs on slices of this many elements
TICKET = 2048         # partial[2048]: the ticket word of sumsq_decide_k


class Optim:
    """State and scratch of one optimiser, as Trainer allocates them, and the entry points."""

    def __init__(self):
        lib = _lib.load()
        self.state = torch.zeros(lib.cgv_optim_state_floats(), device=DEV)
        self.partial = torch.zeros(lib.cgv_optim_partial_floats(), device=DEV)
        assert self.state.numel() == R.STATE_FLOATS and self.partial.numel() > TICKET

    def prepare(self, g, n, max_norm, grad_scale, extra=None, loss=None, threshold=0.0):
        _lib.call("cgv_optim_prepare_extra", g.data_ptr(), n, _lib.ptr(extra), 0 if extra is None else extra.numel(), R.BETA1,
                  R.BETA2, max_norm, grad_scale, _lib.ptr(loss), threshold, _lib.ptr(self.state), _lib.ptr(self.partial),
                  _lib.stream_ptr())

    def adam(self, p, g, m, v, n, lr=R.LR):
        _lib.call("cgv_adam_apply", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, R.BETA1, R.BETA2, R.EPS,
                  _lib.ptr(self.state), _lib.stream_ptr())

    def sgd(self, p, g, n, lr):
        _lib.call("cgv_sgd_apply", p.data_ptr(), g.data_ptr(), n, lr, _lib.ptr(self.state), _lib.stream_ptr())

    def clip_step(self, p, g, m, v, n, max_norm, grad_scale, loss=None, threshold=0.0):
        _lib.call("cgv_adam_clip_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, R.LR, R.BETA1, R.BETA2, R.EPS,
                  max_norm, grad_scale, _lib.ptr(loss), threshold, _lib.ptr(self.state), _lib.ptr(self.partial), _lib.stream_ptr())

    def host_state(self):
        return self.state.double().cpu().tolist()

    def ticket(self):
        return int(self.partial[TICKET:TICKET + 1].view(torch.int32).item())


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _check_decision(st, ref, n, n_extra, what):
    """ST_NORM and ST_CLIP within the bounds derived in optim_restatement (norm_rel_bound: (2 squares + 8) / 2 + 2
    roundings, a function of n; clip_rel_bound: 4 more); the counter and the skip flag exact; the bias corrections, computed
    in double in the kernel and cast, within 1 ulp of fp32."""
    e_n, e_c = R.norm_rel_bound(n, n_extra), R.clip_rel_bound(n, n_extra)
    got, want = st[R.ST_NORM], ref[R.ST_NORM]
    print(f"{what}: norm off by {abs(got - want) / want / e_n:.3f} x its bound {e_n:.3g}, "
          f"clip by {abs(st[R.ST_CLIP] - ref[R.ST_CLIP]) / abs(ref[R.ST_CLIP]) / e_c:.3f} x {e_c:.3g}")
    assert abs(got - want) <= e_n * want, (what, got, want, e_n)
    assert abs(st[R.ST_CLIP] - ref[R.ST_CLIP]) <= e_c * abs(ref[R.ST_CLIP]), (what, st[R.ST_CLIP], ref[R.ST_CLIP], e_c)
    assert st[R.ST_STEP] == ref[R.ST_STEP] and st[R.ST_SKIP] == 0.0 == ref[R.ST_SKIP], (what, st, ref)
    assert st[R.ST_NSKIPPED] == ref[R.ST_NSKIPPED], (what, st, ref)
    for i in (R.ST_BC1, R.ST_BC2SQRT):
        assert abs(st[i] - ref[i]) <= R.ulp32(ref[i]), (what, i, st[i], ref[i])


def _worst(got, want, bound):
    """max |got - want| / bound over the finite reference elements; the NaN masks must be equal."""
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = torch.isfinite(want)
    if not bool(ok.any()):
        return 0.0
    return float(((got.double() - want).abs()[ok] / bound[ok]).max())


def _check_adam(new, old, g, ref_state, e_clip, what):
    """Kernel output ``new`` = (p, m, v) of one step from the fp32 tensors ``old`` against the restatement of that step,
    element by element within adam_bounds (12 roundings on the update and one on p, one and three on m and v, plus the error
    allowed on ST_CLIP once and twice -- see its docstring), slice by slice."""
    n = g.numel()
    worst = [0.0, 0.0, 0.0]
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(lo + CHUNK, n))
        args = [x[sl].double() for x in (old[0], g, old[1], old[2])]
        want = R.adam(*args, R.LR, R.BETA1, R.BETA2, R.EPS, ref_state)
        bounds = R.adam_bounds(*args, R.LR, R.BETA1, R.BETA2, R.EPS, ref_state, e_clip)
        for i in range(3):
            worst[i] = max(worst[i], _worst(new[i][sl], want[i], bounds[i]))
    print(f"{what}: p, m, v off by {worst[0]:.3f}, {worst[1]:.3f}, {worst[2]:.3f} x their bounds")
    assert max(worst) <= 1.0, (what, worst)


def _sumsq_state(g, extra, grad_scale, max_norm, loss, threshold, before):
    return R.decide(g.double(), extra, grad_scale, max_norm, R.BETA1, R.BETA2, loss, threshold, before)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the norm sees every element exactly once


@pytest.mark.parametrize("n,one_launch", N_MODE, ids=N_MODE_IDS)
def test_one_hot_norm_is_exact(n, one_launch, options):
    """g = 0 but for one 3.0 -- first, second, last of the float4 part, last of all (the scalar tail), the middle: the norm
    is exactly 3 (9 and 3 are exact in fp32, every other term is 0) and, with max_norm = 10, the coefficient exactly 1.  A
    dropped element reads 0, one counted twice sqrt(18)."""
    options.set("optim_one_launch", one_launch)
    n4 = n >> 2
    where = [4 * n4 - 1, n - 1] if n == BIG else sorted({j for j in (0, 1, 4 * n4 - 1, n - 1, n // 2) if 0 <= j < n})
    k = Optim()
    g = torch.zeros(n, device=DEV)
    for j in where:
        g[j] = 3.0
        k.prepare(g, n, 10.0, 1.0)
        g[j] = 0.0
        st = k.host_state()
        assert st[R.ST_NORM] == 3.0 and st[R.ST_CLIP] == 1.0, (j, st)
        assert k.ticket() == 0
    assert k.host_state()[R.ST_STEP] == len(where)


# ----------------------------------------------------------------------------------------------------------------------
# 2. random norm and decision


def _extras(n, n_extra, case, gen):
    """n_extra squared norms (fp64): about a third of the total in every case."""
    if n_extra == 0:
        return None
    to_norm = R.CLIP_CASES[case][0]
    total = to_norm ** 2 if to_norm is not None else float(n)
    return torch.rand(n_extra, dtype=torch.float64, device=DEV, generator=gen) * (total / (1.5 * n_extra))


def _decision_cases(n, one_launch, cases, options, seed):
    options.set("optim_one_launch", one_launch)
    gen = _gen(seed)
    k = Optim()
    for case, n_extra in cases:
        extra = _extras(n, n_extra, case, gen)
        g, max_norm, grad_scale = R.gradient(n, gen, DEV, case, extra)
        before = k.host_state()
        k.prepare(g, n, max_norm, grad_scale, extra)
        ref = _sumsq_state(g, extra, grad_scale, max_norm, None, 0.0, before)
        _check_decision(k.host_state(), ref, n, n_extra, (n, case, n_extra))
        if case.startswith("inactive"):
            assert k.host_state()[R.ST_CLIP] == grad_scale
        assert k.ticket() == 0
    return k, g, max_norm, grad_scale, extra


@pytest.mark.parametrize("case", list(R.CLIP_CASES))
@pytest.mark.parametrize("n,one_launch", N_MODE[:-1], ids=N_MODE_IDS[:-1])
def test_norm_and_decision_vs_fp64(n, one_launch, case, options):
    """Clip active (max_norm 0.01, unit-variance g), inactive (max_norm at 10 x the norm) and at the edge (||g|| = 1.05e-4
    against 1e-4, where the 1e-6 of the coefficient is 1 % of it), grad_scale 1 and 0.25, with 0, 3 and 300 extra squared
    norms beside n > 0 (300: more than the decision pass has threads) -- then once more from a step counter of 1000.
    Bounds: _check_decision."""
    k, g, max_norm, grad_scale, extra = _decision_cases(n, one_launch, [(case, ne) for ne in (0, 3, 300)], options, seed=n)
    k.state[R.ST_STEP] = 1000.0
    before = k.host_state()
    k.prepare(g, n, max_norm, grad_scale, extra)
    ref = _sumsq_state(g, extra, grad_scale, max_norm, None, 0.0, before)
    assert ref[R.ST_STEP] == 1001.0
    _check_decision(k.host_state(), ref, n, 300, (n, case, "step 1001"))


def test_norm_and_decision_vs_fp64_above_the_grid_cap(options):
    """40,000,003 elements: every thread of the norm pass makes 20 trips (the bound follows: norm_roundings)."""
    _decision_cases(BIG, 0, [("active-scaled", 300)], options, seed=11)


# ----------------------------------------------------------------------------------------------------------------------
# 3. one launch or two: the same bits


@pytest.mark.parametrize("n", [2055, 1_000_003, BIG])
def test_one_launch_equals_two_launches_bit_for_bit(n, options):
    """sumsq_decide_k sums "the same sums in the same order" as sumsq_partial + optim_finalize: state and the blocks'
    partial sums are bit-identical.  Its ticket word is zero after every launch, a skipped one included, and re-arms: three
    consecutive launches on changing g each match the reference."""
    gen = _gen(n + 3)
    nb = R.norm_blocks(n)
    extra = _extras(n, 70, "active", gen)
    g, max_norm, grad_scale = R.gradient(n, gen, DEV, "active-scaled", extra)
    loss = torch.tensor([5.0], device=DEV)
    runs = []
    for one_launch in (0, 1):
        options.set("optim_one_launch", one_launch)
        k = Optim()
        k.prepare(g, n, max_norm, grad_scale, extra)
        taken = [(k.state.clone(), k.partial[:nb].clone())]
        assert k.ticket() == 0
        k.prepare(g, n, max_norm, grad_scale, extra, loss, 2.0)                  # a skipped launch
        taken.append((k.state.clone(), k.partial[:nb].clone()))
        assert k.ticket() == 0 and k.host_state()[R.ST_SKIP] == 1.0
        runs.append((k, taken))
    for (s0, p0), (s1, p1) in zip(runs[0][1], runs[1][1]):
        assert torch.equal(s0, s1) and torch.equal(p0, p1)
    assert bool((runs[0][1][0][1] > 0).all())                                    # every block left a partial sum
    k = runs[1][0]                                                               # (option still 1)
    for step in range(3):
        g, max_norm, grad_scale = R.gradient(n, gen, DEV, "active" if step % 2 else "inactive-scaled", extra)
        before = k.host_state()
        k.prepare(g, n, max_norm, grad_scale, extra)
        ref = _sumsq_state(g, extra, grad_scale, max_norm, None, 0.0, before)
        _check_decision(k.host_state(), ref, n, 70, (n, "one launch", step))
        assert k.ticket() == 0
    assert k.host_state()[R.ST_STEP] == 4.0 and k.host_state()[R.ST_NSKIPPED] == 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. Adam


def _adam_steps(n, one_launch, case, fresh, options, seed, against_clip_step):
    options.set("optim_one_launch", one_launch)
    gen = _gen(seed)
    p, m, v = R.adam_inputs(n, gen, DEV, fresh)
    k = Optim()
    if against_clip_step:
        k2, p2, m2, v2 = Optim(), p.clone(), m.clone(), v.clone()
    e_clip = R.clip_rel_bound(n)
    for step in range(3):
        g, max_norm, grad_scale = R.gradient(n, gen, DEV, case)
        old, before = (p.clone(), m.clone(), v.clone()), k.host_state()
        k.prepare(g, n, max_norm, grad_scale)
        k.adam(p, g, m, v, n)
        ref = _sumsq_state(g, None, grad_scale, max_norm, None, 0.0, before)
        _check_decision(k.host_state(), ref, n, 0, (n, case, step))
        _check_adam((p, m, v), old, g, ref, e_clip, (n, case, "fresh" if fresh else "moments", step))
        if fresh and step == 0:
            assert ref[R.ST_NORM] > max_norm and ref[R.ST_BC1] == 1.0 - R.BETA1       # the real first step, clipped
        if against_clip_step:
            k2.clip_step(p2, g, m2, v2, n, max_norm, grad_scale)
            assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2) and torch.equal(k.state, k2.state)
    assert k.host_state()[R.ST_STEP] == 3.0


@pytest.mark.parametrize("n,one_launch", N_MODE[:-1], ids=N_MODE_IDS[:-1])
def test_adam_three_steps_vs_fp64(n, one_launch, options):
    """p ~ N(0, 1), m ~ 0.1 N(0, 1), v = 0.01 (0.1 + U), lr 1e-3, eps 1e-8, a fresh unit-variance g each step (clipped to
    0.01).  Each step is compared with the restatement of THAT step from the kernel's own fp32 p, m, v, so no tolerance
    has to cover accumulated differences; bounds: _check_adam.  cgv_adam_clip_step on a second copy gives the same bits as
    cgv_optim_prepare_extra + cgv_adam_apply."""
    _adam_steps(n, one_launch, "active", False, options, seed=100 + n, against_clip_step=True)


@pytest.mark.parametrize("case,fresh", [("inactive-scaled", False), ("edge", False), ("active", True), ("edge", True)],
                         ids=["inactive-scaled", "edge", "fresh", "fresh-edge"])
@pytest.mark.parametrize("one_launch", [0, 1], ids=["two-launch", "one-launch"])
def test_adam_other_clip_cases_and_fresh_optimiser(one_launch, case, fresh, options):
    """Coefficient exactly 1 with grad_scale 0.25; ||g|| at the edge of max_norm = 1e-4; m = v = 0 with a clipped gradient
    (v of the size of the clipped g^2: the inputs on which eps on the wrong side of the square root shows)."""
    _adam_steps(4099, one_launch, case, fresh, options, seed=7, against_clip_step=True)


def test_adam_above_the_grid_cap(options):
    """40,000,003 elements: 16384 blocks, a stride of 4,194,304 float4 against n4 = 10,000,000."""
    _adam_steps(BIG, 0, "active", False, options, seed=8, against_clip_step=False)


# ----------------------------------------------------------------------------------------------------------------------
# 5. ranges of an arena


SENTINEL = -12345.5


@pytest.mark.parametrize("n", [3, 2045, 4099])
@pytest.mark.parametrize("lo", [0, 4, 2048])
@pytest.mark.parametrize("one_launch", [0, 1], ids=["two-launch", "one-launch"])
def test_apply_on_a_sub_range_writes_nothing_outside(one_launch, lo, n, options):
    """Trainer._adam_apply(lo, hi): pointers offset into the arena.  Outside [lo, lo + n) p, m, v and g keep their bits;
    inside they match the reference (bounds of _check_adam; sgd_bound)."""
    options.set("optim_one_launch", one_launch)
    gen = _gen(1000 * lo + n)
    total = lo + n + 64
    inside = torch.zeros(total, dtype=torch.bool, device=DEV)
    inside[lo:lo + n] = True
    arena = [torch.full((total,), SENTINEL, device=DEV) for _ in range(4)]        # p, g, m, v
    p0, m0, v0 = R.adam_inputs(n, gen, DEV)
    g0, max_norm, grad_scale = R.gradient(n, gen, DEV, "active")
    for a, x in zip(arena, (p0, g0, m0, v0)):
        a[lo:lo + n] = x
    start = [a.clone() for a in arena]
    p, g, m, v = (a[lo:] for a in arena)
    k = Optim()
    k.prepare(g, n, max_norm, grad_scale)
    ref = _sumsq_state(g0, None, grad_scale, max_norm, None, 0.0, R.new_state())
    _check_decision(k.host_state(), ref, n, 0, (lo, n))
    e_clip = R.clip_rel_bound(n)

    k.adam(p, g, m, v, n)
    for a, s in zip(arena, start):
        assert torch.equal(a[~inside], s[~inside])
    assert torch.equal(arena[1], start[1])                                        # g is read only
    _check_adam([arena[i][lo:lo + n] for i in (0, 2, 3)], (p0, m0, v0), g0, ref, e_clip, (lo, n, "adam"))

    p1 = arena[0][lo:lo + n].clone()
    lr = R.f32(0.05)
    k.sgd(p, g, n, lr)
    for i in (1, 2, 3):
        assert torch.equal(arena[i][~inside], start[i][~inside])
    assert torch.equal(arena[0][~inside], start[0][~inside]) and torch.equal(arena[1], start[1])
    want, bound = R.sgd(p1.double(), g0.double(), lr, ref), R.sgd_bound(p1.double(), g0.double(), lr, ref, e_clip)
    assert _worst(arena[0][lo:lo + n], want, bound) <= 1.0


def test_empty_range_and_misaligned_pointers():
    """n = 0 returns 0 and launches nothing; a pointer that is not 16-byte aligned is refused (CGV_E_BADARG) before any
    launch."""
    lib = _lib.load()
    gen = _gen(5)
    n = 64
    p, m, v = R.adam_inputs(n, gen, DEV)
    g, max_norm, grad_scale = R.gradient(n, gen, DEV, "active")
    k = Optim()
    k.prepare(g, n, max_norm, grad_scale)
    start = [x.clone() for x in (p, g, m, v, k.state)]
    st, stream = _lib.ptr(k.state), _lib.stream_ptr()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip((p, g, m, v, k.state), start))

    assert lib.cgv_adam_apply(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, R.LR, R.BETA1, R.BETA2, R.EPS, st, stream) == 0
    assert lib.cgv_sgd_apply(p.data_ptr(), g.data_ptr(), 0, R.LR, st, stream) == 0
    assert untouched()
    for off in ([4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 4, 0], [0, 0, 0, 4], [4, 4, 4, 4]):          # lo = 1
        ptrs = [x.data_ptr() + o for x, o in zip((p, g, m, v), off)]
        assert lib.cgv_adam_apply(*ptrs, n - 4, R.LR, R.BETA1, R.BETA2, R.EPS, st, stream) == -1
        assert b"aligned" in lib.cgv_last_error_string()
    for off in ([4, 0], [0, 4], [4, 4]):
        assert lib.cgv_sgd_apply(p.data_ptr() + off[0], g.data_ptr() + off[1], n - 4, R.LR, st, stream) == -1
        assert b"aligned" in lib.cgv_last_error_string()
    assert lib.cgv_optim_prepare_extra(g.data_ptr() + 4, n - 4, None, 0, R.BETA1, R.BETA2, max_norm, grad_scale, None, 0.0, st,
                                       _lib.ptr(k.partial), stream) == -1
    assert b"aligned" in lib.cgv_last_error_string()
    assert untouched() and k.ticket() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 6. SGD


def _sgd_steps(n, one_launch, options, seed):
    options.set("optim_one_launch", one_launch)
    gen = _gen(seed)
    p = torch.randn(n, device=DEV, generator=gen)
    k = Optim()
    lr, e_clip = R.f32(0.05), R.clip_rel_bound(n)
    for case in ("active-scaled", "inactive-scaled"):
        g, max_norm, grad_scale = R.gradient(n, gen, DEV, case)
        old, before = p.clone(), k.host_state()
        k.prepare(g, n, max_norm, grad_scale)
        k.sgd(p, g, n, lr)
        ref = _sumsq_state(g, None, grad_scale, max_norm, None, 0.0, before)
        worst = 0.0
        for lo in range(0, n, CHUNK):
            sl = slice(lo, min(lo + CHUNK, n))
            pd, gd = old[sl].double(), g[sl].double()
            worst = max(worst, _worst(p[sl], R.sgd(pd, gd, lr, ref), R.sgd_bound(pd, gd, lr, ref, e_clip)))
        print(f"{n} {case}: p off by {worst:.3f} x its bound")
        assert worst <= 1.0, (n, case, worst)
        assert not torch.equal(p, old)


@pytest.mark.parametrize("n,one_launch", N_MODE[:-1], ids=N_MODE_IDS[:-1])
def test_sgd_vs_fp64(n, one_launch, options):
    """p -= lr clip g with grad_scale 0.25, clip active and inactive.  Bound: one fma, 2^-24 (|p| + |lr clip g|), plus the
    error allowed on ST_CLIP (sgd_bound)."""
    _sgd_steps(n, one_launch, options, seed=200 + n)


def test_sgd_above_the_grid_cap(options):
    """40,000,003 elements: 4096 blocks, 10 trips per thread."""
    _sgd_steps(BIG, 0, options, seed=9)


# ----------------------------------------------------------------------------------------------------------------------
# 7. the skip rule at kernel level


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
@pytest.mark.parametrize("one_launch", [0, 1], ids=["two-launch", "one-launch"])
def test_skip_rule_at_kernel_level(one_launch, optimizer, options):
    """loss >= 2.0 or NaN skips (scripts/utils.py:145): below the threshold a step; exactly 2.0, NaN and +inf skipped --
    p, m, v keep their bits, the counter, the coefficient and the bias corrections stay, ST_NORM is written, ST_NSKIPPED
    counts; the next call is a normal step with the counter one up."""
    options.set("optim_one_launch", one_launch)
    n = 4099
    gen = _gen(17)
    p, m, v = R.adam_inputs(n, gen, DEV)
    k = Optim()
    lr = R.LR if optimizer == "adam" else R.f32(0.05)
    loss = torch.zeros(1, device=DEV)
    steps = skipped = 0
    for value in (1.5, 2.0, float("nan"), float("inf"), 1.9999999):
        loss.fill_(value)
        g, max_norm, grad_scale = R.gradient(n, gen, DEV, "active-scaled")
        old, before = (p.clone(), m.clone(), v.clone()), k.host_state()
        k.prepare(g, n, max_norm, grad_scale, None, loss, 2.0)
        k.adam(p, g, m, v, n) if optimizer == "adam" else k.sgd(p, g, n, lr)
        st = k.host_state()
        ref = _sumsq_state(g, None, grad_scale, max_norm, float(loss.item()), 2.0, before)
        assert abs(st[R.ST_NORM] - ref[R.ST_NORM]) <= R.norm_rel_bound(n) * ref[R.ST_NORM] and st[R.ST_NORM] != before[R.ST_NORM]
        assert k.ticket() == 0
        if value < 2.0:
            steps += 1
            assert st[R.ST_SKIP] == 0.0 and st[R.ST_STEP] == before[R.ST_STEP] + 1 == steps
            _check_decision(st, ref, n, 0, (optimizer, value))
            assert not torch.equal(p, old[0])
            if optimizer == "adam":
                _check_adam((p, m, v), old, g, ref, R.clip_rel_bound(n), (optimizer, value))
        else:
            skipped += 1
            assert st[R.ST_SKIP] == 1.0 == ref[R.ST_SKIP]
            assert torch.equal(p, old[0]) and torch.equal(m, old[1]) and torch.equal(v, old[2])
            for i in (R.ST_STEP, R.ST_CLIP, R.ST_BC1, R.ST_BC2SQRT):
                assert st[i] == before[i], (value, i)
        assert st[R.ST_NSKIPPED] == skipped
    assert (steps, skipped) == (2, 3)


# ----------------------------------------------------------------------------------------------------------------------
# 8. non-finite gradients with a finite loss (torch's behaviour: tests/test_optim_cpu.py)


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("one_launch", [0, 1], ids=["two-launch", "one-launch"])
def test_non_finite_gradient(one_launch, bad, options):
    """One NaN in the scalar tail: ST_NORM NaN and every p, m, v NaN.  One +inf: ST_CLIP == 0, NaN at that element and a
    step on a zero gradient elsewhere (bounds of _check_adam).  SGD likewise."""
    options.set("optim_one_launch", one_launch)
    n, j = 4099, 4098
    gen = _gen(23)
    p, m, v = R.adam_inputs(n, gen, DEV)
    g, max_norm, grad_scale = R.gradient(n, gen, DEV, "active")
    g[j] = float(bad)
    old = (p.clone(), m.clone(), v.clone())
    q = p.clone()
    k = Optim()
    k.prepare(g, n, max_norm, grad_scale, None, torch.tensor([0.5], device=DEV), 2.0)
    k.adam(p, g, m, v, n)
    k.sgd(q, g, n, R.f32(0.05))
    st = k.host_state()
    ref = _sumsq_state(g, None, grad_scale, max_norm, 0.5, 2.0, R.new_state())
    assert st[R.ST_SKIP] == 0.0 and st[R.ST_STEP] == 1.0 and k.ticket() == 0
    if bad == "nan":
        assert st[R.ST_NORM] != st[R.ST_NORM] and st[R.ST_CLIP] != st[R.ST_CLIP]
        for x in (p, m, v, q):
            assert bool(torch.isnan(x).all())
        return
    assert st[R.ST_NORM] == float("inf") and st[R.ST_CLIP] == 0.0 == ref[R.ST_CLIP]
    only = torch.zeros(n, dtype=torch.bool, device=DEV)
    only[j] = True
    for x in (p, m, v, q):
        assert torch.equal(torch.isnan(x), only)
    _check_adam((p, m, v), old, g, ref, R.clip_rel_bound(n), ("inf",))
    zero = R.adam(old[0].double(), torch.zeros(n, dtype=torch.float64, device=DEV), old[1].double(), old[2].double(), R.LR,
                  R.BETA1, R.BETA2, R.EPS, ref)
    want = R.adam(old[0].double(), g.double(), old[1].double(), old[2].double(), R.LR, R.BETA1, R.BETA2, R.EPS, ref)
    for a, b in zip(want, zero):
        assert torch.equal(a[~only], b[~only])                                   # the reference: a zero gradient elsewhere
    assert torch.equal(q[~only], old[0][~only])                                  # SGD with a zero coefficient


# ----------------------------------------------------------------------------------------------------------------------
# 9. captured


@pytest.mark.parametrize("one_launch", [0, 1], ids=["two-launch", "one-launch"])
def test_captured_steps_equal_eager_steps(one_launch, options):
    """cgv_optim_prepare_extra + cgv_adam_apply captured in one graph (one stream, no branches), replayed three times with
    a new g copied into the static buffer: state, p, m, v bit-identical to the same three eager steps; the counter reads 3."""
    options.set("optim_one_launch", one_launch)
    n = 4099
    gen = _gen(31)
    p0, m0, v0 = R.adam_inputs(n, gen, DEV)
    grads = [R.gradient(n, gen, DEV, "active")[0] for _ in range(3)]
    extra = _extras(n, 3, "active", gen)
    max_norm = R.CLIP_CASES["active"][1]
    runs = []
    for captured in (False, True):
        k, g = Optim(), torch.zeros(n, device=DEV)
        p, m, v = p0.clone(), m0.clone(), v0.clone()

        def step():
            k.prepare(g, n, max_norm, 1.0, extra)
            k.adam(p, g, m, v, n)

        graph = None
        if captured:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            torch.cuda.synchronize()
            assert k.host_state()[R.ST_STEP] == 0.0                              # nothing ran during the capture
        for x in grads:
            g.copy_(x)
            graph.replay() if captured else step()
        torch.cuda.synchronize()
        assert k.ticket() == 0
        runs.append((k.state.clone(), p, m, v))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[1][0][R.ST_STEP]) == 3.0 and not torch.equal(runs[1][1], p0)
