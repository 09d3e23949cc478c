"""The loss-skip rule on one GPU (scripts/utils.py:145): a step whose loss is >= 200 gamma or NaN runs no backward, no
clip and no optimizer step.  Here the decision is taken on the device (csrc/optim.hip: ST_SKIP), and every kernel that
applies Adam or SGD -- the flat passes, the rank-update launches, the strip launches with the Adam epilogue -- must return
early on it.  The skip is triggered through the supplied noise, so a captured step takes it as well: eps scaled by 100
(loss above the threshold) or an eps with one NaN entry (NaN loss)."""
import pytest
import torch

from coarsegrainingvae_amd.trainer import Trainer
from oracle import cgvae_oracle as O
from test_full_size_parity import _check_moments, _check_parameters, _setup, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = 32
ST_STEP, ST_BC1, ST_BC2SQRT, ST_SKIP, ST_NSKIPPED = 0, 3, 4, 5, 6       # csrc/cgv_common.h

# (rank_update, defer_update, optimizer, rank_rows_mfma, frames).  The rank update only runs with Adam and without a
# deferred update, so it is varied there; the last entry takes the two-pass MFMA rank update and its strip launches (8
# frames: the three stacked heads' 72 rows), beside the FMA-per-row one of the 24-row layers.
CONFIGS = [(True, False, "adam", -1, 4), (False, False, "adam", -1, 4), (False, True, "adam", -1, 4),
           (False, False, "sgd", -1, 4), (False, True, "sgd", -1, 4), (True, False, "adam", 128, 8)]
IDS = ["rank", "norank", "defer", "sgd", "sgd-defer", "mfma"]
LR = {"adam": 1e-4, "sgd": 0.05}


def _noise(n_beads, seeds, kind=None):
    gen = torch.Generator().manual_seed(seeds)
    e = torch.randn(n_beads, F, generator=gen)
    if kind == "large":
        e = e * 1e2
    elif kind == "nan":
        e[n_beads // 2, F // 3] = float("nan")
    return e


def _trainer(cfg, options, frames=None):
    rank, defer, opt, mfma, n_frames = cfg
    options.set("rank_rows_mfma", mfma)
    w, batch, cpu_batch, model, hp, P = _setup("dipeptide", frames or n_frames, F, enc=2, dec=2)
    tr = Trainer(model, lr=LR[opt], beta=w["beta"], gamma=w["gamma"], rank_update=rank, defer_update=defer, optimizer=opt)
    return w, batch, cpu_batch, model, hp, P, tr


def _step(tr, batch, eps, replay, train=True):
    """One step; ``replay``: through a captured graph (captured now if this mode / pending state has none yet)."""
    eps = eps.to(DEV)
    if replay and not tr.has_graph(train):
        tr.capture(batch, warmup=0, train=train, eps=eps)
    before = tr.replays
    loss = float(tr.step(batch, eps=eps, train=train))
    assert tr.replays == before + (1 if replay else 0)
    return loss


def _assert_skip_worthy(loss, kind, gamma):
    if kind == "nan":
        assert loss != loss, loss
    else:
        assert loss >= 200.0 * gamma, (loss, 200.0 * gamma)        # the branch condition really holds


def _rank_path_taken(tr, cfg):
    rank, defer, opt, mfma, _frames = cfg
    if rank and not defer and opt == "adam":
        assert tr._rank_hi > 0 and tr.rank_steps >= 1 and tr.rank_fallbacks == 0
        if mfma > 0:
            assert tr.rank_steps_mfma >= 1


@pytest.mark.parametrize("kind", ["large", "nan"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_skipped_step_leaves_parameters_moments_and_counters(captured, cfg, kind, options):
    """A skipped step: parameters, m and v bit-identical; step counter and bias corrections unchanged; the skip counted."""
    w, batch, _cpu, _model, _hp, _P, tr = _trainer(cfg, options)
    n = batch["CG_nxyz"].shape[0]
    for k in range(2):                                              # arena, then the step the graph would capture
        _step(tr, batch, _noise(n, k), replay=False)
    tr.flush()                                                      # (deferred update: nothing may be pending)
    p0, st0 = tr.arena.p.clone(), tr.state.clone()
    m0, v0 = (tr.m.clone(), tr.v.clone()) if tr.m is not None else (None, None)
    skipped0 = tr.skipped_steps()

    loss = _step(tr, batch, _noise(n, 7, kind), replay=captured)
    _assert_skip_worthy(loss, kind, w["gamma"])
    tr.flush()                                                      # a deferred update of a skipped step applies nothing
    torch.cuda.synchronize()
    _rank_path_taken(tr, cfg)
    st = tr.state.cpu()
    assert float(st[ST_SKIP]) == 1.0
    assert torch.equal(tr.arena.p, p0), "a skipped step moved parameters"
    if m0 is not None:
        assert torch.equal(tr.m, m0) and torch.equal(tr.v, v0), "a skipped step touched Adam's moments"
    for i, name in ((ST_STEP, "step counter"), (ST_BC1, "bias correction 1"), (ST_BC2SQRT, "bias correction 2")):
        assert float(st[i]) == float(st0[i]), f"a skipped step changed the {name}: {float(st0[i])} -> {float(st[i])}"
    assert float(st[ST_NSKIPPED]) == float(st0[ST_NSKIPPED]) + 1
    assert tr.skipped_steps() == skipped0 + 1

    # ... and the next step is a normal one again
    _step(tr, batch, _noise(n, 8), replay=captured)
    tr.flush()
    torch.cuda.synchronize()
    assert float(tr.state[ST_SKIP]) == 0.0 and float(tr.state[ST_STEP]) == float(st0[ST_STEP]) + 1
    assert not torch.equal(tr.arena.p, p0)


class ReferenceLoop:
    """scripts/utils.py:110-157 literally, on the CPU oracle: forward, loss; a loss >= 200 gamma or NaN skips the rest
    (no zero_grad, no backward, no clip, no optimizer step); else backward, clip_grad_norm_(0.01), Adam / SGD step."""

    def __init__(self, cpu_batch, P, hp, w, lr, optimizer):
        self.batch, self.P, self.hp, self.w, self.lr, self.optimizer = cpu_batch, P, hp, w, lr, optimizer
        self.live, self.opt, self.skipped = None, None, 0

    def step(self, eps):
        out = O.model_forward(self.batch, self.P, self.hp, eps=eps)
        loss = O.loss_terms(out, self.batch, self.w["beta"], self.w["gamma"])[0]
        lv = float(loss.detach())
        if lv >= self.w["gamma"] * 200.0 or lv != lv:
            self.skipped += 1
            return lv
        for p in self.P.values():
            p.grad = None
        loss.backward()
        if self.opt is None:
            self.live = {k: p for k, p in self.P.items() if p.grad is not None}
            params = list(self.live.values())
            self.opt = torch.optim.Adam(params, lr=self.lr) if self.optimizer == "adam" else torch.optim.SGD(params, lr=self.lr)
        torch.nn.utils.clip_grad_norm_(list(self.live.values()), 0.01)
        self.opt.step()
        return lv


SEQUENCE = [None, None, "large", None, None]           # two normal steps (arena, rank update), a skip, two normal steps


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_trajectory_with_a_skipped_step_matches_the_reference_loop(captured, cfg, options):
    """normal, normal, skip, normal, normal against the reference loop: if the skip advanced the step counter, every later
    bias correction would differ; if it touched the moments or applied an update, they and the parameters would."""
    w, batch, cpu_batch, model, hp, P, tr = _trainer(cfg, options)
    opt = cfg[2]
    P0 = {k: v.detach().clone() for k, v in P.items()}
    ref = ReferenceLoop(cpu_batch, P, hp, w, LR[opt], opt)
    n = batch["CG_nxyz"].shape[0]
    for k, kind in enumerate(SEQUENCE):
        eps = _noise(n, 20 + k, kind)
        want = ref.step(eps)
        got = _step(tr, batch, eps, replay=captured and k >= 2)
        if kind is None:
            assert abs(got - want) <= 1e-4 * abs(want), (k, got, want)
        else:
            _assert_skip_worthy(got, kind, w["gamma"])
            _assert_skip_worthy(want, kind, w["gamma"])
    tr.flush()
    torch.cuda.synchronize()
    _rank_path_taken(tr, cfg)
    updates = len(SEQUENCE) - 1
    assert ref.skipped == 1 and tr.skipped_steps() == 1
    assert int(tr.state[ST_STEP].item()) == updates
    if opt == "adam":
        _check_moments(tr, model, ref, "after the skipped step")
        _check_parameters(tr, model, ref, P0, updates, LR[opt], "after the skipped step")
    else:
        # SGD: the parameters' displacement (lr x the clipped gradients of the four applied steps) against the reference's,
        # to 1e-3 of the tensor's largest displacement plus the fp32 rounding of four updates on each side (an update
        # applied on the skipped step would add a quarter to it)
        names = {id(p): k for k, p in model.named_parameters()}
        for p in tr.arena.params:
            k = names[id(p)]
            moved = ref.live[k].detach().double() - P0[k].double()
            got = p.detach().cpu().double() - P0[k].double()
            bound = 1e-3 * moved.abs().max() + 8 * 2.0 ** -23 * P0[k].double().abs()
            worst = float(((got - moved).abs() / bound.clamp_min(1e-30)).max())
            assert worst <= 1.0, f"{k}: SGD displacement off by {worst:.2f} x the bound"


def _state(tr):
    tr.flush()
    torch.cuda.synchronize()
    return ([tr.arena.p.clone()] + ([tr.m.clone(), tr.v.clone()] if tr.m is not None else []), tr.state.clone())


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_a_nan_step_leaves_no_trace(captured, cfg, options):
    """After a NaN-loss step (NaN everywhere in its backward: loss-tail tickets, split-K partials, rank sums of squares,
    the gradient arena) the next steps equal those of a trainer that never saw that step."""
    runs = []
    for with_nan in (True, False):
        _w, batch, _cpu, _model, _hp, _P, tr = _trainer(cfg, options)
        n = batch["CG_nxyz"].shape[0]
        losses = []
        for k in range(5):
            if k == 2 and not with_nan:
                continue
            loss = _step(tr, batch, _noise(n, 30 + k, "nan" if k == 2 else None), replay=captured and k >= 2)
            if k == 2:
                assert loss != loss
            else:
                losses.append(loss)
        runs.append((losses, _state(tr), tr.skipped_steps()))
    (l_nan, (t_nan, s_nan), sk_nan), (l_ref, (t_ref, s_ref), sk_ref) = runs
    assert sk_nan == 1 and sk_ref == 0
    for a, b in zip(l_nan, l_ref):
        assert abs(a - b) <= 1e-6 * abs(b), (l_nan, l_ref)
    for a, b in zip(t_nan, t_ref):
        assert rel_err(a, b) <= 1e-6
    assert float(s_nan[ST_STEP]) == float(s_ref[ST_STEP])


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_deferred_update_across_a_skip_worthy_validation_step(captured, options):
    """defer_update: a training step leaves its parameter pass for the next step -- here a validation step whose loss would
    be skipped (backward only, no optimizer: utils.py:145, 159-160).  train, eval, train must equal the same sequence with
    the update applied at the end of each training step."""
    runs = []
    for defer in (True, False):
        w, batch, _cpu, _model, _hp, _P, tr = _trainer((False, defer, "adam", -1, 4), options)
        n = batch["CG_nxyz"].shape[0]
        losses = []
        for k, (train, kind) in enumerate([(True, None), (True, None), (True, None), (False, "large"), (True, None),
                                           (True, None)]):
            loss = _step(tr, batch, _noise(n, 40 + k, kind), replay=captured and k >= 2, train=train)
            if kind:
                _assert_skip_worthy(loss, kind, w["gamma"])
            losses.append(loss)
        assert tr.skipped_steps() == 0
        runs.append((losses, _state(tr)))
    (l_def, (t_def, s_def)), (l_ref, (t_ref, s_ref)) = runs
    for a, b in zip(l_def, l_ref):
        assert abs(a - b) <= 1e-6 * abs(b), (l_def, l_ref)
    for a, b in zip(t_def, t_ref):
        assert rel_err(a, b) <= 1e-6
    assert float(s_def[ST_STEP]) == float(s_ref[ST_STEP]) == 5
