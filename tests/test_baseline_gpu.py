"""The baseline models on the device (csrc/baseline.hip, baseline.py, run_baseline.py): step parity of the linear kinds
against the reference's stored outputs and the fp64 restatement in both kernel forms, bitwise reproducibility, forward
mode, the loss kernel of the MLP, the trajectory fixtures, forced forms at 300 atoms, and the CLI end to end.

Tolerances.  Deviation = max |got - fp64| / max |fp64| (baseline_restatement.rel_dev).  The generator measured the
deviation of the REFERENCE's own fp32 outputs from the fp64 restatement and stored it in every fixture (``dev_*``); a kernel
result is allowed four times the value stored IN ITS OWN FIXTURE for that quantity (``partial_*`` quantities have their own).
The two scalar losses alone have a floor of 2^-24 = 6.0e-08: they are returned as one fp32 number, and rounding the exact
value to fp32 already moves it by up to half an ulp, 2^-24 of its size, while a stored loss can sit closer to fp64 than
that by luck (1.7e-09 in one fixture).  Arrays have no floor.  Stored values, smallest .. largest over the fixtures
(linear / equilinear):
    xyz_recon 1.6e-07..2.0e-07 / 1.3e-07..2.2e-07   loss_recon 1.7e-09..3.2e-08 / 1.5e-08..4.5e-08
    loss_dist 1.6e-08..6.1e-08 / 3.7e-08..1.2e-07   grad 9.9e-08..2.3e-07 / 1.2e-07..2.5e-06
    B_after1 2.8e-08..4.4e-08 / 2.9e-08..4.5e-08    B_after10 9.3e-08..1.5e-06 / 3.0e-07..2.6e-06
    trajectory B_final 3.7e-07 / 4.7e-07, loss log 1.4e-07 / 7.7e-08
MLP fixtures: xyz_recon 1.8e-07..2.9e-07, loss_recon 5.5e-08..1.1e-07, loss_dist 6.6e-08..7.6e-08, grad_recon
8.0e-08..2.7e-07, parameter gradients 1.2e-07..2.0e-07.
The trainer holds its intermediates in double (csrc/baseline.hip), so its results sit at the rounding of the fp32 outputs.
Measured on an MI355X, largest over the fixtures, identical in both forms (linear / equilinear; in brackets the largest
fraction of its own bound that any fixture used):
    xyz_recon 4.7e-08 / 4.0e-08 (0.10)   loss_recon 3.2e-08 / 4.6e-08 (0.25)   loss_dist 1.6e-08 / 2.7e-08 (0.25)
    grad 4.8e-08 / 4.3e-08 (0.11)        B_after1 4.5e-08 / 4.5e-08 (0.25)     B_after10 2.9e-07 / 2.4e-07 (0.41)
    trajectory B_final equilinear 3.9e-07 of 1.9e-06, loss log 3.8e-08 of 3.1e-07
MLP: loss_recon <= 2.8e-08, loss_dist <= 2.7e-08, grad_recon <= 1.4e-07, xyz_recon <= 2.3e-07, parameter gradients <= 1.6e-07,
each below 0.4 of its fixture's bound.  Every test prints its figures (``PARITY`` / ``LOSS`` / ``MLP`` / ``TRAJ`` / ``FORCED``).
The resident and the global form run the same arithmetic in the same order and are required to agree bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_restatement as R  # noqa: E402

from coarsegrainingvae_amd import baseline as B, run_baseline  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = [B.RESIDENT, B.GLOBAL]
FORM_IDS = ["resident", "global"]
_RESTATED = {}
SCALAR_FLOOR = 2.0 ** -24                   # half an ulp of an fp32 loss value, relative
SCALARS = ("loss_recon", "loss_dist", "partial_loss_recon", "partial_loss_dist")


def _allowed(f, q):
    """Four times the deviation the reference's own fp32 result has in THIS fixture; the scalar losses not below half an ulp."""
    bound = 4.0 * float(f["dev_" + q])
    return max(bound, SCALAR_FLOOR) if q in SCALARS else bound


def _restated(golden, name):
    if name not in _RESTATED:
        _RESTATED[name] = R.restate_step_fixture(golden(name))
    return _RESTATED[name]


def _model(f, B0=None):
    kind, K, knn, n = str(f["kind"]), int(f["K"]), int(f["knn"]), int(f["xyz"].shape[1])
    pool = B.FixedPool(f["mapping"], K)
    m = B.Baseline(pool, K, n) if kind == "linear" else B.EquiLinear(pool, K, n, False, knn)
    m.load_reference_state({"B": torch.from_numpy(f["B"] if B0 is None else B0).clone()})
    return m.cuda()


def _same_batch_order(bsz, steps):
    return np.tile(np.arange(bsz, dtype=np.int32), (steps, 1))


def _check(tag, got, want, f):
    failures = []
    for q, a in got.items():
        allowed, dev, dev_ref = _allowed(f, q), R.rel_dev(a, want[q]), R.rel_dev(a, f[q])
        print(f"PARITY {tag} {q}: {dev:.2e} / {allowed:.2e}  (against the stored fp32 output {dev_ref:.2e})")
        if dev > allowed or dev_ref > allowed + float(f["dev_" + q]):   # the stored output sits dev_q from fp64: triangle
            failures.append((q, dev, dev_ref, allowed))
    assert not failures, failures


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", R.STEP_FIXTURES)
def test_step_parity_with_the_reference(golden, name, form):
    f = golden(name)
    kind, bsz = str(f["kind"]), int(f["xyz"].shape[0])
    want = _restated(golden, name)
    args = dict(lr=float(f["lr"]), gamma=float(f["gamma"]), edges=f["edges"], form=form)
    m = _model(f)
    order = _same_batch_order(bsz, 10)
    log, out = m.run_steps(f["xyz"], order, bsz, 0, 1, mode=B.TRAIN, probe=True, **args)
    n3 = bsz * m.n_atoms * 3
    got = {"xyz_recon": out[:n3].view(bsz, -1, 3).cpu().numpy(), "grad": out[n3:].view_as(m.B).cpu().numpy(),
           "loss_recon": float(log[0, 0]), "loss_dist": float(log[0, 1]), "B_after1": m.B.detach().cpu().numpy()}
    m.run_steps(f["xyz"], order, bsz, 1, 9, mode=B.TRAIN, **args)
    got["B_after10"] = m.B.detach().cpu().numpy()
    if "xyz_partial" in f:                                              # the epoch's last batch holds 3 of 4 frames
        p = _model(f)
        frames = np.concatenate([f["xyz"], f["xyz_partial"]])
        # two steps with lr = 0 (B stays put): the probe holds the second, the partial batch
        log, out = p.run_steps(frames, np.arange(bsz + 3, dtype=np.int32)[None], bsz, 0, 2, mode=B.TRAIN, probe=True, **dict(args, lr=0.0))
        assert torch.equal(p.B.detach().cpu(), torch.from_numpy(f["B"]))
        got.update(partial_xyz_recon=out[:n3].view(bsz, -1, 3)[:3].cpu().numpy(), partial_grad=out[n3:].view_as(p.B).cpu().numpy(),
                   partial_loss_recon=float(log[1, 0]), partial_loss_dist=float(log[1, 1]))
    _check(f"{name} {B.FORM_NAMES[form]}", got, want, f)


def test_determinism_and_agreement_of_the_forms(golden):
    """One launch of ten steps = ten launches of one = a repeated launch, bit for bit; resident = global, bit for bit."""
    for name in ("g19_baseline_step_equilinear_n166_k6_knn5_g05", "g19_baseline_step_linear_n22_k3_knn2_g05"):
        f = golden(name)
        bsz = int(f["xyz"].shape[0])
        frames = np.concatenate([f["xyz"], f["xyz_partial"]]) if "xyz_partial" in f else f["xyz"]
        order = np.tile(np.arange(frames.shape[0], dtype=np.int32), (10, 1))
        runs = []
        for form in FORMS:
            for split in (False, True, False):
                m = _model(f)
                logs = [m.run_steps(frames, order, bsz, s, c, mode=B.TRAIN, lr=1e-3, gamma=0.5, edges=f["edges"], form=form)[0]
                        for s, c in ([(i, 1) for i in range(10)] if split else [(0, 10)])]
                runs.append((m.B.detach().cpu(), m.moments[0].cpu(), m.moments[1].cpu(), torch.cat(logs).cpu()))
        assert not torch.equal(runs[0][0], torch.from_numpy(f["B"]))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert torch.equal(a, b)


def _schedule_case(kind):
    """The shared schedule rule on the smallest table that reaches it: 5 atoms in beads [0,0,1,1,1], 3 hyperedges, 8 frames,
    two epochs of n_train = 7 in batches of 3 (3 steps per epoch, the last batch of an epoch holds 1 frame), 6 steps.
    Returns the inputs and the fp64 restatement walking the same table: B after the 6 steps and the [6, 2] loss log."""
    n, K, knn, batch, gamma, lr = 5, 2, 1, 3, 0.5, 1e-3
    gen = torch.Generator().manual_seed(17)
    xyz = (torch.cumsum(torch.randn(8, n, 3, generator=gen) * 1.5, dim=1) + 3.0).numpy()     # coordinates of a few Angstrom
    mapping, edges = np.array([0, 0, 1, 1, 1]), np.array([[0, 1], [1, 2], [2, 4]])
    order = np.array([[3, 0, 7, 5, 1, 6, 2], [4, 2, 0, 6, 7, 1, 3]], dtype=np.int32)
    B0 = (0.01 * torch.randn(*((K, n) if kind == "linear" else (n, K * knn)), generator=gen)).numpy()
    batches = [xyz[row[s:s + batch]] for row in order for s in range(0, order.shape[1], batch)]
    (want_B,), want_log = R.adam_steps(kind, [B0], batches, mapping, edges, gamma, K, knn, lr=lr)
    return dict(xyz=xyz, mapping=mapping, edges=edges, order=order, B=B0, K=K, knn=knn, batch=batch, gamma=gamma, lr=lr), want_B, want_log


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kind", R.LINEAR_KINDS)
def test_schedule_partial_batches_and_epoch_boundary(golden, kind, form):
    """(a) one call of 6 steps = calls of 1, 2 and 3 steps, bit for bit, in B, both Adam moments and the loss log; (b) B and
    every row of the loss log against the fp64 restatement walking the same table, under the bound of
    test_step_parity_with_the_reference: four times the reference's own deviation as stored in a fixture (_allowed).  No
    fixture holds this schedule; the bounds are those of the kind's knn = 1, gamma = 0.5 step fixture, the 6-step B under its
    B_after10 entry (the loosest of that horizon) and the loss rows under loss_recon / loss_dist."""
    case, want_B, want_log = _schedule_case(kind)
    f = golden(f"g19_baseline_step_{kind}_n22_k3_knn1_g05")
    runs = []
    for split in ((6,), (1, 2, 3)):
        pool = B.FixedPool(case["mapping"], case["K"])
        m = B.Baseline(pool, case["K"], 5) if kind == "linear" else B.EquiLinear(pool, case["K"], 5, False, case["knn"])
        m.load_reference_state({"B": torch.from_numpy(case["B"]).clone()})
        m, logs, done = m.cuda(), [], 0
        for cnt in split:
            logs.append(m.run_steps(case["xyz"], case["order"], case["batch"], done, cnt, mode=B.TRAIN, lr=case["lr"],
                                    gamma=case["gamma"], edges=case["edges"], form=form)[0])
            done += cnt
        runs.append((m.B.detach().cpu(), m.moments[0].cpu(), m.moments[1].cpu(), torch.cat(logs).cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    got_B, got_log = runs[0][0].numpy(), runs[0][3].numpy()
    assert got_log.shape == (6, 2) and not np.array_equal(got_B, case["B"])
    devs = {"B_after10": R.rel_dev(got_B, want_B), "loss_recon": max(R.rel_dev(got_log[s, 0], want_log[s, 0]) for s in range(6)),
            "loss_dist": max(R.rel_dev(got_log[s, 1], want_log[s, 1]) for s in range(6))}
    print(f"SCHEDULE {kind} {B.FORM_NAMES[form]} " + " ".join(f"{q}={d:.2e}/{_allowed(f, q):.2e}" for q, d in devs.items()))
    for q, d in devs.items():
        assert d <= _allowed(f, q), (q, d, _allowed(f, q))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_forward_mode(golden, form):
    f = golden("g19_baseline_step_equilinear_n22_k3_knn2_g05")
    bsz = int(f["xyz"].shape[0])
    frames = np.concatenate([f["xyz"], f["xyz_partial"]])
    order = np.tile(np.arange(bsz + 3, dtype=np.int32), (2, 1))
    args = dict(gamma=0.5, edges=f["edges"], form=form)
    m = _model(f)
    m.run_steps(frames, order, bsz, 0, 2, mode=B.TRAIN, lr=1e-3, **args)
    before = [t.clone() for t in (m.B.data, *m.moments)]
    fwd, out = m.run_steps(frames, order, bsz, 2, 2, mode=B.FORWARD, probe=True, **args)
    assert all(torch.equal(a, b) for a, b in zip(before, (m.B.data, *m.moments)))
    trained, _ = m.run_steps(frames, order, bsz, 2, 2, mode=B.TRAIN, lr=1e-3, **args)
    assert torch.equal(fwd[0], trained[0]) and not torch.equal(fwd[1], trained[1])      # the second step saw updated parameters
    xyz, recon = m.eval()(torch.from_numpy(frames[:bsz]).cuda())
    want = R.model_forward("equilinear", [torch.from_numpy(m.B.detach().cpu().numpy()).double()], torch.from_numpy(frames[:bsz]).double(),
                           f["mapping"], 3, 2)[1]
    assert R.rel_dev(recon.cpu().numpy(), want.numpy()) <= _allowed(f, "xyz_recon")
    assert torch.equal(xyz.cpu(), torch.from_numpy(frames[:bsz]))
    lin = golden("g19_baseline_step_linear_n22_k3_knn2_g00")
    xyz, recon = _model(lin)(torch.from_numpy(lin["xyz"]).cuda())
    assert R.rel_dev(recon.cpu().numpy(), lin["xyz_recon"]) <= 1.25 * _allowed(lin, "xyz_recon")
    assert torch.allclose(xyz.cpu(), torch.from_numpy(lin["xyz"] - lin["xyz"].mean(1, keepdims=True)), atol=1e-5)


def _mlp_allowed(f):
    return {q: _allowed(f, q) for q in ("xyz_recon", "loss_recon", "loss_dist", "grad_recon", "param_grads")}


@pytest.mark.parametrize("name", R.MLP_FIXTURES)
def test_loss_kernel_and_mlp_against_the_restatement(golden, name):
    """cgv_baseline_loss on the reference's own reconstruction, then the whole MLP step: forward through the package's
    linears, the loss through the autograd function, parameter gradients (the shared hidden layer's summed over its uses)."""
    f = golden(name)
    allowed = _mlp_allowed(f)
    depth, K, gamma = int(f["depth"]), int(f["K"]), float(f["gamma"])
    names = ("mlp.0", "mlp.2", f"mlp.{2 * depth + 2}")
    weights = [f[f"p.{nm}.{w}"] for nm in names for w in ("weight", "bias")]
    want = R.step_outputs("mlp", weights, f["xyz"], f["mapping"], f["edges"], gamma, K, depth=depth)
    loss_fn = B.ReconLoss(f["edges"], gamma, "cuda")
    xyz = torch.from_numpy(f["xyz"]).cuda()
    recon = torch.from_numpy(want["xyz_recon"]).float().cuda().requires_grad_(True)
    loss, terms = loss_fn(recon, xyz)
    loss.backward()
    again = loss_fn(recon.detach(), xyz)[1]
    assert torch.equal(terms, again)                                    # the ticket left the workspace ready; same bits
    got = {"loss_recon": float(terms[0]), "loss_dist": float(terms[1]), "grad_recon": recon.grad.cpu().numpy()}
    for q, a in got.items():
        dev = R.rel_dev(a, want[q])
        print(f"LOSS {name} {q}: {dev:.2e} / {allowed[q]:.2e}")
        assert dev <= allowed[q], (q, dev, allowed[q])
    assert float(loss.detach()) == pytest.approx(want["loss_recon"] + gamma * want["loss_dist"], rel=1e-6)
    mlp = B.MLP(B.FixedPool(f["mapping"], K), K, 22, width=1, depth=depth)
    mlp.load_reference_state({str(k): torch.from_numpy(f["p." + str(k)]) for k in f["state_keys"]})
    mlp = mlp.cuda()
    _, out = mlp(xyz)
    loss, terms = loss_fn(out, xyz)
    loss.backward()
    dev = R.rel_dev(out.detach().cpu().numpy(), want["xyz_recon"])
    print(f"MLP {name} xyz_recon: {dev:.2e} / {allowed['xyz_recon']:.2e}")
    assert dev <= allowed["xyz_recon"]
    mods = dict(mlp.mlp.named_children())
    grads = [getattr(mods[nm.split(".")[1]], w).grad.cpu().numpy() for nm in names for w in ("weight", "bias")]
    dev = max(R.rel_dev(g, w) for g, w in zip(grads, want["grads"]))
    print(f"MLP {name} parameter gradients: {dev:.2e} / {allowed['param_grads']:.2e}")
    assert dev <= allowed["param_grads"]


def test_loss_kernel_edge_rules(golden):
    """An empty hyperedge list gives loss_dist = 0 and the recon gradient alone; a constructed coincident pair gives a finite
    loss and contributes nothing to the gradient (the restatement states both rules)."""
    f = golden("g19_baseline_mlp_w1_d1_g05")
    allowed = _mlp_allowed(f)
    xyz = torch.from_numpy(f["xyz"]).cuda()
    base = f["xyz_recon"].copy()
    base[:, 5] = base[:, 4]                                             # atoms 4 and 5 coincide; (4, 5) is a chain bond
    assert any((e == [4, 5]).all() for e in f["edges"])
    for edges in (f["edges"], np.zeros((0, 2), dtype=np.int64), None):
        recon64 = torch.from_numpy(base).double().requires_grad_(True)
        l_recon, l_dist = R.losses(recon64, torch.from_numpy(f["xyz"]).double(), np.zeros((0, 2)) if edges is None else edges)
        (l_recon + 0.5 * l_dist).backward()
        recon = torch.from_numpy(base).cuda().requires_grad_(True)
        loss, terms = B.ReconLoss(edges, 0.5, "cuda")(recon, xyz)
        loss.backward()
        assert torch.isfinite(terms).all() and torch.isfinite(recon.grad).all()
        assert R.rel_dev(float(terms[0]), float(l_recon)) <= allowed["loss_recon"]
        assert R.rel_dev(recon.grad.cpu().numpy(), recon64.grad.numpy()) <= allowed["grad_recon"]
        if edges is None or len(edges) == 0:
            assert float(terms[1]) == 0.0
        else:
            assert R.rel_dev(float(terms[1]), float(l_dist)) <= allowed["loss_dist"]
    # the trainer follows the same rules: no hyperedges, then a model whose reconstruction collapses every atom (B = 0)
    lin = golden("g19_baseline_step_linear_n22_k3_knn2_g05")
    m = _model(lin)
    log, _ = m.run_steps(lin["xyz"], _same_batch_order(4, 1), 4, 0, 1, mode=B.TRAIN, lr=1e-3, gamma=0.5, edges=None)
    assert float(log[0, 1]) == 0.0 and torch.isfinite(m.B).all()
    z = _model(lin, B0=np.zeros_like(lin["B"]))
    log, _ = z.run_steps(lin["xyz"], _same_batch_order(4, 1), 4, 0, 1, mode=B.TRAIN, lr=1e-3, gamma=0.5, edges=lin["edges"])
    assert torch.isfinite(log).all() and torch.isfinite(z.B).all() and float(log[0, 1]) > 0


@pytest.mark.parametrize("kind", R.LINEAR_KINDS)
def test_trajectory_fixture(golden, kind):
    """320 steps in the stored batch order through ``fit``: B within four times the reference's own deviation from the fp64
    restatement of the same schedule; the final loss_recon below the first."""
    f = golden(f"g19_baseline_traj_{kind}")
    K, knn, bs, gamma, lr = int(f["K"]), int(f["knn"]), int(f["batch"]), float(f["gamma"]), float(f["lr"])
    batches = [f["xyz"][row[s:s + bs]] for row in f["order"] for s in range(0, f["order"].shape[1], bs)]
    want, want_log = R.adam_steps(kind, [f["B"]], batches, f["mapping"], f["edges"], gamma, K, knn, lr=lr)
    m = _model(f)
    log = B.fit(m, f["xyz"], f["order"], bs, lr, gamma, edges=f["edges"]).cpu().numpy()
    assert log.shape == (len(batches), 2) and m.adam_steps == len(batches)
    dev, dev_log = R.rel_dev(m.B.detach().cpu().numpy(), want[0]), R.rel_dev(log, want_log)
    print(f"TRAJ {kind}: B_final {dev:.2e} / {4 * float(f['dev_B_final']):.2e}  loss_log {dev_log:.2e} / {4 * float(f['dev_loss_log']):.2e}  "
          f"loss_recon {log[0, 0]:.4f} -> {log[-1, 0]:.4f}")
    assert dev <= 4.0 * float(f["dev_B_final"]) and dev_log <= 4.0 * float(f["dev_loss_log"])
    assert log[-1, 0] < log[0, 0]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_forced_form_at_300_atoms_8_beads(options, form):
    """n = 300, K = 8, knn = 3 (C = 24), 16 frames, E = 597: the global form forced at a size the rule runs resident, and the
    resident form beyond 64 KB of LDS; three steps against the fp64 restatement.  No stored fixture covers this size, so the
    allowance is measured here the same way: four times the deviation of the same tensor ops in fp32 from fp64."""
    n, K, knn, bsz, gamma, lr = 300, 8, 3, 16, 0.5, 1e-3
    gen = torch.Generator().manual_seed(3)
    mapping = np.sort(np.concatenate([np.arange(K), torch.randint(0, K, (n - K,), generator=gen).numpy()]))
    xyz = torch.cumsum(torch.randn(bsz, n, 3, generator=gen) * 0.9, dim=1).numpy()
    edges = np.array([(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)])
    B0 = (0.01 * torch.randn(n, K * knn, generator=gen)).numpy()
    assert B.choose_form(B.EQUILINEAR, n, K * knn, bsz) == B.RESIDENT and B.choose_form(B.EQUILINEAR, n, K * 7, bsz) == B.GLOBAL
    options.set("baseline_form", form)
    assert B.choose_form(B.EQUILINEAR, n, K * knn, bsz) == form
    m = B.EquiLinear(B.FixedPool(mapping, K), K, n, False, knn)
    m.load_reference_state({"B": torch.from_numpy(B0).clone()})
    m = m.cuda()
    args = dict(lr=lr, gamma=gamma, edges=edges)
    log, out = m.run_steps(xyz, _same_batch_order(bsz, 3), bsz, 0, 1, mode=B.TRAIN, probe=True, **args)
    got = {"xyz_recon": out[: bsz * n * 3].view(bsz, n, 3).cpu().numpy(), "grad": out[bsz * n * 3:].view(n, -1).cpu().numpy(),
           "loss_recon": float(log[0, 0]), "loss_dist": float(log[0, 1])}
    m.run_steps(xyz, _same_batch_order(bsz, 3), bsz, 1, 2, mode=B.TRAIN, **args)
    got["B_after3"] = m.B.detach().cpu().numpy()
    res = {}
    for dtype in (torch.float64, torch.float32):
        o = R.step_outputs("equilinear", [B0], xyz, mapping, edges, gamma, K, knn, dtype=dtype)
        res[dtype] = {"xyz_recon": o["xyz_recon"], "grad": o["grads"][0], "loss_recon": o["loss_recon"], "loss_dist": o["loss_dist"],
                      "B_after3": R.adam_steps("equilinear", [B0], [xyz] * 3, mapping, edges, gamma, K, knn, lr=lr, dtype=dtype)[0][0]}
    for q, a in got.items():
        dev, allowed = R.rel_dev(a, res[torch.float64][q]), 4.0 * R.rel_dev(res[torch.float32][q], res[torch.float64][q])
        print(f"FORCED {B.FORM_NAMES[form]} {q}: {dev:.2e} / {allowed:.2e}")
        assert dev <= allowed, (q, dev, allowed)


@pytest.mark.parametrize("model", run_baseline.MODELS)
def test_cli(tmp_path, capsys, model):
    out = tmp_path / "run"
    run_baseline.main(f"-logdir {out} -device 0 -model {model} --synthetic -dataset dipeptide -N_cg 3 -ndata 60 -n_epochs 2 "
                      "-n_splits 2 -gamma 0.5".split())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["model"] == model and summary["folds"] == 2 and not summary["failed"]
    assert summary["all_rmsd"]["mean"] > 0 and summary["heavy_rmsd"]["mean"] > 0 and summary["all_ged"] is not None
    rows = (out / "cv_stats.csv").read_text().strip().splitlines()
    assert rows[0].split(",") == run_baseline.CV_STATS_COLUMNS and len(rows) == 3
    for row in rows[1:]:
        cells = dict(zip(run_baseline.CV_STATS_COLUMNS, row.split(",")))
        assert cells["train_tetra"] == "" and cells["test_tetra"] == "" and float(cells["test_all_recon"]) > 0
    for fold in (0, 1):
        log = (out / f"fold{fold}" / "train_log.csv").read_text().strip().splitlines()
        assert log[0].split(",") == run_baseline.TRAIN_LOG_COLUMNS and len(log) == 3
        state = torch.load(out / f"fold{fold}" / "model.pt", map_location="cpu")
        assert all(not k.startswith("pooler.") for k in state) and ("B" in state) == (model != "mlp")
    print(f"CLI {model} {summary}")
