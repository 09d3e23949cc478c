#!/usr/bin/env python3
"""Generate the baseline-model goldens ``g19_baseline_*.npz`` FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is present (see make_golden.py).  It imports the reference's own
``CoarseGrainingVAE/baseline.py`` (Baseline, EquiLinear, MLP) and ``CoarseGrainingVAE/diffpoolvae.py`` (CGpool) unmodified,
after ``make_golden.load_reference()`` has installed the stand-ins of absent third-party modules, and drives them with the
loss of the reference's training loop: the mean squared error plus gamma times the hyperedge-distance term, the latter by
calling the function of the reference's own scripts/run_baseline.py, imported unmodified as well (``load_training_script``);
torch.optim.Adam(lr).  Only arrays are written.

Step fixtures ``g19_baseline_step_{kind}_n{n}_k{K}_knn{knn}_g{gamma}.npz``: inputs B, xyz (one full batch), mapping, bonds'
hyperedges, gamma, lr; the reference's fp32 outputs xyz_recon, loss_recon, loss_dist, the gradient of B, B after 1 and after
10 Adam steps on that batch; for the first case also a final partial batch of 3 frames with its forward outputs and
gradient.  ``dev_<quantity>``: the deviation (baseline_restatement.rel_dev) of each of those fp32 outputs from the fp64
restatement of the stored inputs -- the GPU tests allow the kernels four times that.

Trajectory fixtures ``g19_baseline_traj_{kind}.npz``: 22 atoms, 3 beads, 60 frames, 40 epochs of batches of 8 (the last of
an epoch holds 4) in a stored order: the reference's B at the end and its loss log.

MLP fixtures ``g19_baseline_mlp_w1_d{depth}_g{gamma}.npz``: the state_dict (with the shared hidden layer under each of its
names), one batch, the reference's xyz_recon, losses, gradient with respect to xyz_recon and parameter gradients.

Usage:  python tests/golden/make_golden_baseline.py          (rewrites tests/golden/g19_baseline_*)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402
import make_golden_eval  # noqa: E402
import baseline_restatement as R  # noqa: E402
from make_golden_cgae import chain_frames, segment_trajectory  # noqa: E402

LR = 1e-3
TRAJ_LR, TRAJ_EPOCHS, TRAJ_BATCH, TRAJ_FRAMES, TRAJ_GAMMA = 1e-2, 40, 8, 60, 0.5


def load_models():
    make_golden.load_reference()
    base = importlib.import_module("CoarseGrainingVAE.baseline")
    pool = importlib.import_module("CoarseGrainingVAE.diffpoolvae")
    return base, pool.CGpool, load_training_script()


def mapping_of(n, K, seed):
    """Unequal bead sizes with a one-atom bead: bead 0 = atom 0 alone, the others contiguous runs of random lengths."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(2, n), size=K - 2, replace=False)) if K > 2 else np.zeros(0, dtype=np.int64)
    marks = np.zeros(n, dtype=np.int64)
    marks[1] = 1
    marks[cuts] = 1
    return np.cumsum(marks)


def molecule(n):
    """Chain bonds plus a side bond every seventh atom; hyperedges of order 2 (datasets.py:449-458)."""
    from coarsegrainingvae_amd.data import get_high_order_edge
    bonds = [(i, i + 1) for i in range(n - 1)] + [(i, i + 3) for i in range(0, n - 3, 7)]
    bonds = np.array(bonds, dtype=np.int64)
    return bonds, get_high_order_edge(torch.from_numpy(bonds), 2, n).numpy().astype(np.int64)


def batch_of(xyz, bonds, edges):
    """The collated batch the reference's models and loss read (DiffPool_collate): per-frame index in column 0."""
    b = xyz.shape[0]
    stack = lambda e: torch.cat([torch.cat([torch.full((len(e), 1), i, dtype=torch.long), torch.from_numpy(e)], dim=1) for i in range(b)])
    return {"xyz": xyz, "z": torch.ones(b, xyz.shape[1]), "nbr_list": torch.zeros(0, 3, dtype=torch.long),
            "bonds": stack(bonds), "hyperedges": stack(edges)}


class _Absent(types.ModuleType):
    """Stand-in for a module the reference's training script imports at its top and the loss never touches."""
    __all__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_training_script():
    """The reference's scripts/run_baseline.py as a module, imported unmodified (after ``load_models``): whatever its
    top-level imports miss here (plotting, progress bars, tables, dataset readers) becomes an ``_Absent`` stand-in.  Only
    its hyperedge-distance loss is called."""
    make_golden_eval.load_reference_scripts()
    for _ in range(64):
        try:
            return importlib.import_module("run_baseline")
        except ImportError as err:
            if not err.name:
                raise
            sys.modules[err.name] = _Absent(err.name)
    raise ImportError("scripts/run_baseline.py of the reference does not import")


def reference_losses(script, model, batch, gamma):
    """One forward of the reference's model and both loss terms in its own fp32 arithmetic: the hyperedge term is the
    training script's function, called as its loop calls it; the other term is the mean squared error over all elements."""
    out = model(batch)
    target, recon = out[1], out[2]
    recon.retain_grad()
    mse = torch.nn.functional.mse_loss(recon, target)
    hyper = script.dist_loss(target, recon, batch["hyperedges"])
    return target, recon, mse, hyper, mse + gamma * hyper


def build(ref, kind, n, K, knn, mapping, seed, width=1, depth=1):
    base, CGpool, _ = ref
    torch.manual_seed(seed)
    pooler = CGpool(1, 16, n_atoms=n, n_cgs=K, assign_idx=torch.LongTensor(mapping))
    if kind == "linear":
        return base.Baseline(pooler, K, n)
    if kind == "equilinear":
        return base.EquiLinear(pooler, K, n, cross=False, knn=knn)
    return base.MLP(pooler, K, n, width=width, depth=depth, activation="ReLU")


def with_deviations(out, want, quantities):
    for q in quantities:
        out["dev_" + q] = np.float64(R.rel_dev(out[q], want[q]))
    return out


def step_fixture(ref, kind, n, K, knn, bsz, gamma, partial):
    seed = n + K + knn + bsz
    mapping = mapping_of(n, K, seed)
    bonds, edges = molecule(n)
    model = build(ref, kind, n, K, knn, mapping, seed)
    B0 = model.B.detach().clone()
    xyz = torch.from_numpy(chain_frames(n, bsz + 3, seed + 100))
    full, part = xyz[:bsz], xyz[bsz:]
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    out = {"kind": np.array(kind), "K": np.int64(K), "knn": np.int64(knn), "B": B0.numpy(), "xyz": full.numpy(),
           "mapping": mapping, "bonds": bonds, "edges": edges, "gamma": np.float32(gamma), "lr": np.float32(LR)}
    if partial:
        opt.zero_grad()
        _, recon, l_recon, l_dist, loss = reference_losses(ref[2], model, batch_of(part, bonds, edges), gamma)
        loss.backward()
        out.update(xyz_partial=part.numpy(), partial_xyz_recon=recon.detach().numpy().copy(),
                   partial_loss_recon=np.float32(l_recon.item()), partial_loss_dist=np.float32(l_dist.item()),
                   partial_grad=model.B.grad.numpy().copy())
    batch = batch_of(full, bonds, edges)
    for step in range(10):
        opt.zero_grad()
        _, recon, l_recon, l_dist, loss = reference_losses(ref[2], model, batch, gamma)
        loss.backward()
        if step == 0:
            out.update(xyz_recon=recon.detach().numpy().copy(), loss_recon=np.float32(l_recon.item()),
                       loss_dist=np.float32(l_dist.item()), grad=model.B.grad.numpy().copy())
        opt.step()
        if step in (0, 9):
            out[f"B_after{step + 1}"] = model.B.detach().numpy().copy()
    quantities = list(R.QUANTITIES) + (["partial_xyz_recon", "partial_loss_recon", "partial_loss_dist", "partial_grad"] if partial else [])
    return with_deviations(out, R.restate_step_fixture(out), quantities)


def traj_fixture(ref, kind):
    n, K, knn = 22, 3, 2
    xyz, seg = segment_trajectory(T=TRAJ_FRAMES)
    mapping = seg.astype(np.int64)
    bonds, edges = molecule(n)
    model = build(ref, kind, n, K, knn, mapping, seed=19)
    B0 = model.B.detach().clone()
    order = np.random.default_rng(19).permuted(np.tile(np.arange(TRAJ_FRAMES, dtype=np.int32), (TRAJ_EPOCHS, 1)), axis=1)
    opt = torch.optim.Adam(model.parameters(), lr=TRAJ_LR)
    frames, log, batches = torch.from_numpy(xyz), [], []
    for row in order:
        for s in range(0, TRAJ_FRAMES, TRAJ_BATCH):
            idx = torch.from_numpy(row[s:s + TRAJ_BATCH].astype(np.int64))
            batches.append(xyz[idx.numpy()])
            opt.zero_grad()
            _, _, l_recon, l_dist, loss = reference_losses(ref[2], model, batch_of(frames[idx], bonds, edges), TRAJ_GAMMA)
            loss.backward()
            opt.step()
            log.append((l_recon.item(), l_dist.item()))
    out = {"kind": np.array(kind), "K": np.int64(K), "knn": np.int64(knn), "B": B0.numpy(), "xyz": xyz, "mapping": mapping,
           "edges": edges, "order": order, "batch": np.int64(TRAJ_BATCH), "gamma": np.float32(TRAJ_GAMMA),
           "lr": np.float32(TRAJ_LR), "B_final": model.B.detach().numpy().copy(), "loss_log": np.array(log, dtype=np.float32)}
    want, want_log = R.adam_steps(kind, [out["B"]], batches, mapping, edges, TRAJ_GAMMA, K, knn, lr=float(out["lr"]))
    out["dev_B_final"] = np.float64(R.rel_dev(out["B_final"], want[0]))
    out["dev_loss_log"] = np.float64(R.rel_dev(out["loss_log"], want_log))
    print(f"{kind}: {len(log)} steps, loss_recon {log[0][0]:.4f} -> {log[-1][0]:.4f}, dev_B_final {out['dev_B_final']:.2e}")
    return out


def mlp_fixture(ref, depth, gamma):
    n, K, bsz = 22, 3, 4
    mapping = mapping_of(n, K, 7)
    bonds, edges = molecule(n)
    model = build(ref, "mlp", n, K, 0, mapping, seed=40 + depth, width=1, depth=depth)
    xyz = torch.from_numpy(chain_frames(n, bsz, 77))
    _, recon, l_recon, l_dist, loss = reference_losses(ref[2], model, batch_of(xyz, bonds, edges), gamma)
    loss.backward()
    state = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if not k.startswith("pooler.")}
    last = 2 * depth + 2
    names = ("mlp.0", "mlp.2", f"mlp.{last}")
    out = {"depth": np.int64(depth), "K": np.int64(K), "xyz": xyz.numpy(), "mapping": mapping, "edges": edges,
           "gamma": np.float32(gamma), "state_keys": np.array(sorted(state)), "xyz_recon": recon.detach().numpy().copy(),
           "loss_recon": np.float32(l_recon.item()), "loss_dist": np.float32(l_dist.item()),
           "grad_recon": recon.grad.numpy().copy()}
    out.update({"p." + k: v for k, v in state.items()})
    mods = dict(model.mlp.named_children())
    for name in names:
        lin = mods[name.split(".")[1]]
        out["g." + name + ".weight"], out["g." + name + ".bias"] = lin.weight.grad.numpy().copy(), lin.bias.grad.numpy().copy()
    weights = [out[f"p.{nm}.{w}"] for nm in names for w in ("weight", "bias")]
    want = R.step_outputs("mlp", weights, out["xyz"], mapping, edges, gamma, K, depth=depth)
    for q in ("xyz_recon", "loss_recon", "loss_dist", "grad_recon"):
        out["dev_" + q] = np.float64(R.rel_dev(out[q], want[q]))
    got = [out[f"g.{nm}.{w}"] for nm in names for w in ("weight", "bias")]
    out["dev_param_grads"] = np.float64(max(R.rel_dev(g, w) for g, w in zip(got, want["grads"])))
    return out


def main():
    torch.set_num_threads(1)
    ref = load_models()

    def write(name, arrays):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        devs = " ".join(f"{k[4:]}={float(v):.1e}" for k, v in arrays.items() if k.startswith("dev_"))
        print(f"wrote {name}  ({os.path.getsize(path) / 1024:.1f} KiB)  {devs}")

    for kind in R.LINEAR_KINDS:
        for ci, (tag, n, K, knn, bsz) in enumerate(R.LINEAR_CASES):
            for g in R.GAMMAS:
                write(f"g19_baseline_step_{kind}_{tag}_g{str(g).replace('.', '')}",
                      step_fixture(ref, kind, n, K, knn, bsz, g, partial=(ci == 0)))
        write(f"g19_baseline_traj_{kind}", traj_fixture(ref, kind))
    for depth in (1, 2):
        for g in R.GAMMAS:
            write(f"g19_baseline_mlp_w1_d{depth}_g{str(g).replace('.', '')}", mlp_fixture(ref, depth, g))


if __name__ == "__main__":
    main()
