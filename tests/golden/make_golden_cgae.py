#!/usr/bin/env python3
"""Generate the mapping-learner goldens ``g13_cgae_*.npz`` FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is present (see make_golden.py).  It imports the reference's own
``CoarseGrainingVAE/cgae.py`` unmodified (the file does ``from data import *``, so the reference's package directory
goes on ``sys.path`` after ``make_golden.load_reference()`` has installed the stand-ins of absent third-party modules)
and drives it with the loop of ``learn_map`` (datasets.py:204-239: Adam(lr = 4e-3), loss_recon + reg_weight *
loss_reg, batches of 32, the last partial batch kept).  Only arrays are written.

Step fixtures ``g13_cgae_step_n{n}_k{K}_b{B}.npz``: inputs W, D, the centred X the reference's forward returns and the
Gumbel noise it consumed -- re-drawn under the same torch generator state with F.gumbel_softmax's own expression
(``-empty_like(logits).exponential_().log()``) and checked to reproduce the reference's M bit for bit -- and the
reference's fp32 outputs: M, cg_xyz, recon, both losses, dW, dD, and the parameters after 1 and after 10 Adam steps
(same batch, the stored noise of each step).

Trajectory fixture ``g13_cgae_traj.npz``: 22 atoms, 200 frames, three chain segments that move independently; the
reference's final W, D and argmax mapping after 300 epochs for seeds 0, 1, 2 on the training subset of
``cgmap.train_subset``.

Usage:  python tests/golden/make_golden_cgae.py          (rewrites tests/golden/g13_cgae_*)
"""
import importlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402

REG_WEIGHT, LR = 0.25, 4e-3
STEP_CASES = ((22, 3, 32), (22, 3, 4), (166, 6, 8))
TRAJ_EPOCHS, TRAJ_BATCH, TRAJ_SEEDS = 300, 32, (0, 1, 2)


def load_cgae():
    make_golden.load_reference()
    pkg = os.path.join(make_golden.REF, "CoarseGrainingVAE")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    return importlib.import_module("cgae").cgae


def chain_frames(n, T, seed, sigma=0.3):
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)
    return (base[None] + sigma * rng.standard_normal((T, n, 3))).astype(np.float32)


def segment_trajectory(T=200, seed=7):
    """22 atoms as three chain segments (7 + 8 + 7 atoms); per frame every segment gets its own rigid displacement
    (sigma 1.0 A) on top of small per-atom noise (0.05 A): the atoms of a segment move together."""
    rng = np.random.default_rng(seed)
    seg = np.repeat(np.arange(3), (7, 8, 7))
    base = np.cumsum(rng.standard_normal((22, 3)) * 0.9, axis=0)
    shift = rng.standard_normal((T, 3, 3))
    xyz = base[None] + shift[:, seg, :] + 0.05 * rng.standard_normal((T, 22, 3))
    return xyz.astype(np.float32), seg


def losses(ae, X):
    """datasets.py:225-231 (the caller's own centring, 222-223, is repeated by forward)."""
    xyz, xyz_recon, M, cg_xyz = ae(X, 1.0)
    xyz_recon = torch.einsum("bnj,ni->bij", cg_xyz, ae.decode)
    X_lift = torch.einsum("bij,ni->bnj", cg_xyz, M)
    loss_reg = (xyz - X_lift).pow(2).sum(-1).mean()
    loss_recon = (xyz - xyz_recon).pow(2).mean()
    return xyz, xyz_recon, M, cg_xyz, loss_recon, loss_reg


def consumed_noise(ae, state):
    """The noise F.gumbel_softmax drew from generator state ``state`` (its own expression)."""
    keep = torch.get_rng_state()
    torch.set_rng_state(state)
    g = -torch.empty_like(ae.assign_map, memory_format=torch.legacy_contiguous_format).exponential_().log()
    torch.set_rng_state(keep)
    return g


def step_fixture(cgae, n, K, B, seed):
    torch.manual_seed(seed)
    ae = cgae(n, K)
    W0, D0 = ae.assign_map.detach().clone(), ae.decode.detach().clone()
    raw = torch.from_numpy(chain_frames(n, B, seed + 100))
    X = raw - raw.mean(1, keepdim=True)
    opt = torch.optim.Adam(list(ae.parameters()), lr=LR)
    out, noise = {}, []
    for step in range(10):
        state = torch.get_rng_state()
        xyz, recon, M, cg, l_recon, l_reg = losses(ae, X)
        g = consumed_noise(ae, state)
        assert torch.equal(torch.softmax(ae.assign_map.detach() + g, -1), M.detach()), "noise re-draw does not reproduce M"
        noise.append(g.numpy().copy())
        opt.zero_grad()
        (l_recon + REG_WEIGHT * l_reg).backward()
        if step == 0:
            # stored X = what the reference computed on; re-centring it in later steps is a no-op up to the fp32
            # rounding of a mean of ~1e-8
            X = xyz.detach().clone()
            out.update(X=X.numpy().copy(), M=M.detach().numpy().copy(), cg_xyz=cg.detach().numpy().copy(),
                       recon=recon.detach().numpy().copy(), loss_recon=np.float32(l_recon.item()),
                       loss_reg=np.float32(l_reg.item()), dW=ae.assign_map.grad.numpy().copy(),
                       dD=ae.decode.grad.numpy().copy())
        opt.step()
        if step in (0, 9):
            out[f"W_after{step + 1}"] = ae.assign_map.detach().numpy().copy()
            out[f"D_after{step + 1}"] = ae.decode.detach().numpy().copy()
    out.update(W=W0.numpy(), D=D0.numpy(), noise=np.stack(noise), reg_weight=np.float32(REG_WEIGHT), lr=np.float32(LR))
    return out


def traj_fixture(cgae):
    from coarsegrainingvae_amd import cgmap
    xyz, seg = segment_trajectory()
    out = {"xyz": xyz, "segments": seg.astype(np.int64), "epochs": np.int64(TRAJ_EPOCHS), "batch": np.int64(TRAJ_BATCH),
           "reg_weight": np.float32(REG_WEIGHT)}
    for seed in TRAJ_SEEDS:
        train = cgmap.train_subset(len(xyz), seed).numpy()
        frames = torch.from_numpy(xyz[train])
        torch.manual_seed(seed)
        ae = cgae(22, 3)
        opt = torch.optim.Adam(list(ae.parameters()), lr=LR)
        t0, steps = time.time(), 0
        for _ in range(TRAJ_EPOCHS):
            perm = torch.randperm(len(frames))
            for s in range(0, len(frames), TRAJ_BATCH):
                l = losses(ae, frames[perm[s:s + TRAJ_BATCH]])
                opt.zero_grad()
                (l[4] + REG_WEIGHT * l[5]).backward()
                opt.step()
                steps += 1
        mapping = ae.assign_map.argmax(-1).detach().numpy()
        print(f"seed {seed}: {steps} steps, {1e3 * (time.time() - t0) / steps:.2f} ms/step, mapping {mapping.tolist()}")
        out[f"train_index_{seed}"] = train.astype(np.int64)
        out[f"W_{seed}"], out[f"D_{seed}"] = ae.assign_map.detach().numpy(), ae.decode.detach().numpy()
        out[f"mapping_{seed}"] = mapping.astype(np.int64)
    return out


def main():
    cgae = load_cgae()
    for n, K, B in STEP_CASES:
        path = os.path.join(HERE, f"g13_cgae_step_n{n}_k{K}_b{B}.npz")
        np.savez_compressed(path, **step_fixture(cgae, n, K, B, seed=n + K + B))
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")
    path = os.path.join(HERE, "g13_cgae_traj.npz")
    np.savez_compressed(path, **traj_fixture(cgae))
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
