"""Learn the atom -> bead assignment from a trajectory (``-cg_method cgae``) on the device.

Reference: ``learn_map`` (CoarseGrainingVAE/datasets.py:190-249) on the auto-encoder of CoarseGrainingVAE/cgae.py, called
from ``get_cg_and_xyz`` (datasets.py:303-312) and retried by scripts/run_ala.py:168-173 until every bead is used.  The
optimiser loop -- tens of thousands of steps on two ``n_atoms x n_cgs`` matrices -- runs inside ``cgv_cgae_steps``
(csrc/cgae.hip): the host uploads the centred training frames and the frame order of the whole schedule once, launches,
and reads the loss log at the end.  There is no tensor-op path: a missing kernel is an error."""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from . import _lib, options

RESIDENT, STREAMED = 1, 2                 # include/cgvae_hip.h: CGV_CGAE_RESIDENT / CGV_CGAE_STREAMED
FORM_NAMES = {RESIDENT: "resident", STREAMED: "streamed"}
MAX_ATTEMPTS = 5
CHUNK_STEPS = 8192                        # steps per call of the entry point (bounds one launch of the resident form)


def train_subset(n_frames: int, seed: int) -> torch.Tensor:
    """A seeded random 90 % of ``range(n_frames)``, in drawn order (datasets.py:197: train_test_split(test_size=0.1), which
    holds out ceil(0.1 T) frames; the held-out frames stay unused, as in the reference)."""
    perm = torch.randperm(n_frames, generator=torch.Generator().manual_seed(int(seed)))
    return perm[: n_frames - math.ceil(0.1 * n_frames)]


def initial_parameters(n_atoms: int, n_cgs: int, seed: int):
    """cgae.__init__ (cgae.py:13-14): assign_map first, then decode, from one CPU generator."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randn(n_atoms, n_cgs, generator=gen), torch.randn(n_cgs, n_atoms, generator=gen)


def frame_order(n_train: int, batch_size: int, n_epochs: int, seed: int) -> np.ndarray:
    """int32 [n_epochs, n_train]: one permutation of the training subset's positions per epoch (DataLoader(shuffle=True)).
    Step s takes ``batch_size`` consecutive entries of its epoch's row; the last batch of a row is the partial one."""
    rng = np.random.default_rng([int(seed), 1])
    return rng.permuted(np.tile(np.arange(n_train, dtype=np.int32), (n_epochs, 1)), axis=1)


def steps_per_epoch(n_train: int, batch_size: int) -> int:
    return -(-n_train // batch_size)


def choose_form(n_atoms: int, n_cgs: int, batch_size: int) -> int:
    """The one rule: everything in one workgroup's LDS when n_atoms * n_cgs (and the batch's bead coordinates) fit it
    (cgv_cgae_resident_fits), the multi-block form otherwise.  options ``cgae_form`` = 1 / 2 forces a form."""
    forced = options.get("cgae_form")
    if forced in (RESIDENT, STREAMED):
        return forced
    return RESIDENT if _lib.load().cgv_cgae_resident_fits(n_atoms, n_cgs, batch_size) else STREAMED


class Learner:
    """Device state of one learning run: parameters, Adam moments, frames, order table, loss log, workspace."""

    def __init__(self, frames, W, D, order, batch_size, reg_weight, lr=4e-3, seed=0, device="cuda", form=None):
        dev = torch.device(device)
        frames = torch.as_tensor(frames, dtype=torch.float32)
        self.n_frames, self.n, _ = frames.shape
        self.K = int(W.shape[1])
        assert tuple(W.shape) == (self.n, self.K) and tuple(D.shape) == (self.K, self.n)
        order = np.ascontiguousarray(order, dtype=np.int32)
        self.n_train, self.batch = int(order.shape[1]), int(batch_size)
        if order.min() < 0 or order.max() >= self.n_frames:
            raise ValueError("frame order table points outside the frames")
        self.total_steps = int(order.shape[0]) * steps_per_epoch(self.n_train, self.batch)
        self.form = choose_form(self.n, self.K, self.batch) if form is None else int(form)
        frames = frames - frames.mean(1, keepdim=True)                    # datasets.py:222-223, once
        self.frames = frames.contiguous().to(dev)
        self.order = torch.from_numpy(order.reshape(-1)).to(dev)
        self.W, self.D = W.detach().float().contiguous().to(dev), D.detach().float().contiguous().to(dev)
        self.moments = [torch.zeros_like(t) for t in (self.W, self.W, self.D, self.D)]      # mW, vW, mD, vD
        self.loss_log = torch.zeros(self.total_steps, 2, device=dev)
        nbytes = int(_lib.load().cgv_cgae_workspace_bytes(self.n, self.K, self.batch, self.form))
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.reg_weight, self.lr, self.seed, self.done = float(reg_weight), float(lr), int(seed), 0

    def run(self, steps=None, noise=None, probe=False):
        """``steps`` more optimiser steps (default: the rest of the schedule).  ``noise`` [steps, n, K]: explicit Gumbel noise
        instead of the generator's.  ``probe``: returns M, dW, dD, cg_xyz of the last step."""
        steps = self.total_steps - self.done if steps is None else int(steps)
        if steps < 0 or self.done + steps > self.total_steps:
            raise ValueError("more steps than the frame order table holds")
        if noise is not None:
            noise = noise.to(self.W.device, torch.float32).contiguous()
            assert tuple(noise.shape) == (steps, self.n, self.K)
        nk = self.n * self.K
        out = torch.zeros(3 * nk + self.batch * self.K * 3, device=self.W.device) if probe else None
        with torch.cuda.device(self.W.device):
            start = 0
            while start < steps:
                cnt = min(CHUNK_STEPS, steps - start)
                _lib.call("cgv_cgae_steps", self.form, _lib.ptr(self.W), _lib.ptr(self.D), *(_lib.ptr(m) for m in self.moments),
                          _lib.ptr(self.frames), self.n_frames, _lib.ptr(self.order), self.order.numel(), self.n_train,
                          self.batch, self.n, self.K, self.done, cnt, self.reg_weight, self.lr, 0.9, 0.999, 1e-8, self.seed,
                          _lib.ptr(noise[start:]) if noise is not None else None, _lib.ptr(self.loss_log[self.done:]),
                          _lib.ptr(out) if probe and start + cnt == steps else None,
                          _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
                start += cnt
                self.done += cnt
        if not probe:
            return None
        last = self.done - 1
        spe = steps_per_epoch(self.n_train, self.batch)
        cnt = min(self.batch, self.n_train - (last % spe) * self.batch)
        return {"M": out[:nk].view(self.n, self.K), "dW": out[nk:2 * nk].view(self.n, self.K),
                "dD": out[2 * nk:3 * nk].view(self.K, self.n), "cg_xyz": out[3 * nk:].view(self.batch, self.K, 3)[:cnt]}


def kernel_noise(seed: int, step0: int, steps: int, n_atoms: int, n_cgs: int, device="cuda") -> torch.Tensor:
    """The Gumbel noise [steps, n, K] the kernels draw for steps ``step0 ..`` under ``seed`` (cgv_cgae_noise)."""
    out = torch.empty(steps, n_atoms, n_cgs, device=device)
    with torch.cuda.device(out.device):
        _lib.call("cgv_cgae_noise", int(seed), int(step0), int(steps), int(n_atoms), int(n_cgs), _lib.ptr(out), _lib.stream_ptr())
    return out


def learn_once(xyz, n_cgs, reg_weight=0.25, n_data=1000, n_epochs=1500, lr=4e-3, batch_size=32, seed=123, device="cuda"):
    """One run of the reference's learn_map.  Returns (mapping LongTensor[n], info, (W, D) on the host)."""
    xyz = torch.as_tensor(np.asarray(xyz), dtype=torch.float32)
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError("xyz must be [T, n_atoms, 3]")
    xyz = xyz[: min(int(n_data), xyz.shape[0])]
    train = train_subset(xyz.shape[0], seed)
    if len(train) == 0:
        raise ValueError("no training frames")
    W, D = initial_parameters(xyz.shape[1], int(n_cgs), seed)
    order = frame_order(len(train), batch_size, n_epochs, seed)
    t0 = time.time()
    learner = Learner(xyz[train], W, D, order, batch_size, reg_weight, lr=lr, seed=seed, device=device)
    learner.run()
    final = learner.loss_log[-1].cpu() if learner.total_steps else torch.full((2,), float("nan"))   # the one read of the log (synchronises)
    W, D = learner.W.cpu(), learner.D.cpu()
    info = {"method": "cgae", "steps": learner.total_steps, "seconds": time.time() - t0, "loss_recon": float(final[0]),
            "loss_reg": float(final[1]), "attempts": 1, "form": FORM_NAMES[learner.form], "seed": int(seed)}
    return W.argmax(-1), info, (W, D)


def learn_map(xyz, n_cgs, reg_weight=0.25, n_data=1000, n_epochs=1500, lr=4e-3, batch_size=32, seed=123, device="cuda"):
    """``learn_map`` with the caller's retry rule (scripts/run_ala.py:168-173): while fewer than ``n_cgs`` distinct beads
    come out, learn again with ``seed + attempt``.  The reference loops forever; here the fifth failure raises.

    Frames: the first ``min(n_data, T)``, a seeded random 90 % of them.  Returns (mapping LongTensor[n], info) with info =
    {method, steps, seconds, loss_recon, loss_reg (last step), attempts, form ("resident" / "streamed"), seed}."""
    seconds = 0.0
    for attempt in range(MAX_ATTEMPTS):
        mapping, info, _ = learn_once(xyz, n_cgs, reg_weight=reg_weight, n_data=n_data, n_epochs=n_epochs, lr=lr,
                                      batch_size=batch_size, seed=seed + attempt, device=device)
        seconds += info["seconds"]
        if len(set(mapping.tolist())) == n_cgs:
            return mapping.long(), {**info, "attempts": attempt + 1, "seconds": seconds}
    raise RuntimeError(f"cgae mapping: {MAX_ATTEMPTS} attempts (seeds {seed}..{seed + MAX_ATTEMPTS - 1}) on {len(mapping)} atoms "
                       f"never used all n_cgs = {n_cgs} beads; choose fewer beads or pass a mapping in the trajectory file")


def select_mapping(cg_method, file_mapping, xyz, n_cgs, reg_weight, device, learner=None):
    """Which atom -> bead map a ``-traj`` run uses (datasets.py:303-312 for cgae).  Returns (mapping array, info or None):
    the file's mapping when it has one; else, for ``-cg_method cgae``, the learned one; else contiguous equal blocks."""
    if file_mapping is not None:
        return np.asarray(file_mapping), None
    if not n_cgs:
        raise SystemExit("the trajectory file has no mapping: pass -n_cgs (learned with -cg_method cgae, else contiguous equal blocks of atoms)")
    if cg_method == "cgae":
        mapping, info = (learner or learn_map)(xyz, n_cgs, reg_weight=reg_weight, device=device)
        return np.asarray(mapping), info
    n_atoms = np.asarray(xyz).shape[1]
    return (np.arange(n_atoms) * n_cgs) // n_atoms, None
