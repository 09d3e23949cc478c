#!/usr/bin/env python3
"""Time the mapping learner's full schedule (1500 epochs over 900 training frames in batches of 32 = 43 500 optimiser steps,
datasets.py:190-192) against a tensor-op restatement of the reference loop on the same GPU.

    python tools/probes/cgae_bench.py                     # every part, each in a child process under its own time limit
    python tools/probes/cgae_bench.py --part kernel --shape chignolin

Shapes: dipeptide 22 x 3 and chignolin 166 x 6 (resident form), protein 2000 x 64 (streamed form; 150 epochs = 4 350 steps
on both sides, rates are per step).  The comparison side is how the reference itself would run on the device -- the same
tensor ops (F.gumbel_softmax, einsum, autograd, torch.optim.Adam) on device tensors with the batch gathered by a device
index -- and is not the code under test.  It is given two advantages: the reference's three ``.item()`` synchronisations
per step and its DataLoader collation are left out.  Each part: one warm-up run of 300 steps on a learner of its own, then
``--repeats`` timed runs of the whole schedule from fresh parameters, host clock around work that ends in a device
synchronise.  Prints one line per part: median steps/s and the spread."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"dipeptide": (22, 3, 1500), "chignolin": (166, 6, 1500), "protein2000": (2000, 64, 150)}
LIMITS = {"kernel": 240, "tensor_ops": 420}           # seconds per part (child process)
N_FRAMES, BATCH, SEED = 1000, 32, 123


def frames_of(n):
    import torch
    gen = torch.Generator().manual_seed(n)
    base = torch.cumsum(torch.randn(n, 3, generator=gen) * 0.9, dim=0)
    return base[None] + 0.3 * torch.randn(N_FRAMES, n, 3, generator=gen)


def run_kernel(n, K, epochs, repeats):
    import torch
    from coarsegrainingvae_amd import cgmap
    xyz = frames_of(n)
    train = cgmap.train_subset(N_FRAMES, SEED)

    def learner(n_epochs):
        W, D = cgmap.initial_parameters(n, K, SEED)
        return cgmap.Learner(xyz[train], W, D, cgmap.frame_order(len(train), BATCH, n_epochs, SEED), BATCH, 0.25, seed=SEED)
    warm = learner(11)
    warm.run(300)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        ln = learner(epochs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ln.run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    losses = ln.loss_log[-1].tolist()
    return ln.total_steps, times, f"form {cgmap.FORM_NAMES[ln.form]} beads used {len(set(ln.W.argmax(-1).tolist()))} last losses {losses[0]:.4f} {losses[1]:.4f}"


def run_tensor_ops(n, K, epochs, repeats):
    import torch
    import torch.nn.functional as F
    from coarsegrainingvae_amd import cgmap
    dev = torch.device("cuda")
    train = cgmap.train_subset(N_FRAMES, SEED)
    xyz = frames_of(n)[train].to(dev)
    xyz = xyz - xyz.mean(1, keepdim=True)

    def schedule(n_epochs, max_steps=None):
        W0, D0 = cgmap.initial_parameters(n, K, SEED)
        W, D = W0.to(dev).requires_grad_(True), D0.to(dev).requires_grad_(True)
        opt = torch.optim.Adam([W, D], lr=4e-3)
        order = torch.from_numpy(cgmap.frame_order(len(train), BATCH, n_epochs, SEED)).long().to(dev)
        steps = 0
        for e in range(n_epochs):
            for s in range(0, len(train), BATCH):
                X = xyz[order[e, s:s + BATCH]]
                M = F.gumbel_softmax(W, dim=-1)
                cg = torch.einsum("bij,in->bnj", X, M / M.sum(-2).unsqueeze(-2))
                recon = torch.einsum("bnj,ni->bij", cg, D)
                lift = torch.einsum("bij,ni->bnj", cg, M)
                loss_reg = (X - lift).pow(2).sum(-1).mean()
                loss_recon = (X - recon).pow(2).mean()
                opt.zero_grad()
                (loss_recon + 0.25 * loss_reg).backward()
                opt.step()
                steps += 1
                if max_steps and steps >= max_steps:
                    return steps, W.detach(), (loss_recon.detach(), loss_reg.detach())
        return steps, W.detach(), (loss_recon.detach(), loss_reg.detach())
    schedule(11, 300)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps, W, losses = schedule(epochs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return steps, times, f"beads used {len(set(W.argmax(-1).tolist()))} last losses {float(losses[0]):.4f} {float(losses[1]):.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "tensor_ops"])
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.part:
        n, K, epochs = SHAPES[args.shape]
        steps, times, note = (run_kernel if args.part == "kernel" else run_tensor_ops)(n, K, epochs, args.repeats)
        rates = sorted(steps / t for t in times)
        print(f"{args.shape:12s} {n:5d} x {K:2d}  {args.part:10s} {steps:6d} steps  median {statistics.median(rates):12.0f} steps/s  "
              f"(min {rates[0]:.0f}, max {rates[-1]:.0f}, {len(times)} runs, median {1e6 / statistics.median(rates):.1f} us/step)  {note}", flush=True)
        return 0
    for shape in ("dipeptide", "chignolin", "protein2000"):
        for part in ("kernel", "tensor_ops"):
            repeats = args.repeats if part == "kernel" else 1
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--shape", shape, "--repeats", str(repeats)]
            try:
                rc = subprocess.run(cmd, timeout=LIMITS[part]).returncode
            except subprocess.TimeoutExpired:
                print(f"{shape} {part}: no result within {LIMITS[part]} s; stopping", flush=True)
                return 1
            if rc != 0:
                print(f"{shape} {part}: exit status {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
