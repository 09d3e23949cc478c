#!/usr/bin/env python3
"""Time K32 (cgv_relax; csrc/relax.hip) against the tensor-op form of the same iteration on the same GPU -- dense
``[S, n, n]`` differences, distances, masks and sums in torch, a dozen launches a step -- at three sizes:

    dipeptide       22 atoms, 4 structures a block    chignolin   138 atoms    protein   2 000 atoms (88 KB of LDS a structure)

    python tools/relax_probe.py [--repeats 7] [--limit 150] [--out profiles/relax.txt]

The molecule is synthetic: a random-walk chain of 1.5 A steps, all carbon, bonds between consecutive atoms, restraints on
the bonds and the 1-3 pairs at the distances of the unperturbed chain, every structure the chain plus 0.3 A of noise.  The
sizes, not the chemistry, decide the time.

Method: every (form, shape) runs in a child process of its own under a time limit of ``--limit`` seconds, one after the
other (one process with the GPU open at a time); the first child that fails or runs out of time ends the probe.  In a child:
device tensors, THREE copies of the input that the passes take in turn (no pass finds its own input in a cache), one warm-up
pass, then ``--repeats`` passes, device events around a pass, nothing read back inside the window; the median and the spread
are printed.  K32's pass is one ``cgv_relax`` of all structures; the tensor-op pass takes fewer structures and steps (its
cost per structure-step is what is compared) in chunks of at most 2^25 pair components.  A structure-step is one step of one
structure; a pair test is one ordered pair (i, j) of one structure-step, n^2 of them.  Outside the window the RMS distance every form moved its atoms is printed: the two forms
take different numbers of structures and sum in another order, so that is a plausibility check, not an equality.  No GPU:
the probe fails, it does not fall back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"dipeptide": dict(n=22, S=65536, steps=50, S_torch=4096, steps_torch=10),
          "chignolin": dict(n=138, S=8192, steps=50, S_torch=512, steps_torch=10),
          "protein": dict(n=2000, S=512, steps=50, S_torch=8, steps_torch=5)}
FORMS = ("relax", "torch")
PAR = dict(k_pos=0.05, k_rep=1.0, tol=0.4, damp=1.0, cap=0.25)


def one(form, shape, repeats):
    """A child: the timings of one form at one shape as a JSON line."""
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, relax
    from coarsegrainingvae_amd.contacts import excluded_pairs
    from coarsegrainingvae_amd.ensemble import pack_mask
    if not torch.cuda.is_available():
        raise SystemExit("relax_probe needs a GPU")
    dev = torch.device("cuda", 0)
    _lib.load()
    p = SHAPES[shape]
    n = p["n"]
    S, steps = (p["S"], p["steps"]) if form == "relax" else (p["S_torch"], p["steps_torch"])
    rng = np.random.default_rng(n)
    step = rng.normal(size=(n, 3))
    chain = np.cumsum(1.5 * step / np.linalg.norm(step, axis=1, keepdims=True), axis=0)
    z, bonds = np.full(n, 6), np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    tab = relax.restraints(z, bonds, np.stack([chain, chain]).astype(np.float32))
    excl = excluded_pairs(bonds, n, np.arange(n), 3)
    copies = [torch.from_numpy((chain[None] + np.random.default_rng(n + 1 + c).normal(0, 0.3, (S, n, 3))).astype(np.float32)).to(dev)
              for c in range(3)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    radii = np.full(n, 1.7, np.float32)

    if form == "relax":
        d_rp, d_pa, d_d0, d_w, d_ws = (up(tab[k]) for k in ("row_ptr", "partner", "d0_e", "w_e", "wsum"))
        d_r = up(radii)
        d_ex = up(pack_mask(excl).view(np.int32))
        out = torch.empty(S, n, 3, dtype=torch.float32, device=dev)
        cl, en = torch.zeros(S, 2, dtype=torch.int32, device=dev), torch.zeros(S, 2, dtype=torch.float64, device=dev)
        d2, bad = torch.zeros(S, dtype=torch.float32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)

        def fn(x):
            _lib.call("cgv_relax", _lib.ptr(x), _lib.ptr(x), _lib.ptr(d_rp), _lib.ptr(d_pa), _lib.ptr(d_d0), _lib.ptr(d_w), _lib.ptr(d_ws),
                      _lib.ptr(d_r), _lib.ptr(d_ex), S, n, int(tab["partner"].shape[0]), PAR["k_pos"], PAR["k_rep"], PAR["tol"], PAR["damp"],
                      PAR["cap"], steps, _lib.ptr(out), _lib.ptr(cl), _lib.ptr(en), _lib.ptr(d2), _lib.ptr(bad), _lib.stream_ptr())
            return out
        chunk = S
    else:
        Wm, D0 = np.zeros((n, n), np.float32), np.ones((n, n), np.float32)
        for (i, j), d0, w in zip(tab["pairs"].tolist(), tab["d0"].tolist(), tab["w"].tolist()):
            Wm[i, j] = Wm[j, i] = w
            D0[i, j] = D0[j, i] = d0
        C = (radii[:, None] + radii[None, :]) - np.float32(PAR["tol"])
        t_W, t_D0, t_C, t_ok, t_Ws = up(Wm), up(D0), up(C), up(~excl & (C > 0)), up(Wm.sum(1))
        chunk = max(1, min(S, (1 << 25) // (3 * n * n)))
        cap2 = PAR["cap"] ** 2

        def fn(x):
            res = torch.empty_like(x)
            for s0 in range(0, S, chunk):
                y, a = x[s0:s0 + chunk].clone(), x[s0:s0 + chunk]
                for _ in range(steps):
                    D = y[:, :, None, :] - y[:, None, :, :]
                    q = (D * D).sum(-1)
                    d = q.sqrt()
                    hit = t_ok & (q < t_C * t_C) & (q > 0)
                    coef = torch.where(q > 0, t_W * (d - t_D0) / d, 0.0) + torch.where(hit, PAR["k_rep"] * (d - t_C) / d, 0.0)
                    g = PAR["k_pos"] * (y - a) + (coef[..., None] * D).sum(2)
                    h = (PAR["k_pos"] + 2 * t_Ws) + 2 * PAR["k_rep"] * hit.sum(2)
                    delta = torch.where(h[..., None] > 0, -PAR["damp"] * g / h[..., None], 0.0)
                    m = (delta * delta).sum(-1, keepdim=True)
                    y = y + delta * torch.where(m > cap2, PAR["cap"] / m.sqrt(), 1.0)
                res[s0:s0 + chunk] = y
            return res
    out = fn(copies[0])
    torch.cuda.synchronize()
    ms = []
    for k in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(copies[(k + 1) % 3])
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    moved = float((out - copies[repeats % 3]).pow(2).sum(-1).mean().sqrt())
    print(json.dumps({"form": form, "shape": shape, "n": n, "S": S, "steps": steps, "chunk": chunk, "med": statistics.median(ms), "min": min(ms),
                      "max": max(ms), "rms_move": moved, "pack": relax.pack_of(n)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=float, default=150.0, help="seconds a child may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--one", nargs=2, default=None, metavar=("FORM", "SHAPE"), help="run one form at one shape (what a child does)")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.repeats)
    lines = ["K32 (csrc/relax.hip) against the dense tensor-op form of the same iteration in torch -- tools/relax_probe.py",
             f"command: python tools/relax_probe.py --repeats {args.repeats} --out profiles/relax.txt",
             f"random-walk chains of 1.5 A steps plus 0.3 A of noise; default parameters; three rotating inputs; median of {args.repeats} passes after "
             f"one warm-up, device events; every form in a process of its own under a limit of {args.limit:g} s"]
    names = {"relax": "cgv_relax        ", "torch": "torch tensor form"}
    failed = None
    for shape in SHAPES:
        got = {}
        for form in FORMS:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--one", form, shape]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                failed = f"{form} at {shape}: no result within {args.limit:g} s"
                break
            if res.returncode != 0:
                failed = f"{form} at {shape}: exit status {res.returncode}: {res.stderr.strip().splitlines()[-1:] or ''}"
                break
            r = got[form] = json.loads(res.stdout.strip().splitlines()[-1])
            if form == FORMS[0]:
                lines += ["", f"{shape}: {r['n']} atoms, {r['pack']} structure(s) a block"]
            ss = r["S"] * r["steps"]
            r["rate"] = ss / r["med"] * 1e3
            lines.append(f"{names[form]}  {r['S']:6d} structures x {r['steps']:2d} steps  {r['med']:10.3f} ms  (min {r['min']:.3f}, max {r['max']:.3f})   "
                         f"{r['rate'] / 1e6:9.4f} M structure-steps / s   {r['rate'] * r['n'] ** 2 / 1e9:8.2f} G pair tests / s   rms move {r['rms_move']:.3f} A"
                         + (f"   chunk {r['chunk']} structures" if form == "torch" else ""))
        if failed:
            lines.append("STOPPED: " + failed)
            break
        lines.append(f"ratio of structure-steps / s, kernel / torch {got['relax']['rate'] / got['torch']['rate']:9.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
