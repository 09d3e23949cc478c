#!/usr/bin/env python3
"""Time K30 (cgv_dist_moments; csrc/dist_moments.hip) against the obvious tensor-op formulation of the same two moments --
chunked ``torch.cdist``, then ``sum`` of d and of d * d over the structures into fp64 tables -- and against K20
(cgv_contact_counts; csrc/contact_map.hip: one distance and one comparison per pair over the same triangle, the ceiling for
a kernel of this shape) on the same input and the same GPU:

    m = 128, 512 and 2 048 atoms, 1 024 structures; random clouds in a 30 A box; all atoms selected, no mask, no centre

    python tools/distmat_probe.py [--repeats 7] [--limit 120] [--out profiles/distmat.txt]

Method: every (form, size) runs in a child process of its own under a time limit of ``--limit`` seconds, one after the other
(one process with the GPU open at a time); the first child that fails or runs out of time ends the probe.  In a child: device
tensors, one warm-up pass, then ``--repeats`` passes, device events around a pass, nothing read back inside the window; the
median and the spread are printed.  K30's pass is ``cgv_dist_moments`` on all structures at once (the gather, then the pair
kernel), its tables zeroed inside the window; K20's is ``cgv_contact_counts`` at 8 A likewise.  The tensor-op pass works in
chunks sized for 2^25 distances.  A pair distance is one unordered pair of one structure: ``S m (m - 1) / 2`` per pass (the
tensor form computes both triangles).  Outside the window K30's mean map is compared with the tensor form's: they differ by
roundings of the distance and the 2^-20 fixed point.  No GPU: the probe fails, it does not fall back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 1024), (512, 1024), (2048, 1024))
FORMS = ("dist_moments", "torch", "contacts")
CUTOFF = 8.0


def one(form, m, S, repeats):
    """A child: the timings of one form at one size as a JSON line."""
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("distmat_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    x = torch.from_numpy(np.random.default_rng(m).uniform(0.0, 30.0, size=(S, m, 3)).astype(np.float32)).to(dev)
    d_sel = torch.arange(m, dtype=torch.int32, device=dev)
    bad = torch.zeros(S, dtype=torch.int32, device=dev)
    chunk = max(1, min(S, (1 << 25) // (m * m)))

    def tensor_moments():
        s1, s2 = torch.zeros(m, m, dtype=torch.float64, device=dev), torch.zeros(m, m, dtype=torch.float64, device=dev)
        for s0 in range(0, S, chunk):
            d = torch.cdist(x[s0:s0 + chunk], x[s0:s0 + chunk])
            s1.add_(d.sum(0, dtype=torch.float64))
            s2.add_((d * d).sum(0, dtype=torch.float64))
        return s1, s2

    extra = {}
    if form == "dist_moments":
        a1, a2 = (torch.zeros(m, m, dtype=torch.int64, device=dev) for _ in range(2))
        dev2 = torch.zeros(S, dtype=torch.int64, device=dev)
        need = int(lib.cgv_dist_moments_workspace_bytes(S, m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

        def fn():
            a1.zero_(), a2.zero_(), dev2.zero_()
            _lib.call("cgv_dist_moments", _lib.ptr(x), _lib.ptr(d_sel), None, None, S, m, m, _lib.ptr(a1), _lib.ptr(a2), _lib.ptr(dev2),
                      _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
    elif form == "torch":
        fn = tensor_moments
    else:
        counts = torch.zeros(m, m, dtype=torch.int32, device=dev)
        nc, nn = (torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2))
        rg2 = torch.zeros(S, dtype=torch.float64, device=dev)
        excl = torch.zeros(m, (m + 31) // 32, dtype=torch.int32, device=dev)
        need = int(lib.cgv_contact_workspace_bytes(S, m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

        def fn():
            counts.zero_()
            _lib.call("cgv_contact_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(excl), None, S, m, m, CUTOFF * CUTOFF, _lib.ptr(counts),
                      _lib.ptr(nc), _lib.ptr(nn), _lib.ptr(rg2), _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    if form == "dist_moments":
        s1, _ = tensor_moments()
        off = ~torch.eye(m, dtype=torch.bool, device=dev)
        extra["mean_diff"] = float(((a1.double() / 2.0 ** 20 - s1) / S)[off].abs().max())
        extra["bad"] = int(bad.sum())
    print(json.dumps({"form": form, "m": m, "S": S, "med": statistics.median(ms), "min": min(ms), "max": max(ms), "chunk": chunk, **extra}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a child may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--one", nargs=3, default=None, metavar=("FORM", "M", "S"), help="run one form at one size (what a child does)")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], int(args.one[1]), int(args.one[2]), args.repeats)
    lines = ["K30 (csrc/dist_moments.hip) against chunked torch.cdist + sum, and against K20 (csrc/contact_map.hip) -- tools/distmat_probe.py",
             f"command: python tools/distmat_probe.py --repeats {args.repeats} --out profiles/distmat.txt",
             f"random clouds in a 30 A box; no mask, no centre; K20 at {CUTOFF} A; median of {args.repeats} passes after one warm-up, device "
             f"events; every form in a process of its own under a limit of {args.limit:g} s"]
    names = {"dist_moments": "cgv_dist_moments  ", "torch": "torch cdist form  ", "contacts": "cgv_contact_counts"}
    failed = None
    for m, S in SHAPES:
        pairs = m * (m - 1) // 2
        lines += ["", f"m = {m}, {S} structures: {pairs * S / 1e6:.1f} M pair distances"]
        got = {}
        for form in FORMS:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--one", form, str(m), str(S)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                failed = f"{form} at m = {m}: no result within {args.limit:g} s"
                break
            if res.returncode != 0:
                failed = f"{form} at m = {m}: exit status {res.returncode}: {res.stderr.strip().splitlines()[-1:] or ''}"
                break
            r = got[form] = json.loads(res.stdout.strip().splitlines()[-1])
            tail = {"dist_moments": f"   mean map against the tensor form's: max |diff| {r.get('mean_diff', 0.0):.2e} A, {r.get('bad', 0)} bad",
                    "torch": f"   chunk {r['chunk']} structures", "contacts": ""}[form]
            lines.append(f"{names[form]}  {r['med']:9.3f} ms  (min {r['min']:.3f}, max {r['max']:.3f})   "
                         f"{pairs * S / r['med'] / 1e6:.1f} G pair distances / s{tail}")
        if failed:
            lines.append("STOPPED: " + failed)
            break
        k = got["dist_moments"]["med"]
        lines.append(f"ratio torch / kernel {got['torch']['med'] / k:9.2f}   kernel's rate as a share of K20's: {got['contacts']['med'] / k:.3f}")
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
