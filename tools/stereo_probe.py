#!/usr/bin/env python3
"""Time K31 (cgv_stereo_counts; csrc/stereo.hip) against the obvious tensor-op formulation of the same three predicates on
the same GPU -- chunked torch gathers, ``torch.cross``, products, comparisons and sums -- at two sets of table sizes:

    protein      2 000 atoms: 140 centres, 124 torsions, 30 rings, 2 030 bonds; 4 096 structures
    chignolin      138 atoms:  11 centres,   9 torsions,  4 rings,   141 bonds; 32 768 structures

    python tools/stereo_probe.py [--repeats 7] [--limit 120] [--out profiles/stereo.txt]

The molecule is synthetic: a random-walk chain of 1.5 A steps, bonds between consecutive atoms and a few random ones, rings
of 5 and 6 consecutive atoms, centres and torsions of four consecutive atoms, every (ring, bond) pair tested unless the bond
has an atom in the ring.  The sizes, not the chemistry, decide the time.

Method: every (form, shape) runs in a child process of its own under a time limit of ``--limit`` seconds, one after the
other (one process with the GPU open at a time); the first child that fails or runs out of time ends the probe.  In a child:
device tensors, one warm-up pass, then ``--repeats`` passes, device events around a pass, nothing read back inside the
window; the median and the spread are printed.  K31's pass is ``cgv_stereo_counts`` on all structures at once (the gather,
the light pass, the ring pass), its tables zeroed inside the window.  The tensor-op pass works in chunks sized for 2^24
(ring, triangle, bond) elements.  A ring-pair test is one tested (ring, bond) pair of one structure.  Outside the window the
two forms' totals are compared: the tensor form sums a ring's centre in another order, so a pair on a boundary may differ.
No GPU: the probe fails, it does not fall back."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"protein": dict(n=2000, C=140, Q=124, R=30, extra=31, S=4096), "chignolin": dict(n=138, C=11, Q=9, R=4, extra=4, S=32768)}
FORMS = ("stereo", "torch")


def molecule(n, C, Q, R, extra, seed):
    """The synthetic tables of the docstring, atom indices: ``(centres, torsions, rings, bonds, tested)``."""
    import numpy as np
    rng = np.random.default_rng(seed)
    quads = lambda k: (rng.choice(n - 3, size=k, replace=False)[:, None] + np.arange(4)[None]).astype(np.int32)
    rings = np.full((R, 8), -1, np.int32)
    for r, start in enumerate(rng.choice(n - 6, size=R, replace=False)):
        k = 5 + r % 2
        rings[r, :k] = start + np.arange(k)
    far = rng.choice(n, size=(extra, 2), replace=False) if extra else np.zeros((0, 2), int)
    bonds = np.unique(np.sort(np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), far]), axis=1), axis=0).astype(np.int32)
    tested = np.stack([~(np.isin(bonds[:, 0], row[row >= 0]) | np.isin(bonds[:, 1], row[row >= 0])) for row in rings])
    return quads(C), quads(Q), rings, bonds, tested


def one(form, shape, repeats):
    """A child: the timings of one form at one shape as a JSON line."""
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib
    from coarsegrainingvae_amd.ensemble import pack_mask
    if not torch.cuda.is_available():
        raise SystemExit("stereo_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    p = SHAPES[shape]
    n, S = p["n"], p["S"]
    centres, torsions, rings, bonds, tested = molecule(p["n"], p["C"], p["Q"], p["R"], p["extra"], seed=n)
    C, Q, R, B = centres.shape[0], torsions.shape[0], rings.shape[0], bonds.shape[0]
    rng = np.random.default_rng(n + 1)
    step = rng.normal(size=(S, n, 3))
    x = torch.from_numpy(np.cumsum(1.5 * step / np.linalg.norm(step, axis=2, keepdims=True), axis=1).astype(np.float32)).to(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_c, d_q, d_r, d_b, d_t = up(centres), up(torsions), up(rings), up(bonds), up(tested)
    extra = {"pair_tests": int(tested.sum()) * S, "C": C, "Q": Q, "R": R, "B": B}

    if form == "stereo":
        d_sel = torch.arange(n, dtype=torch.int32, device=dev)       # every atom is named by a bond: places are atoms
        d_mask = up(pack_mask(tested).view(np.int32))
        neg, flat, cis = (torch.zeros(k, dtype=torch.int64, device=dev) for k in (C, C, Q))
        pierced = torch.zeros(R, B, dtype=torch.int32, device=dev)
        counts, bad = torch.zeros(S, 3, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
        need = int(lib.cgv_stereo_workspace_bytes(S, n, R))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

        def fn():
            neg.zero_(), flat.zero_(), cis.zero_(), pierced.zero_()
            _lib.call("cgv_stereo_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_c), _lib.ptr(d_q), _lib.ptr(d_r), _lib.ptr(d_b), _lib.ptr(d_mask),
                      None, None, S, n, n, C, Q, R, B, _lib.ptr(neg), _lib.ptr(flat), _lib.ptr(cis), _lib.ptr(pierced), _lib.ptr(counts), _lib.ptr(bad),
                      _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())
            return neg, cis, pierced
    else:
        valid = d_r >= 0                                             # [R, 8]
        k = valid.sum(1)
        nxt = torch.where(torch.arange(8, device=dev)[None] + 1 < k[:, None], torch.arange(1, 9, device=dev)[None], torch.zeros(1, 8, dtype=torch.long, device=dev))
        ring_at, next_at = d_r.clamp(min=0).long(), torch.gather(d_r.clamp(min=0).long(), 1, nxt)
        chunk = max(1, min(S, (1 << 24) // (R * 8 * B)))
        c_at, q_at, b_at = d_c.long(), d_q.long(), d_b.long()
        dot = lambda a, b: (a * b).sum(-1)

        def fn():
            neg, cis = torch.zeros(C, dtype=torch.int64, device=dev), torch.zeros(Q, dtype=torch.int64, device=dev)
            pierced = torch.zeros(R, B, dtype=torch.int64, device=dev)
            for s0 in range(0, S, chunk):
                y = x[s0:s0 + chunk]
                a = y[:, c_at]                                       # [s, C, 4, 3]
                e = a[:, :, 1:] - a[:, :, :1]
                neg.add_((dot(e[:, :, 0], torch.cross(e[:, :, 1], e[:, :, 2], dim=-1)) < 0).sum(0))
                t = y[:, q_at]
                b1, b2, b3 = t[:, :, 1] - t[:, :, 0], t[:, :, 2] - t[:, :, 1], t[:, :, 3] - t[:, :, 2]
                cis.add_((dot(torch.cross(b1, b2, dim=-1), torch.cross(b2, b3, dim=-1)) > 0).sum(0))
                v = y[:, ring_at]                                    # [s, R, 8, 3]
                g = (v * valid[None, :, :, None]).sum(2) / k[None, :, None]
                e1 = (v - g[:, :, None])[:, :, :, None]              # [s, R, 8, 1, 3]
                e2 = (y[:, next_at] - g[:, :, None])[:, :, :, None]
                p0 = y[:, b_at[:, 0]][:, None, None]                 # [s, 1, 1, B, 3]
                d = (y[:, b_at[:, 1]] - y[:, b_at[:, 0]])[:, None, None].expand(-1, R, 8, -1, -1)
                tv = p0 - g[:, :, None, None]
                pv = torch.cross(d, e2.expand(-1, -1, -1, B, -1), dim=-1)
                det, u = dot(e1, pv), dot(tv, pv)
                qv = torch.cross(tv.expand(-1, -1, 8, -1, -1), e1.expand(-1, -1, -1, B, -1), dim=-1)
                w, tt = dot(d, qv), dot(e2, qv)
                sgn = torch.sign(det)
                u, w, tt, det = u * sgn, w * sgn, tt * sgn, det * sgn
                hit = (det > 0) & (u >= 0) & (w >= 0) & (u + w <= det) & (tt >= 0) & (tt <= det) & valid[None, :, :, None]
                pierced.add_((hit.any(2) & d_t[None]).sum(0))
            return neg, cis, pierced
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    extra.update(neg=int(out[0].sum()), cis=int(out[1].sum()), pierced=int(out[2].sum()), chunk=chunk if form == "torch" else S)
    print(json.dumps({"form": form, "shape": shape, "S": S, "med": statistics.median(ms), "min": min(ms), "max": max(ms), **extra}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a child may take")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--one", nargs=2, default=None, metavar=("FORM", "SHAPE"), help="run one form at one shape (what a child does)")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args.repeats)
    lines = ["K31 (csrc/stereo.hip) against chunked torch gathers, torch.cross and comparisons -- tools/stereo_probe.py",
             f"command: python tools/stereo_probe.py --repeats {args.repeats} --out profiles/stereo.txt",
             f"random-walk chains of 1.5 A steps; synthetic tables; no want; median of {args.repeats} passes after one warm-up, device events; "
             f"every form in a process of its own under a limit of {args.limit:g} s"]
    names = {"stereo": "cgv_stereo_counts", "torch": "torch tensor form"}
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
                lines += ["", f"{shape}: {r['C']} centres, {r['Q']} torsions, {r['R']} rings, {r['B']} bonds, {r['S']} structures: "
                              f"{r['pair_tests'] / 1e6:.1f} M ring-pair tests"]
            lines.append(f"{names[form]}  {r['med']:9.3f} ms  (min {r['min']:.3f}, max {r['max']:.3f})   {r['pair_tests'] / r['med'] / 1e6:.2f} G ring-pair tests / s"
                         f"   negative {r['neg']}, cis {r['cis']}, pierced {r['pierced']}" + (f"   chunk {r['chunk']} structures" if form == "torch" else ""))
        if failed:
            lines.append("STOPPED: " + failed)
            break
        lines.append(f"ratio torch / kernel {got['torch']['med'] / got['stereo']['med']:9.2f}")
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
