#!/usr/bin/env python3
"""Time K26 (cgv_dssp_assign; csrc/dssp.hip) against a batched tensor-op form of its ENERGY STAGE ALONE on the same GPU,
at two shapes:

    chignolin   R = 10 residues, 100 000 structures   (one wave per structure)
    protein     R = 256 residues,  4 096 structures   (one block per structure)

    python tools/dssp_probe.py [--repeats 9] [--torch_repeats 3] [--out profiles/dssp.txt]

The structures are seeded and made on the device: one chain of R residues, atoms N CA C O per residue, the CA uniform in a
ball at one per 130 A^3 (what a folded protein has, so the share of pairs inside the 9 A pre-filter is a protein's), N, C and
O 1.46, 1.52 and 2.4 A from their CA in random directions; ``prev`` of a residue is the C and O in front of it.  Method: one
warm-up pass of each form, then ``--repeats`` passes of the kernel and ``--torch_repeats`` of the tensor-op form, device
events around a pass, nothing read back inside the window; the passes rotate over ``COPIES`` independent copies of the
structures (together larger than the 256 MB memory-side cache at the first shape), so no pass finds its input where the
last one left it; median, min and max are printed.  The kernel's pass is ``cgv_dssp_assign`` on all structures at once --
the WHOLE assignment: virtual hydrogens, energies, turns, bridges, ladders, bends, classes and counts -- once without and
once with ``codes`` and ``hb_bits``.  The tensor-op pass forms, for a piece of at most 2^22 (structure, pair) entries at a
time, the virtual hydrogen, the CA and the four squared distances, e and the comparison in the operation order of the
kernel, and sums hb over the pieces: the energy stage and nothing after it.  Its hb is compared with the kernel's hb_bits
outside the window (eager fp32 tensor ops round every operation; the number of differing entries is printed).  No ratio is
fixed in advance; if the kernel is the slower one the output says so.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("chignolin", 10, 100000), ("protein", 256, 4096))
COPIES = 4
PIECE = 1 << 22
VOLUME = 130.0


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--torch_repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dssp_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["K26 (csrc/dssp.hip), the whole assignment, against a batched tensor-op form of its energy stage alone -- tools/dssp_probe.py",
             f"CA uniform in a ball at one per {VOLUME:.0f} A^3; median of {args.repeats} kernel passes and {args.torch_repeats} tensor-op passes "
             f"after one warm-up each, rotating over {COPIES} copies of the structures, device events"]

    def timed(fn, repeats):
        fn(0)
        torch.cuda.synchronize()
        ms = []
        for k in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k + 1)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, R, S in SHAPES:
        n, W = 4 * R, (R + 63) // 64
        gen = torch.Generator(device=dev)
        gen.manual_seed(R)
        radius = (3.0 * R * VOLUME / (4.0 * np.pi)) ** (1.0 / 3.0)
        unit = lambda: torch.nn.functional.normalize(torch.randn(S, R, 3, device=dev, generator=gen), dim=2)
        xs = []
        for _ in range(COPIES):
            ca = unit() * (radius * torch.rand(S, R, 1, device=dev, generator=gen) ** (1.0 / 3.0))
            xs.append(torch.stack([ca + 1.46 * unit(), ca, ca + 1.52 * unit(), ca + 2.4 * unit()], dim=2).reshape(S, n, 3).contiguous())
        res = np.arange(n, dtype=np.int32).reshape(R, 4)
        prev = np.concatenate([[[-1, -1]], res[:-1, 2:4]]).astype(np.int32)
        link = np.array([1] * (R - 1) + [0], dtype=np.int32)
        d_res, d_prev, d_link = (torch.from_numpy(a).to(dev) for a in (res, prev, link))
        counts = torch.zeros(R, 8, dtype=torch.int64, device=dev)
        n_class = torch.zeros(S, 8, dtype=torch.int32, device=dev)
        bad = torch.zeros(S, dtype=torch.int32, device=dev)
        codes = torch.zeros(S, R, dtype=torch.uint8, device=dev)
        bits = torch.zeros(S, R, W, dtype=torch.int64, device=dev)

        def kernel(k, full=False):
            counts.zero_()
            _lib.call("cgv_dssp_assign", _lib.ptr(xs[k % COPIES]), _lib.ptr(d_res), _lib.ptr(d_prev), _lib.ptr(d_link), S, n, R,
                      _lib.ptr(counts), _lib.ptr(n_class), _lib.ptr(bad), _lib.ptr(codes) if full else None,
                      _lib.ptr(bits) if full else None, _lib.stream_ptr())

        piece = max(1, PIECE // (R * R))
        idx = torch.arange(R, device=dev)
        eligible = (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] + 1) & (idx[None, :] >= 1)
        t_hb = torch.zeros(R, R, dtype=torch.int64, device=dev)
        hb_of_piece = []

        def sq(v):
            return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]

        def tensor_ops(k, keep=False):
            x = xs[k % COPIES].view(S, R, 4, 3)
            t_hb.zero_()
            for s0 in range(0, S, piece):
                c = x[s0:s0 + piece]
                N, CA, C, O = c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3]
                w = C[:, :-1] - O[:, :-1]
                H = N.clone()
                H[:, 1:] = N[:, 1:] + w / sq(w).sqrt()[..., None]
                pair = lambda a, b: sq(a[:, :, None, :] - b[:, None, :, :])
                ca, on, ch, oh, cn = pair(CA, CA), pair(O, N), pair(C, H), pair(O, H), pair(C, N)
                e = 27.888 * (((1.0 / on.sqrt() + 1.0 / ch.sqrt()) - 1.0 / oh.sqrt()) - 1.0 / cn.sqrt())
                e = torch.where((on < 0.25) | (ch < 0.25) | (oh < 0.25) | (cn < 0.25), torch.full_like(e, -9.9), e)
                hb = eligible[None] & (ca < 81.0) & (e < -0.5)
                t_hb.add_(hb.sum(dim=0))
                if keep:
                    hb_of_piece.append(hb)

        k_med, k_min, k_max = timed(kernel, args.repeats)
        f_med, f_min, f_max = timed(lambda k: kernel(k, True), args.repeats)
        t_med, t_min, t_max = timed(tensor_ops, args.torch_repeats)
        kernel(0, True)                                                       # both forms on the same copy
        tensor_ops(0, keep=True)
        hb = torch.cat(hb_of_piece)
        shifts = torch.arange(64, device=dev)
        from_bits = ((bits[:, :, :, None] >> shifts) & 1).bool().reshape(S, R, 64 * W)[:, :, :R]
        differ = int((from_bits != hb).sum().item())
        pairs = float(S) * R * R
        inside = float(hb.numel())
        lines += ["", f"{name}: R = {R}, {n} atoms, {S} structures: {pairs / 1e9:.3f} G ordered pairs, {100 * float(hb.sum().item()) / pairs:.2f} % "
                      f"bonded, {S * n * 12 / 1e6:.0f} MB of coordinates; classes H B E G I T S -: {counts.sum(dim=0).tolist()}",
                  f"cgv_dssp_assign (whole assignment)       {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {S / k_med / 1e3:9.2f} M structures / s",
                  f"cgv_dssp_assign with codes and hb_bits   {f_med:10.3f} ms  (min {f_min:.3f}, max {f_max:.3f})   {S / f_med / 1e3:9.2f} M structures / s",
                  f"tensor-op form (energy stage alone)      {t_med:10.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   pieces of {piece} structures",
                  f"ratio torch energy stage / whole kernel  {t_med / k_med:10.2f}   " +
                  ("K26 is SLOWER than the tensor-op energy stage alone   " if k_med > t_med else "") +
                  f"entries of hb that differ: {differ} of {int(inside)}"]
        print("\n".join(lines[-6:]), flush=True)
        xs = hb = from_bits = None
        hb_of_piece.clear()
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
