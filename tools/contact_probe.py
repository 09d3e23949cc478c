#!/usr/bin/env python3
"""Time K20 (cgv_contact_counts; csrc/contact_map.hip) against the obvious tensor-op formulation -- a chunked
``torch.cdist`` + compare + sum -- on the same GPU, at two shapes:

    chignolin   93 selected atoms of 175, 10 000 structures
    protein     2000 atoms, all selected, 1 000 structures

    python tools/contact_probe.py [--repeats 7] [--out profiles/contacts.txt]

The structures are seeded uniform coordinates in a box sized for about 12 neighbours within the 4.5 A cutoff (the kernel's
work does not depend on the values, only its number of atomics on the number of pairs ever in contact); the exclusions
are those of a chain, depth 3.  Method: device tensors, one warm-up pass of each form, then ``--repeats`` passes, device
events around a pass, nothing read back inside the window; the median and the spread are printed.  The kernel's pass is
``cgv_contact_counts`` on all structures at once (gather + Rg, then the pair kernel), counts table zeroed inside the
window.  The tensor-op pass computes only the count table ([chunk, m, m] distances, compared with the cutoff, masked and
summed over the chunk, chunk sized for 2^28 distances) -- no per-structure counts, no Rg -- so it does less.  The two
tables are compared outside the window: ``cdist`` rounds differently from ``sq_dist2``, so a few pairs on the threshold
may differ; the number of differing entries is printed, not asserted.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("chignolin", 175, 93, 10000), ("protein", 2000, 2000, 1000))
CUTOFF = 4.5


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, contacts, ensemble
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contact_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    c2 = contacts.cutoff2_of(CUTOFF)
    lines = ["K20 (csrc/contact_map.hip) against chunked torch.cdist + compare + sum -- tools/contact_probe.py",
             f"cutoff {CUTOFF} A, exclusions of a chain at depth 3, median of {args.repeats} passes after one warm-up, device events"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    for name, n, m, S in SHAPES:
        rng = np.random.default_rng(m)
        box = float((m * 4.0 / 3.0 * np.pi * CUTOFF ** 3 / 12.0) ** (1.0 / 3.0))
        x = torch.from_numpy(rng.uniform(0, box, (S, n, 3)).astype(np.float32)).to(dev)
        sel = np.sort(rng.permutation(n)[:m])
        excl = contacts.excluded_pairs(np.stack([np.arange(n - 1), np.arange(1, n)], 1), n, sel, 3)
        d_sel = torch.from_numpy(sel.astype(np.int32)).to(dev)
        d_excl = torch.from_numpy(ensemble.pack_mask(excl).view(np.int32)).to(dev)
        allowed = torch.from_numpy(~excl).to(dev)
        counts = torch.zeros(m, m, dtype=torch.int32, device=dev)
        per = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(3)]
        rg2 = torch.zeros(S, dtype=torch.float64, device=dev)
        need = int(lib.cgv_contact_workspace_bytes(S, m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)

        def kernel():
            counts.zero_()
            _lib.call("cgv_contact_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_excl), None, S, n, m, float(c2), _lib.ptr(counts),
                      _lib.ptr(per[0]), _lib.ptr(per[1]), _lib.ptr(rg2), _lib.ptr(per[2]), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

        chunk = max(1, min(S, (1 << 28) // (m * m)))
        table = torch.zeros(m, m, dtype=torch.int64, device=dev)

        def tensor_ops():
            table.zero_()
            for s0 in range(0, S, chunk):
                p = x[s0:s0 + chunk, d_sel.long()]
                table.add_(((torch.cdist(p, p) < CUTOFF) & allowed).sum(0))

        k_med, k_min, k_max = timed(kernel)
        t_med, t_min, t_max = timed(tensor_ops)
        differ = int((counts.long() != table).sum().item())
        pairs = m * (m - 1) // 2
        lines += ["", f"{name}: n = {n}, m = {m}, {S} structures = {pairs * S / 1e6:.1f} M pair tests, {int((counts > 0).sum().item()) // 2} "
                      f"of {pairs} pairs ever in contact",
                  f"cgv_contact_counts   {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {pairs * S / k_med / 1e6:.1f} G pair tests / s",
                  f"torch cdist form     {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   chunk {chunk} structures; table only",
                  f"ratio torch / kernel {t_med / k_med:9.2f}   entries of the two tables that differ (threshold rounding): {differ} of {m * m}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
