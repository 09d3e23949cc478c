#!/usr/bin/env python3
"""Time K29 (cgv_pairdist_counts; csrc/pair_hist.hip) against the obvious tensor-op formulation of the same histogram --
chunked ``torch.cdist``, a bucket index, one ``bincount`` over (class pair, bin) -- on the same GPU, on a random-walk chain
(1.5 A steps) at three sizes, with one class and with four:

    m = 128, 512 (4 096 structures) and 2 048 (1 024 structures); all atoms selected; r_max 20 A, 100 bins

    python tools/pairdist_probe.py [--repeats 7] [--out profiles/pairdist.txt]

Method: device tensors, one warm-up pass of each form, then ``--repeats`` passes, device events around a pass, nothing read
back inside the window; the median and the spread are printed.  The kernel's pass is ``cgv_pairdist_counts`` on all
structures at once (the gather, then the pair kernel), ``hist`` and ``beyond`` zeroed inside the window.  The tensor-op pass
works in chunks sized for 2^25 distances.  A pair test is one unordered pair of one structure: ``S m (m - 1) / 2`` per pass.
The rate is also given as a fraction of K20's (``profiles/contacts.txt``, its protein row: one distance and one comparison
per pair over the same triangle -- the ceiling for a kernel of this shape).  The two tables are compared outside the window,
entry by entry: ``cdist`` rounds a distance differently from ``sqrtf(sq_dist2)``, so a pair that sits on a bin edge may land
in the neighbouring bin; the entries that differ and the pairs they differ by are counted and printed, and every class
pair's total must agree exactly.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 4096), (512, 4096), (2048, 1024))
R_MAX, N_BINS = 20.0, 100


def k20_rate():
    """G pair tests / s of K20 at its largest recorded shape, from profiles/contacts.txt."""
    with open(os.path.join(ROOT, "profiles", "contacts.txt")) as f:
        rates = [float(v) for v in re.findall(r"cgv_contact_counts\s.*?([0-9.]+) G pair tests / s", f.read())]
    return max(rates)


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, ensemble, pairdist
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pairdist_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rmax2, scale = float(pairdist.cutoff2_of(R_MAX)), float(pairdist.scale_of(R_MAX, N_BINS))
    ceiling = k20_rate()
    lines = ["K29 (csrc/pair_hist.hip) against chunked torch.cdist + bucket index + bincount -- tools/pairdist_probe.py",
             f"command: python tools/pairdist_probe.py --repeats {args.repeats} --out profiles/pairdist.txt",
             f"random-walk chain, 1.5 A steps; r_max {R_MAX} A, {N_BINS} bins, pairs at most 3 bonds apart excluded; median of "
             f"{args.repeats} passes after one warm-up, device events; K20's rate (profiles/contacts.txt): {ceiling:.1f} G pair tests / s"]

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

    for m, S in SHAPES:
        rng = np.random.default_rng(m)
        step = rng.normal(size=(S, m, 3))
        step *= 1.5 / np.linalg.norm(step, axis=2, keepdims=True)
        x = torch.from_numpy(np.cumsum(step, axis=1).astype(np.float32)).to(dev)
        i = np.arange(m)
        band = np.abs(i[:, None] - i[None, :]) <= 3
        d_excl = torch.from_numpy(ensemble.pack_mask(band).view(np.int32)).to(dev)
        counted = torch.from_numpy(np.triu(~band, 1)).to(dev)
        d_sel = torch.arange(m, dtype=torch.int32, device=dev)
        need = int(lib.cgv_pairdist_workspace_bytes(S, m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        bad = torch.zeros(S, dtype=torch.int32, device=dev)
        for C in (1, 4):
            P = pairdist.n_pairs_of(C)
            cls = (np.arange(m) * 7 // 3) % C                        # neighbours mostly differ, as the elements of a peptide do
            d_cls = torch.from_numpy(cls.astype(np.int32)).to(dev)
            pc = torch.from_numpy(pairdist.pair_index(cls[:, None], cls[None, :], C)).to(dev)
            hist = torch.zeros(P, N_BINS, dtype=torch.int64, device=dev)
            beyond = torch.zeros(P, dtype=torch.int64, device=dev)

            def kernel():
                hist.zero_(), beyond.zero_()
                _lib.call("cgv_pairdist_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_cls), _lib.ptr(d_excl), S, m, m, C, N_BINS,
                          rmax2, scale, _lib.ptr(hist), _lib.ptr(beyond), _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

            chunk = max(1, min(S, (1 << 25) // (m * m)))
            table = torch.zeros(P * (N_BINS + 1), dtype=torch.int64, device=dev)
            row = (pc * (N_BINS + 1))[counted]                       # of the counted pairs, in the order of the mask

            def tensor_ops():
                table.zero_()
                for s0 in range(0, S, chunk):
                    p = x[s0:s0 + chunk]
                    d = torch.cdist(p, p)[:, counted]                # [chunk, counted pairs]
                    slot = torch.where(d < R_MAX, (d * scale).long().clamp_(max=N_BINS - 1), N_BINS)
                    table.add_(torch.bincount((slot + row[None, :]).reshape(-1), minlength=P * (N_BINS + 1)))

            k_med, k_min, k_max = timed(kernel)
            t_med, t_min, t_max = timed(tensor_ops)
            mine = torch.cat([hist, beyond[:, None]], dim=1)
            theirs = table.reshape(P, N_BINS + 1)
            differ = int((mine != theirs).sum())
            moved = int((mine - theirs).abs().sum()) // 2
            assert torch.equal(mine.sum(1), theirs.sum(1)), "a class pair's total differs: not a matter of rounding"
            assert int(bad.sum()) == 0
            pairs = m * (m - 1) // 2
            rate = pairs * S / k_med / 1e6
            lines += ["", f"m = {m}, {S} structures, C = {C} ({P} class pairs): {pairs * S / 1e6:.1f} M pair tests, "
                          f"{int(hist.sum()) / max(int(mine.sum()), 1):.3f} of the counted pairs in range",
                      f"cgv_pairdist_counts  {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {rate:.1f} G pair tests / s = "
                      f"{rate / ceiling:.3f} of K20's rate",
                      f"torch cdist form     {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   chunk {chunk} structures",
                      f"ratio torch / kernel {t_med / k_med:9.2f}   entries of the two tables that differ: {differ} of {mine.numel()}, by "
                      f"{moved} pairs of {int(mine.sum())} (a differently rounded distance at a bin edge)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
