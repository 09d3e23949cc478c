#!/usr/bin/env python3
"""Time K33 (cgv_saxs_hist; csrc/saxs_hist.hip) against two other forms of a weighted per-structure distance histogram on
the same GPU and the same input -- random-walk chains of 1.5 A steps, all atoms selected, mixed-sign weights, bins of 0.1 A
out to twice the largest centroid distance (so nothing is beyond r_max):

    protein    2 048 atoms x    512 structures
    chignolin    138 atoms x  8 192 structures
    dipeptide     22 atoms x 65 536 structures

    python tools/saxs_probe.py [--repeats 7] [--out profiles/saxs.txt]

  tensor-op form   chunked ``torch.cdist`` over the pairs i < j, a bin index, one weighted ``index_add_`` into ``[S, n_bins]``
  K29              ``cgv_pairdist_counts`` with one class and no exclusion: NOT the same result -- one histogram for the whole
                   ensemble, unweighted, 256 bins at the most -- but the same pairs through the same bin rule: what the
                   per-structure, weighted, 64-bit cells cost
  K33 split = 1    at the protein's size: one block per structure, against the library's choice of blocks per structure

Method: device tensors, one warm-up pass of each form, then ``--repeats`` passes, device events around a pass, nothing read
back inside the window; the median and the spread are printed.  K33's pass is ``cgv_saxs_hist`` on all structures at once (the
gather, then the pair kernel), ``hist`` and ``beyond`` zeroed inside the window.  A pair test is one unordered pair of one
structure.  Outside the window the two weighted tables are compared: every structure's total must agree exactly (nothing is
beyond r_max), single entries may differ where ``cdist`` rounds a distance onto the other side of a bin edge.  No GPU: the
probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("protein", 2048, 512), ("chignolin", 138, 8192), ("dipeptide", 22, 65536))
BIN = 0.1


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import _lib, ensemble, pairdist, saxs
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("saxs_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = ["K33 (csrc/saxs_hist.hip) against chunked torch.cdist + bin index + weighted index_add_, and against K29 -- tools/saxs_probe.py",
             f"command: python tools/saxs_probe.py --repeats {args.repeats} --out profiles/saxs.txt",
             f"random-walk chains, 1.5 A steps; all atoms, mixed-sign weights; bins of {BIN} A, nothing beyond r_max; median of "
             f"{args.repeats} passes after one warm-up, device events"]

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

    for name, m, S in SHAPES:
        rng = np.random.default_rng(m)
        step = rng.normal(size=(S, m, 3))
        step *= 1.5 / np.linalg.norm(step, axis=2, keepdims=True)
        host = np.cumsum(step, axis=1).astype(np.float32)
        r_max, n_bins = saxs.default_r_max(host, np.arange(m), BIN)
        if n_bins > saxs.limits()["bins"]:
            raise SystemExit(f"{name}: {n_bins} bins")
        x = torch.from_numpy(host).to(dev)
        wq = saxs.quantise(rng.uniform(-4.0, 9.0, m))
        rmax2, scale = float(pairdist.cutoff2_of(r_max)), float(pairdist.scale_of(r_max, n_bins))
        d_sel, d_wq = torch.arange(m, dtype=torch.int32, device=dev), torch.from_numpy(wq).to(dev)
        need = int(lib.cgv_saxs_workspace_bytes(S, m))
        ws = torch.empty((need + 15) // 16 * 4, dtype=torch.float32, device=dev)
        hist = torch.zeros(S, n_bins, dtype=torch.int64, device=dev)
        beyond, bad = torch.zeros(S, dtype=torch.int64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)

        def kernel(split=0):
            hist.zero_(), beyond.zero_()
            _lib.call("cgv_saxs_hist", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_wq), S, m, m, n_bins, rmax2, scale, split, _lib.ptr(hist),
                      _lib.ptr(beyond), _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

        iu, ju = (torch.from_numpy(v).to(dev) for v in np.triu_indices(m, 1))
        ww = (d_wq.long()[iu] * d_wq.long()[ju])[None, :]
        chunk = max(1, min(S, (1 << 24) // max(m * m, 1)))
        table = torch.zeros(S * n_bins, dtype=torch.int64, device=dev)
        rows = (torch.arange(chunk, device=dev) * n_bins)[:, None]

        def tensor_ops():
            table.zero_()
            for s0 in range(0, S, chunk):
                p = x[s0:s0 + chunk]
                d = torch.cdist(p, p)[:, iu, ju]                     # [chunk, pairs]
                inside = d < r_max
                slot = (d * scale).long().clamp_(max=n_bins - 1) + rows[:p.shape[0]] + s0 * n_bins
                table.index_add_(0, slot[inside], ww.expand_as(slot)[inside])

        # K29 on the same pairs: one class, nothing excluded but the diagonal, its own 256 bins at the most
        nb29 = min(n_bins, pairdist.limits()["bins"])
        scale29 = float(pairdist.scale_of(r_max, nb29))
        d_cls = torch.zeros(m, dtype=torch.int32, device=dev)
        d_excl = torch.from_numpy(ensemble.pack_mask(np.eye(m, dtype=bool)).view(np.int32)).to(dev)
        hist29, beyond29 = torch.zeros(1, nb29, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)

        def k29():
            hist29.zero_(), beyond29.zero_()
            _lib.call("cgv_pairdist_counts", _lib.ptr(x), _lib.ptr(d_sel), _lib.ptr(d_cls), _lib.ptr(d_excl), S, m, m, 1, nb29, rmax2, scale29,
                      _lib.ptr(hist29), _lib.ptr(beyond29), _lib.ptr(bad), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr())

        pairs = m * (m - 1) // 2
        k_med, k_min, k_max = timed(kernel)
        mine = hist.clone()
        assert int(bad.sum()) == 0 and int(beyond.sum()) == 0
        t_med, t_min, t_max = timed(tensor_ops)
        theirs = table.reshape(S, n_bins)
        assert torch.equal(mine.sum(1), theirs.sum(1)), "a structure's total differs: not a matter of rounding"
        differ = int((mine != theirs).sum())
        p_med, p_min, p_max = timed(k29)
        assert int(hist29.sum()) == pairs * S
        rate = pairs * S / k_med / 1e6
        small = m <= lib.cgv_saxs_small()
        layout = f"{lib.cgv_saxs_pack(m, n_bins)} structure(s) a block, a wave each" if small else \
            f"{lib.cgv_saxs_blocks(S, m, 0)} block(s) a structure"
        lines += ["", f"{name}: {m} atoms x {S} structures, r_max {r_max:.1f} A, {n_bins} bins: {pairs * S / 1e6:.1f} M pair tests; {layout}",
                  f"cgv_saxs_hist        {k_med:9.3f} ms  (min {k_min:.3f}, max {k_max:.3f})   {rate:.1f} G pair tests / s",
                  f"torch cdist form     {t_med:9.3f} ms  (min {t_min:.3f}, max {t_max:.3f})   chunk {chunk} structures",
                  f"cgv_pairdist_counts  {p_med:9.3f} ms  (min {p_min:.3f}, max {p_max:.3f})   {pairs * S / p_med / 1e6:.1f} G pair tests / s; "
                  f"one unweighted histogram of {nb29} bins for the ensemble",
                  f"ratio torch / K33 {t_med / k_med:9.2f}   ratio K33 / K29 {k_med / p_med:6.2f}   entries of the two weighted tables that differ: "
                  f"{differ} of {mine.numel()} (a differently rounded distance at a bin edge)"]
        if not small and lib.cgv_saxs_blocks(S, m, 0) != 1:
            s_med, s_min, s_max = timed(lambda: kernel(1))
            assert torch.equal(hist, mine)
            lines += [f"cgv_saxs_hist, split = 1 (one block a structure)  {s_med:9.3f} ms  (min {s_min:.3f}, max {s_max:.3f})   "
                      f"{pairs * S / s_med / 1e6:.1f} G pair tests / s"]
        del table, hist, theirs, mine
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
