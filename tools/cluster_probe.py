#!/usr/bin/env python3
"""Time K24 (cgv_cluster_pack + cgv_cluster_gromos; csrc/cluster.hip) against a tensor-op form of the SAME definition on
the same GPU:

    chignolin   93 heavy atoms, 10 000 structures      adjacency + gromos against dense + threshold + argmax loop
    dipeptide   10 atoms, 32 768 structures            (the limit)
    path graph  32 768 structures                      gromos alone: the longest loop, 10 923 iterations
    identity    32 768 structures                      gromos alone: 32 768 clusters (the singleton pass)

    python tools/cluster_probe.py [--repeats 5] [--torch_repeats 1] [--out profiles/cluster.txt]

The structures are seeded: noisy copies (0.3 A) of 40 random-walk templates in uneven shares, cutoff 1.0 A.  Method:
device tensors, one warm-up pass of each form, then ``--repeats`` passes of the kernels and ``--torch_repeats`` of the
tensor-op form, device events around a pass (the one read-back of the labels is inside the window of both forms); median,
min and max are printed.  The tensor-op form is the dense ``[S, S]`` fp64 matrix from the same chunked ``cgv_superpose``
calls, thresholded with torch (upper triangle mirrored, diagonal by ``isnan``) into a boolean matrix, and the loop as
``(adj & alive).sum(1)`` masked to the alive, ``argmax`` (the first of equal maxima), one ``.item()`` per iteration.  Its
labels are compared with the kernel's outside the window.  For the two synthetic graphs the boolean matrix is built
directly.  No GPU: the probe fails, it does not fall back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("chignolin", 93, 10000), ("dipeptide", 10, 32768))
LIMIT = 32768
CUTOFF = 1.0


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import cluster, coverage
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch_repeats", type=int, default=1)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_probe needs a GPU")
    dev = torch.device("cuda", 0)
    lines = ["K24 (csrc/cluster.hip) against a tensor-op form of the same definition -- tools/cluster_probe.py",
             f"cutoff {CUTOFF} A, chunks of 4096 structures; median of {args.repeats} kernel passes and {args.torch_repeats} "
             "tensor-op passes after one warm-up each, device events, the read-back of the labels inside the window"]

    def timed(fn, repeats):
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
        return statistics.median(ms), min(ms), max(ms)

    def torch_loop(adj, good):
        """The greedy loop on a boolean [S, S] device matrix; host label array."""
        S = adj.shape[0]
        alive = good.clone()
        label = torch.full((S,), -1, dtype=torch.int32, device=dev)
        k = 0
        while bool(alive.any().item()):
            count = (adj & alive[None, :]).sum(dim=1)
            c = int(torch.where(alive, count, -1).argmax().item())
            members = adj[c] & alive
            members[c] = True
            label[members] = k
            alive &= ~members
            k += 1
        return label.cpu().numpy()

    def dense_adjacency(x, sel):
        S = int(x.shape[0])
        dense = torch.empty(S, S, dtype=torch.float64, device=dev)
        state = coverage.new_state(S, S, dev)
        for oa in range(0, S, 4096):
            for ob in range(oa, S, 4096):
                ea, eb = min(oa + 4096, S), min(ob + 4096, S)
                piece = torch.empty(ea - oa, eb - ob, dtype=torch.float64, device=dev)
                coverage.superpose_launch(x[oa:ea], x[ob:eb], sel, state["row_min"][oa:ea], state["row_arg"][oa:ea],
                                          state["col_min"][ob:eb], state["col_arg"][ob:eb], oa, ob, False, dense=piece)
                dense[oa:ea, ob:eb] = piece
        good = ~torch.isnan(dense.diagonal())
        upper = torch.triu(dense <= CUTOFF * CUTOFF, diagonal=1)
        adj = upper | upper.T
        adj.diagonal().copy_(good)
        return adj, good

    for name, m, S in SHAPES:
        rng = np.random.default_rng(m)
        templates = np.cumsum(rng.normal(0, 1.0, (40, m, 3)), axis=1)
        which = rng.choice(40, size=S, p=np.arange(40, 0, -1) / 820.0)
        xyz = (templates[which] + rng.normal(0, 0.3, (S, m, 3))).astype(np.float32)
        x = torch.from_numpy(xyz).to(dev)
        sel = torch.arange(m, dtype=torch.int32, device=dev)
        out = {}

        def kernel():
            bits = cluster.adjacency(x, None, CUTOFF)
            out["adjacency"] = bits
            out["kernel"] = cluster.gromos(bits, S)

        def only_gromos():
            out["kernel"] = cluster.gromos(out["adjacency"], S)

        def tensor_ops():
            adj, good = dense_adjacency(x, sel)
            out["torch"] = torch_loop(adj, good)

        k_med, k_min, k_max = timed(kernel, args.repeats)
        g_med, g_min, g_max = timed(only_gromos, args.repeats)
        t_med, t_min, t_max = timed(tensor_ops, args.torch_repeats)
        label, centres, sizes = out["kernel"]
        differ = int((label != out["torch"]).sum())
        lines += ["", f"{name}: {m} atoms, {S} structures: {len(centres)} clusters, the largest of {int(sizes.max())}",
                  f"adjacency + gromos   {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})",
                  f"  of which gromos    {g_med:10.3f} ms  (min {g_min:.3f}, max {g_max:.3f})",
                  f"tensor-op form       {t_med:10.3f} ms  (min {t_min:.3f}, max {t_max:.3f})",
                  f"ratio torch / kernel {t_med / k_med:10.2f}   labels of the two forms that differ: {differ} of {S}"]
        print("\n".join(lines[-6:]), flush=True)
        del x, out

    i = torch.arange(LIMIT, device=dev)
    graphs = (("path graph", torch.cat([i, i[:-1], i[1:]]), torch.cat([i, i[1:], i[:-1]])), ("identity", i, i))
    for name, p, q in graphs:
        W = LIMIT // 64
        flat = torch.zeros(LIMIT * W, dtype=torch.int64, device=dev)
        flat.index_put_((p * W + (q >> 6),), torch.ones_like(q) << (q & 63), accumulate=True)
        bits = flat.view(LIMIT, W)
        adj = torch.zeros(LIMIT, LIMIT, dtype=torch.bool, device=dev)
        adj[p, q] = True
        good = torch.ones(LIMIT, dtype=torch.bool, device=dev)
        out = {}

        def kernel():
            out["kernel"] = cluster.gromos(bits, LIMIT)

        def tensor_ops():
            out["torch"] = torch_loop(adj, good)

        k_med, k_min, k_max = timed(kernel, args.repeats)
        t_med, t_min, t_max = timed(tensor_ops, args.torch_repeats)
        label, centres, sizes = out["kernel"]
        differ = int((label != out["torch"]).sum())
        lines += ["", f"{name}: {LIMIT} structures: {len(centres)} clusters",
                  f"gromos               {k_med:10.3f} ms  (min {k_min:.3f}, max {k_max:.3f})",
                  f"tensor-op loop       {t_med:10.3f} ms  (min {t_min:.3f}, max {t_max:.3f})",
                  f"ratio torch / kernel {t_med / k_med:10.2f}   labels of the two forms that differ: {differ} of {LIMIT}"]
        print("\n".join(lines[-4:]), flush=True)
        del adj, bits, flat
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
            f.flush()


if __name__ == "__main__":
    main()
