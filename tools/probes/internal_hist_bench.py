#!/usr/bin/env python3
"""Time one K15 launch (cgv_internal_hist, csrc/internal_hist.hip) at chignolin size: 166 atoms, the full feature table of
the bond graph, the (phi, psi) pairs of the backbone, S = 16 384 structures, 36 bins and 36 x 36 pair bins.

    python tools/probes/internal_hist_bench.py [--structures 16384] [--launches 200] [--repeats 5]

The molecule is a capped 16-residue peptide written out residue by residue (ACE, 14 ALA and 2 GLY, NME: 166 atoms) -- the
atom count of chignolin with a bond graph that needs no topology file; the structures are a seeded random embedding of it
with Gaussian displacements (the kernel's work does not depend on the values, only a histogram's contention does).
Method: 20 warm-up launches, then ``--repeats`` windows of ``--launches`` back-to-back launches each, device events around
a window, the counts zeroed once before it (the launch adds).  Prints the median time per launch and the spread beside
the bytes of coordinates the launch reads (12 S n, once per tile when L2 holds them) and the items (structure x feature
values) it evaluates."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def peptide(residues):
    """``(z, bonds)`` of ACE - residues - NME; a residue is ``"A"`` (N H CA HA CB HB1 HB2 HB3 C O) or ``"G"`` (N H CA HA2 HA3 C O)."""
    z, bonds = [1, 6, 1, 1, 6, 8], [(0, 1), (1, 2), (1, 3), (1, 4), (4, 5)]           # ACE: H CH3 H H C O
    prev_c = 4
    for r in residues:
        n0 = len(z)
        if r == "A":
            z += [7, 1, 6, 1, 6, 1, 1, 1, 6, 8]
            bonds += [(n0, n0 + 1), (n0, n0 + 2), (n0 + 2, n0 + 3), (n0 + 2, n0 + 4), (n0 + 4, n0 + 5), (n0 + 4, n0 + 6),
                      (n0 + 4, n0 + 7), (n0 + 2, n0 + 8), (n0 + 8, n0 + 9)]
            c = n0 + 8
        else:
            z += [7, 1, 6, 1, 1, 6, 8]
            bonds += [(n0, n0 + 1), (n0, n0 + 2), (n0 + 2, n0 + 3), (n0 + 2, n0 + 4), (n0 + 2, n0 + 5), (n0 + 5, n0 + 6)]
            c = n0 + 5
        bonds.append((prev_c, n0))
        prev_c = c
    n0 = len(z)
    z += [7, 1, 6, 1, 1, 1]                                                           # NME: N H CH3 H H H
    bonds += [(prev_c, n0), (n0, n0 + 1), (n0, n0 + 2), (n0 + 2, n0 + 3), (n0 + 2, n0 + 4), (n0 + 2, n0 + 5)]
    return z, bonds


def main():
    import numpy as np
    import torch
    from coarsegrainingvae_amd import distributions as D
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bins", type=int, default=36)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("internal_hist_bench: no GPU; a time per launch cannot be measured here", file=sys.stderr)
        return 1
    z, bonds = peptide("AAAAAAAGAAAAAAAG")
    z, bonds = np.array(z), np.array(bonds)
    n = len(z)
    coords, rows = D.backbone_pairs(D.internal_coords(z, bonds), z, bonds)
    rng = np.random.default_rng(0)
    x0 = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)
    S, nb = args.structures, args.bins
    xyz = torch.from_numpy((x0[None] + 0.1 * rng.standard_normal((S, n, 3))).astype(np.float32)).cuda()
    table = D._DeviceTable(coords, xyz.device)
    counts = torch.zeros(coords.n_features, nb + 3, dtype=torch.int32, device=xyz.device)
    pair_counts = torch.zeros(coords.n_pairs, nb, nb, dtype=torch.int32, device=xyz.device)

    def launch():
        D.internal_hist(xyz, table, nb, nb, D.DEFAULT_BOND_RANGE, counts, pair_counts)
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    assert int(counts.sum()) == 20 * S * coords.n_features
    times = []
    for _ in range(args.repeats):
        counts.zero_(), pair_counts.zero_()
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        for _ in range(args.launches):
            launch()
        end.record()
        torch.cuda.synchronize()
        times.append(beg.elapsed_time(end) * 1e3 / args.launches)
    kinds = [int((coords.kind == k).sum()) for k in (2, 3, 4)]
    items = S * (coords.n_features + 2 * coords.n_pairs)
    med = statistics.median(times)
    print(f"internal_hist  n {n}  S {S}  features {coords.n_features} (bonds {kinds[0]}, angles {kinds[1]}, torsions {kinds[2]})  "
          f"pairs {coords.n_pairs}  bins {nb}  |  median {med:.1f} us/launch (min {min(times):.1f}, max {max(times):.1f}, "
          f"{args.repeats} windows of {args.launches})  |  coordinates {12 * S * n / 1e6:.2f} MB  items {items / 1e6:.2f} M  "
          f"{items / med / 1e3:.2f} G items/s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
