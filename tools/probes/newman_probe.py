#!/usr/bin/env python3
"""Time the Girvan-Newman partition (cgmap.partition_newman, csrc/newman.hip) on the bond graph of each bench workload
(data.WORKLOADS: the chain bonds of data.synthetic_frames, at the workload's n_cgs) and, where networkx imports, networkx
on the same graph (what the reference's get_partition calls, datasets.py:373-385).

    python tools/probes/newman_probe.py [--workloads dipeptide chignolin protein2000] [--repeat 3] [--no-networkx]
    python tools/probes/newman_probe.py --option newman_form=2        # the streamed form at every size

Prints one line per workload and a JSON line at the end.  GPU time is wall time of the whole call (uploads, every launch,
the per-batch counter reads, the final download), best of --repeat after one warm-up call."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from coarsegrainingvae_amd import cgmap, data, options  # noqa: E402


def networkx_seconds(n, bonds, n_cgs):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(map(tuple, bonds.tolist()))
    t0 = time.time()
    for communities in itertools.islice(nx.community.girvan_newman(G), n_cgs - 1):
        pass
    seconds = time.time() - t0
    mapping = np.zeros(n, dtype=np.int64)
    for k, group in enumerate(tuple(sorted(c) for c in communities)):
        mapping[list(group)] = k
    return seconds, mapping


def main(argv=None):
    argv = options.pop_cli(list(sys.argv[1:] if argv is None else argv))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(data.WORKLOADS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-networkx", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    rows = []
    for name in a.workloads:
        w = data.WORKLOADS[name]
        n, k = w["n_atoms"], w["n_cgs"]
        bonds = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
        cgmap.partition_newman(bonds, n, k, device=a.device)                     # warm-up (module load, allocator)
        best, info, mapping = None, None, None
        for _ in range(max(a.repeat, 1)):
            mapping, info = cgmap.partition_newman(bonds, n, k, device=a.device)
            best = info["seconds"] if best is None else min(best, info["seconds"])
        row = {"workload": name, "n_atoms": n, "n_cgs": k, "removals": info["removals"], "launches": info["launches"],
               "form": info["form"], "gpu_seconds": best, "networkx_seconds": None, "same_mapping": None}
        if not a.no_networkx:
            try:
                row["networkx_seconds"], ref = networkx_seconds(n, bonds, k)
                row["same_mapping"] = bool(np.array_equal(ref, mapping.numpy()))
            except ImportError:
                pass
        rows.append(row)
        print(f"{name}: n {n} n_cgs {k} removals {row['removals']} launches {row['launches']} form {row['form']} "
              f"gpu {best:.4f} s networkx {row['networkx_seconds']} same mapping {row['same_mapping']}", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
