"""The front end of the stand-alone command lines that compare generated structures with a reference (``sasa``,
``cluster``, ``hbonds``, ``dssp``, ``pca``, ``lddt``, ``pairdist``, ``distmat``, ``stereo``, ``relax``, ``saxs``): the options and files they all take, the refusals that need no device, and the way they end.  Pure
host code: it launches no kernel and imports none of the analyses; they import it, and add their own options and checks
between ``base_parser`` and ``finish_parser``, and after ``read_sets``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os

import numpy as np


def base_parser(prog: str, description: str, *, top_help: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog=prog, description=description)
    p.add_argument("-gen", required=True, help="npz with xyz [T,K,n,3] or [S,n,3]: the generated structures (backmap -out)")
    p.add_argument("-ref", required=True, help="npz with xyz [T,n,3]: the reference frames, at least two")
    p.add_argument("-top", default=None, help=top_help)
    return p


def finish_parser(p: argparse.ArgumentParser, out_default: str) -> argparse.ArgumentParser:
    """The two options that come after a tool's own."""
    p.add_argument("-out", default=out_default, help=f"where the full statistics go ({out_default})")
    p.add_argument("-device", default="cuda")
    return p


def read_npz(path: str, need) -> dict:
    if not os.path.exists(path):
        raise SystemExit(f"{path}: no such file")
    with np.load(path, allow_pickle=False) as f:
        missing = sorted(set(need) - set(f.files))
        if missing:
            raise SystemExit(f"{path}: missing {missing}")
        return {k: f[k] for k in f.files}


def read_sets(args, need=("z", "bonds")):
    """``(ref_xyz [Sr,n,3], gen_xyz [S,n,3], z [n] int64, top, ref)`` from ``-ref``, ``-gen`` and ``-top``: the two sets as
    fp32 arrays (a ``-gen`` of ``[T,K,n,3]`` flattened), and the files the topology (``need``) and the frames came from, for
    whatever else the caller picks out of them -- ``top`` is ``ref`` without ``-top``.  ``SystemExit`` for a missing file or
    key, frames that do not have the topology's atoms, and fewer than two reference frames."""
    ref = read_npz(args.ref, ["xyz"])
    top = read_npz(args.top, need) if args.top else ref
    if any(key not in top for key in need):
        raise SystemExit(f"{args.ref}: missing {' / '.join(need)} (or pass -top)")
    z = np.asarray(top["z"]).astype(np.int64).reshape(-1)
    n = z.shape[0]
    ref_xyz = np.asarray(ref["xyz"], dtype=np.float32)
    if ref_xyz.ndim != 3 or ref_xyz.shape[1:] != (n, 3):
        raise SystemExit(f"{args.ref}: xyz is {ref_xyz.shape}, the topology has {n} atoms")
    if ref_xyz.shape[0] < 2:
        raise SystemExit(f"{args.ref}: at least two reference frames are needed")
    gen_xyz = np.asarray(read_npz(args.gen, ["xyz"])["xyz"], dtype=np.float32)
    if gen_xyz.ndim not in (3, 4) or gen_xyz.shape[-2:] != (n, 3):
        raise SystemExit(f"{args.gen}: xyz is {gen_xyz.shape}, the topology has {n} atoms")
    return ref_xyz, gen_xyz.reshape(int(np.prod(gen_xyz.shape[:-2])), n, 3), z, top, ref    # not -1: n may be 0 until the caller looks


@contextlib.contextmanager
def refusing(prefix: str = ""):
    """A ``ValueError`` of the block ends the command line with its message."""
    try:
        yield
    except ValueError as err:
        raise SystemExit(prefix + str(err))


def write_stats(stats: dict, out: str) -> None:
    with open(out, "w") as f:
        json.dump(stats, f)


def print_summary(stem: str, summary: dict, out: str) -> None:
    print(json.dumps({stem + "_stats": summary, "out": out}), flush=True)


def finish(stem: str, stats: dict, summary: dict, out: str) -> None:
    """The full statistics to ``out``, then the one JSON line to stdout."""
    write_stats(stats, out)
    print_summary(stem, summary, out)
