"""Build libcgvae_hip.so in-tree with hipcc for gfx950 (no JIT cache, no torch extension).

    python -m coarsegrainingvae_amd.build            # incremental
    python -m coarsegrainingvae_amd.build --force

hipcc cross-compiles without a GPU, so this also is the "does it build" check of
``__graft_entry__.build()``.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJDIR = os.path.join(PKG, "build")
LIB = os.path.join(PKG, "libcgvae_hip.so")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-ffp-contract=fast", "-I", INCLUDE, "-I", CSRC]
# per-source additions (after FLAGS, so they win): the sample-quality kernels compare bit-reproducible squared sums
# (csrc/sq_dist.h) against host-derived thresholds -- no product may fuse into a sum there; the histogram kernel's fp64
# path from coordinates to bin index is restated on the host operation for operation; the TICA kernels' fp32 distances
# are restated in numpy.float32 bit for bit; the two forms of the betweenness kernel and of the baseline trainer must
# round alike; the contact kernels test sq_dist2 against a cutoff that the host restates bit for bit; the alignment
# kernel's rotation solve (csrc/superpose_rot.h) is the text a host program compiles to measure it against LAPACK; the
# surface kernel builds a sphere point as a rounded product plus a rounded sum and tests sq_dist2 against a rounded r * r,
# all restated on the host bit for bit; the hydrogen-bond kernel tests sq_dist2 against a cutoff and the square of a rounded
# dot product against a rounded product of three, restated the same way; the secondary-structure kernel places a virtual
# hydrogen by a rounded square root and quotient and tests a sum of four rounded reciprocal distances, a sq_dist2 and a bend
# like the hydrogen-bond angle, all restated bit for bit; the principal-component kernel's feature is a widened coordinate
# minus an fp64 centre (and, in the projection, minus an fp64 mean before the product), restated in numpy bit for bit; the
# lDDT kernel compares the rounded difference of two rounded square roots of sq_dist2 with thresholds, and sq_dist2 with the
# square of a rounded sum of radii, restated the same way; the pair-distance kernel truncates the rounded product of a
# rounded square root of sq_dist2 and a host-made scale to a bin index, restated the same way; the distance-moments kernel
# rounds the rounded square root of sq_dist2 minus a centre, and the rounded square of that, to fixed point, restated the
# same way; the stereochemistry kernel reads the SIGN of a rounded triple product, of a rounded dot product of two rounded
# cross products, and of the rounded numerators of a segment-triangle intersection against each other, restated the same way;
# the relaxation kernel's whole step -- rounded products, quotients and square roots of sq_dist2, 25 steps deep -- is restated
# in numpy.float32 and its coordinates compared bit for bit; the scattering kernel bins by K29's rule, restated the same way.
# kde.hip has NO entry: its fp32 stage sums are checked against an error bound, not restated bit for bit, and its one
# contraction that matters (the minimum image) is written as an explicit fmaf -- the default flags do; cluster.hip has none
# either: its only floating-point operation is a comparison of doubles that K17 wrote
SOURCE_FLAGS = {"newman.hip": ["-ffp-contract=off"], "baseline.hip": ["-ffp-contract=off"],
                "sample_quality.hip": ["-ffp-contract=off"], "ensemble_check.hip": ["-ffp-contract=off"],
                "internal_hist.hip": ["-ffp-contract=off"], "tica.hip": ["-ffp-contract=off"],
                "contact_map.hip": ["-ffp-contract=off"], "align_mean.hip": ["-ffp-contract=off"],
                "sasa.hip": ["-ffp-contract=off"], "hbond.hip": ["-ffp-contract=off"],
                "dssp.hip": ["-ffp-contract=off"], "pca.hip": ["-ffp-contract=off"], "lddt.hip": ["-ffp-contract=off"],
                "pair_hist.hip": ["-ffp-contract=off"], "dist_moments.hip": ["-ffp-contract=off"],
                "stereo.hip": ["-ffp-contract=off"], "relax.hip": ["-ffp-contract=off"],
                "saxs_hist.hip": ["-ffp-contract=off"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libcgvae_hip.so cannot be built")
    return exe


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _compile(src: str, force: bool) -> str:
    obj = os.path.join(OBJDIR, os.path.basename(src).rsplit(".", 1)[0] + ".o")
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(INCLUDE, "cgvae_hip.h"))
    if not force and _newer(obj, [src] + headers):
        return obj
    cmd = [_hipcc(), *FLAGS, *SOURCE_FLAGS.get(os.path.basename(src), []), "-x", "hip", "-c", src, "-o", obj]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{res.stderr[-4000:]}")
    return obj


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJDIR, exist_ok=True)
    srcs = sources()
    with cf.ThreadPoolExecutor(max_workers=min(6, len(srcs))) as pool:
        objs = list(pool.map(lambda s: _compile(s, force), srcs))
    if force or not _newer(LIB, objs):
        cmd = [_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB, *objs]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"link failed:\n{res.stderr[-4000:]}")
    if verbose:
        print(f"built {LIB} ({os.path.getsize(LIB) / 1024:.0f} KiB) from {len(objs)} objects")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
