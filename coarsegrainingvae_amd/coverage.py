"""Does every conformation of the data have a generated structure near it (coverage, recall), and is every generated
structure near some conformation of the data (precision)?  "Near" is the whole-structure RMSD after optimal
superposition, computed for every pair of the two sets on the device (K17, ``cgv_superpose``; ``csrc/superpose.hip``).

Nothing in the reference computes this: its RMSDs are unaligned (``sampling.py: compute_rmsd``), which is meaningful only
between a sample and its own source frame.  ``build_dataset`` gives every frame a random rotation, so a frame cannot be
compared with another frame's samples without superposition, and two ensembles can agree in every histogram of
``distributions.compare`` and still miss whole conformations.

``rmsd^2(i, j) = max(0, G_a[i] + G_b[j] - 2 lambda(i, j)) / m`` over the ``m`` selected atoms: ``G`` the sum of squared
centred coordinates, ``lambda`` the largest eigenvalue of the quaternion key matrix of the 3 x 3 cross-covariance --
proper rotations only, a mirror image is not a superposition.  The nine cross-covariance entries of all pairs are one
fp64 GEMM on the matrix cores, the rotation solve and the nearest-neighbour reductions are the kernel's epilogue: no
``[Sa, Sb]`` tensor exists unless ``rmsd_matrix`` asks for it.  A structure with a non-finite selected coordinate is
*bad*: NaN in the dense matrix, never a nearest neighbour, its own minimum ``+inf`` with index ``-1``.

The host pieces shared with the other analyses (``structures``, ``selection``, ``read_back``, ...) live in ``ensemble``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, ensemble
from .ensemble import check_sets, device_of, read_back, select_atoms, structures

MAX_DENSE_PAIRS = 1 << 24


def limits() -> Dict[str, int]:
    return ensemble.limits("superpose")


def _pair_of_sets(a, b, sel):
    """Both sets as tensors and the selection as the kernel takes it (it may name an atom more than once)."""
    a, b = structures(a), structures(b)
    if int(a.shape[1]) != int(b.shape[1]):
        raise ValueError(f"the two sets have different atom counts (mismatched n): {int(a.shape[1])} and {int(b.shape[1])}")
    return a, b, ensemble.selection(sel, int(a.shape[1]), purpose="superpose", unique=False, max_atoms=limits()["atoms"])


def new_state(sa: int, sb: int, device) -> Dict[str, torch.Tensor]:
    """Running nearest neighbours as ``cgv_superpose`` merges into them: ``(+inf, -1)`` everywhere."""
    return {"row_min": torch.full((sa,), float("inf"), dtype=torch.float64, device=device),
            "row_arg": torch.full((sa,), -1, dtype=torch.int32, device=device),
            "col_min": torch.full((sb,), float("inf"), dtype=torch.float64, device=device),
            "col_arg": torch.full((sb,), -1, dtype=torch.int32, device=device)}


def superpose_launch(a: torch.Tensor, b: torch.Tensor, sel: torch.Tensor, row_min: torch.Tensor, row_arg: torch.Tensor,
                     col_min: torch.Tensor, col_arg: torch.Tensor, off_a: int = 0, off_b: int = 0, same: bool = False,
                     dense: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> None:
    """One ``cgv_superpose`` call on device tensors: ``a [sa,n,3]``, ``b [sb,n,3]`` fp32, ``sel [m]`` int32.  The SQUARED
    minima of this rectangle are MERGED into ``row_min [sa]`` / ``col_min [sb]`` (fp64) and ``row_arg`` / ``col_arg``
    (int32, global indices ``off_b + j`` / ``off_a + i``); ``dense [sa,sb]`` fp64, when given, is overwritten."""
    sa, sb, n, m = int(a.shape[0]), int(b.shape[0]), int(a.shape[1]), int(sel.shape[0])
    if a.dtype != torch.float32 or b.dtype != torch.float32 or sel.dtype != torch.int32:
        raise ValueError("a and b must be float32, sel int32")
    if a.dim() != 3 or b.dim() != 3 or tuple(a.shape[1:]) != (n, 3) or tuple(b.shape[1:]) != (n, 3):
        raise ValueError("a [sa,n,3] and b [sb,n,3] must have the same atom count")
    if not 1 <= m <= n:
        raise ValueError(f"the selection must list 1..{n} atoms, it lists {m}")
    for t, size, dt in ((row_min, sa, torch.float64), (row_arg, sa, torch.int32), (col_min, sb, torch.float64), (col_arg, sb, torch.int32)):
        if tuple(t.shape) != (size,) or t.dtype != dt:
            raise ValueError("row_min [sa] / col_min [sb] must be float64, row_arg [sa] / col_arg [sb] int32")
    if dense is not None and (tuple(dense.shape) != (sa, sb) or dense.dtype != torch.float64):
        raise ValueError("dense must be [sa, sb] float64")
    need = int(_lib.load().cgv_superpose_workspace_bytes(sa, sb))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = ensemble.workspace(need, a.device)
    _lib.call("cgv_superpose", _lib.ptr(a), _lib.ptr(b), _lib.ptr(sel), sa, sb, n, m, int(off_a), int(off_b), int(bool(same)),
              _lib.ptr(row_min), _lib.ptr(row_arg), _lib.ptr(col_min), _lib.ptr(col_arg), _lib.ptr(dense), _lib.ptr(workspace),
              workspace.numel() * workspace.element_size(), _lib.stream_ptr(), tag="superpose")


def rmsd_matrix(a, b, sel=None, device="cuda") -> np.ndarray:
    """The dense superposed RMSD ``[Sa, Sb]`` (host, fp64; NaN for a pair with a bad structure) of two small sets over the
    atoms ``sel`` (default: all).  More than 2^24 pairs are refused: use ``nearest``."""
    a, b, table = _pair_of_sets(a, b, sel)
    sa, sb = int(a.shape[0]), int(b.shape[0])
    if sa * sb > MAX_DENSE_PAIRS:
        raise ValueError(f"{sa} x {sb} pairs: a dense matrix is limited to {MAX_DENSE_PAIRS} pairs (nearest() needs no matrix)")
    lim = limits()["structures"]
    if max(sa, sb) > lim:
        raise ValueError(f"a launch holds {lim} structures per set")
    if sa == 0 or sb == 0:
        return np.zeros((sa, sb), dtype=np.float64)
    dev = device_of(a, device)
    xa, xb = a.detach().to(dev, torch.float32).contiguous(), b.detach().to(dev, torch.float32).contiguous()
    dense = torch.empty(sa, sb, dtype=torch.float64, device=dev)
    superpose_launch(xa, xb, torch.from_numpy(table).to(dev), **new_state(sa, sb, dev), dense=dense)
    return np.sqrt(read_back([dense])[0])


def nearest(a, b, sel=None, exclude_self: bool = False, structures_per_launch: int = 4096, device="cuda"):
    """``row_min [Sa]``, ``row_arg [Sa]``, ``col_min [Sb]``, ``col_arg [Sb]`` (host; fp64 RMSD, not squared, and int64):
    for every structure of ``a`` the superposed RMSD to its nearest structure of ``b`` and that structure's index, and
    the same for every structure of ``b``.  Equal distances go to the lower index.  A structure without a partner (a bad
    one, or every partner bad) has ``(+inf, -1)``.  ``exclude_self``: the pairs ``i == j`` are skipped (``b`` is the same
    set as ``a``).  Both sets are cut into chunks of ``structures_per_launch``, one launch per pair of chunks, the running
    minima stay on the device (the result does not depend on the chunk size, bit for bit); ONE read-back."""
    a, b, table = _pair_of_sets(a, b, sel)
    sa, sb = int(a.shape[0]), int(b.shape[0])
    M = min(max(int(structures_per_launch), 1), limits()["structures"])
    if max(sa, sb) > 2 ** 31 - 1:
        raise ValueError("structure indices are int32")
    dev = device_of(a, device)
    state = new_state(sa, sb, dev)
    if sa and sb:
        stab = torch.from_numpy(table).to(dev)
        xa = a.detach().to(dev, torch.float32).contiguous()
        xb = xa if b is a else b.detach().to(dev, torch.float32).contiguous()
        need = int(_lib.load().cgv_superpose_workspace_bytes(min(M, sa), min(M, sb)))
        workspace = ensemble.workspace(need, dev)
        for oa in range(0, sa, M):
            for ob in range(0, sb, M):
                ea, eb = min(oa + M, sa), min(ob + M, sb)
                superpose_launch(xa[oa:ea], xb[ob:eb], stab, state["row_min"][oa:ea], state["row_arg"][oa:ea],
                                 state["col_min"][ob:eb], state["col_arg"][ob:eb], oa, ob, exclude_self, workspace=workspace)
    row_min, row_arg, col_min, col_arg = read_back([state[k] for k in ("row_min", "row_arg", "col_min", "col_arg")])
    return np.sqrt(row_min), row_arg.astype(np.int64), np.sqrt(col_min), col_arg.astype(np.int64)


# ----------------------------------------------------------------------------- metrics (host)
def _side(minima: np.ndarray, thresholds) -> dict:
    v = np.asarray(minima, dtype=np.float64).reshape(-1)
    matched = v[np.isfinite(v)]
    return {"cov": [float((v <= float(d)).mean()) if v.size else None for d in thresholds],
            "mat_mean": float(matched.mean()) if matched.size else None,
            "mat_median": float(np.median(matched)) if matched.size else None,
            "unmatched": int(v.size - matched.size)}


def metrics_from_nearest(row_min, col_min, thresholds: Sequence[float]) -> dict:
    """Coverage and matching from the nearest-neighbour RMSDs of ``nearest(data, generated)``; pure host.

      thresholds            the deltas, as given
      cov_r  [len]          COV-R(delta): the fraction of data frames with a generated structure within delta (recall)
      mat_r_mean, mat_r_median   MAT-R: mean and median of ``row_min``
      cov_p, mat_p_mean, mat_p_median   the same from ``col_min``: generated structures near the data (precision)
      unmatched_r, unmatched_p   entries that are not finite (``+inf``: no partner).  They count as NOT covered at every
                            delta and are left out of the mean and the median (``None`` when nothing is left)."""
    th = [float(d) for d in thresholds]
    r, p = _side(row_min, th), _side(col_min, th)
    return {"thresholds": th, "cov_r": r["cov"], "mat_r_mean": r["mat_mean"], "mat_r_median": r["mat_median"],
            "cov_p": p["cov"], "mat_p_mean": p["mat_mean"], "mat_p_median": p["mat_median"],
            "unmatched_r": r["unmatched"], "unmatched_p": p["unmatched"]}


METRIC_KEYS = ("thresholds", "cov_r", "mat_r_mean", "mat_r_median", "cov_p", "mat_p_mean", "mat_p_median", "unmatched_r",
               "unmatched_p")


def compare(ref_xyz, gen_xyz, z, thresholds=(0.5, 1.0, 2.0), atoms="heavy", structures_per_launch: int = 4096,
            device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference frames ``ref_xyz [Sr,n,3]`` (at least two) by
    superposed RMSD over ``select_atoms(z, atoms)``, in Angstrom.  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, atoms (the selection used), and the keys of ``metrics_from_nearest`` for ``nearest(ref, gen)``
      floor        the same metrics between the even and the odd reference frames (rows: even, columns: odd): what the
                   data's own sampling gives, the convention of ``distributions.compare``.  Adjacent frames of a
                   molecular-dynamics trajectory are correlated, so an even frame has an odd neighbour closer than an
                   independent sample of the same size would be: the floor is a LOWER bound on MAT and an upper bound
                   on COV, not the value a perfect generator reaches.
      nearest_ref  [n_ref] how many generated structures have reference frame r as their nearest (sums to ``n_gen``
                   less ``unmatched_p``): frames no sample chose, and frames that attract most samples, are visible"""
    ref, gen = structures(ref_xyz), structures(gen_xyz)
    sel = select_atoms(z, atoms)
    check_sets(ref, gen, z, gen_width=False)                  # nearest() refuses a generated set of another width
    kw = dict(structures_per_launch=structures_per_launch, device=device)
    row_min, _, col_min, col_arg = nearest(ref, gen, sel, **kw)
    even_min, _, odd_min, _ = nearest(ref[0::2], ref[1::2], sel, **kw)
    chosen = np.bincount(col_arg[col_arg >= 0], minlength=int(ref.shape[0]))
    return {"n_ref": int(ref.shape[0]), "n_gen": int(gen.shape[0]), "atoms": [int(i) for i in sel],
            **metrics_from_nearest(row_min, col_min, thresholds), "floor": metrics_from_nearest(even_min, odd_min, thresholds),
            "nearest_ref": chosen.tolist()}


COV_STATS_KEYS = ("n_ref", "n_gen", "atoms") + METRIC_KEYS + ("floor", "nearest_ref")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"cov_stats"`` in their JSON summary line."""
    return {k: stats[k] for k in ("n_ref", "n_gen") + METRIC_KEYS + ("floor",)}
