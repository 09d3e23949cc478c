"""Repair what the checks find: a restrained geometry relaxation of every structure of an ensemble on the device (K32,
``cgv_relax``; ``csrc/relax.hip``).

``lddt`` counts the steric clashes of a backmapped sample, ``distributions`` its stretched bonds, and ``stereo`` opens by
naming the failures "no minimisation repairs".  This module is that minimisation.  It is no force field: it removes bond
lengths and 1-3 distances away from the data's, and non-bonded atoms closer than K28's clash distance, and stays as close
to the generated structure as it can.  The whole loop runs in one launch, a structure resident in LDS for all its steps.

Definition.  Inputs of a launch: ``xyz [S, n, 3]``; ``anchor [S, n, 3]`` (default: ``xyz``); the restraints in per-atom CSR
form (``row_ptr [n+1]``, ``partner``, ``d0``, ``w``: every restraint ``{i, j}`` under both atoms, an atom's entries in
ascending order of the host table's row); ``W_i``, the fp32 sum of atom i's ``w`` in that order, made on the host;
``radii [n]``; ``excl [n, ceil(n/32)]`` (``ensemble.pack_mask``); the scalars.  All arithmetic is fp32, every operation
rounded on its own, ``sqrtf`` and ``/`` correctly rounded.  One step works on atom ``i`` from the positions of the PREVIOUS
step (Jacobi: two buffers and a barrier, so nothing depends on which thread owns which atom):

    g = k_pos * (x_i - a_i)                                                   per component
    for the atom's restraints in table order:
        D = x_i - x_j      q = (D.x*D.x + D.y*D.y) + D.z*D.z                  (csrc/sq_dist.h)
        if q > 0:   d = sqrtf(q)    s = (w * (d - d0)) / d      g = g + s * D
    for j = 0 .. n-1 ascending, j != i, not excl[i][j]:
        c = (r_i + r_j) - tol      D, q as above
        if c > 0 and q < c * c and q > 0:   d = sqrtf(q)   s = (k_rep * (d - c)) / d   g = g + s * D   nc += 1
    h = (k_pos + 2 * W_i) + (2 * k_rep) * float(nc)
    if h > 0:   f = damp / h     delta = (-f) * g     m = (delta.x*delta.x + delta.y*delta.y) + delta.z*delta.z
                if m > cap * cap:   delta = delta * (cap / sqrtf(m))
    else:       delta = 0
    x_i' = x_i + delta

Every comparison is strict and false for a NaN; the clash predicate ``c > 0 and q < c * c`` is K28's exactly, so the count
``relax`` reports is the count ``lddt`` reports.  The doubled diagonal is why ``damp = 1`` is stable: a restraint moves both of
its ends, and a weighted graph Laplacian ``L`` satisfies ``L <= 2 diag(L)``, so a lone pair is satisfied in one step and the
linearised iteration does not grow.

Outputs: ``xyz_out [S, n, 3]`` fp32; ``clashes [S, 2]`` int32, the clashing pairs ``i < j`` before the first step and after
the last (``q = 0`` clashes, though it pushes nothing); ``energy [S, 2]`` fp64, before and after,

    E = sum 1/2 k_pos |x - a|^2  +  sum 1/2 w (d - d0)^2  +  sum 1/2 k_rep (c - d)^2

to which atom ``i`` adds, in fp64 and in this order, ``(0.5 * k_pos) * p`` with ``p = sq_dist2(x_i, a_i)`` in fp32, then
``(0.25 * w) * (t * t)`` with ``t = fp32(sqrtf(q) - d0)`` for each of its restraints, then ``(0.25 * k_rep) * (t * t)`` with
``t = fp32(sqrtf(q) - c)`` for each clashing ``j`` (pair terms at half weight: both ends add them); the atoms are joined by a
fixed tree (``csrc/relax.hip``), no floating-point atomics; ``disp2 [S]`` fp32, the largest ``p`` after the last step;
``bad [S]``.  A structure with a non-finite coordinate (or anchor) is bad: its coordinates are copied through unchanged and
its other outputs are 0.  ``steps = 0`` copies the input and reports the same before and after.  A ``numpy.float32``
restatement reproduces ``xyz_out``, ``clashes``, ``disp2`` and ``bad`` bit for bit, and two calls give the same bits however
the structures are cut into launches.

    python -m coarsegrainingvae_amd.relax -gen samples.npz -ref traj.npz [-top top.npz] [-relax_steps 50] [-relax_kpos 0.05]
        [-relax_krep 1] [-relax_cap 0.25] [-relax_tol 0.4] [-relaxed relaxed.npz] [-out relax_stats.json]

The restraint distances are the means of ``-ref``; ``-relaxed`` takes ``xyz`` in the shape ``-gen`` had (and ``bad``), so
every other tool reads it.  The full statistics of ``compare`` go to ``-out``, one JSON line with ``"relax_stats"`` to stdout.
"""
from __future__ import annotations

import argparse
import math
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, compare_cli, ensemble, stereo
from .contacts import excluded_pairs
from .distributions import ANGLE, BOND, internal_coords
from .ensemble import check_sets, device_of, read_back, structures
from .sasa import radii_of

KIND_BOND, KIND_13 = 0, 1


def limits() -> Dict[str, int]:
    return ensemble.limits("relax", ("structures", "atoms", "steps"))


def pack_of(n_atoms: int) -> int:
    """The structures that share a block at this size (0: more atoms than the kernel holds)."""
    return int(_lib.load().cgv_relax_pack(int(n_atoms)))


# ----------------------------------------------------------------------------- host: the restraint table
def table_of(pairs, d0, w, n_atoms: int, kind=None) -> dict:
    """A restraint table from the caller's rows -- ``pairs [R, 2]``, ``d0 [R]``, ``w [R]`` -- with its CSR form:

      pairs [R,2] int32, kind [R] int32 (0 bond, 1 1-3 pair), d0, w [R] fp32, n_atoms
      row_ptr [n+1] int32, partner [2R] int32, d0_e, w_e [2R] fp32     every restraint under both of its atoms, an atom's
                                                                       entries in ascending order of the table's row
      wsum [n] fp32            the sum of an atom's ``w_e`` in that order, each addition rounded to fp32

    ``ValueError`` for an atom outside ``[0, n_atoms)``, a restraint of an atom with itself, a ``d0`` that is 0 or not
    finite (negative included) and a ``w`` that is no finite number >= 0."""
    n = int(n_atoms)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    R = int(p.shape[0])
    d = np.asarray(d0, dtype=np.float64).reshape(-1).astype(np.float32)
    ww = np.asarray(w, dtype=np.float64).reshape(-1).astype(np.float32)
    k = np.zeros(R, dtype=np.int32) if kind is None else np.asarray(kind, dtype=np.int32).reshape(-1)
    if d.shape[0] != R or ww.shape[0] != R or k.shape[0] != R:
        raise ValueError(f"pairs lists {R} restraints, d0 {d.shape[0]}, w {ww.shape[0]}, kind {k.shape[0]}")
    if R and (p.min() < 0 or p.max() >= n):
        raise ValueError(f"a restraint names atom {int(p.max() if p.max() >= n else p.min())}, a structure has {n} atoms")
    if (p[:, 0] == p[:, 1]).any():
        raise ValueError(f"restraint {int(np.flatnonzero(p[:, 0] == p[:, 1])[0])} ties an atom to itself")
    off = ~(np.isfinite(d) & (d > 0))
    if off.any():
        r = int(np.flatnonzero(off)[0])
        raise ValueError(f"restraint {r} ({int(p[r, 0])}, {int(p[r, 1])}) has the reference distance {float(d[r])}: it must be finite and > 0")
    if not (np.isfinite(ww) & (ww >= 0)).all():
        raise ValueError("a restraint's weight must be a finite number >= 0")
    atom = np.concatenate([p[:, 0], p[:, 1]])
    other = np.concatenate([p[:, 1], p[:, 0]])
    row = np.concatenate([np.arange(R), np.arange(R)])
    order = np.lexsort((row, atom))                            # by atom, then by the table's row
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(atom, minlength=n), out=row_ptr[1:])
    w_e = np.ascontiguousarray(ww[row[order]])
    wsum = np.zeros(n, dtype=np.float32)
    for i in range(n):
        acc = np.float32(0)
        for v in w_e[row_ptr[i]:row_ptr[i + 1]]:
            acc = np.float32(acc + v)
        wsum[i] = acc
    return {"pairs": np.ascontiguousarray(p.astype(np.int32)), "kind": k, "d0": d, "w": ww, "n_atoms": n, "row_ptr": row_ptr,
            "partner": np.ascontiguousarray(other[order].astype(np.int32)), "d0_e": np.ascontiguousarray(d[row[order]]), "w_e": w_e,
            "wsum": wsum}


def pair_lists(z, bonds):
    """``(bonds [B,2], pairs_13 [P,2])`` int64 of the bond graph: the bonds of ``distributions.internal_coords`` and the end
    atoms of its angle rows, each pair once with ``i < j`` in ascending order, without those that are themselves bonds (the
    1-3 pairs of a three-ring)."""
    ic = internal_coords(z, bonds)
    b = ic.feat[ic.kind == BOND][:, :2].astype(np.int64)
    ends = ic.feat[ic.kind == ANGLE][:, [0, 2]].astype(np.int64)
    bonded = {(int(i), int(j)) for i, j in b.tolist()}
    p13 = sorted({(min(i, j), max(i, j)) for i, j in ends.tolist()} - bonded)
    return b.reshape(-1, 2), np.asarray(p13, dtype=np.int64).reshape(-1, 2)


def mean_distances(ref_xyz, pairs) -> np.ndarray:
    """fp64 ``[R]``: the mean distance of every pair over the good frames (all coordinates finite) of ``ref_xyz [T,n,3]``,
    computed in fp64 on the host; NaN without a good frame."""
    ref = structures(ref_xyz).detach().cpu().numpy().astype(np.float64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    good = np.isfinite(ref).all(axis=(1, 2))
    if not good.any():
        return np.full(p.shape[0], np.nan)
    ref = ref[good]
    return np.linalg.norm(ref[:, p[:, 0]] - ref[:, p[:, 1]], axis=-1).mean(axis=0)


def restraints(z, bonds, ref_xyz, *, w_bond: float = 1.0, w_13: float = 0.5) -> dict:
    """The restraint table of a molecule (``table_of``): its bonds at weight ``w_bond``, then its 1-3 pairs at ``w_13``
    (``pair_lists``), each at its mean distance over the good reference frames (``mean_distances``, rounded to fp32 once).
    ``ValueError`` for a restraint whose reference mean is 0 or not finite."""
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    ref = structures(ref_xyz)
    if int(ref.shape[1]) != zz.shape[0]:
        raise ValueError(f"z lists {zz.shape[0]} atoms, a reference frame has {int(ref.shape[1])}")
    b, p13 = pair_lists(zz, bonds)
    pairs = np.concatenate([b, p13])
    kind = np.concatenate([np.full(b.shape[0], KIND_BOND), np.full(p13.shape[0], KIND_13)]).astype(np.int32)
    w = np.where(kind == KIND_BOND, float(w_bond), float(w_13))
    return table_of(pairs, mean_distances(ref, pairs), w, zz.shape[0], kind)


# ----------------------------------------------------------------------------- the launches
def _scalar(name: str, v, positive: bool = False) -> float:
    f = np.float32(v)
    if not np.isfinite(f) or f < 0 or (positive and f == 0):
        raise ValueError(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, got {v}")
    return float(f)


def relax(xyz, tab: dict, z, bonds, *, anchor=None, steps: int = 50, k_pos: float = 0.05, k_rep: float = 1.0, tol: float = 0.4,
          damp: float = 1.0, cap: float = 0.25, exclude: int = 3, radii=None, chunk: int = 4096, device="cuda",
          keep_on_device: bool = False) -> dict:
    """``steps`` steps of the iteration above on the structures ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a
    device tensor decides the device) of the molecule ``z [n]`` / ``bonds`` under the restraints ``tab`` (``restraints`` or
    ``table_of``).  ``anchor [S,n,3]``: where the position spring holds the atoms (default: ``xyz``).  ``radii``: ``{z: R}`` on
    top of the Bondi table (``sasa.radii_of``), or an array ``[n]``; pairs at most ``exclude`` bonds apart never clash
    (``contacts.excluded_pairs``).  Host arrays:

      xyz [S,n,3] fp32         the relaxed structures (``keep_on_device``: a device tensor, and no copy of it to the host)
      clashes [S,2] int32, energy [S,2] fp64     before and after
      disp2 [S] fp32, bad [S] bool, n_good
      table, radii [n] fp32, excl [n,n] bool, and the parameters as the kernel took them (fp32): steps, k_pos, k_rep, tol, damp,
      cap, exclude

    The structures go through in launches of ``chunk`` (``ensemble.chunks``); ONE read-back at the end.  Everything that can be
    refused is a ``ValueError`` before any launch."""
    x = structures(xyz)
    S, n = int(x.shape[0]), int(x.shape[1])
    zz = np.asarray(z).astype(np.int64).reshape(-1)
    if zz.shape[0] != n:
        raise ValueError(f"z lists {zz.shape[0]} atoms, the structures have {n}")
    if int(tab["n_atoms"]) != n:
        raise ValueError(f"the restraint table was made for {int(tab['n_atoms'])} atoms, the structures have {n}")
    lim = limits()
    if n < 1 or n > lim["atoms"]:
        raise ValueError(f"{n} atoms per structure (the kernel holds 1..{lim['atoms']})")
    if not 0 <= int(steps) <= lim["steps"]:
        raise ValueError(f"steps must be in 0..{lim['steps']}, got {steps}")
    if not 1 <= int(chunk) <= lim["structures"]:
        raise ValueError(f"chunk must be in 1..{lim['structures']}, got {chunk}")
    par = {"k_pos": _scalar("k_pos", k_pos), "k_rep": _scalar("k_rep", k_rep), "tol": _scalar("tol", tol),
           "damp": _scalar("damp", damp, positive=True), "cap": _scalar("cap", cap, positive=True)}
    if par["damp"] > 1.0:
        raise ValueError(f"damp must be in (0, 1], got {damp}")
    t = table_of(tab["pairs"], tab["d0"], tab["w"], n, tab.get("kind"))      # the caller's rows, checked again
    anc = x if anchor is None else structures(anchor)
    if tuple(anc.shape) != tuple(x.shape):
        raise ValueError(f"anchor must be {tuple(x.shape)}, got {tuple(anc.shape)}")
    every = np.arange(n)
    if radii is None or isinstance(radii, dict):
        r32 = radii_of(zz, every, radii).astype(np.float32)
    else:
        r32 = np.ascontiguousarray(np.asarray(radii, dtype=np.float32).reshape(-1))
        if r32.shape[0] != n or not np.isfinite(r32).all() or (r32 < 0).any():
            raise ValueError(f"radii must be {n} finite lengths >= 0")
    excl = excluded_pairs(bonds, n, every, exclude)
    dev = device_of(x, device)
    out = {"xyz": torch.empty(S, n, 3, dtype=torch.float32, device=dev), "clashes": torch.zeros(S, 2, dtype=torch.int32, device=dev),
           "energy": torch.zeros(S, 2, dtype=torch.float64, device=dev), "disp2": torch.zeros(S, dtype=torch.float32, device=dev),
           "bad": torch.zeros(S, dtype=torch.int32, device=dev)}
    if S:
        _lib.load()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else None
        d_rp, d_pa, d_d0, d_w, d_ws, d_r = (up(a) for a in (t["row_ptr"], t["partner"], t["d0_e"], t["w_e"], t["wsum"], r32))
        d_ex = up(ensemble.pack_mask(excl).view(np.int32))
        M = min(int(chunk), lim["structures"])
        anchors = iter(()) if anchor is None else ensemble.chunks(anc, M, dev)
        for start, part in ensemble.chunks(x, M, dev):
            k = int(part.shape[0])
            hold = part if anchor is None else next(anchors)[1]
            _lib.call("cgv_relax", _lib.ptr(part), _lib.ptr(hold), _lib.ptr(d_rp), _lib.ptr(d_pa), _lib.ptr(d_d0), _lib.ptr(d_w),
                      _lib.ptr(d_ws), _lib.ptr(d_r), _lib.ptr(d_ex), k, n, int(t["partner"].shape[0]), par["k_pos"], par["k_rep"],
                      par["tol"], par["damp"], par["cap"], int(steps), _lib.ptr(out["xyz"][start:start + k]),
                      _lib.ptr(out["clashes"][start:start + k]), _lib.ptr(out["energy"][start:start + k]),
                      _lib.ptr(out["disp2"][start:start + k]), _lib.ptr(out["bad"][start:start + k]), _lib.stream_ptr(), tag="relax")
    names = ["clashes", "energy", "disp2", "bad"] + ([] if keep_on_device else ["xyz"])
    got = dict(zip(names, read_back([out[k] for k in names])))
    bad = got["bad"].astype(bool)
    return {"xyz": out["xyz"] if keep_on_device else got["xyz"], "clashes": got["clashes"], "energy": got["energy"], "disp2": got["disp2"],
            "bad": bad, "n_good": int(S - int(bad.sum())), "table": t, "radii": r32, "excl": excl, "steps": int(steps), **par,
            "exclude": int(exclude)}


# ----------------------------------------------------------------------------- host statistics
def violation_rms(xyz, tab: dict, good=None) -> Dict[str, Optional[float]]:
    """``{"bonds", "pairs_13"}``: the RMS of ``d - d0`` over the restraints of a kind and the good structures, fp64 on the
    host; ``None`` where there is nothing to average."""
    x = np.asarray(xyz, dtype=np.float64)
    keep = np.isfinite(x).all(axis=(1, 2)) if good is None else np.asarray(good, dtype=bool)
    x = x[keep]
    p, d0, kind = tab["pairs"].astype(np.int64), tab["d0"].astype(np.float64), np.asarray(tab["kind"])
    dev = np.linalg.norm(x[:, p[:, 0]] - x[:, p[:, 1]], axis=-1) - d0[None, :]
    out = {}
    for name, k in (("bonds", KIND_BOND), ("pairs_13", KIND_13)):
        v = dev[:, kind == k]
        out[name] = float(np.sqrt(np.mean(v * v))) if v.size else None
    return out


def stereo_changes(before, after, exp: dict, *, chunk: int = 4096, device="cuda") -> np.ndarray:
    """``[S, 2]`` bool: the structures in which at least one kept centre has another sign (-, flat, +), at least one omega
    another state (cis / trans), after than before.  ``stereo.counts`` reports per structure how many items differ from a
    ``want``, so every item goes through on its own against a fixed ``want``, both sets in one call: 2 calls a centre (not +,
    not -) and 1 an omega."""
    tab = exp["tables"]
    both = np.concatenate([np.asarray(before, dtype=np.float32), np.asarray(after, dtype=np.float32)])
    S = both.shape[0] // 2
    changed = np.zeros((S, 2), dtype=bool)
    none = {"centres": np.zeros((0, 4), np.int32), "torsions": np.zeros((0, 4), np.int32), "rings": np.zeros((0, stereo.MAX_RING), np.int32),
            "bonds": np.zeros((0, 2), np.int32), "tested": np.zeros((0, 0), bool)}
    for row in np.asarray(tab["centres"]).reshape(-1, 4):
        for sign in (1, -1):
            c = stereo.counts(both, {**none, "centres": row[None]}, {"want_sign": [sign]}, chunk=chunk, device=device)["counts"][:, 0]
            changed[:, 0] |= c[:S] != c[S:]
    for row in np.asarray(tab["torsions"]).reshape(-1, 4)[:int(tab.get("n_omega", 0))]:
        c = stereo.counts(both, {**none, "torsions": row[None]}, {"want_cis": [0]}, chunk=chunk, device=device)["counts"][:, 1]
        changed[:, 1] |= c[:S] != c[S:]
    return changed


def _moments(v) -> Optional[dict]:
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "median": float(np.median(v)), "max": float(v.max())} if v.size else None


def _compare(gen_xyz, ref_xyz, z, bonds, *, w_bond=1.0, w_13=0.5, steps=50, k_pos=0.05, k_rep=1.0, tol=0.4, damp=1.0, cap=0.25,
             exclude=3, radii=None, chunk=4096, device="cuda"):
    ref, gen, zz = check_sets(ref_xyz, gen_xyz, z)
    tab = restraints(zz, bonds, ref, w_bond=w_bond, w_13=w_13)
    res = relax(gen, tab, zz, bonds, steps=steps, k_pos=k_pos, k_rep=k_rep, tol=tol, damp=damp, cap=cap, exclude=exclude, radii=radii,
                chunk=chunk, device=device)
    before, after = gen.detach().cpu().numpy().astype(np.float32), res["xyz"]
    good = ~res["bad"]
    refs = ref.detach().cpu().numpy()
    halves = refs[0::2], refs[1::2]
    n_bad_ref = int((~np.isfinite(refs).all(axis=(1, 2))).sum())
    viol = {"before": violation_rms(before, tab, good), "after": violation_rms(after, tab, good),
            "ref_even": violation_rms(halves[0], tab), "ref_odd": violation_rms(halves[1], tab)}
    cl = res["clashes"][good].astype(np.int64)
    clashes = {k: {"clash_free_share": float((cl[:, c] == 0).mean()) if cl.shape[0] else None,
                   "mean": float(cl[:, c].mean()) if cl.shape[0] else None} for c, k in enumerate(("before", "after"))}
    en = res["energy"][good]
    energy = {k: (None if not en.shape[0] else {"mean": float(en[:, c].mean()), "median": float(np.median(en[:, c]))})
              for c, k in enumerate(("before", "after"))}
    move = after[good].astype(np.float64) - before[good].astype(np.float64)
    rmsd = _moments(np.sqrt((move * move).sum(-1).mean(-1)))
    stab = stereo.tables(zz, bonds)
    exp = stereo.expected(ref, stab, chunk=chunk, device=device)
    want = {"want_sign": exp["want_sign"], "want_cis": exp["want_cis"]}
    err = [stereo.counts(s, exp["tables"], want, chunk=chunk, device=device)["counts"][good][:, :2].astype(np.int64) for s in (before, after)]
    changed = stereo_changes(before, after, exp, chunk=chunk, device=device)[good]
    st = {"n_centres": int(exp["tables"]["centres"].shape[0]), "n_omega": int(stab["n_omega"]),
          "wrong_centres": {"before": int(err[0][:, 0].sum()), "after": int(err[1][:, 0].sum())},
          "wrong_torsions": {"before": int(err[0][:, 1].sum()), "after": int(err[1][:, 1].sum())},
          "structures_with_errors": {"before": int((err[0].sum(1) > 0).sum()), "after": int((err[1].sum(1) > 0).sum())},
          "structures_changed": int(changed.any(1).sum()), "structures_changed_centre": int(changed[:, 0].sum()),
          "structures_changed_omega": int(changed[:, 1].sum())}
    params = {k: res[k] for k in ("steps", "k_pos", "k_rep", "tol", "damp", "cap", "exclude")}
    params.update(w_bond=float(w_bond), w_13=float(w_13))
    stats = {"n_ref": int(refs.shape[0]), "n_gen": int(before.shape[0]), "n_bad_ref": n_bad_ref, "n_bad_gen": int(res["bad"].sum()),
             "params": params, "n_atoms": int(zz.shape[0]),
             "n_restraints": {"bonds": int((tab["kind"] == KIND_BOND).sum()), "pairs_13": int((tab["kind"] == KIND_13).sum())},
             "clashes": clashes, "bonds": {k: v["bonds"] for k, v in viol.items()}, "pairs_13": {k: v["pairs_13"] for k, v in viol.items()},
             "energy": energy, "rmsd": rmsd, "disp": _moments(np.sqrt(res["disp2"][good].astype(np.float64))), "stereo": st}
    return stats, res


def compare(gen_xyz, ref_xyz, z, bonds, **kw) -> dict:
    """Relax the generated structures ``gen_xyz [S,n,3]`` under the restraints that the reference frames ``ref_xyz [T,n,3]``
    (at least two) give (``restraints``), and say what that did.  Keyword arguments: those of ``restraints`` and ``relax``.
    Returns a dict that ``json.dump`` takes (``RELAX_STATS_KEYS``); ``before`` / ``after`` are over the good structures:

      n_ref, n_gen, n_bad_ref, n_bad_gen, params, n_atoms, n_restraints {bonds, pairs_13}
      clashes     {before, after}: {clash_free_share, mean}: the share of structures without a clash, the mean clash count
      bonds, pairs_13   {before, after, ref_even, ref_odd}: the RMS restraint violation in Angstrom, next to what the
                  reference's own even and odd frames have against their common mean
      energy      {before, after}: {mean, median}
      rmsd, disp  {mean, median, max} of the non-superposed RMSD between the input and the relaxed structure, and of the
                  largest displacement of an atom
      stereo      through ``stereo.counts`` with ``expected`` from the reference: n_centres, n_omega, wrong_centres and
                  wrong_torsions {before, after}, structures_with_errors {before, after}, and -- on its own --
                  structures_changed (and _centre, _omega): the structures in which relaxation CHANGED any centre's sign or
                  any omega's state, whether that repaired or broke it (``stereo_changes``)
    """
    return _compare(gen_xyz, ref_xyz, z, bonds, **kw)[0]


RELAX_STATS_KEYS = ("n_ref", "n_gen", "n_bad_ref", "n_bad_gen", "params", "n_atoms", "n_restraints", "clashes", "bonds", "pairs_13",
                    "energy", "rmsd", "disp", "stereo")


def summary_of(stats: dict) -> dict:
    """What the command line puts under ``"relax_stats"`` in its JSON summary line: everything but the parameters."""
    return {k: stats[k] for k in RELAX_STATS_KEYS if k != "params"}


# ----------------------------------------------------------------------------- command line
def parser() -> argparse.ArgumentParser:
    p = compare_cli.base_parser("python -m coarsegrainingvae_amd.relax",
                                "relax generated structures towards the reference's bond lengths and 1-3 distances and out of their clashes",
                                top_help="npz with z and bonds; default: those of -ref")
    p.add_argument("-relax_steps", type=int, default=50, help="steps of the iteration (50)")
    p.add_argument("-relax_kpos", type=float, default=0.05, help="stiffness of the spring that holds an atom where it was (0.05)")
    p.add_argument("-relax_krep", type=float, default=1.0, help="stiffness of the clash repulsion (1)")
    p.add_argument("-relax_cap", type=float, default=0.25, help="the most an atom moves in one step, in Angstrom (0.25)")
    p.add_argument("-relax_tol", type=float, default=0.4, help="overlap allowed before a pair clashes, in Angstrom (0.4)")
    p.add_argument("-relaxed", default=None, help="npz that takes the relaxed xyz in the shape -gen had (not written)")
    return compare_cli.finish_parser(p, "relax_stats.json")


def read_inputs(args) -> dict:
    """The command line's files as ``ref_xyz``, ``gen_xyz``, ``z``, ``bonds``, ``shape`` (of ``-gen``'s xyz), with everything
    that can be refused without a device refused here (``SystemExit``)."""
    if args.relax_steps < 0:
        raise SystemExit("-relax_steps must be >= 0")
    for name in ("relax_kpos", "relax_krep", "relax_tol"):
        v = getattr(args, name)
        if not (math.isfinite(v) and v >= 0):
            raise SystemExit(f"-{name} must be a finite number >= 0")
    if not (math.isfinite(args.relax_cap) and args.relax_cap > 0):
        raise SystemExit("-relax_cap must be a finite length > 0 in Angstrom")
    ref_xyz, gen_xyz, z, top, _ = compare_cli.read_sets(args)
    shape = tuple(compare_cli.read_npz(args.gen, ["xyz"])["xyz"].shape)
    with compare_cli.refusing():
        lim = limits()
        if not 1 <= z.shape[0] <= lim["atoms"]:
            raise ValueError(f"{z.shape[0]} atoms per structure (the kernel holds 1..{lim['atoms']})")
        if args.relax_steps > lim["steps"]:
            raise ValueError(f"-relax_steps must be <= {lim['steps']}")
    return {"ref_xyz": ref_xyz, "gen_xyz": gen_xyz, "z": z, "bonds": np.asarray(top["bonds"]), "shape": shape}


def main(argv=None) -> dict:
    args = parser().parse_args(argv)
    inp = read_inputs(args)
    with compare_cli.refusing():
        stats, res = _compare(inp["gen_xyz"], inp["ref_xyz"], inp["z"], inp["bonds"], steps=args.relax_steps, k_pos=args.relax_kpos,
                              k_rep=args.relax_krep, cap=args.relax_cap, tol=args.relax_tol, device=args.device)
    if args.relaxed:
        np.savez(args.relaxed, xyz=res["xyz"].reshape(inp["shape"]), bad=res["bad"].reshape(inp["shape"][:-2]),
                 clashes=res["clashes"], energy=res["energy"])
    compare_cli.finish("relax", stats, summary_of(stats), args.out)
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
