"""Does a generated ensemble reproduce the distribution of the all-atom data?  Internal-coordinate histograms on the device
(K15, ``cgv_internal_hist``) and their Jensen-Shannon divergences on the host.

The reference answers this offline in ``CoarseGrainingVAE/plots.py`` with backbone torsions (``ramachandran_plot``) and
bond lengths (``get_bonds``) through mdtraj / pyemma.  Here the feature table comes from the bond graph alone
(``internal_coords``, ``peptide_backbone_torsions``: element and connectivity, no atom names), the histograms of all
features and of the (phi, psi) pairs come from ONE launch per chunk of structures, and no ``[S, features]`` tensor is ever
stored.  The counts are exact integers; everything after them (``js_divergence``, ``compare``) is fp64 on the host.

Row layout of a feature's histogram: ``[under, n_bins bins, over, invalid]`` (``UNDER``, ``OVER``, ``INVALID`` below).

The host pieces shared with the other analyses (``adjacency``, ``peptide_residues``, ``js_divergence``, ``read_back``)
live in ``ensemble``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ensemble
from .ensemble import adjacency, device_of, js_divergence, peptide_residues, read_back

BOND, ANGLE, TORSION = 2, 3, 4
KIND_NAMES = {BOND: "bond", ANGLE: "angle", TORSION: "torsion"}
DEFAULT_BOND_RANGE = (0.5, 2.5)          # Angstrom: covers every covalent bond of the elements evaluate.COVALENT_RADII lists


@dataclass
class InternalCoords:
    """A feature table as K15 takes it: ``feat [Nf,4]`` int32 atom ids (the first ``kind`` of a row are used, the rest is
    0), ``kind [Nf]`` int32 (2 bond, 3 angle, 4 torsion), ``pairs [Np,2]`` int32 feature ids of two torsions each."""
    feat: np.ndarray
    kind: np.ndarray
    pairs: np.ndarray
    n_atoms: int

    @property
    def n_features(self) -> int:
        return int(self.kind.shape[0])

    @property
    def n_pairs(self) -> int:
        return int(self.pairs.shape[0])

    def atoms(self, f: int) -> Tuple[int, ...]:
        return tuple(int(a) for a in self.feat[f, :int(self.kind[f])])

    def find(self, atoms: Sequence[int]) -> int:
        """The row that holds the feature over ``atoms`` in either direction (a bond, an angle and a proper torsion read
        the same backwards); ``-1`` when the table does not hold it."""
        want = tuple(int(a) for a in atoms)
        for f in np.nonzero(self.kind == len(want))[0]:
            if self.atoms(f) in (want, want[::-1]):
                return int(f)
        return -1

    def with_pairs(self, pairs) -> "InternalCoords":
        return InternalCoords(self.feat, self.kind, np.asarray(pairs, dtype=np.int32).reshape(-1, 2), self.n_atoms)


def internal_coords(z, bonds, which: str = "all") -> InternalCoords:
    """Every bond, angle and proper torsion of the bond graph, each once: bonds ``(i, j)`` with ``i < j``; angles
    ``i-j-k`` with ``i < k`` around every atom ``j``; torsions ``i-j-k-l`` for every bond ``j-k`` (``j < k``), every
    neighbour ``i`` of ``j`` and ``l`` of ``k`` (``i != l``: three-rings have none).  ``which="heavy"`` keeps the
    features whose atoms all have ``z != 1``.  Order: bonds, angles, torsions, each sorted.  No pairs."""
    if which not in ("all", "heavy"):
        raise ValueError("which must be 'all' or 'heavy'")
    z = np.asarray(z).astype(np.int64).reshape(-1)
    n = z.shape[0]
    nbrs = adjacency(n, bonds)
    rows = []
    for i in range(n):
        rows += [(BOND, i, j, 0, 0) for j in nbrs[i] if i < j]
    for j in range(n):
        rows += [(ANGLE, i, j, k, 0) for a, i in enumerate(nbrs[j]) for k in nbrs[j][a + 1:]]
    for j in range(n):
        for k in nbrs[j]:
            if j < k:
                rows += [(TORSION, i, j, k, l) for i in nbrs[j] if i != k for l in nbrs[k] if l != j and l != i]
    if which == "heavy":
        rows = [r for r in rows if all(z[a] != 1 for a in r[1:1 + r[0]])]
    table = np.array(rows, dtype=np.int32).reshape(-1, 5)
    return InternalCoords(np.ascontiguousarray(table[:, 1:]), np.ascontiguousarray(table[:, 0]), np.zeros((0, 2), np.int32), n)


def peptide_backbone_torsions(z, bonds):
    """``(phi, psi, pairs)`` of a peptide from element and connectivity only (trajectory files carry no atom names).
    An amide carbon is a carbon bonded to exactly one oxygen of degree 1 and to a nitrogen.  A residue is ``N-CA-C``: a
    nitrogen, a carbon neighbour of it that is no amide carbon, an amide carbon bonded to that.  phi = ``C'-N-CA-C`` for
    an amide carbon ``C'`` on N other than C; psi = ``N-CA-C-N'`` for a nitrogen ``N'`` on C other than N.  ``phi`` and
    ``psi`` are lists of atom 4-tuples, ``pairs`` lists ``(index into phi, index into psi)`` of the residues that have
    both.  Nothing matches (a hydrocarbon): three empty lists."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    nbrs = adjacency(z.shape[0], bonds)
    is_amide, residues = peptide_residues(z, nbrs)
    phi, psi, pairs = [], [], []
    for N, CA, C in residues:
        mine_phi = [(Cp, N, CA, C) for Cp in nbrs[N] if is_amide[Cp] and Cp not in (C, CA)]
        mine_psi = [(N, CA, C, Np) for Np in nbrs[C] if z[Np] == 7 and Np not in (N, CA)]
        pairs += [(len(phi) + a, len(psi) + b) for a in range(len(mine_phi)) for b in range(len(mine_psi))]
        phi += mine_phi
        psi += mine_psi
    return phi, psi, pairs


def backbone_pairs(coords: InternalCoords, z, bonds) -> Tuple[InternalCoords, List[Tuple[int, int]]]:
    """``coords`` with the (phi, psi) pairs of ``peptide_backbone_torsions`` as its pair table (rows of ``coords`` found
    by their atoms), and the pairs as ``(phi row, psi row)``."""
    phi, psi, pairs = peptide_backbone_torsions(z, bonds)
    rows = [(coords.find(phi[a]), coords.find(psi[b])) for a, b in pairs]
    rows = [r for r in rows if r[0] >= 0 and r[1] >= 0]
    return coords.with_pairs(rows), rows


# ----------------------------------------------------------------------------- the launch
def limits() -> Dict[str, int]:
    return ensemble.limits("internal_hist", ("features", "pairs", "bins", "bins2", "atoms", "staged_atoms"))


class _DeviceTable:
    """The feature table of an ``InternalCoords`` on a device (one upload)."""

    def __init__(self, coords: InternalCoords, device):
        nf, npair = coords.n_features, coords.n_pairs
        flat = np.concatenate([coords.feat.reshape(-1), coords.kind.reshape(-1), coords.pairs.reshape(-1)]).astype(np.int32)
        pack = torch.from_numpy(flat).to(device)
        self.feat, self.kind, self.pairs = pack[:4 * nf], pack[4 * nf:5 * nf], pack[5 * nf:]
        self.n_features, self.n_pairs = nf, npair


def internal_hist(xyz: torch.Tensor, table: _DeviceTable, n_bins: int, n_bins2: int, bond_range, counts: torch.Tensor,
                  pair_counts: torch.Tensor) -> None:
    """One K15 launch: the histograms of ``xyz [S,n,3]`` (device, fp32) are ADDED to ``counts [Nf, n_bins + 3]`` and
    ``pair_counts [Np, n_bins2, n_bins2]`` (device, int32)."""
    S, n = int(xyz.shape[0]), int(xyz.shape[1])
    if tuple(counts.shape) != (table.n_features, n_bins + 3) or tuple(pair_counts.shape) != (table.n_pairs, n_bins2, n_bins2):
        raise ValueError("counts / pair_counts do not have the shape of the table and the bin counts")
    if counts.dtype != torch.int32 or pair_counts.dtype != torch.int32 or xyz.dtype != torch.float32:
        raise ValueError("xyz must be float32, counts and pair_counts int32")
    _lib.call("cgv_internal_hist", _lib.ptr(xyz), _lib.ptr(table.feat) if table.n_features else None,
              _lib.ptr(table.kind) if table.n_features else None, _lib.ptr(table.pairs) if table.n_pairs else None, S, n,
              table.n_features, table.n_pairs, int(n_bins), int(n_bins2), float(bond_range[0]), float(bond_range[1]),
              _lib.ptr(counts) if table.n_features else None, _lib.ptr(pair_counts) if table.n_pairs else None,
              _lib.stream_ptr(), tag="internal_hist")


def histograms(xyz, coords: InternalCoords, n_bins: int = 36, n_bins2: int = 36, bond_range=DEFAULT_BOND_RANGE,
               structures_per_launch: int = 16384, device="cuda") -> Dict[str, np.ndarray]:
    """``counts [Nf, n_bins + 3]`` and ``pair_counts [Np, n_bins2, n_bins2]`` (host, int64) of the structures
    ``xyz [S,n,3]`` (a host array, or a tensor on any device -- a device tensor decides the device).  One launch per
    ``structures_per_launch`` structures into int32 counts, added to int64 totals after every launch (a slot of one launch
    holds at most its structure count); ONE read-back per call."""
    lim = limits()
    if coords.n_features > lim["features"] or coords.n_pairs > lim["pairs"]:
        raise ValueError(f"{coords.n_features} features / {coords.n_pairs} pairs in one launch (the kernel holds "
                         f"{lim['features']} / {lim['pairs']})")
    if not 1 <= int(n_bins) <= lim["bins"] or not 1 <= int(n_bins2) <= lim["bins2"]:
        raise ValueError(f"n_bins must be in 1..{lim['bins']}, n_bins2 in 1..{lim['bins2']}")
    if not float(bond_range[0]) < float(bond_range[1]):
        raise ValueError("bond_range must be (lo, hi) with lo < hi")
    x = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)))
    if x.dim() != 3 or x.shape[2] != 3 or int(x.shape[1]) != coords.n_atoms:
        raise ValueError(f"xyz must be [structures, {coords.n_atoms}, 3], got {tuple(x.shape)}")
    if coords.n_atoms > lim["atoms"]:
        raise ValueError(f"{coords.n_atoms} atoms per structure (the kernel holds {lim['atoms']})")
    dev = device_of(x, device)
    M = max(int(structures_per_launch), 1)
    table = _DeviceTable(coords, dev)
    shape, shape2 = (coords.n_features, n_bins + 3), (coords.n_pairs, n_bins2, n_bins2)
    total, total2 = torch.zeros(shape, dtype=torch.int64, device=dev), torch.zeros(shape2, dtype=torch.int64, device=dev)
    part, part2 = torch.zeros(shape, dtype=torch.int32, device=dev), torch.zeros(shape2, dtype=torch.int32, device=dev)
    for start, chunk in ensemble.chunks(x, M, dev):
        if start:
            part.zero_(), part2.zero_()
        internal_hist(chunk, table, n_bins, n_bins2, bond_range, part, part2)
        total += part
        total2 += part2
    counts, pair_counts = read_back([total, total2])
    return {"counts": counts, "pair_counts": pair_counts}


def internal_values(xyz: torch.Tensor, table: _DeviceTable, values: torch.Tensor, n_invalid: torch.Tensor) -> None:
    """One ``cgv_internal_values`` launch: the features of ``xyz [S,n,3]`` (device, fp32) are written to ``values [S,Nf]``
    (device, fp64; NaN: invalid), and the invalid items are ADDED to ``n_invalid [1]`` (device, int32)."""
    S, n = int(xyz.shape[0]), int(xyz.shape[1])
    if tuple(values.shape) != (S, table.n_features) or values.dtype != torch.float64 or xyz.dtype != torch.float32:
        raise ValueError("xyz must be float32 and values float64 [structures, features]")
    if tuple(n_invalid.shape) != (1,) or n_invalid.dtype != torch.int32:
        raise ValueError("n_invalid must be int32 [1]")
    if S == 0 or table.n_features == 0:
        return
    _lib.call("cgv_internal_values", _lib.ptr(xyz), _lib.ptr(table.feat), _lib.ptr(table.kind), S, n, table.n_features,
              _lib.ptr(values), _lib.ptr(n_invalid), _lib.stream_ptr(), tag="internal_values")


def feature_values(xyz, coords: InternalCoords, rows=None, structures_per_launch: int = 16384, device="cuda",
                   return_invalid: bool = False):
    """The internal coordinates themselves: ``values [S, F]`` (host, fp64) of the structures ``xyz [S,n,3]`` (a host
    array, or a tensor on any device -- a device tensor decides the device) for the rows ``rows`` of ``coords`` (default:
    all, ``F = Nf``), computed by the device function that K15 bins with.  An invalid item (a non-finite coordinate, an
    atom outside the structure) is NaN; ``return_invalid=True`` also returns their number.  One launch per
    ``structures_per_launch`` structures, ONE read-back."""
    lim = limits()
    sub = coords
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        if r.shape[0] and (r.min() < 0 or r.max() >= coords.n_features):
            raise ValueError(f"rows name feature {int(r.max() if r.max() >= coords.n_features else r.min())}, the table has {coords.n_features}")
        sub = InternalCoords(np.ascontiguousarray(coords.feat[r]), np.ascontiguousarray(coords.kind[r]), np.zeros((0, 2), np.int32),
                             coords.n_atoms)
    if sub.n_features > lim["features"]:
        raise ValueError(f"{sub.n_features} features in one launch (the kernel holds {lim['features']})")
    x = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)))
    if x.dim() != 3 or x.shape[2] != 3 or int(x.shape[1]) != coords.n_atoms:
        raise ValueError(f"xyz must be [structures, {coords.n_atoms}, 3], got {tuple(x.shape)}")
    if not 1 <= coords.n_atoms <= lim["atoms"]:
        raise ValueError(f"{coords.n_atoms} atoms per structure (the kernel holds 1..{lim['atoms']})")
    dev = device_of(x, device)
    M = max(int(structures_per_launch), 1)
    table = _DeviceTable(sub, dev)
    values = torch.empty((int(x.shape[0]), sub.n_features), dtype=torch.float64, device=dev)
    n_invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    for start, chunk in ensemble.chunks(x, M, dev):
        internal_values(chunk, table, values[start:start + M], n_invalid)
    out, bad = read_back([values, n_invalid])
    return (out, int(bad[0])) if return_invalid else out


# ----------------------------------------------------------------------------- host statistics
UNDER, OVER, INVALID = 0, -2, -1         # slots of a feature's row next to its bins [1 : -2]


def outside(row) -> Dict[str, int]:
    """What a feature's row counted outside its bins."""
    row = np.asarray(row)
    return {"under": int(row[UNDER]), "over": int(row[OVER]), "invalid": int(row[INVALID])}


def _mean(values) -> Optional[float]:
    v = [x for x in values if x is not None]
    return float(np.mean(v)) if v else None


def _divergences(a: Dict[str, np.ndarray], b: Dict[str, np.ndarray], coords: InternalCoords, heavy: np.ndarray) -> dict:
    jsd = [js_divergence(a["counts"][f, 1:-2], b["counts"][f, 1:-2]) for f in range(coords.n_features)]
    pair = [js_divergence(a["pair_counts"][p], b["pair_counts"][p]) for p in range(coords.n_pairs)]
    mean = {scope: {name: _mean(jsd[f] for f in range(coords.n_features) if coords.kind[f] == k and (scope == "all" or heavy[f]))
                    for k, name in KIND_NAMES.items()} for scope in ("all", "heavy")}
    return {"jsd": jsd, "pair_jsd": pair, "mean": {**mean, "pair": _mean(pair)}}


def compare(ref_xyz, gen_xyz, z, bonds, n_bins: int = 36, n_bins2: int = 36, bond_range=DEFAULT_BOND_RANGE,
            structures_per_launch: int = 16384, device="cuda") -> dict:
    """Generated structures ``gen_xyz [Sg,n,3]`` against reference structures ``ref_xyz [Sr,n,3]`` of the molecule
    ``z [n]`` / ``bonds [Eb,2]``, over every internal coordinate of the bond graph and the (phi, psi) maps of a peptide's
    backbone.  Three sets of histograms: the generated structures, the even and the odd frames of the reference (their
    integer sum is the reference's).  Returns a dict that ``json.dump`` takes:

      n_ref, n_gen, n_bins, n_bins2, bond_range
      features   atoms [Nf][kind], kind [Nf], heavy [Nf] (no hydrogen among its atoms), jsd [Nf] (``None``: an empty
                 histogram), floor [Nf] (the same between the even and the odd reference frames), outside_ref /
                 outside_gen [Nf] ({under, over, invalid}: counted, and left out of the distributions)
      pairs      phi [Np], psi [Np] (feature rows), jsd [Np], floor [Np]
      mean       {all: {bond, angle, torsion}, heavy: {...}, pair}  means of jsd over the features of a kind / the pairs
      floor      the same means of the noise floor: two finite samples of one distribution do not have JSD 0, and this is
                 what ``mean`` is to be read against
      counts     {ref, gen}: the histograms [Nf][n_bins + 3] themselves, pair_counts {ref, gen} [Np][n_bins2][n_bins2]
    """
    z = np.asarray(z).astype(np.int64).reshape(-1)
    coords, rows = backbone_pairs(internal_coords(z, bonds, "all"), z, bonds)
    ref = ref_xyz if torch.is_tensor(ref_xyz) else torch.from_numpy(np.ascontiguousarray(np.asarray(ref_xyz, dtype=np.float32)))
    kw = dict(n_bins=n_bins, n_bins2=n_bins2, bond_range=bond_range, structures_per_launch=structures_per_launch, device=device)
    even, odd = histograms(ref[0::2], coords, **kw), histograms(ref[1::2], coords, **kw)
    gen = histograms(gen_xyz, coords, **kw)
    whole = {k: even[k] + odd[k] for k in even}
    heavy = np.array([all(z[a] != 1 for a in coords.atoms(f)) for f in range(coords.n_features)], dtype=bool)
    d, floor = _divergences(whole, gen, coords, heavy), _divergences(even, odd, coords, heavy)
    return {"n_ref": int(ref.shape[0]), "n_gen": int(gen_xyz.shape[0]), "n_bins": int(n_bins), "n_bins2": int(n_bins2),
            "bond_range": [float(bond_range[0]), float(bond_range[1])],
            "features": {"atoms": [list(coords.atoms(f)) for f in range(coords.n_features)], "kind": coords.kind.tolist(),
                         "heavy": heavy.tolist(), "jsd": d["jsd"], "floor": floor["jsd"],
                         "outside_ref": [outside(r) for r in whole["counts"]], "outside_gen": [outside(r) for r in gen["counts"]]},
            "pairs": {"phi": [r[0] for r in rows], "psi": [r[1] for r in rows], "jsd": d["pair_jsd"], "floor": floor["pair_jsd"]},
            "mean": d["mean"], "floor": floor["mean"],
            "counts": {"ref": whole["counts"].tolist(), "gen": gen["counts"].tolist()},
            "pair_counts": {"ref": whole["pair_counts"].tolist(), "gen": gen["pair_counts"].tolist()}}


DIST_STATS_KEYS = ("n_ref", "n_gen", "n_bins", "n_bins2", "bond_range", "features", "pairs", "mean", "floor", "counts", "pair_counts")


def summary_of(stats: dict) -> dict:
    """What the command-line tools put under ``"dist_stats"`` in their JSON summary line: the means and their floors."""
    return {"mean": stats["mean"], "floor": stats["floor"], "n_ref": stats["n_ref"], "n_gen": stats["n_gen"]}
