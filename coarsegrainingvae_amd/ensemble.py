"""What the analyses of ensembles share (``evaluate``, ``distributions``, ``tica``, ``coverage``, ``contacts``,
``flexibility``, ``density``, ``sasa``, ``cluster``, ``hbonds``, ``dssp``, ``pca``, ``lddt``, ``pairdist``, ``distmat``, ``stereo``, ``relax``, ``saxs``): the host plumbing around their kernels and the topology helpers more
than one of them reads.  This module imports none of them, so each imports it at module level; what is here is public, and nothing here
launches a kernel.  The front end of the stand-alone command lines (``sasa``, ``cluster``, ``hbonds``, ``dssp``, ``pca``, ``lddt``, ``pairdist``, ``distmat``, ``stereo``, ``relax``, ``saxs``: files, parser, summary line) is
``compare_cli``, which imports this module and is imported by them.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

WORKSPACE_BYTES = 1 << 28              # structures_per_launch is lowered until the packed copy of a launch fits this


# ----------------------------------------------------------------------------- device plumbing
def structures(x) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"structures must be [S, n, 3], got {tuple(t.shape)}")
    return t


def device_of(x: torch.Tensor, device) -> torch.device:
    """A device tensor decides the device; a host tensor goes to ``device``."""
    return x.device if x.is_cuda else torch.device(device)


def read_back(tensors: Sequence[torch.Tensor]) -> List[np.ndarray]:
    """ONE device-to-host copy for a set of tensors (widest element type first, so every piece stays aligned)."""
    order = sorted(range(len(tensors)), key=lambda i: -tensors[i].element_size())
    flat = torch.cat([tensors[i].detach().contiguous().reshape(-1).view(torch.uint8) for i in order]).cpu()
    out, at = [None] * len(tensors), 0
    for i in order:
        t = tensors[i]
        nbytes = t.numel() * t.element_size()
        out[i] = flat[at:at + nbytes].view(t.dtype).reshape(t.shape).numpy()
        at += nbytes
    return out


def limits(prefix: str, keys=("structures", "atoms")) -> Dict[str, int]:
    """What a kernel family holds, as its library says: ``cgv_<prefix>_max_<key>()`` for every key."""
    lib = _lib.load()
    return {k: int(getattr(lib, f"cgv_{prefix}_max_{k}")()) for k in keys}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch of at least ``nbytes`` bytes, in whole doubles (the kernels keep fp64 partial sums in it)."""
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.float64, device=device)


def structures_per_launch(requested: int, limit: int, bytes_per_structure: int) -> int:
    """The request lowered to what a launch holds and to what keeps its packed copy within ``WORKSPACE_BYTES`` (never
    below 64 for the budget's sake); at least 1."""
    return max(1, min(int(requested), limit, max(64, WORKSPACE_BYTES // bytes_per_structure)))


def chunks(x: torch.Tensor, M: int, dev) -> Iterator[Tuple[int, torch.Tensor]]:
    """``(start, chunk)`` for every ``M`` structures of ``x``, the chunk on ``dev``, fp32 and contiguous."""
    for start in range(0, int(x.shape[0]), M):
        yield start, x[start:start + M].detach().to(dev, torch.float32).contiguous()


# ----------------------------------------------------------------------------- the map of two components (tica, pca)
def check_hist2(spec, k: int, lim: Dict[str, int], bins_name: str = "n_bins2"):
    """``(comp_a, comp_b, n_bins2, (lo_a, hi_a), (lo_b, hi_b))`` of a projection onto ``k`` components as plain numbers, or
    ``ValueError``: more bins than the family's ``lim["bins2"]``, a component outside ``[0, k)``, a range without ``lo < hi``."""
    ca, cb, nb, ra, rb = spec[:5]
    if not 1 <= int(nb) <= lim["bins2"]:
        raise ValueError(f"{bins_name} must be in 1..{lim['bins2']}")
    if not (0 <= int(ca) < k and 0 <= int(cb) < k):
        raise ValueError(f"the histogram's components must be in [0, {k})")
    if not (float(ra[0]) < float(ra[1]) and float(rb[0]) < float(rb[1])):
        raise ValueError("histogram ranges must be (lo, hi) with lo < hi")
    return int(ca), int(cb), int(nb), (float(ra[0]), float(ra[1])), (float(rb[0]), float(rb[1]))


def hist2_args(hist, k: int, lim: Dict[str, int]) -> tuple:
    """The nine trailing arguments of ``cgv_tica_project`` / ``cgv_pca_project`` from what a ``project_launch`` is handed:
    ``None`` (no histogram) or ``(*spec, counts [nb,nb] int32, outside [1] int32)``, checked (``check_hist2``)."""
    if hist is None:
        return 0, 0, 0, 0.0, 1.0, 0.0, 1.0, None, None
    ca, cb, nb, ra, rb = check_hist2(hist, k, lim)
    counts, outside = hist[5], hist[6]
    if tuple(counts.shape) != (nb, nb) or counts.dtype != torch.int32 or outside.numel() != 1 or outside.dtype != torch.int32:
        raise ValueError("counts [n_bins2, n_bins2] and outside [1] must be int32")
    return ca, cb, nb, ra[0], ra[1], rb[0], rb[1], _lib.ptr(counts), _lib.ptr(outside)


class Hist2:
    """The map of two components over the launches of one ``project``: the kernel adds a launch's structures into an
    int32 pair, the running totals are int64 (a set may hold more than 2^31 structures).  The spec is checked before
    anything is allocated."""

    def __init__(self, spec, k: int, lim: Dict[str, int], device, bins_name: str = "n_bins2"):
        self.spec = check_hist2(spec, k, lim, bins_name)
        nb = self.spec[2]
        self.counts, self.outside = (torch.zeros(s, dtype=torch.int32, device=device) for s in ((nb, nb), (1,)))
        self.total, self.total_out = (torch.zeros(s, dtype=torch.int64, device=device) for s in ((nb, nb), (1,)))
        self.used = False

    def launch(self, run) -> None:
        """``run(hist)`` is one ``project_launch``: the int32 pair is zeroed before every launch after the first and
        added to the totals after it."""
        if self.used:
            self.counts.zero_(), self.outside.zero_()
        self.used = True
        run((*self.spec, self.counts, self.outside))
        self.total += self.counts
        self.total_out += self.outside

    def totals(self) -> List[torch.Tensor]:
        """``[counts [nb,nb], outside [1]]`` int64, to append to the one ``read_back``."""
        return [self.total, self.total_out]


# ----------------------------------------------------------------------------- selections and sets
def selection(sel, n_atoms: int, *, purpose: str, at_least: int = 1, unique: bool = True,
              max_atoms: Optional[int] = None) -> np.ndarray:
    """The selection as a kernel takes it (int32 ``[m]``, in the caller's order; default: every atom); ``ValueError``
    before any launch for a structure of more than ``max_atoms`` atoms, an empty selection (there are no atoms to
    ``purpose``), fewer than ``at_least`` atoms, an index outside ``[0, n_atoms)`` and, with ``unique``, an atom named
    twice.  Without ``unique`` an atom may repeat, but not more entries than atoms."""
    if max_atoms is not None and n_atoms > max_atoms:
        raise ValueError(f"{n_atoms} atoms per structure (the kernel holds {max_atoms})")
    s = np.arange(n_atoms, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64).reshape(-1)
    if s.shape[0] == 0:
        raise ValueError(f"the selection is empty (m = 0): no atoms to {purpose}")
    if s.shape[0] < at_least:
        raise ValueError(f"the selection lists {s.shape[0]} atoms: a rotation needs at least {at_least}")
    if not unique and s.shape[0] > n_atoms:
        raise ValueError(f"the selection lists {s.shape[0]} atoms, a structure has {n_atoms}")
    if s.min() < 0 or s.max() >= n_atoms:
        raise ValueError(f"the selection names atom {int(s.max() if s.max() >= n_atoms else s.min())}, a structure has {n_atoms} atoms")
    if unique and np.unique(s).shape[0] != s.shape[0]:
        raise ValueError("the selection names an atom twice")
    return np.ascontiguousarray(s.astype(np.int32))


def select_atoms(z, atoms="heavy") -> np.ndarray:
    """``"heavy"``: every atom that is not hydrogen; ``"all"``; or an index array, taken as it is."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    if isinstance(atoms, str):
        if atoms not in ("heavy", "all"):
            raise ValueError("atoms must be 'heavy', 'all' or an index array")
        return np.flatnonzero(z != 1) if atoms == "heavy" else np.arange(z.shape[0])
    return np.asarray(atoms, dtype=np.int64).reshape(-1)


def check_sets(ref_xyz, gen_xyz, z, *, groups=None, gen_width: bool = True):
    """What every ``compare`` checks first, in this order: both sets are ``[S, n, 3]``, there are at least two reference
    frames, ``z`` lists as many atoms as a frame has (``gen_width``: a generated structure too), ``groups`` is a known
    kind.  Returns ``(ref, gen, z)``: the sets as tensors, ``z`` as int64 ``[n]``."""
    ref, gen = structures(ref_xyz), structures(gen_xyz)
    z = np.asarray(z).astype(np.int64).reshape(-1)
    n = int(ref.shape[1])
    if int(ref.shape[0]) < 2:
        raise ValueError("at least two reference frames are needed (the floor compares the even with the odd ones)")
    if not gen_width:
        if z.shape[0] != n:
            raise ValueError(f"z lists {z.shape[0]} atoms, a reference frame has {n}")
    elif z.shape[0] != n or int(gen.shape[1]) != n:
        raise ValueError(f"z lists {z.shape[0]} atoms, the frames have {n} and {int(gen.shape[1])}")
    if groups not in (None, "bead", "residue"):
        raise ValueError("groups must be None, 'bead' or 'residue'")
    return ref, gen, z


# ----------------------------------------------------------------------------- pair masks of the packed pair kernels
def square_mask(mask, m: int, what: str) -> np.ndarray:
    """``mask`` as it is when it is a symmetric bool array ``[m, m]``; ``ValueError`` naming ``what`` otherwise."""
    a = np.asarray(mask)
    if a.dtype != np.bool_ or a.shape != (m, m):
        raise ValueError(f"{what} must be a bool array [{m}, {m}], got {a.dtype} {a.shape}")
    if not np.array_equal(a, a.T):
        raise ValueError(f"{what} must be symmetric")
    return a


def pack_mask(mask) -> np.ndarray:
    """``[r, c]`` bool as the pair kernels' ``[r, ceil(c/32)]`` uint32: bit ``j & 31`` of word ``j >> 5``."""
    a = np.asarray(mask, dtype=bool)
    r, c = a.shape
    words = max((c + 31) // 32, 1)
    padded = np.zeros((r, 32 * words), dtype=bool)
    padded[:, :c] = a
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").astype(np.uint32)


# ----------------------------------------------------------------------------- topology (host)
def adjacency(n: int, bonds) -> List[List[int]]:
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    if b.shape[0] and (b.min() < 0 or b.max() >= n):
        raise ValueError(f"bonds name atom {int(b.max())}, z has {n} atoms")
    nbrs = [set() for _ in range(n)]
    for i, j in b.tolist():
        if i != j:
            nbrs[i].add(j)
            nbrs[j].add(i)
    return [sorted(s) for s in nbrs]


def peptide_residues(z, nbrs):
    """The rule of ``distributions.peptide_backbone_torsions``: ``(is_amide [n], [(N, CA, C), ...])`` in the order of N,
    then of its neighbours CA, then of CA's neighbours C (``tica.backbone_atoms`` selects the same atoms)."""
    n = z.shape[0]

    def amide(c):
        if z[c] != 6:
            return False
        carbonyl = [o for o in nbrs[c] if z[o] == 8 and len(nbrs[o]) == 1]
        return len(carbonyl) == 1 and any(z[a] == 7 for a in nbrs[c])
    is_amide = [amide(c) for c in range(n)]
    residues = []
    for N in range(n):
        if z[N] != 7:
            continue
        for CA in nbrs[N]:
            if z[CA] != 6 or is_amide[CA]:
                continue
            residues += [(N, CA, C) for C in nbrs[CA] if is_amide[C] and C != N]
    return is_amide, residues


def groups_of(z, bonds, mapping=None, kind: str = "bead") -> np.ndarray:
    """A group label for every atom of the molecule, ``[n]`` int64.  ``"bead"``: the coarse-graining ``mapping``.
    ``"residue"``: the residues of a peptide found from elements and connectivity (``peptide_residues``: N - CA - C'),
    numbered in the order of their N; every other atom joins the residue whose backbone is the fewest bonds away (a
    carbonyl O its C', a side chain its CA, a terminal cap the residue it is bonded to).  ``ValueError`` when the molecule
    has no such backbone, or an atom is not connected to one."""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    n = z.shape[0]
    if kind == "bead":
        if mapping is None:
            raise ValueError("groups of kind 'bead' need the coarse-graining mapping")
        m = np.asarray(mapping, dtype=np.int64).reshape(-1)
        if m.shape[0] != n:
            raise ValueError(f"the mapping lists {m.shape[0]} atoms, z has {n}")
        return m
    if kind != "residue":
        raise ValueError("kind must be 'bead' or 'residue'")
    nbrs = adjacency(n, bonds)
    _, residues = peptide_residues(z, nbrs)
    if not residues:
        raise ValueError("groups of kind 'residue' need a peptide: no N - CA - C' backbone was found in the bond graph")
    label = np.full(n, -1, dtype=np.int64)
    r = 0
    for triple in residues:                                   # in the order of N
        if all(label[a] < 0 for a in triple):
            label[list(triple)] = r
            r += 1
    frontier = [a for a in range(n) if label[a] >= 0]         # ascending: ties go to the atom met first
    while frontier:
        nxt = []
        for a in frontier:
            for b in nbrs[a]:
                if label[b] < 0:
                    label[b] = label[a]
                    nxt.append(b)
        frontier = nxt
    if (label < 0).any():
        raise ValueError(f"atom {int(np.flatnonzero(label < 0)[0])} is not connected to a peptide backbone: it belongs to no residue")
    return label


# ----------------------------------------------------------------------------- host statistics
def js_divergence(counts_a, counts_b) -> Optional[float]:
    """Jensen-Shannon divergence, base 2 (in [0, 1]), of two histograms given as integer counts over the same bins (any
    shape; a feature's row without its under / over / invalid slots, or a pair's ``[n_bins2, n_bins2]`` map).  fp64.
    Bins empty in both are skipped.  ``None`` when either histogram is empty: there is no distribution to compare."""
    a = np.asarray(counts_a, dtype=np.float64).reshape(-1)
    b = np.asarray(counts_b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("the histograms have different bins")
    na, nb = a.sum(), b.sum()
    if na <= 0 or nb <= 0:
        return None
    keep = (a > 0) | (b > 0)
    p, q = a[keep] / na, b[keep] / nb
    m = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl_p = np.where(p > 0, p * np.log2(p / m), 0.0).sum()
        kl_q = np.where(q > 0, q * np.log2(q / m), 0.0).sum()
    return float(min(max(0.5 * (kl_p + kl_q), 0.0), 1.0))


def hist(values: np.ndarray, lo: float, hi: float, n_bins: int) -> dict:
    """``n_bins`` equal bins on ``[lo, hi]`` (the upper edge belongs to the last bin); what falls outside is counted in
    ``under`` / ``over`` and left out, as ``distributions`` does."""
    v = np.asarray(values, dtype=np.float64)
    inside = v[(v >= lo) & (v <= hi)]
    counts = np.histogram(inside, bins=int(n_bins), range=(lo, hi))[0] if hi > lo else np.zeros(int(n_bins), dtype=np.int64)
    return {"counts": counts.astype(np.int64).tolist(), "under": int((v < lo).sum()), "over": int((v > hi).sum())}


def moments(v: np.ndarray):
    return (float(v.mean()), float(v.std())) if v.size else (None, None)


def scalar_block(ref_e, ref_o, gen, lo, hi, n_bins) -> dict:
    """Histograms, JSD with its even / odd floor, and the moments of one per-structure quantity."""
    ref = np.concatenate([ref_e, ref_o])
    he, ho, hg = hist(ref_e, lo, hi, n_bins), hist(ref_o, lo, hi, n_bins), hist(gen, lo, hi, n_bins)
    hr = {"counts": (np.asarray(he["counts"]) + np.asarray(ho["counts"])).tolist(), "under": he["under"] + ho["under"],
          "over": he["over"] + ho["over"]}
    (mr, sr), (mg, sg) = moments(ref), moments(gen)
    return {"range": [float(lo), float(hi)], "hist_ref": hr, "hist_gen": hg, "jsd": js_divergence(hr["counts"], hg["counts"]),
            "floor": js_divergence(he["counts"], ho["counts"]), "mean_ref": mr, "std_ref": sr, "mean_gen": mg, "std_gen": sg}


MOMENTS = ("jsd", "mean_ref", "std_ref", "mean_gen", "std_gen")


def short_block(block: Optional[dict], names=MOMENTS) -> Optional[dict]:
    """What a ``summary_of`` keeps of a ``scalar_block``: no histograms."""
    return None if block is None else {name: block[name] for name in names}


def set_sizes(even: dict, odd: dict, gen: dict) -> Dict[str, int]:
    """The structures of the reference (its even and odd frames) and of the generated set, and those left out as bad,
    from the ``bad [S]`` of three results."""
    n_of = lambda *rs: int(sum(np.asarray(r["bad"]).shape[0] for r in rs))
    n_bad = lambda *rs: int(sum(np.asarray(r["bad"], dtype=bool).sum() for r in rs))
    return {"n_ref": n_of(even, odd), "n_gen": n_of(gen), "n_bad_ref": n_bad(even, odd), "n_bad_gen": n_bad(gen)}
