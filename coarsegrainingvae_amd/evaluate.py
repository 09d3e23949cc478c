"""Test-time evaluation: reconstruction quality, conditional ensemble sampling and the sample-quality metrics of the
reference (scripts/sampling.py:120-399, scripts/utils.py:193-268), batched for the device.

The reference evaluates one frame at a time: ``n_ensemble`` decoder calls in a Python loop, every sample copied to the
host and, per sample, four dense ``[n,n]`` distance matrices.  Here a chunk of frames is ONE prior call, ONE decoder call
on the disjoint union of ``frames x samples`` replicated bead graphs, ONE metric launch (K12, ``cgv_sample_quality``:
no ``[n,n]`` tensor) and ONE host read-back.  The host side below only turns the kernel's integer counts and fp64 sums
into the reference's tuples -- pure functions of those outputs (``assemble_*``), quirks included.

Everything runs under ``torch.no_grad()`` and leaves ``model.training`` as it found it; the device generator of
``ops.reparam_sample`` advances when latents are drawn (``ops.get_sample_rng_state`` / ``set_sample_rng_state`` to
bracket an evaluation inside a training run).

``read_back``, the one device-to-host copy every analysis ends with, lives in ``ensemble`` with what else they share.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .data import CG_collate, prepare_batch
from .ensemble import read_back
from .graph import BatchGraph, cutoff_threshold_sq

# Covalent radii in Angstrom behind the bond cutoffs (r_a + r_b) * scale: the CSD legacy covalent radii as published
# (Meng & Lewis, J. Comput. Chem. 12 (1991) 891, table of bonding radii from the Cambridge Structural Database).
# Elements outside this table need ``radii=`` from the caller.
COVALENT_RADII = {1: 0.23, 6: 0.68, 7: 0.68, 8: 0.68, 9: 0.64, 15: 1.05, 16: 1.02, 17: 0.99}

RawQuality = namedtuple("RawQuality", "counts sums")        # [B,K,6] int32, [B,K,2] float64 (device tensors)
DIFF_ALL, DIFF_HEAVY, SIGNED_ALL, SIGNED_HEAVY, REFSUM_ALL, REFSUM_HEAVY = range(6)

# the one-row cv_stats.csv of the reference (scripts/run_ala.py:387-399)
CV_STATS_COLUMNS = ["train_all_recon", "train_heavy_recon", "test_all_recon", "test_heavy_recon", "train_KL", "test_KL",
                    "train_graph", "test_graph", "recon_all_ged", "recon_heavy_ged", "recon_all_valid_ratio",
                    "recon_heavy_valid_ratio", "sample_all_ged", "sample_heavy_ged", "sample_all_valid_ratio",
                    "sample_heavy_valid_ratio", "sample_all_rmsd", "sample_heavy_rmsd"]


# ----------------------------------------------------------------------------- cutoffs
def _host_ints(x) -> np.ndarray:
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()                       # a device tensor is read back here (host values: no sync)
    return np.asarray(x).astype(np.int64).reshape(-1)


def bond_radii(z, radii: Optional[Dict[int, float]] = None) -> np.ndarray:
    """Covalent radius of every atomic number in ``z`` (float64 array): ``COVALENT_RADII``, extended / overridden by
    ``radii``.  An element in neither raises."""
    table = dict(COVALENT_RADII)
    if radii:
        table.update({int(k): float(v) for k, v in radii.items()})
    zs = _host_ints(z)
    missing = sorted({int(e) for e in zs.tolist()} - set(table))
    if missing:
        raise KeyError(f"no covalent radius for atomic number(s) {missing}: the built-in table covers "
                       f"{sorted(COVALENT_RADII)}; pass radii={{Z: radius_in_angstrom}}")
    return np.array([table[int(e)] for e in zs.tolist()], dtype=np.float64)


_THR_CACHE = {}


def bond_thresholds(elements: Sequence[int], scale: float = 1.3, radii: Optional[Dict[int, float]] = None) -> torch.Tensor:
    """``[T,T]`` fp32 table for the sorted ``elements``: the largest squared distance that the reference still calls a
    bond.  The cutoff is ``float32((r_a + r_b) * scale)`` computed exactly as ``compute_bond_cutoff`` does (fp32 tensor
    add, then multiply; sampling.py:120-126); the reference tests ``sqrt(s) < cutoff`` with the host's fp32 sqrt, the
    kernel the bit-reproducible ``s <= cutoff_threshold_sq(cutoff, strict=True)``."""
    elements = [int(e) for e in elements]
    r = bond_radii(elements, radii)
    key = (tuple(elements), float(scale), tuple(r.tolist()))
    hit = _THR_CACHE.get(key)
    if hit is None:
        vdw = torch.Tensor(r.tolist())
        cutoff = (vdw[None, :] + vdw[:, None]) * scale
        hit = torch.tensor([[cutoff_threshold_sq(float(c), strict=True) for c in row] for row in cutoff.tolist()],
                           dtype=torch.float32).reshape(len(elements), len(elements))
        _THR_CACHE[key] = hit
    return hit


class QualityPlan:
    """Host-derived inputs of the metric launch for one set of frames: element classes, heavy flags, thresholds and
    ``frame_ptr`` on the device, frame sizes on the host."""

    def __init__(self, z, frame_ptr, device, scale: float = 1.3, radii: Optional[Dict[int, float]] = None,
                 thresholds=None):
        """``thresholds``: a ``[T,T]`` table for the sorted elements present, used instead of ``bond_thresholds`` --
        the reference's ``sqrt(s) < cutoff`` depends on the host's fp32 sqrt (hosts with the same torch build disagree in
        the last bit), so reproducing bond matrices recorded elsewhere takes the thresholds recorded with them."""
        zs, fp = _host_ints(z), _host_ints(frame_ptr)
        if fp.shape[0] < 1 or fp[0] != 0 or fp[-1] != zs.shape[0] or np.any(np.diff(fp) < 0):
            raise ValueError("frame_ptr must be the [B+1] prefix sum of atoms per frame, ending at len(z)")
        elements = sorted(set(zs.tolist()))
        if len(elements) > int(_lib.load().cgv_sample_quality_max_classes()):
            raise ValueError(f"{len(elements)} different elements in one launch (the kernel holds {_lib.load().cgv_sample_quality_max_classes()})")
        self.z, self.frame_ptr_host = zs, fp
        self.sizes = np.diff(fp)
        self.n_frames, self.n_atoms = int(fp.shape[0] - 1), int(zs.shape[0])
        self.max_atoms = int(self.sizes.max()) if self.n_frames else 0
        self.heavy_host = zs != 1
        run = np.concatenate([[0], np.cumsum(self.heavy_host.astype(np.int64))])
        self.n_heavy = run[fp[1:]] - run[fp[:-1]]
        self.n_classes = max(len(elements), 1)
        if thresholds is not None:
            thr = torch.as_tensor(np.asarray(thresholds), dtype=torch.float32)
            if tuple(thr.shape) != (len(elements), len(elements)) or not torch.equal(thr, thr.t()):
                raise ValueError(f"thresholds must be a symmetric [{len(elements)},{len(elements)}] table for elements {elements}")
        else:
            thr = bond_thresholds(elements, scale, radii) if elements else torch.zeros(1, 1)
        pack = np.concatenate([fp, np.searchsorted(elements, zs), self.heavy_host.astype(np.int64)]).astype(np.int32)
        dev_pack = torch.from_numpy(pack).to(device)
        B, N = self.n_frames, self.n_atoms
        self.frame_ptr, self.cls, self.heavy = dev_pack[:B + 1], dev_pack[B + 1:B + 1 + N], dev_pack[B + 1 + N:]
        self.thr_sq = thr.to(device).contiguous()
        self.device = torch.device(device)


def sample_quality(ref_xyz: torch.Tensor, gen_xyz: torch.Tensor, z=None, frame_ptr=None, n_samples: int = 1,
                   scale: float = 1.3, radii: Optional[Dict[int, float]] = None, plan: Optional[QualityPlan] = None,
                   thresholds=None) -> RawQuality:
    """Raw per-(frame, sample) outputs of K12 as device tensors: ``counts [B,K,6]`` int32 (``DIFF_ALL .. REFSUM_HEAVY``)
    and ``sums [B,K,2]`` float64 (sum of squared deviations over all / heavy atoms).  ``ref_xyz [N,3]`` holds the B
    frames of ``frame_ptr``; ``gen_xyz [K*N,3]`` is frame-major, sample-major inside a frame (include/cgvae_hip.h).
    ``z`` and ``frame_ptr`` are host values (array / CPU tensor: no device sync; device tensors are read back once), or
    pass a ``QualityPlan`` built before."""
    if plan is None:
        plan = QualityPlan(z, frame_ptr, ref_xyz.device, scale, radii, thresholds)
    K = int(n_samples)
    ref = ref_xyz.detach().contiguous().float()
    gen = gen_xyz.detach().contiguous().float()
    if tuple(ref.shape) != (plan.n_atoms, 3) or tuple(gen.shape) != (K * plan.n_atoms, 3):
        raise ValueError(f"expected ref_xyz [{plan.n_atoms},3] and gen_xyz [{K * plan.n_atoms},3], got {tuple(ref.shape)} and {tuple(gen.shape)}")
    counts = torch.empty(plan.n_frames, K, 6, dtype=torch.int32, device=ref.device)
    sums = torch.empty(plan.n_frames, K, 2, dtype=torch.float64, device=ref.device)
    if counts.numel():
        _lib.call("cgv_sample_quality", _lib.ptr(ref), _lib.ptr(gen), _lib.ptr(plan.frame_ptr), _lib.ptr(plan.cls),
                  _lib.ptr(plan.heavy), _lib.ptr(plan.thr_sq), plan.n_frames, plan.n_atoms, K, plan.n_classes, plan.max_atoms,
                  _lib.ptr(counts), _lib.ptr(sums), _lib.stream_ptr(), tag="sample_quality")
    return RawQuality(counts, sums)


# ----------------------------------------------------------------------------- reference-free checks (K14)
RawEnsembleCheck = namedtuple("RawEnsembleCheck", "counts pair_sums")   # [B,K,4] int32, [B,K,K,2] float64 (device tensors)
MISSING_ALL, EXTRA_ALL, MISSING_HEAVY, EXTRA_HEAVY = range(4)
EnsembleCheck = namedtuple("EnsembleCheck", "valid_all valid_heavy missing_all extra_all missing_heavy extra_heavy "
                                            "pair_rmsd_all pair_rmsd_heavy diversity_all diversity_heavy")


def validate_bonds(bonds, sizes, bond_ptr=None):
    """The topology of a K14 launch as host arrays ``(bonds [Eb,2] int32, bond_ptr [B+1] int32)``.  ``bonds`` holds atom
    ids local to their frame; without ``bond_ptr`` the one list belongs to every frame (a trajectory of one molecule).
    Raises ``ValueError`` unless every pair has ``i < j``, occurs once in its frame and lies inside the frame: the
    kernel's ``missing = Eb - H``, ``extra = P - H`` count on it."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    b = _host_ints(bonds).reshape(-1, 2)
    B = sizes.shape[0]
    if bond_ptr is None:
        ptr = np.arange(B + 1, dtype=np.int64) * b.shape[0]
        b = np.tile(b, (B, 1))
    else:
        ptr = _host_ints(bond_ptr)
        if ptr.shape[0] != B + 1 or ptr[0] != 0 or ptr[-1] != b.shape[0] or np.any(np.diff(ptr) < 0):
            raise ValueError("bond_ptr must be the [B+1] prefix sum of bonds per frame, ending at len(bonds)")
    frame_of = np.repeat(np.arange(B), np.diff(ptr))
    if np.any(b[:, 0] >= b[:, 1]):
        raise ValueError("bonds must be pairs (i, j) with i < j")
    if b.shape[0] and (b.min() < 0 or np.any(b[:, 1] >= sizes[frame_of])):
        raise ValueError("bonds hold atom ids outside their frame")
    if b.shape[0] and np.unique(np.column_stack([frame_of, b]), axis=0).shape[0] != b.shape[0]:
        raise ValueError("bonds must list every pair once")
    return b.astype(np.int32), ptr.astype(np.int32)


class BondList:
    """A validated topology on the device for the frames of one ``QualityPlan`` (``validate_bonds``)."""

    def __init__(self, bonds, plan: QualityPlan, bond_ptr=None):
        b, ptr = validate_bonds(bonds, plan.sizes, bond_ptr)
        self.n_bonds, self.n_frames = int(b.shape[0]), plan.n_frames
        pack = torch.from_numpy(np.concatenate([ptr, b.reshape(-1)])).to(plan.device)
        self.bond_ptr, self.bonds = pack[:plan.n_frames + 1], pack[plan.n_frames + 1:]


def ensemble_check(gen_xyz: torch.Tensor, n_samples: int, plan: QualityPlan, bonds, bond_ptr=None) -> RawEnsembleCheck:
    """Raw outputs of K14 as device tensors for the frames of ``plan``: ``counts [B,K,4]`` int32 (``MISSING_ALL ..
    EXTRA_HEAVY``: unordered atom pairs of the topology that the sample does not bond / that it bonds outside the
    topology) and ``pair_sums [B,K,K,2]`` float64 (sum over all / heavy atoms of the squared distance between samples
    k and l).  ``gen_xyz [K*N,3]`` is frame-major, sample-major inside a frame, as for ``sample_quality``.  ``bonds``:
    ``[Eb,2]`` frame-local atom ids with ``i < j`` (``bond_ptr [B+1]``: per-frame lists; without it the list belongs to
    every frame), a ``BondList`` built before, or ``None``: no topology -- the counts stay zero.  One launch."""
    K = int(n_samples)
    lib = _lib.load()
    if K > int(lib.cgv_ensemble_check_max_samples()):
        raise ValueError(f"{K} samples per frame in one launch (the kernel holds {lib.cgv_ensemble_check_max_samples()})")
    gen = gen_xyz.detach().contiguous().float()
    if tuple(gen.shape) != (K * plan.n_atoms, 3):
        raise ValueError(f"expected gen_xyz [{K * plan.n_atoms},3], got {tuple(gen.shape)}")
    if bonds is not None and not isinstance(bonds, BondList):
        bonds = BondList(bonds, plan, bond_ptr)
    if bonds is not None and bonds.n_frames != plan.n_frames:
        raise ValueError("the BondList was built for another set of frames")
    counts = torch.empty(plan.n_frames, K, 4, dtype=torch.int32, device=gen.device)
    pair_sums = torch.empty(plan.n_frames, K, K, 2, dtype=torch.float64, device=gen.device)
    if counts.numel():
        _lib.call("cgv_ensemble_check", _lib.ptr(gen), _lib.ptr(plan.frame_ptr), _lib.ptr(plan.cls), _lib.ptr(plan.heavy),
                  _lib.ptr(plan.thr_sq), _lib.ptr(bonds.bond_ptr) if bonds is not None else None,
                  _lib.ptr(bonds.bonds) if bonds is not None and bonds.n_bonds else None, plan.n_frames, plan.n_atoms, K,
                  plan.n_classes, plan.max_atoms, bonds.n_bonds if bonds is not None else 0, _lib.ptr(counts),
                  _lib.ptr(pair_sums), _lib.stream_ptr(), tag="ensemble_check")
    return RawEnsembleCheck(counts, pair_sums)


def assemble_ensemble_check(counts, pair_sums, n_atoms: int, n_heavy: int) -> EnsembleCheck:
    """ONE frame's K14 outputs (``counts [K,4]``, ``pair_sums [K,K,2]``) as an ``EnsembleCheck``: ``valid_* [K]`` bool
    (missing + extra == 0), the four count columns, ``pair_rmsd_* [K,K] = sqrt(sum / n)`` and ``diversity_*``, the mean
    pairwise RMSD over ``k < l`` -- ``nan`` for a single sample, and for the heavy graph without heavy atoms."""
    counts = np.asarray(counts).astype(np.int64).reshape(-1, 4)
    K = counts.shape[0]
    sums = np.asarray(pair_sums, dtype=np.float64).reshape(K, K, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        rmsd_all = np.sqrt(sums[..., 0] / np.float64(n_atoms))
        rmsd_heavy = np.sqrt(sums[..., 1] / np.float64(n_heavy)) if n_heavy else np.full((K, K), np.nan)
    upper = np.triu_indices(K, 1)
    mean = lambda m: float(m[upper].mean()) if K > 1 else float("nan")
    return EnsembleCheck(counts[:, MISSING_ALL] + counts[:, EXTRA_ALL] == 0, counts[:, MISSING_HEAVY] + counts[:, EXTRA_HEAVY] == 0,
                         counts[:, MISSING_ALL], counts[:, EXTRA_ALL], counts[:, MISSING_HEAVY], counts[:, EXTRA_HEAVY],
                         rmsd_all, rmsd_heavy, mean(rmsd_all), mean(rmsd_heavy))


# ----------------------------------------------------------------------------- host assembly (pure functions)
def assemble_sample_qualities(counts, sums, n_atoms: int, n_heavy: int):
    """The reference's 6-tuple of ``eval_sample_qualities`` for ONE frame (sampling.py:324-333) from the kernel's
    ``counts [K,6]`` / ``sums [K,2]`` of its K samples: ``(all_rmsds, heavy_rmsds, valid_ratio, valid_allatom_ratio,
    graph_val_ratio, graph_allatom_val_ratio)``.  Quirks kept: ``all_rmsds`` rows are ``[aa_rmsd, heavy_rmsd]`` of the
    samples whose ALL-ATOM graph is valid, ``heavy_rmsds`` the same two columns for those whose HEAVY graph is valid,
    ``None`` when no sample is valid; the ratio lists are ``abs(signed sum) / reference sum`` per sample, divided the
    way torch divides two int64 scalars (float32; 0 / 0 = nan)."""
    counts = np.asarray(counts).astype(np.int64).reshape(-1, 6)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    K = counts.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        rmsd = np.stack([np.sqrt(sums[:, 0] / np.float64(n_atoms)), np.sqrt(sums[:, 1] / np.float64(n_heavy))], axis=1)

    def ratios(signed, refsum):
        out = torch.from_numpy(np.abs(counts[:, signed])) / torch.from_numpy(counts[:, refsum].copy())
        return [float(v) for v in out.tolist()]

    valid = np.nonzero(counts[:, DIFF_HEAVY] == 0)[0]
    valid_all = np.nonzero(counts[:, DIFF_ALL] == 0)[0]
    heavy_rmsds = rmsd[valid] if len(valid) else None
    all_rmsds = rmsd[valid_all] if len(valid_all) else None
    return (all_rmsds, heavy_rmsds, len(valid) / K, len(valid_all) / K, ratios(SIGNED_HEAVY, REFSUM_HEAVY),
            ratios(SIGNED_ALL, REFSUM_ALL))


def assemble_ensemble(per_frame: List[tuple]):
    """Last six entries of ``sample_ensemble``'s 10-tuple (sampling.py:385-397) from the per-frame 6-tuples."""
    all_r = [t[0] for t in per_frame if t[0] is not None]
    heavy_r = [t[1] for t in per_frame if t[1] is not None]
    return (np.concatenate(all_r) if all_r else None, np.concatenate(heavy_r) if heavy_r else None,
            [t[2] for t in per_frame], [t[3] for t in per_frame], [t[4] for t in per_frame], [t[5] for t in per_frame])


def assemble_reconstruction(per_frame: List[tuple]):
    """``(all_valid_ratio, heavy_valid_ratio, all_ged, heavy_ged)`` of ``get_all_true_reconstructed_structures``
    (utils.py:249-266) from the per-frame 6-tuples of its one-sample evaluations."""
    with np.errstate(invalid="ignore"), _quiet_empty_mean():
        return (np.array([t[3] for t in per_frame]).mean(), np.array([t[2] for t in per_frame]).mean(),
                np.array([t[5] for t in per_frame]).mean(), np.array([t[4] for t in per_frame]).mean())


class _quiet_empty_mean:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._w.__exit__(*exc)


# ----------------------------------------------------------------------------- device plumbing
def settle(model):
    """A deferred parameter update of the trainer may still run on its side stream (``CGequiVAE.before_decoder``): wait
    for it before the decoder's weights are read outside ``model.forward``."""
    hook = getattr(model, "before_decoder", None)
    if hook is not None:
        hook()
        model.before_decoder = None


def _mirrored(frame: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The frame reflected through the x-z plane (sampling.py:257-261) as a NEW dict: the caller's tensors stay."""
    out = dict(frame)
    out.pop("_graph", None)                                # its records belong to the unmirrored coordinates
    for key in ("nxyz", "CG_nxyz"):
        t = frame[key].clone()
        t[:, 2] *= -1                                       # column 0 is the type id: y is column 2
        out[key] = t
    return out


def model_device(model) -> torch.device:
    return next(model.parameters()).device


def ensemble_batch(frames: Sequence[Dict[str, torch.Tensor]], n_samples: int, device="cuda") -> Dict[str, object]:
    """The bead-level batch of ``n_samples`` copies of every frame as one disjoint union, frame-major and sample-major
    inside a frame (copy k of frame f holds beads ``K * b_f + k * nb_f ..``, atoms ``K * a_f + k * n_f ..``): built from
    the frames' own bead lists by offsets only -- no second radius search.  ``frames`` are per-frame dicts (host) with
    frame-local ``CG_nbr_list`` / ``CG_mapping``.  Returns the decoder's inputs (``CG_nxyz``, ``CG_nbr_list``,
    ``CG_mapping``, ``num_CGs``, ``num_atoms``, ``_graph``) and ``src_bead``: for every replicated bead the row of the
    collated (unreplicated) batch it copies."""
    K = int(n_samples)
    if K < 1 or not len(frames):
        raise ValueError("ensemble_batch needs at least one frame and one sample")
    cg_rows, nbrs, maps, src, nb_all, na_all = [], [], [], [], [], []
    b0 = a0 = 0
    for fr in frames:
        nb, na = int(fr["CG_nxyz"].shape[0]), int(fr["nxyz"].shape[0])
        ks = np.arange(K, dtype=np.int64)
        bead0 = K * b0 + ks * nb                            # first bead of copy k
        cg_rows.append(fr["CG_nxyz"].detach().cpu().float().repeat(K, 1))
        nbr = fr["CG_nbr_list"].detach().cpu().numpy().astype(np.int64).reshape(-1, 2)
        nbrs.append((nbr[None, :, :] + bead0[:, None, None]).reshape(-1, 2))
        mp = fr["CG_mapping"].detach().cpu().numpy().astype(np.int64).reshape(-1)
        maps.append((mp[None, :] + bead0[:, None]).reshape(-1))
        src.append(np.tile(b0 + np.arange(nb, dtype=np.int64), K))
        nb_all += [nb] * K
        na_all += [na] * K
        b0, a0 = b0 + nb, a0 + na
    dev = torch.device(device)
    cg_nxyz = torch.cat(cg_rows).to(dev)
    cg_nbr = torch.from_numpy(np.concatenate(nbrs)).to(dev)
    mapping = torch.from_numpy(np.concatenate(maps)).to(dev)
    n_atoms = K * a0
    # the decoder reads the bead plan, the atom -> bead plan and the bead ranks: the atom graph of the bundle stays empty
    graph = BatchGraph(torch.zeros(n_atoms, 3, device=dev), cg_nxyz[:, 1:], mapping,
                       torch.zeros(0, 2, dtype=torch.int64, device=dev), cg_nbr)
    return {"CG_nxyz": cg_nxyz, "CG_nbr_list": cg_nbr, "CG_mapping": mapping, "num_CGs": torch.tensor(nb_all).to(dev),
            "num_atoms": torch.tensor(na_all).to(dev), "_graph": graph, "src_bead": torch.from_numpy(np.concatenate(src)).to(dev),
            "n_samples": K}


def _as_frames(source) -> List[Dict[str, torch.Tensor]]:
    frames = []
    for item in (source[i] for i in range(len(source))) if hasattr(source, "__getitem__") and hasattr(source, "__len__") else source:
        if int(item["num_atoms"].numel()) != 1:
            raise ValueError("sample_ensemble takes per-frame dicts (a CGDataset, or a loader with batch_size=1 as the "
                             "reference's sampler, sampling.py:335-338); it collates frames_per_launch of them itself")
        frames.append({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in item.items() if k != "_graph"})
    return frames


def sample_ensemble(dataset_or_loader, model, n_sample: int, reflection: bool = False, graph_eval: bool = True,
                    frames_per_launch: int = 8, eps: Optional[torch.Tensor] = None, scale: float = 1.3,
                    radii: Optional[Dict[int, float]] = None):
    """The reference's ``sample_ensemble`` (sampling.py:335-399): for every frame ``n_sample`` structures decoded from
    latents drawn from the prior of its bead graph.  Returns its 10-tuple ``(sample_xyzs [T, n_sample * n, 3],
    data_xyzs [T,n,3], cg_xyzs [T,n_cg,3], recon_xyzs [T,n,3], all_rmsds, all_heavy_rmsds, sample_valid,
    sample_allatom_valid, sample_graph_val_ratio_list, sample_graph_allatom_val_ratio_list)``; the last six are ``None``
    without ``graph_eval``.  (Frames of different sizes: the four coordinate entries are lists of per-frame arrays.)

    Per chunk of ``frames_per_launch`` frames: one ``model.prior_net`` call, the latents of all ``frames x n_sample``
    copies drawn by the device generator (``ops.reparam_sample``) -- or ``mu + eps * sigma`` with the rows of ``eps``
    ``[n_sample * total beads, F]`` in output order (frame, sample, bead) for parity runs --, one ``model.decoder`` call on
    the replicated bead graph, one metric launch, ``model(batch)`` once for ``recon_xyzs``, one host read-back.
    ``reflection``: y of atom and bead coordinates is mirrored first; the caller's frames are not modified."""
    from . import ops
    K = int(n_sample)
    frames = _as_frames(dataset_or_loader)
    if reflection:
        frames = [_mirrored(f) for f in frames]
    dev = model_device(model)
    sample_l, data_l, cg_l, recon_l, per_frame = [], [], [], [], []
    eps_at = 0
    with torch.no_grad():
        settle(model)
        for start in range(0, len(frames), max(int(frames_per_launch), 1)):
            chunk = frames[start:start + max(int(frames_per_launch), 1)]
            sizes = [int(f["nxyz"].shape[0]) for f in chunk]
            beads = [int(f["CG_nxyz"].shape[0]) for f in chunk]
            z_host = np.concatenate([f["nxyz"][:, 0].numpy() for f in chunk])
            batch = prepare_batch(CG_collate(chunk), dev)
            graph = batch["_graph"]
            rep = ensemble_batch(chunk, K, dev)
            _z, cg_z, _xyz, cg_xyz, _nbrs, cg_nbrs, _mapping, _n = model.get_inputs(batch)
            mu, sigma = model.prior_net(cg_z, graph.cg_xyz, cg_nbrs, graph=graph)
            mu_r, sigma_r = mu[rep["src_bead"]], sigma[rep["src_bead"]]
            if eps is not None:
                e = eps[eps_at:eps_at + mu_r.shape[0]].to(dev)
                eps_at += mu_r.shape[0]
                H = e.mul(sigma_r).add_(mu_r)               # sample_normal, sampling.py:247-250
            else:
                H = ops.reparam_sample(mu_r.contiguous(), sigma_r.contiguous())
            g_rep = rep["_graph"]
            gen = model.decoder(g_rep.cg_xyz, rep["CG_nbr_list"], H, H, rep["CG_mapping"], rep["num_CGs"], graph=g_rep)
            out = [gen, graph.xyz, graph.cg_xyz]
            if graph_eval:
                plan = QualityPlan(z_host, np.concatenate([[0], np.cumsum(sizes)]), dev, scale, radii)
                raw = sample_quality(graph.xyz, gen, n_samples=K, plan=plan)
                out += [raw.counts, raw.sums]
            recon = model(batch)[5]
            out.append(recon)
            host = read_back(out)
            a0 = b0 = 0
            for f, (n, nb) in enumerate(zip(sizes, beads)):
                sample_l.append(host[0][K * a0:K * (a0 + n)])
                data_l.append(host[1][a0:a0 + n])
                cg_l.append(host[2][b0:b0 + nb])
                recon_l.append(host[-1][a0:a0 + n])
                if graph_eval:
                    per_frame.append(assemble_sample_qualities(host[3][f], host[4][f], n, int(plan.n_heavy[f])))
                a0, b0 = a0 + n, b0 + nb
    head = (sample_l, data_l, cg_l, recon_l)
    if data_l and len({a.shape for a in data_l}) == 1 and len({a.shape for a in cg_l}) == 1:
        head = tuple(np.stack(xs) for xs in head)           # one molecule: the reference's [T, ., 3] arrays
    if not graph_eval:
        return head + (None,) * 6
    return head + assemble_ensemble(per_frame)


def eval_sample_qualities(ref_xyz, gen_xyzs, z, scale: float = 1.3, radii: Optional[Dict[int, float]] = None, device="cuda",
                          thresholds=None):
    """The reference's ``eval_sample_qualities(ref_atoms, atoms_list, scale)`` (sampling.py:324-333) for one frame:
    ``ref_xyz [n,3]``, ``gen_xyzs [K,n,3]`` (or a list of K ``[n,3]`` arrays), ``z [n]`` atomic numbers.  One launch, one
    read-back; returns exactly its 6-tuple (see ``assemble_sample_qualities``)."""
    ref = torch.as_tensor(np.asarray(ref_xyz.detach().cpu() if torch.is_tensor(ref_xyz) else ref_xyz), dtype=torch.float32)
    if not torch.is_tensor(gen_xyzs):
        gen_xyzs = np.stack([np.asarray(g.detach().cpu() if torch.is_tensor(g) else g) for g in gen_xyzs])
    gen = torch.as_tensor(np.asarray(gen_xyzs.detach().cpu()) if torch.is_tensor(gen_xyzs) else gen_xyzs, dtype=torch.float32)
    n, K = int(ref.shape[0]), int(gen.shape[0])
    plan = QualityPlan(z, [0, n], device, scale, radii, thresholds)
    raw = sample_quality(ref.to(device), gen.reshape(K * n, 3).to(device), n_samples=K, plan=plan)
    counts, sums = read_back([raw.counts, raw.sums])
    return assemble_sample_qualities(counts[0], sums[0], n, int(plan.n_heavy[0]))


def reconstruction_quality(batches: Iterable[Dict[str, torch.Tensor]], model, reflection: bool = False, scale: float = 1.3,
                           radii: Optional[Dict[int, float]] = None):
    """``get_all_true_reconstructed_structures`` (utils.py:193-268) over collated batches (prepared or not):
    ``(true_xyzs [N,3], recon_xyzs [N,3], cg_xyzs [N_cg,3], all_valid_ratio, heavy_valid_ratio, all_ged, heavy_ged)``,
    the four statistics being means over frames of the one-sample evaluation ``reconstruction vs frame``.  The metric is
    the same kernel with ``n_samples = 1``; per batch one forward, one metric launch, one read-back.  Like the reference
    it evaluates in ``model.eval()``; the mode found is restored.  ``reflection`` mirrors y first, on copies."""
    dev = model_device(model)
    was_training = model.training
    model.eval()
    true_l, recon_l, cg_l, per_frame = [], [], [], []
    try:
        with torch.no_grad():
            settle(model)
            for batch in batches:
                if reflection:
                    batch = _mirrored(batch)
                z_host, sizes = read_back([batch["nxyz"][:, 0], batch["num_atoms"]]) if batch["nxyz"].is_cuda else \
                    (batch["nxyz"][:, 0].numpy(), batch["num_atoms"].numpy())
                if "_graph" not in batch:
                    batch = prepare_batch(dict(batch), dev)
                graph = batch["_graph"]
                recon = model(batch)[5]
                plan = QualityPlan(z_host, np.concatenate([[0], np.cumsum(_host_ints(sizes))]), dev, scale, radii)
                raw = sample_quality(graph.xyz, recon, n_samples=1, plan=plan)
                xyz_h, recon_h, cg_h, counts, sums = read_back([graph.xyz, recon, graph.cg_xyz, raw.counts, raw.sums])
                true_l.append(xyz_h), recon_l.append(recon_h), cg_l.append(cg_h)
                for f in range(plan.n_frames):
                    per_frame.append(assemble_sample_qualities(counts[f], sums[f], int(plan.sizes[f]), int(plan.n_heavy[f])))
    finally:
        model.train(was_training)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros((0, 3), np.float32)
    return (cat(true_l), cat(recon_l), cat(cg_l)) + assemble_reconstruction(per_frame)
