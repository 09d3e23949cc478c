#!/usr/bin/env python3
"""Generate the sample-quality goldens ``g12_sample_quality_*.npz`` FROM THE REFERENCE ITSELF.

Runs only where the reference checkout is present (see make_golden.py).  It imports the reference's own
``scripts/sampling.py`` and ``scripts/utils.py`` unmodified and records, per case, the inputs (atomic numbers, one
reference frame, K generated frames, the scale, the radii the reference looked up for the elements present) and what
the reference computes from them: the bond-matrix difference counts, signed sums and reference sums of
``get_bond_graphs`` per sample for the all-atom and the heavy-atom graph, the 6-tuple of ``eval_sample_qualities``
(``None`` stored as an empty array + flag) and the four statistics of ``get_all_true_reconstructed_structures`` when
every sample is handed to it as a one-sample reconstruction.

Absent third-party modules the two scripts import are registered as stubs: ``ase`` (an ``Atoms`` container with
``get_positions`` / ``get_atomic_numbers`` / ``__len__``, positions kept as float64 as ase does), ``mdshare``,
``pyemma``, ``torch_scatter``, ``networkx``, ``sklearn`` -- none of them computes anything on this path.

Usage:  python tests/golden/make_golden_eval.py          (rewrites tests/golden/g12_*)
"""
import importlib
import json
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
K_SAMPLES = 16


# ------------------------------------------------------------------ stubs + import
class Atoms:
    def __init__(self, numbers=None, positions=None):
        self.numbers = np.asarray(numbers).astype(np.int64).ravel()
        self.positions = np.array(positions, dtype=np.float64)

    def get_positions(self):
        return self.positions.copy()

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def __len__(self):
        return len(self.numbers)


def load_reference_scripts():
    for name in ("ase", "mdshare", "pyemma", "torch_scatter", "networkx", "sklearn", "sklearn.utils"):
        try:
            importlib.import_module(name)
        except Exception:                                 # noqa: BLE001  (absent: a stub will do, nothing is called)
            sys.modules[name] = types.ModuleType(name)
    ase = sys.modules["ase"]
    if not hasattr(ase, "Atoms") or ase.__dict__.get("__file__") is None:
        ase.Atoms, ase.io = Atoms, types.ModuleType("ase.io")
    sys.modules["torch_scatter"].__dict__.setdefault("scatter_mean", None)
    sys.modules["sklearn.utils"].__dict__.setdefault("shuffle", None)
    scripts = os.path.join(REF, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import warnings
    warnings.filterwarnings("ignore")
    keep = os.environ.get("CUDA_LAUNCH_BLOCKING")
    sampling = importlib.import_module("sampling")
    utils = importlib.import_module("utils")
    if keep is None:
        os.environ.pop("CUDA_LAUNCH_BLOCKING", None)       # utils.py:13 sets it at import: not this process's business
    return sampling, utils


# ------------------------------------------------------------------ molecules
def zigzag(with_h=True):
    """10 heavy atoms C N C C O C N C C O, consecutive ones (1.25, +-0.83, 0) A apart, one H per heavy atom 1.05 A
    along +-z (interleaved: heavy, its H, heavy, ...)."""
    zs, pos = [], []
    for i, el in enumerate([6, 7, 6, 6, 8, 6, 7, 6, 6, 8]):
        p = np.array([1.25 * i, 0.83 * (i % 2), 0.0])
        zs.append(el), pos.append(p)
        if with_h:
            zs.append(1), pos.append(p + np.array([0.0, 0.0, 1.05 if i % 2 == 0 else -1.05]))
    return np.array(zs, dtype=np.int64), np.array(pos, dtype=np.float32)


def noisy(ref, sigma, k=K_SAMPLES, seed=0):
    rng = np.random.default_rng(seed)
    return (ref[None].astype(np.float64) + sigma * rng.standard_normal((k,) + ref.shape)).astype(np.float32)


def ulp_step(x, k):
    a = np.float32(x)
    for _ in range(abs(k)):
        a = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf))
    return np.float32(a)


def strict_threshold(c):
    """Largest fp32 s with torch.sqrt(s) < c, by brute force over bit patterns around c*c."""
    c = np.float32(c)
    bits = int(np.array(c * c, dtype=np.float32).view(np.uint32))
    pat = np.arange(bits - 200, bits + 201, dtype=np.uint32).view(np.float32).copy()
    ok = (torch.sqrt(torch.from_numpy(pat)) < torch.tensor(c)).numpy()
    k = int(np.nonzero(ok)[0].max())
    assert ok[: k + 1].all() and not ok[k + 1:].any() and 0 < k < len(pat) - 1
    return np.float32(pat[k])


def squared_sum(a, b):
    """The reference's own arithmetic (sampling.py:128-133) without the sqrt."""
    xyz = torch.Tensor(np.array([a, b], dtype=np.float64))
    return np.float32((xyz[:, None, :] - xyz[None, :, :]).pow(2).sum(-1)[0, 1].item())


def pair_at(target):
    """(x, y) such that atoms (0,0,0) and (x,y,0) have the fp32 squared sum ``target`` exactly."""
    root = np.float32(np.sqrt(np.float64(target)))
    for kx in range(0, 4000):
        x = ulp_step(root, -kx)
        rest = np.float64(target) - np.float64(np.float32(x * x))
        if rest < 0:
            continue
        y0 = np.float32(np.sqrt(rest))
        for ky in range(-3, 4):
            y = ulp_step(y0, ky) if y0 > 0 else np.float32(0)
            if squared_sum([0, 0, 0], [x, y, 0]) == np.float32(target):
                return float(x), float(y)
    raise RuntimeError(f"no pair found for squared sum {target!r}")


def ulp_case(sampling):
    """Pairs of classes (a, b) whose squared sum sits at the strict class-pair threshold + k ulp, k in -2..2: bonded
    iff k <= 0.  The reference frame holds the k-pattern, the three samples hold it shifted, so every side of the
    strict ``<`` is crossed in both directions."""
    pairs = [(1, 1), (1, 6), (6, 6), (6, 8), (7, 16), (8, 1), (16, 16), (9, 17)]
    steps = (-2, -1, 0, 1, 2)
    zs, frames = [], [[] for _ in range(4)]
    slot = 0
    for a, b in pairs:
        cutoff = sampling.compute_bond_cutoff(Atoms(numbers=[a, b], positions=np.zeros((2, 3))), scale=1.3)[0, 1].item()
        s_star = strict_threshold(cutoff)
        xy = {k: pair_at(ulp_step(s_star, k)) for k in steps}
        for idx, k in enumerate(steps):
            zs += [a, b]
            base = np.array([0.0, 0.0, 25.0 * slot])
            slot += 1
            for fi in range(4):                           # frame 0 = reference, 1..3 = samples
                kk = steps[(idx + fi) % len(steps)] if fi else k
                x, y = xy[kk]
                frames[fi] += [base, base + np.array([x, y, 0.0])]
            # the reference itself says: bonded iff k <= 0
            at = Atoms(numbers=[a, b], positions=np.array([[0, 0, 0], [xy[k][0], xy[k][1], 0]], dtype=np.float32))
            assert int(sampling.get_bond_graphs(at, scale=1.3)[0, 1]) == (1 if k <= 0 else 0), (a, b, k)
    f = np.array(frames, dtype=np.float32)
    return np.array(zs, dtype=np.int64), f[0], f[1:]


# ------------------------------------------------------------------ the reference's outputs
class _Replay:
    """Stands in for the model in get_all_true_reconstructed_structures: hands back the recorded frames."""

    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, batch):
        return None, None, None, None, batch["nxyz"][:, 1:], batch["recon"]


def record(sampling, utils, z, ref, gen, scale=1.3):
    K, n = gen.shape[0], ref.shape[0]
    ref_atoms = Atoms(numbers=z, positions=ref)
    atoms_list = [Atoms(numbers=z, positions=g) for g in gen]
    out = {"z": z, "ref": ref, "gen": gen, "scale": np.float64(scale)}
    elements = sorted(set(z.tolist()))
    out["radii.z"] = np.array(elements, dtype=np.int64)
    out["radii.r"] = np.array([sampling.COVCUTOFFTABLE[e] for e in elements], dtype=np.float64)
    # the strict squared-distance threshold per class pair WITH THIS HOST'S torch.sqrt: the reference's `sqrt(s) < cutoff`
    # is host dependent (two hosts with the same torch build round sqrt(3.1258237) differently), so the recorded bond
    # matrices belong to these thresholds
    cut = sampling.compute_bond_cutoff(Atoms(numbers=elements, positions=np.zeros((len(elements), 3))), scale=scale)
    out["thr.sq"] = np.array([[strict_threshold(c) for c in row] for row in cut.tolist()], dtype=np.float32)
    for tag, drop in (("all", False), ("heavy", True)):
        r_at = sampling.dropH(ref_atoms) if drop else ref_atoms
        diff, signed, refsum = [], [], []
        for at in atoms_list:
            at = sampling.dropH(at) if drop else at
            diff.append(sampling.compare_graph(r_at, at, scale=scale))
            g_ref, g_gen = sampling.get_bond_graphs(r_at, scale=scale), sampling.get_bond_graphs(at, scale=scale)
            signed.append(int((g_ref - g_gen).sum())), refsum.append(int(g_ref.sum()))
        out[f"diff.{tag}"], out[f"signed.{tag}"], out[f"refsum.{tag}"] = (np.array(v, dtype=np.int64) for v in (diff, signed, refsum))
    six = sampling.eval_sample_qualities(ref_atoms, atoms_list, scale=scale)
    for name, val in zip(("all_rmsds", "heavy_rmsds"), six[:2]):
        out[f"six.{name}"] = np.zeros((0, 2)) if val is None else np.asarray(val, dtype=np.float64)
        out[f"six.{name}.none"] = np.array(val is None)
    out["six.valid_ratio"], out["six.valid_allatom_ratio"] = np.float64(six[2]), np.float64(six[3])
    out["six.graph_val_ratio"] = np.array(six[4], dtype=np.float64)
    out["six.graph_allatom_val_ratio"] = np.array(six[5], dtype=np.float64)
    # reconstruction path: every sample as the one-sample reconstruction of a frame of its own
    nxyz = torch.cat([torch.tensor(z, dtype=torch.float32)[:, None], torch.from_numpy(ref)], dim=1).repeat(K, 1)
    batch = {"nxyz": nxyz, "CG_nxyz": torch.zeros(K, 4), "num_atoms": torch.tensor([n] * K),
             "recon": torch.from_numpy(gen.reshape(K * n, 3))}
    seven = utils.get_all_true_reconstructed_structures([batch], "cpu", _Replay(), tqdm_flag=False)
    assert np.array_equal(seven[1], gen.reshape(K * n, 3))
    out["recon.stats"] = np.array([seven[3], seven[4], seven[5], seven[6]], dtype=np.float64)
    return out


def build_cases():
    sampling, utils = load_reference_scripts()
    cases = {}
    z, ref = zigzag()
    g0 = sampling.get_bond_graphs(Atoms(numbers=z, positions=ref))
    assert int(g0.sum()) == 38 and int(sampling.get_bond_graphs(sampling.dropH(Atoms(numbers=z, positions=ref))).sum()) == 18
    for name, sigma in (("valid", 0.02), ("mixed_all", 0.06), ("mixed_heavy", 0.12), ("all_none", 0.20), ("both_none", 0.40)):
        cases[name] = record(sampling, utils, z, ref, noisy(ref, sigma))
        cases[name]["sigma"] = np.float64(sigma)
    c = cases
    assert c["valid"]["six.valid_ratio"] == 1.0 and c["valid"]["six.valid_allatom_ratio"] == 1.0
    # a "mixed" case exercises the selection logic only when the graph it is about is valid for a real fraction of samples
    assert 0.25 <= c["mixed_all"]["six.valid_allatom_ratio"] <= 0.75, c["mixed_all"]["six.valid_allatom_ratio"]
    assert 0.25 <= c["mixed_heavy"]["six.valid_ratio"] <= 0.75, c["mixed_heavy"]["six.valid_ratio"]
    assert bool(c["all_none"]["six.all_rmsds.none"]) and not bool(c["all_none"]["six.heavy_rmsds.none"])
    assert bool(c["both_none"]["six.all_rmsds.none"]) and bool(c["both_none"]["six.heavy_rmsds.none"])
    zh, refh = zigzag(with_h=False)
    cases["no_hydrogen"] = record(sampling, utils, zh, refh, noisy(refh, 0.12, k=8, seed=1))
    assert 0.25 <= cases["no_hydrogen"]["six.valid_ratio"] <= 0.75
    # no bond at all: atoms 5 A apart, reference sums are zero -> the ratios are 0 / 0 = nan
    zn = np.array([6, 1, 8, 1, 7, 6], dtype=np.int64)
    refn = (np.arange(6)[:, None] * np.array([5.0, 0.3, -0.2])[None, :]).astype(np.float32)
    cases["no_bond"] = record(sampling, utils, zn, refn, noisy(refn, 0.05, k=3, seed=2))
    assert np.isnan(cases["no_bond"]["six.graph_val_ratio"]).all() and int(cases["no_bond"]["refsum.all"].sum()) == 0
    zu, refu, genu = ulp_case(sampling)
    cases["ulp"] = record(sampling, utils, zu, refu, genu)
    assert int(cases["ulp"]["diff.all"].min()) > 0 and int(cases["ulp"]["diff.heavy"].min()) > 0
    return cases


def cv_stats_columns():
    """Keys of the ``test_stats`` dict the reference writes as cv_stats.csv (scripts/run_ala.py:387-399), in order."""
    lines = open(os.path.join(REF, "scripts", "run_ala.py")).read().splitlines()[386:399]
    return re.findall(r"'([A-Za-z_]+)'\s*:", "\n".join(lines))


def main():
    for name, arrays in build_cases().items():
        path = os.path.join(HERE, f"g12_sample_quality_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)  heavy valid {float(arrays['six.valid_ratio']):.4f}  "
              f"all-atom valid {float(arrays['six.valid_allatom_ratio']):.4f}")
    with open(os.path.join(HERE, "g12_cv_stats_columns.json"), "w") as f:
        json.dump(cv_stats_columns(), f)


if __name__ == "__main__":
    main()
