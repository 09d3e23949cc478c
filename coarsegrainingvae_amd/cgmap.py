"""The atom -> bead assignment of a ``-traj`` run, made on the device.

``-cg_method cgae`` learns it from the trajectory.  Reference: ``learn_map`` (CoarseGrainingVAE/datasets.py:190-249) on the
auto-encoder of CoarseGrainingVAE/cgae.py, called from ``get_cg_and_xyz`` (datasets.py:303-312) and retried by
scripts/run_ala.py:168-173 until every bead is used.  The optimiser loop -- tens of thousands of steps on two
``n_atoms x n_cgs`` matrices -- runs inside ``cgv_cgae_steps`` (csrc/cgae.hip): the host uploads the centred training frames
and the frame order of the whole schedule once, launches, and reads the loss log at the end.

``-cg_method newman`` is the Girvan-Newman partition of the bond graph (datasets.py:277-297, 363-385): edge betweenness by
Brandes' algorithm, remove the highest edge, relabel the components -- three launches per removal (csrc/newman.hip),
enqueued in batches, one 4-byte read of the component counter per batch.  ``backbonepartition``, ``seqpartition`` and
``random`` (datasets.py:73-105, 314-328, 412-420) are seeded host / tensor code: none of them is a hot path.

There is no tensor-op path for the kernels: a missing kernel is an error."""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from . import _lib
from .steploop import check_order, check_steps, chunks, forced_form, steps_per_epoch

RESIDENT, STREAMED = 1, 2                 # include/cgvae_hip.h: CGV_CGAE_RESIDENT / CGV_CGAE_STREAMED
FORM_NAMES = {RESIDENT: "resident", STREAMED: "streamed"}
MAX_ATTEMPTS = 5
CHUNK_STEPS = 8192                        # steps per call of the entry point (bounds one launch of the resident form)


def train_subset(n_frames: int, seed: int) -> torch.Tensor:
    """A seeded random 90 % of ``range(n_frames)``, in drawn order (datasets.py:197: train_test_split(test_size=0.1), which
    holds out ceil(0.1 T) frames; the held-out frames stay unused, as in the reference)."""
    perm = torch.randperm(n_frames, generator=torch.Generator().manual_seed(int(seed)))
    return perm[: n_frames - math.ceil(0.1 * n_frames)]


def initial_parameters(n_atoms: int, n_cgs: int, seed: int):
    """cgae.__init__ (cgae.py:13-14): assign_map first, then decode, from one CPU generator."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randn(n_atoms, n_cgs, generator=gen), torch.randn(n_cgs, n_atoms, generator=gen)


def frame_order(n_train: int, batch_size: int, n_epochs: int, seed: int) -> np.ndarray:
    """int32 [n_epochs, n_train]: one permutation of the training subset's positions per epoch (DataLoader(shuffle=True)).
    Step s takes ``batch_size`` consecutive entries of its epoch's row; the last batch of a row is the partial one."""
    rng = np.random.default_rng([int(seed), 1])
    return rng.permuted(np.tile(np.arange(n_train, dtype=np.int32), (n_epochs, 1)), axis=1)


def choose_form(n_atoms: int, n_cgs: int, batch_size: int) -> int:
    """The one rule: everything in one workgroup's LDS when n_atoms * n_cgs (and the batch's bead coordinates) fit it
    (cgv_cgae_resident_fits), the multi-block form otherwise.  options ``cgae_form`` = 1 / 2 forces a form."""
    return forced_form("cgae_form", lambda: RESIDENT if _lib.load().cgv_cgae_resident_fits(n_atoms, n_cgs, batch_size) else STREAMED)


class Learner:
    """Device state of one learning run: parameters, Adam moments, frames, order table, loss log, workspace."""

    def __init__(self, frames, W, D, order, batch_size, reg_weight, lr=4e-3, seed=0, device="cuda", form=None):
        dev = torch.device(device)
        frames = torch.as_tensor(frames, dtype=torch.float32)
        self.n_frames, self.n, _ = frames.shape
        self.K = int(W.shape[1])
        assert tuple(W.shape) == (self.n, self.K) and tuple(D.shape) == (self.K, self.n)
        order = check_order(np.ascontiguousarray(order, dtype=np.int32), self.n_frames)
        self.n_train, self.batch = int(order.shape[1]), int(batch_size)
        self.total_steps = int(order.shape[0]) * steps_per_epoch(self.n_train, self.batch)
        self.form = choose_form(self.n, self.K, self.batch) if form is None else int(form)
        frames = frames - frames.mean(1, keepdim=True)                    # datasets.py:222-223, once
        self.frames = frames.contiguous().to(dev)
        self.order = torch.from_numpy(order.reshape(-1)).to(dev)
        self.W, self.D = W.detach().float().contiguous().to(dev), D.detach().float().contiguous().to(dev)
        self.moments = [torch.zeros_like(t) for t in (self.W, self.W, self.D, self.D)]      # mW, vW, mD, vD
        self.loss_log = torch.zeros(self.total_steps, 2, device=dev)
        nbytes = int(_lib.load().cgv_cgae_workspace_bytes(self.n, self.K, self.batch, self.form))
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.reg_weight, self.lr, self.seed, self.done = float(reg_weight), float(lr), int(seed), 0

    def run(self, steps=None, noise=None, probe=False):
        """``steps`` more optimiser steps (default: the rest of the schedule).  ``noise`` [steps, n, K]: explicit Gumbel noise
        instead of the generator's.  ``probe``: returns M, dW, dD, cg_xyz of the last step."""
        steps = self.total_steps - self.done if steps is None else int(steps)
        check_steps(self.done, steps, self.order.numel() // self.n_train, self.n_train, self.batch)
        if noise is not None:
            noise = noise.to(self.W.device, torch.float32).contiguous()
            assert tuple(noise.shape) == (steps, self.n, self.K)
        nk = self.n * self.K
        out = torch.zeros(3 * nk + self.batch * self.K * 3, device=self.W.device) if probe else None
        with torch.cuda.device(self.W.device):
            for start, cnt in chunks(steps, CHUNK_STEPS):
                _lib.call("cgv_cgae_steps", self.form, _lib.ptr(self.W), _lib.ptr(self.D), *(_lib.ptr(m) for m in self.moments),
                          _lib.ptr(self.frames), self.n_frames, _lib.ptr(self.order), self.order.numel(), self.n_train,
                          self.batch, self.n, self.K, self.done, cnt, self.reg_weight, self.lr, 0.9, 0.999, 1e-8, self.seed,
                          _lib.ptr(noise[start:]) if noise is not None else None, _lib.ptr(self.loss_log[self.done:]),
                          _lib.ptr(out) if probe and start + cnt == steps else None,
                          _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
                self.done += cnt
        if not probe:
            return None
        cnt = min(self.batch, self.n_train - ((self.done - 1) % steps_per_epoch(self.n_train, self.batch)) * self.batch)
        return {"M": out[:nk].view(self.n, self.K), "dW": out[nk:2 * nk].view(self.n, self.K),
                "dD": out[2 * nk:3 * nk].view(self.K, self.n), "cg_xyz": out[3 * nk:].view(self.batch, self.K, 3)[:cnt]}


def kernel_noise(seed: int, step0: int, steps: int, n_atoms: int, n_cgs: int, device="cuda") -> torch.Tensor:
    """The Gumbel noise [steps, n, K] the kernels draw for steps ``step0 ..`` under ``seed`` (cgv_cgae_noise)."""
    out = torch.empty(steps, n_atoms, n_cgs, device=device)
    with torch.cuda.device(out.device):
        _lib.call("cgv_cgae_noise", int(seed), int(step0), int(steps), int(n_atoms), int(n_cgs), _lib.ptr(out), _lib.stream_ptr())
    return out


def learn_once(xyz, n_cgs, reg_weight=0.25, n_data=1000, n_epochs=1500, lr=4e-3, batch_size=32, seed=123, device="cuda"):
    """One run of the reference's learn_map.  Returns (mapping LongTensor[n], info, (W, D) on the host)."""
    xyz = torch.as_tensor(np.asarray(xyz), dtype=torch.float32)
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError("xyz must be [T, n_atoms, 3]")
    xyz = xyz[: min(int(n_data), xyz.shape[0])]
    train = train_subset(xyz.shape[0], seed)
    if len(train) == 0:
        raise ValueError("no training frames")
    W, D = initial_parameters(xyz.shape[1], int(n_cgs), seed)
    order = frame_order(len(train), batch_size, n_epochs, seed)
    t0 = time.time()
    learner = Learner(xyz[train], W, D, order, batch_size, reg_weight, lr=lr, seed=seed, device=device)
    learner.run()
    final = learner.loss_log[-1].cpu() if learner.total_steps else torch.full((2,), float("nan"))   # the one read of the log (synchronises)
    W, D = learner.W.cpu(), learner.D.cpu()
    info = {"method": "cgae", "steps": learner.total_steps, "seconds": time.time() - t0, "loss_recon": float(final[0]),
            "loss_reg": float(final[1]), "attempts": 1, "form": FORM_NAMES[learner.form], "seed": int(seed)}
    return W.argmax(-1), info, (W, D)


def learn_map(xyz, n_cgs, reg_weight=0.25, n_data=1000, n_epochs=1500, lr=4e-3, batch_size=32, seed=123, device="cuda"):
    """``learn_map`` with the caller's retry rule (scripts/run_ala.py:168-173): while fewer than ``n_cgs`` distinct beads
    come out, learn again with ``seed + attempt``.  The reference loops forever; here the fifth failure raises.

    Frames: the first ``min(n_data, T)``, a seeded random 90 % of them.  Returns (mapping LongTensor[n], info) with info =
    {method, steps, seconds, loss_recon, loss_reg (last step), attempts, form ("resident" / "streamed"), seed}."""
    seconds = 0.0
    for attempt in range(MAX_ATTEMPTS):
        mapping, info, _ = learn_once(xyz, n_cgs, reg_weight=reg_weight, n_data=n_data, n_epochs=n_epochs, lr=lr,
                                      batch_size=batch_size, seed=seed + attempt, device=device)
        seconds += info["seconds"]
        if len(set(mapping.tolist())) == n_cgs:
            return mapping.long(), {**info, "attempts": attempt + 1, "seconds": seconds}
    raise RuntimeError(f"cgae mapping: {MAX_ATTEMPTS} attempts (seeds {seed}..{seed + MAX_ATTEMPTS - 1}) on {len(mapping)} atoms "
                       f"never used all n_cgs = {n_cgs} beads; choose fewer beads or pass a mapping in the trajectory file")


# ------------------------------------------------------------------ graph-partition maps (csrc/newman.hip)
NEWMAN_BATCH = 64                         # removals enqueued between two reads of the component counter, at most


def bond_csr(bonds, n_atoms: int):
    """The bond list as the kernels take it: ``edges`` int32 [m,2] with u < v, every bond once, in ascending (u, v) order
    (so edge ids follow networkx's ``G.edges()`` order for nodes added 0..n-1), and the CSR over atoms ``rowptr`` [n+1],
    ``col`` [2m], ``edge_id`` [2m] with every row's slots in ascending neighbour order."""
    n_atoms = int(n_atoms)
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    if b.size and (b.min() < 0 or b.max() >= n_atoms):
        raise ValueError(f"the bond list names atom {int(b.max() if b.max() >= n_atoms else b.min())}, the molecule has {n_atoms} atoms")
    b = np.sort(b[b[:, 0] != b[:, 1]], axis=1)
    edges = np.unique(b, axis=0).reshape(-1, 2)                       # sorted rows: lexicographic (u, v)
    m = edges.shape[0]
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    eid = np.concatenate([np.arange(m), np.arange(m)])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(n_atoms + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n_atoms), out=rowptr[1:])
    return (edges.astype(np.int32), rowptr.astype(np.int32), dst[order].astype(np.int32), eid[order].astype(np.int32))


def choose_newman_form(n_atoms: int, n_edges: int) -> int:
    """Per-source state in the workgroup's LDS when it fits (cgv_newman_resident_fits), in the workspace otherwise.
    options ``newman_form`` = 1 / 2 forces a form."""
    return forced_form("newman_form", lambda: RESIDENT if _lib.load().cgv_newman_resident_fits(int(n_atoms), int(n_edges)) else STREAMED)


class _NewmanGraph:
    """Device copies of one bond graph, its ``alive`` mask and the kernels' workspace."""

    def __init__(self, bonds, n_atoms, device, groups=0, form=None):
        self.n, self.groups = int(n_atoms), int(groups)
        if self.n < 1:
            raise ValueError("a molecule has at least one atom")
        self.edges, rowptr, col, eid = bond_csr(bonds, self.n)
        self.m = int(self.edges.shape[0])
        self.form = choose_newman_form(self.n, self.m) if form is None else int(form)
        self.dev = torch.device(device)

        def up(a):                                                    # never an empty buffer: the C ABI refuses NULL
            return torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(2, dtype=np.int32))).to(self.dev)
        self.d_edges, self.rowptr, self.col, self.eid = up(self.edges.reshape(-1)), up(rowptr), up(col), up(eid)
        self.alive = torch.ones(max(self.m, 1), dtype=torch.int32, device=self.dev)
        nbytes = int(_lib.load().cgv_newman_workspace_bytes(self.n, self.m, self.form, self.groups))
        if nbytes == 0:
            raise ValueError(f"{self.n} atoms / {self.m} bonds are beyond what the partition kernels hold")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)

    def csr(self):
        return (_lib.ptr(self.rowptr), _lib.ptr(self.col), _lib.ptr(self.eid))

    def ws(self):
        return (_lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())


def edge_betweenness(bonds, n_atoms, alive=None, device="cuda", groups=0, form=None):
    """(edges int32 [m,2], betweenness fp64 [m] on the device) of the bond graph under ``alive`` (default: every edge):
    cgv_newman_betweenness, the sums over all sources (twice networkx's unnormalised values)."""
    g = _NewmanGraph(bonds, n_atoms, device, groups, form)
    if alive is not None:
        g.alive = torch.as_tensor(np.asarray(alive), dtype=torch.int32).to(g.dev).contiguous()
        assert g.alive.numel() == g.m
    bet = torch.zeros(g.m, dtype=torch.float64, device=g.dev)
    with torch.cuda.device(g.dev):
        _lib.call("cgv_newman_betweenness", *g.csr(), _lib.ptr(g.alive), g.n, g.m, g.form, g.groups, _lib.ptr(bet), *g.ws())
    return g.edges, bet


def partition_newman(bonds, n_atoms, n_cgs, device="cuda", groups=0, form=None):
    """Girvan-Newman partition of the bond graph into ``n_cgs`` beads (datasets.py:373-385 + parition2mapping, 363-371).
    Returns (mapping LongTensor[n] on the host, info) with info = {method, removals, launches, seconds, form,
    removed_edges: [[u, v], ...] in removal order}.  Bead k is the component with the k-th smallest lowest atom index.
    A graph that starts in several components is fine as long as there are at most ``n_cgs`` of them."""
    n_atoms, n_cgs = int(n_atoms), int(n_cgs)
    if n_cgs < 1 or n_cgs > n_atoms:
        raise ValueError(f"newman mapping: n_cgs = {n_cgs} beads for {n_atoms} atoms (need 1 <= n_cgs <= n_atoms)")
    t0 = time.time()
    g = _NewmanGraph(bonds, n_atoms, device, groups, form)
    labels = torch.empty(g.n, dtype=torch.int32, device=g.dev)
    state = torch.zeros(2, dtype=torch.int32, device=g.dev)
    log = torch.zeros(max(g.m, 1), dtype=torch.int32, device=g.dev)
    common = (*g.csr(), _lib.ptr(g.d_edges), _lib.ptr(g.alive))
    launches, enqueued = 1, 0
    with torch.cuda.device(g.dev):
        _lib.call("cgv_newman_components", *common, g.n, g.m, g.form, g.groups, _lib.ptr(labels), _lib.ptr(state), *g.ws())
        comps = int(state[0].item())
        if comps > n_cgs:
            raise ValueError(f"newman mapping: the bond graph already has {comps} connected components, more than n_cgs = {n_cgs}")
        while comps < n_cgs and enqueued < g.m:
            # a split takes at least one removal, so the first n_cgs - comps rounds of a batch are never wasted
            batch = min(n_cgs - comps, g.m - enqueued, NEWMAN_BATCH)
            _lib.call("cgv_newman_partition", *common, _lib.ptr(labels), _lib.ptr(state), _lib.ptr(log), g.n, g.m, n_cgs, batch,
                      g.form, g.groups, *g.ws())
            enqueued += batch
            launches += 3 * batch
            comps = int(state[0].item())                              # the one 4-byte read of the batch
        removals = int(state[1].item())
    if comps != n_cgs:
        raise RuntimeError(f"newman mapping: {comps} components after removing all {g.m} edges, wanted {n_cgs}")
    mapping = torch.unique(labels.cpu().long(), sorted=True, return_inverse=True)[1]
    removed = g.edges[log[:removals].cpu().numpy()].tolist()
    info = {"method": "newman", "removals": removals, "launches": launches, "seconds": time.time() - t0,
            "form": FORM_NAMES[g.form], "removed_edges": removed}
    return mapping, info


def _cut_points(n_items: int, n_cgs: int, rng) -> np.ndarray:
    """Segment index of ``n_items`` items in a row cut at ``n_cgs - 1`` distinct points drawn from 1 .. n_items - 1: every
    segment is non-empty (the reference draws from 0 .. n_items - 1 and so may leave bead 0 empty; deliberately not kept)."""
    if n_cgs < 1 or n_cgs > n_items:
        raise ValueError(f"n_cgs = {n_cgs} beads for {n_items} items in sequence")
    marks = np.zeros(n_items, dtype=np.int64)
    marks[rng.choice(np.arange(1, n_items), size=n_cgs - 1, replace=False)] = 1
    return np.cumsum(marks)


def partition_sequence(n_atoms, n_cgs, seed=123) -> np.ndarray:
    """``seqpartition`` (datasets.py:314-319): the atoms in file order cut at seeded random points."""
    return _cut_points(int(n_atoms), int(n_cgs), np.random.default_rng([int(seed), 3]))


def partition_random(n_atoms, n_cgs, seed=123, max_draws=100) -> np.ndarray:
    """``random`` (get_random_mapping, datasets.py:412-420): uniform bead labels, drawn again until every bead is used.  The
    reference draws up to 10^7 times and then returns a map with empty beads; here, after ``max_draws`` failures (n_cgs
    close to n_atoms), n_cgs seeded random atoms take one bead each and the others keep a uniform label."""
    n_atoms, n_cgs = int(n_atoms), int(n_cgs)
    if n_cgs < 1 or n_cgs > n_atoms:
        raise ValueError(f"n_cgs = {n_cgs} beads for {n_atoms} atoms")
    rng = np.random.default_rng([int(seed), 4])
    for _ in range(max_draws):
        mapping = rng.integers(0, n_cgs, size=n_atoms)
        if len(np.unique(mapping)) == n_cgs:
            return mapping.astype(np.int64)
    mapping[rng.permutation(n_atoms)[:n_cgs]] = rng.permutation(n_cgs)
    return mapping.astype(np.int64)


def shuffle_mapping(mapping, share, seed=123) -> np.ndarray:
    """``-mapshuffle`` (datasets.py:289-295): a seeded random ``int(share * n)`` of the atoms exchange their bead labels
    among themselves (a permutation of those labels, so every bead keeps its size)."""
    mapping = np.array(mapping, dtype=np.int64)
    count = int(float(share) * mapping.shape[0])
    if count > 1:
        rng = np.random.default_rng([int(seed), 5])
        idx = rng.choice(mapping.shape[0], size=count, replace=False)
        mapping[idx] = rng.permutation(mapping[idx])
    return mapping


def partition_backbone(xyz, z, bonds, n_cgs, seed, skip=100, device="cuda"):
    """``backbonepartition`` (backbone_partition, datasets.py:73-105).  The backbone atoms (``tica.backbone_atoms``: N, CA, C
    from elements and bonds) in index order are cut into ``n_cgs`` non-empty segments at seeded points; every atom goes to
    the segment whose centroid is nearest on average over ``xyz[::skip]``; a backbone atom stays in its own segment (so no
    bead can come out empty -- the reference guarantees neither).  Tensor ops in fp64 on ``device``.  Returns
    (mapping LongTensor[n] on the host, info)."""
    from . import tica
    t0 = time.time()
    n_cgs = int(n_cgs)
    backbone = tica.backbone_atoms(z, bonds)
    if backbone.shape[0] < max(n_cgs, 1):
        raise ValueError(f"N_cg = {n_cgs} is larger than N_backbone = {backbone.shape[0]}")         # datasets.py:78-79
    segment = _cut_points(backbone.shape[0], n_cgs, np.random.default_rng([int(seed), 2]))
    dev = torch.device(device)
    frames = torch.as_tensor(np.asarray(xyz)[:: max(int(skip), 1)], dtype=torch.float64, device=dev)    # [T', n, 3]
    bb, seg = torch.from_numpy(backbone).to(dev), torch.from_numpy(segment).to(dev)
    sums = torch.zeros(frames.shape[0], n_cgs, 3, dtype=torch.float64, device=dev).index_add_(1, seg, frames[:, bb])
    centroid = sums / torch.bincount(seg, minlength=n_cgs).to(torch.float64)[None, :, None]
    dist = (frames[:, :, None, :] - centroid[:, None, :, :]).pow(2).sum(-1).sqrt().mean(0)            # [n, n_cgs]
    mapping = dist.argmin(-1)
    mapping[bb] = seg
    info = {"method": "backbonepartition", "seconds": time.time() - t0, "n_backbone": int(backbone.shape[0]), "seed": int(seed)}
    return mapping.cpu().long(), info


def select_mapping(cg_method, file_mapping, xyz, n_cgs, reg_weight, device, learner=None, *, z=None, bonds=None,
                   mapshuffle=0.0, seed=123):
    """Which atom -> bead map a ``-traj`` run uses (get_cg_and_xyz, datasets.py:252-342).  Returns (mapping array, info or
    None): the file's mapping when it has one; else by ``-cg_method``: ``cgae`` the learned one, ``newman`` the
    Girvan-Newman partition of ``bonds`` (with ``-mapshuffle``), ``backbonepartition`` / ``seqpartition`` / ``random`` the
    seeded ones; ``minimal`` / ``alpha`` (which need atom names) and every other name: contiguous equal blocks."""
    if file_mapping is not None:
        return np.asarray(file_mapping), None
    if not n_cgs:
        raise SystemExit("the trajectory file has no mapping: pass -n_cgs (learned with -cg_method cgae, else contiguous equal blocks of atoms)")
    n_atoms = np.asarray(xyz).shape[1]
    if cg_method == "cgae":
        mapping, info = (learner or learn_map)(xyz, n_cgs, reg_weight=reg_weight, device=device)
        return np.asarray(mapping), info
    if cg_method in ("newman", "backbonepartition") and bonds is None:
        raise SystemExit(f"-cg_method {cg_method} needs the bond graph of the trajectory file")
    if cg_method == "newman":
        mapping, info = partition_newman(bonds, n_atoms, n_cgs, device=device)
        mapping = np.asarray(mapping)
        if mapshuffle > 0.0:
            mapping, info = shuffle_mapping(mapping, mapshuffle, seed), {**info, "mapshuffle": float(mapshuffle)}
        return mapping, info
    if cg_method == "backbonepartition":
        if z is None:
            raise SystemExit("-cg_method backbonepartition needs the atomic numbers of the trajectory file")
        mapping, info = partition_backbone(xyz, z, bonds, n_cgs, seed, device=device)
        return np.asarray(mapping), info
    if cg_method == "seqpartition":
        return partition_sequence(n_atoms, n_cgs, seed), {"method": "seqpartition", "seed": int(seed)}
    if cg_method == "random":
        return partition_random(n_atoms, n_cgs, seed), {"method": "random", "seed": int(seed)}
    return (np.arange(n_atoms) * n_cgs) // n_atoms, None
