"""The baseline models the CGVAE is measured against: linear backmap, equivariant linear, MLP.

Reference: ``Baseline`` (CoarseGrainingVAE/baseline.py:8-36), ``EquiLinear`` (baseline.py:387-443) and ``MLP``
(baseline.py:109-147) under the pooler ``CGpool`` (diffpoolvae.py:105-195) with a fixed ``assign_idx``, ``tau = 0`` and
``gumbel = True``, trained by the loop of scripts/run_baseline.py:121-176 (losses 86-92, 147-149).

What runs where.  The two linear models are one ``n_atoms x C`` matrix each (C = n_cgs, or n_cgs * knn): their whole Adam
loop -- bead means, features, product, both losses, gradient, update -- runs inside ``cgv_baseline_steps``
(csrc/baseline.hip, K19), one launch of one workgroup per chunk of steps, the matrix and its moments in LDS where they fit
(``cgv_baseline_resident_fits``; option ``baseline_form`` forces a form); the host uploads frames and the frame order and
reads the loss log.  ``forward`` runs the same kernel in forward mode.  The MLP's layers are ``primitives.Linear`` (the
package's own products, the activation fused where the kernels know it); its loss and the loss's gradient come from one
launch of ``cgv_baseline_loss`` behind a small ``autograd.Function``; its optimiser is ``train.optim_dict["adam"]``.
There is no tensor-op path for the kernels: a missing kernel is an error.

What is deliberately different.
* The pooler's embedding and update layers never reach an output of these models and receive no gradient: ``FixedPool``
  has no parameters, and ``load_reference_state`` drops the reference's ``pooler.*`` keys.
* ``EquiLinear`` is NOT a k-nearest-neighbour model, here as there: the reference sorts the bead distances and then takes
  ``nonzero()`` of the sorted VALUES, so the second index of every bead pair is the rank position 1..knn, used as a bead id.
  The feature vectors are ``cg[c] - cg[i]`` for i = 0..n_cgs-1, c = 1..knn -- a smooth equivariant linear map over fixed
  bead-pair differences, independent of the sort.  That behaviour is built because the paper's numbers came from it.
* A hyperedge whose reconstructed length is exactly 0 contributes 0 to the gradient (reference: NaN), and an empty
  hyperedge list gives ``loss_dist = 0`` (reference: NaN).
* A mapping that leaves a bead empty is refused (the reference divides by zero); ``cgmap`` retries for that.
* ``EquiLinear``'s ``cross`` is stored and never read, as in the reference.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _lib
from . import primitives as prim
from .steploop import check_order, check_steps, chunks, forced_form, steps_per_epoch

LINEAR, EQUILINEAR = 1, 2                 # include/cgvae_hip.h: CGV_BASELINE_LINEAR / _EQUILINEAR
RESIDENT, GLOBAL = 1, 2                   # CGV_BASELINE_RESIDENT / _GLOBAL
TRAIN, FORWARD = 0, 1                     # CGV_BASELINE_TRAIN / _FORWARD
FORM_NAMES = {RESIDENT: "resident", GLOBAL: "global"}
CHUNK_STEPS = 8192                        # steps per call of the entry point (bounds one launch)
BETAS, EPS = (0.9, 0.999), 1e-8           # torch.optim.Adam defaults (run_baseline.py:304)


def feature_count(kind: int, n_cgs: int, knn: int) -> int:
    return int(n_cgs) if kind == LINEAR else int(n_cgs) * int(knn)


def choose_form(kind: int, n_atoms: int, C: int, batch_size: int) -> int:
    """The one rule: matrix, moments and the batch's features in one workgroup's LDS when they fit
    (cgv_baseline_resident_fits), the same loop on global memory otherwise.  options ``baseline_form`` = 1 / 2 forces a form."""
    return forced_form("baseline_form", lambda: RESIDENT if _lib.load().cgv_baseline_resident_fits(
        int(kind), int(n_atoms), int(C), int(batch_size)) else GLOBAL)


class FixedPool(nn.Module):
    """``CGpool`` with a fixed assignment (diffpoolvae.py:105-195 at tau = 0, gumbel = True): M[a, m(a)] = 1,
    M_norm = M / M.sum(0), cg_xyz = the bead means.  No parameters."""

    def __init__(self, mapping, n_cgs):
        super().__init__()
        mapping = torch.as_tensor(np.asarray(mapping)).long().reshape(-1)
        n_cgs = int(n_cgs)
        if mapping.numel() == 0 or mapping.min() < 0 or mapping.max() >= n_cgs:
            raise ValueError(f"the mapping must name beads 0..{n_cgs - 1} for at least one atom")
        sizes = torch.bincount(mapping, minlength=n_cgs)
        if (sizes == 0).any():
            empty = torch.nonzero(sizes == 0).reshape(-1).tolist()
            raise ValueError(f"the mapping leaves bead(s) {empty} of {n_cgs} empty: a bead mean needs at least one atom "
                             "(cgmap draws again until every bead is used)")
        self.n_cgs, self.n_atoms = n_cgs, int(mapping.numel())
        self.register_buffer("assign_idx", mapping, persistent=False)
        self.register_buffer("sizes", sizes, persistent=False)

    @property
    def M_norm(self) -> torch.Tensor:
        M = torch.zeros(self.n_atoms, self.n_cgs, device=self.assign_idx.device)
        M[torch.arange(self.n_atoms, device=M.device), self.assign_idx] = 1.0
        return M / M.sum(0)

    def cg_xyz(self, xyz: torch.Tensor) -> torch.Tensor:
        """[b, n, 3] -> [b, n_cgs, 3]: one segment reduction over all frames (K1)."""
        from .ops import scatter_mean
        b = xyz.shape[0]
        index = (self.assign_idx[None, :] + self.n_cgs * torch.arange(b, device=xyz.device)[:, None]).reshape(-1)
        return scatter_mean(xyz.reshape(b * self.n_atoms, 3).contiguous(), index, dim=0,
                            dim_size=b * self.n_cgs).reshape(b, self.n_cgs, 3)


def _xyz_of(batch):
    xyz = batch["xyz"] if isinstance(batch, dict) else batch
    if xyz.dim() != 3 or xyz.shape[-1] != 3:
        raise ValueError("xyz must be [frames, n_atoms, 3]")
    return xyz


def _strip_pooler(state_dict):
    return {k: v for k, v in state_dict.items() if not k.startswith("pooler.")}


def _int32(x, device):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x.cpu() if torch.is_tensor(x) else x), dtype=np.int32)).to(device)


def _edges_on(edges, device):
    """(int32 [E,2] on the device -- never an empty buffer -- , E)."""
    if edges is None:
        return torch.zeros(2, dtype=torch.int32, device=device), 0
    e = _int32(edges, device).reshape(-1, 2)
    return (e.contiguous(), int(e.shape[0])) if e.shape[0] else (torch.zeros(2, dtype=torch.int32, device=device), 0)


def _cached(model, slot, source, extra, build):
    """Device copies of the caller's tables (frame order, hyperedges), kept on the model per SOURCE OBJECT: an epoch loop
    that passes the same arrays again uploads and validates nothing.  An array changed in place must be passed as a new object."""
    entries = model.__dict__.setdefault("_tables", {}).setdefault(slot, [])
    for src, ext, val in entries:
        if src is source and ext == extra:
            return val
    val = build()
    entries.append((source, extra, val))
    del entries[:-4]
    return val


def _order_on(model, order, n_frames, dev):
    """(int32 [epochs * n_train] on the device, n_train) of a frame order table, validated once per table."""
    def build():
        table = check_order(order.detach().cpu().numpy() if torch.is_tensor(order) else np.asarray(order), n_frames)
        return torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32).reshape(-1)).to(dev), int(table.shape[1])
    if torch.is_tensor(order) and order.is_cuda and order.dtype == torch.int32 and order.dim() == 2 and order.shape[1] > 0:
        return order.reshape(-1).contiguous(), int(order.shape[1])        # the caller's own device table (the kernel clamps)
    return _cached(model, "order", order, (int(n_frames), str(dev)), build)


class _LinearKind(nn.Module):
    """What ``Baseline`` and ``EquiLinear`` share: the parameter ``B``, its Adam state and the calls of cgv_baseline_steps."""
    kind = 0

    def _setup(self, pooler, n_cgs, n_atoms, knn, shape):
        self.pooler, self.n_cgs, self.n_atoms, self.knn = pooler, int(n_cgs), int(n_atoms), int(knn)
        if pooler.n_cgs != self.n_cgs or pooler.n_atoms != self.n_atoms:
            raise ValueError("the pooler's mapping does not match n_cgs / n_atoms")
        self.C = feature_count(self.kind, self.n_cgs, self.knn)
        self.B = nn.Parameter(0.01 * torch.randn(*shape))
        self.register_buffer("exp_avg", None, persistent=False)          # buffers: they follow ``.to(device)`` with B
        self.register_buffer("exp_avg_sq", None, persistent=False)
        self.adam_steps, self._ws = 0, None

    @property
    def moments(self):
        return None if self.exp_avg is None else [self.exp_avg, self.exp_avg_sq]

    def load_reference_state(self, state_dict):
        """A ``state_dict`` saved by the reference: its ``pooler.*`` keys (layers that reach no output) are dropped, the
        rest is loaded strictly."""
        return self.load_state_dict(_strip_pooler(state_dict), strict=True)

    def reset_optimizer(self):
        self.exp_avg, self.exp_avg_sq, self.adam_steps = None, None, 0

    def run_steps(self, frames, order, batch_size, first_step, steps, *, mode, lr=0.0, gamma=0.0, edges=None, form=None,
                  probe=False):
        """``steps`` steps of the schedule ``order`` (integer [epochs, n_train] indices into ``frames`` [T, n, 3]; a host
        table of any integer type, or an int32 device tensor -- any other device tensor is converted) from schedule position
        ``first_step`` on.  Adam's step count is the schedule position, so training continues where the model's own count
        ``adam_steps`` stands: another ``first_step`` is refused until ``reset_optimizer()``.
        Returns (loss log [steps, 2] on the device, probe tensor or None)."""
        dev = self.B.device
        frames = torch.as_tensor(frames, dtype=torch.float32).to(dev).contiguous()
        if frames.dim() != 3 or tuple(frames.shape[1:]) != (self.n_atoms, 3):
            raise ValueError(f"frames must be [T, {self.n_atoms}, 3]")
        order_dev, n_train = _order_on(self, order, int(frames.shape[0]), dev)
        batch, steps, first_step = int(batch_size), int(steps), int(first_step)
        if mode == TRAIN and steps > 0 and first_step != self.adam_steps:
            raise ValueError(f"training from schedule position {first_step}, but the model's Adam state stands at step "
                             f"{self.adam_steps}: continue there, or reset_optimizer() first")
        check_steps(first_step, steps, order_dev.numel() // n_train, n_train, batch)
        form = choose_form(self.kind, self.n_atoms, self.C, batch) if form is None else int(form)
        edges_dev, E = _cached(self, "edges", edges, str(dev), lambda: _edges_on(edges, dev))
        lib = _lib.load()
        nbytes = int(lib.cgv_baseline_workspace_bytes(self.kind, self.n_atoms, self.n_cgs, self.knn, batch, E, form))
        if nbytes == 0:
            raise ValueError(f"{self.n_atoms} atoms x {self.C} features with batches of {batch} and {E} hyperedges are beyond "
                             "what cgv_baseline_steps holds")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mapping, sizes = _cached(self, "pool", self.pooler, str(dev), lambda: (
            self.pooler.assign_idx.to(dev, torch.int32).contiguous(), self.pooler.sizes.to(dev, torch.int32).contiguous()))
        if mode == TRAIN and self.exp_avg is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.B.data), torch.zeros_like(self.B.data)
        m, v = self.moments if mode == TRAIN else (None, None)
        log = torch.zeros(max(steps, 1), 2, device=dev)
        out = torch.zeros(batch * self.n_atoms * 3 + self.B.numel(), device=dev) if probe else None
        with torch.cuda.device(dev):
            for start, cnt in chunks(steps, CHUNK_STEPS):
                step0 = first_step + start
                # Adam's step count is the schedule position (checked above against the model's own count)
                _lib.call("cgv_baseline_steps", self.kind, form, int(mode), _lib.ptr(self.B.data), _lib.ptr(m), _lib.ptr(v),
                          _lib.ptr(frames), int(frames.shape[0]), _lib.ptr(order_dev), order_dev.numel(), n_train, batch,
                          self.n_atoms, self.n_cgs, self.knn, _lib.ptr(mapping), _lib.ptr(sizes), _lib.ptr(edges_dev), E, step0, cnt,
                          float(gamma), float(lr), BETAS[0], BETAS[1], EPS, _lib.ptr(log[start:]),
                          _lib.ptr(out) if probe and start + cnt == steps else None, _lib.ptr(self._ws), self._ws.numel(),
                          _lib.stream_ptr())
        if mode == TRAIN and steps > 0:
            self.adam_steps = first_step + steps
        return log[:steps], out

    def forward(self, batch):
        """``batch``: {"xyz": [b, n, 3]} (or the tensor) on the device.  Returns (xyz, xyz_recon) as the reference's forward
        does after its ``soft_assign``: the kernel in forward mode on one batch."""
        xyz = _xyz_of(batch).to(self.B.device, torch.float32).contiguous()
        b = int(xyz.shape[0])
        order = np.arange(b, dtype=np.int32)[None, :]
        _, out = self.run_steps(xyz, order, b, 0, 1, mode=FORWARD, probe=True)
        recon = out[: b * self.n_atoms * 3].view(b, self.n_atoms, 3)
        return self._target(xyz), recon

    def _target(self, xyz):
        return xyz


class Baseline(_LinearKind):
    """The linear backmap (baseline.py:8-36): ``x_recon = einsum("bce,ca->bae", cg_xyz - shift, B)`` against
    ``xyz - shift``, shift = the frame's mean over atoms.  ``B [n_cgs, n_atoms] = 0.01 randn``."""
    kind = LINEAR

    def __init__(self, pooler, n_cgs, n_atoms):
        super().__init__()
        self._setup(pooler, n_cgs, n_atoms, 0, (int(n_cgs), int(n_atoms)))

    def _target(self, xyz):
        return xyz - xyz.mean(1, keepdim=True)


class EquiLinear(_LinearKind):
    """The equivariant linear model (baseline.py:387-443): ``dx = einsum("ije,nj->ine", dist_vec, B)`` with
    ``dist_vec[b, i knn + (c-1)] = cg_xyz[b, c] - cg_xyz[b, i]`` (i = 0..n_cgs-1, c = 1..knn), recentred per bead:
    ``xyz_recon = cg_xyz[:, m] - bead_mean(dx)[:, m] + dx``.  ``B [n_atoms, n_cgs knn] = 0.01 randn``.

    ``c`` is a bead index, not a neighbour: the reference sorts the bead distances and takes ``nonzero()`` of the sorted
    values, so the pair's second index is the rank position 1..knn, used as a bead id.  Nothing depends on the sort; this
    module builds that behaviour and no k-nearest-neighbour search, because the paper's numbers came from it.  ``cross`` is
    stored and never read."""
    kind = EQUILINEAR

    def __init__(self, pooler, n_cgs, n_atoms, cross, knn):
        super().__init__()
        if not 1 <= int(knn) <= int(n_cgs) - 1:
            raise ValueError(f"knn = {knn} bead pairs per bead for {n_cgs} beads (need 1 <= knn <= n_cgs - 1)")
        self._setup(pooler, n_cgs, n_atoms, knn, (int(n_atoms), int(n_cgs) * int(knn)))
        self.cross = cross


class _LossFn(torch.autograd.Function):
    """loss_recon + gamma loss_dist of a reconstruction and the gradient with respect to it, one launch (cgv_baseline_loss)."""

    @staticmethod
    def forward(ctx, xyz_recon, xyz, edges, n_edges, gamma, workspace):
        b, n, _ = xyz_recon.shape
        recon, xyz = xyz_recon.detach().float().contiguous(), xyz.detach().float().contiguous()
        losses = torch.empty(2, device=recon.device)
        grad = torch.empty_like(recon)
        with torch.cuda.device(recon.device):
            _lib.call("cgv_baseline_loss", _lib.ptr(recon), _lib.ptr(xyz), _lib.ptr(edges), int(b), int(n), int(n_edges), float(gamma),
                      _lib.ptr(losses), _lib.ptr(grad), _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr())
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(losses)
        return losses[0] + float(gamma) * losses[1], losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        (grad,) = ctx.saved_tensors
        return grad * g_total, None, None, None, None, None


class ReconLoss:
    """The two loss terms of run_baseline.py:147-149 for one molecule's hyperedges.  ``__call__(xyz_recon, xyz)`` returns
    (loss, [loss_recon, loss_dist]); the loss is differentiable with respect to ``xyz_recon``."""

    def __init__(self, edges, gamma, device):
        self.device = torch.device(device)
        self.edges, self.E = _edges_on(edges, self.device)
        self.gamma, self._ws = float(gamma), None

    def __call__(self, xyz_recon, xyz):
        b, n, _ = xyz_recon.shape
        nbytes = int(_lib.load().cgv_baseline_loss_workspace_bytes(int(b), int(n), self.E))
        if nbytes == 0:
            raise ValueError("empty reconstruction")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)       # zero: the kernel's ticket
        return _LossFn.apply(xyz_recon, xyz, self.edges, self.E, self.gamma, self._ws)


_ACT_CODES = {nn.Tanh: prim.ACT_TANH, nn.ReLU: prim.ACT_RELU, prim.Swish: prim.ACT_SWISH}      # fused in the product's epilogue


class MLP(nn.Module):
    """The MLP baseline (baseline.py:109-147): ``Linear(3 n_cgs, W)``, ``depth`` x [act, ``Linear(W, W)``], act,
    ``Linear(W, 3 n_atoms)`` with W = 3 n_atoms width, on ``cg_xyz.reshape(-1, 3 n_cgs)`` without centring.  As in the
    reference the hidden ``Linear`` is ONE module repeated ``depth`` times (``[act, Linear] * depth``): its weights are
    shared, its gradient sums over the uses, and the state_dict lists it under every index it occupies (``mlp.2``,
    ``mlp.4``, ...)."""

    def __init__(self, pooler, n_cgs, n_atoms, width=1, depth=1, activation="ReLU"):
        super().__init__()
        self.pooler, self.n_cgs, self.n_atoms = pooler, int(n_cgs), int(n_atoms)
        if pooler.n_cgs != self.n_cgs or pooler.n_atoms != self.n_atoms:
            raise ValueError("the pooler's mapping does not match n_cgs / n_atoms")
        self.input_dim, self.output_dim = self.n_cgs * 3, self.n_atoms * 3
        self.layer_width = self.output_dim * int(width)
        layers = [prim.Linear(self.input_dim, self.layer_width)] + \
            [prim.to_module(activation), prim.Linear(self.layer_width, self.layer_width)] * int(depth) + \
            [prim.to_module(activation), prim.Linear(self.layer_width, self.output_dim)]
        self.mlp = nn.Sequential(*layers)
        self.optimizer, self.adam_steps = None, 0

    def load_reference_state(self, state_dict):
        """See ``_LinearKind.load_reference_state``; the shared hidden layer arrives under each of its names."""
        return self.load_state_dict(_strip_pooler(state_dict), strict=True)

    def reset_optimizer(self):
        self.optimizer, self.adam_steps = None, 0

    def decode(self, cg_xyz):
        x = cg_xyz.reshape(-1, self.input_dim)
        mods, i = list(self.mlp), 0
        while i < len(mods):
            layer = mods[i]
            code = _ACT_CODES.get(type(mods[i + 1])) if i + 1 < len(mods) else None
            if isinstance(layer, nn.Linear) and code is not None and x.is_cuda:
                x = prim.linear_fn(x, layer.weight, layer.bias, code)             # the activation in the product's epilogue
                i += 2
            else:
                x = layer(x)
                i += 1
        return x.reshape(-1, self.n_atoms, 3)

    def forward(self, batch):
        xyz = _xyz_of(batch).to(self.mlp[0].weight.device, torch.float32).contiguous()
        return xyz, self.decode(self.pooler.cg_xyz(xyz))


def fit(model, frames, order, batch_size, lr, gamma, edges=None, first_step=0, steps=None, train=True, form=None):
    """Steps ``first_step .. first_step + steps`` (default: to the end) of the schedule ``order`` -- int [epochs, n_train]
    frame indices, ``batch_size`` consecutive entries of a row per step, the last batch of a row the partial one -- on
    ``frames`` [T, n, 3].  ``train=False``: forward and losses only (validation, test).  ``lr`` holds for this call, so a
    caller with a schedule calls once per epoch with the position it has reached; Adam's moments and step count stay with
    the model (``model.reset_optimizer()`` forgets them).  For the linear kinds the step count IS the position in the table:
    a ``first_step`` other than the model's ``adam_steps`` is refused.  The order table and the hyperedges are uploaded once
    per object passed and kept with the model.
    Linear kinds: one ``cgv_baseline_steps`` call per chunk of at most ``CHUNK_STEPS`` steps.  MLP: a plain step loop.
    Returns the loss log, a [steps, 2] device tensor of (loss_recon, loss_dist)."""
    batch_size, first_step = int(batch_size), int(first_step)
    if not torch.is_tensor(order):
        order = np.asarray(order)
    if order.ndim != 2 or order.shape[1] == 0:
        raise ValueError("order must be [epochs, n_train]")
    n_train = int(order.shape[1])
    spe = steps_per_epoch(n_train, batch_size)
    total = int(order.shape[0]) * spe
    steps = total - first_step if steps is None else int(steps)
    if isinstance(model, _LinearKind):
        log, _ = model.run_steps(frames, order, batch_size, first_step, steps, mode=TRAIN if train else FORWARD, lr=lr,
                                 gamma=gamma, edges=edges, form=form)
        return log
    if not isinstance(model, MLP):
        raise TypeError("fit takes a Baseline, an EquiLinear or an MLP")
    if steps < 0 or first_step + steps > total:
        raise ValueError("more steps than the frame order table holds")
    from .train import optim_dict
    dev = model.mlp[0].weight.device
    frames = torch.as_tensor(frames, dtype=torch.float32).to(dev)
    table = _cached(model, "order", order, (int(frames.shape[0]), str(dev)), lambda: torch.from_numpy(
        check_order(np.ascontiguousarray(order.cpu().numpy() if torch.is_tensor(order) else order, dtype=np.int64), frames.shape[0])).to(dev))
    loss_fn = _cached(model, "loss", edges, (float(gamma), str(dev)), lambda: ReconLoss(edges, gamma, dev))
    if train:
        if model.optimizer is None:
            model.optimizer = optim_dict["adam"](model.parameters(), lr=float(lr))
        for group in model.optimizer.param_groups:
            group["lr"] = float(lr)
    log = []
    for s in range(first_step, first_step + steps):
        epoch, si = divmod(s, spe)
        idx = table[epoch, si * batch_size: min((si + 1) * batch_size, n_train)]
        xyz = frames[idx].contiguous()
        if train:
            model.optimizer.zero_grad()
            loss, terms = loss_fn(model(xyz)[1], xyz)
            loss.backward()
            model.optimizer.step()
        else:
            with torch.no_grad():
                _, terms = loss_fn(model(xyz)[1], xyz)
        log.append(terms)
    if train:
        model.adam_steps = first_step + steps
    return torch.stack(log) if log else torch.zeros(0, 2, device=dev)
