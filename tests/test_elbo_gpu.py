"""csrc/elbo.hip and csrc/loss_tail.hip called directly (cgv_elbo_fwd, cgv_elbo_scale, cgv_loss_tail through _lib.call, and
once each through ops.elbo_loss) against tests/elbo_restatement.py in fp64 -- at the sizes where their code changes shape
(the tables of elbo_restatement; tests/test_elbo_cpu.py holds each shape to the path it claims and the restatement to
train.loss_terms), with the bounds derived there from the kernels' operation counts.  Every element of every output is
compared; one guard row of NaN stands behind each output buffer and must survive."""
import functools

import pytest
import torch

import elbo_restatement as R
from coarsegrainingvae_amd import _lib
from coarsegrainingvae_amd.graph import EdgePlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
UPSTREAM = 3.0

KL_IDS = [f"{n}x{F}" for n, F, _, _ in R.KL_CASES]
BOND_IDS = [f"{a}-atoms-{m}-bonds-gamma-{g:g}-{'ws' if ws else 'no-ws'}" for a, m, g, ws, _, _, _ in R.BOND_CASES]


def _guarded(n, *rest):
    """[n + 1, ...] of NaN: the kernel is given the first n rows."""
    return torch.full((n + 1,) + rest, NAN, device=DEV)


class Outputs:
    def __init__(self, n_beads, F, n_atoms, with_tail=False):
        self.n_beads, self.n_atoms = n_beads, n_atoms
        self.out4, self.loss = _guarded(1, 4), _guarded(1)
        self.bead = {k: _guarded(n_beads, F) for k in ("g_mu", "g_sigma", "g_prior_mu", "g_prior_std")}
        self.g_xr = _guarded(n_atoms, 3)
        self.xr = _guarded(n_atoms, 3) if with_tail else None
        self.g_V = _guarded(n_beads, F, 3) if with_tail else None

    def grad_ptrs(self):
        return [_lib.ptr(self.bead[k]) for k in ("g_mu", "g_sigma", "g_prior_mu", "g_prior_std")] + [_lib.ptr(self.g_xr)]

    def values(self):
        torch.cuda.synchronize()
        out = {"loss": self.out4[0, 0], "kl": self.out4[0, 1], "recon": self.out4[0, 2], "graph": self.out4[0, 3],
               "loss_copy": self.loss[0], "g_xyz_recon": self.g_xr[:self.n_atoms]}
        out.update({k: v[:self.n_beads] for k, v in self.bead.items()})
        if self.xr is not None:
            out["xyz_recon"], out["g_V"] = self.xr[:self.n_atoms], self.g_V[:self.n_beads]
        return {k: v.detach().cpu().clone() for k, v in out.items()}

    def guards_intact(self):
        rows = [self.out4[1], self.loss[1:], self.g_xr[self.n_atoms]] + [v[self.n_beads] for v in self.bead.values()]
        if self.xr is not None:
            rows += [self.xr[self.n_atoms], self.g_V[self.n_beads]]
        return all(bool(torch.isnan(r).all()) for r in rows)


@functools.lru_cache(maxsize=None)
def _elbo_case(n_beads, F, n_atoms, n_bonds, seed, gamma):
    """Inputs, fp64 reference and bounds of one cgv_elbo_fwd case: computed once, shared, never modified."""
    inp = R.elbo_inputs(n_beads, F, n_atoms, n_bonds, seed)
    ref = R.reference(inp, R.BETA, gamma)
    return inp, ref, R.bounds(inp, ref, R.BETA, gamma)


@functools.lru_cache(maxsize=None)
def _tail_case(name):
    sizes, F, n_bonds, gamma, offset, unsorted = R.TAIL_UNSUPPORTED if name == "3073" else R.TAIL_CASES[name]
    seed = 399 if name == "3073" else 300 + list(R.TAIL_CASES).index(name)
    inp = R.tail_inputs(sizes, F, n_bonds, seed, unsorted)
    ref = R.reference(inp, R.BETA, gamma, offset)
    return inp, ref, R.bounds(inp, ref, R.BETA, gamma, offset), (sizes, F, n_bonds, gamma, offset)


def _to_dev(inp):
    return {k: v.to(DEV).contiguous() for k, v in inp.items()}


def _report(what, got, ref, bounds, names):
    """Print the worst error of every output as a fraction of its bound, then require each <= 1."""
    ratios = {n: R.worst_ratio(got[n], ref[n], bounds[n]) for n in names}
    print(f"{what}: worst error / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    for n, r in ratios.items():
        assert r <= 1.0, (what, n, r)
    assert torch.equal(got["loss_copy"].view(torch.int32), got["loss"].view(torch.int32)), what     # the second copy: same bits


def _elbo_workspace(n_beads, F, mode):
    """mode "full": what cgv_elbo_workspace_bytes asks for, filled with ones (the kernels must not count on zeros);
    "null": no workspace; "short": 8 bytes too few -- the call then runs its single block."""
    need = int(_lib.load().cgv_elbo_workspace_bytes(n_beads, F))
    if mode == "null":
        return None, 0
    nbytes = need if mode == "full" else need - 8
    assert nbytes > 0
    return torch.full((need,), 255, dtype=torch.uint8, device=DEV), nbytes


def _run_elbo(d, dims, gamma, mode):
    n_beads, F, n_atoms, n_bonds = dims
    o = Outputs(n_beads, F, n_atoms)
    ws, nbytes = _elbo_workspace(n_beads, F, mode)
    _lib.call("cgv_elbo_fwd", _lib.ptr(d["mu"]), _lib.ptr(d["sigma"]), _lib.ptr(d["prior_mu"]), _lib.ptr(d["prior_std"]),
              _lib.ptr(d["xyz"]), _lib.ptr(d["xyz_recon"]), _lib.ptr(d["bonds"]) if n_bonds else None, n_beads, F, n_atoms, n_bonds,
              R.BETA, gamma, _lib.ptr(o.out4), _lib.ptr(o.loss), *o.grad_ptrs(), _lib.ptr(ws), nbytes, _lib.stream_ptr())
    return o


ELBO_NAMES = R.SCALARS + R.GRADS
TAIL_NAMES = ELBO_NAMES + R.TAIL_ONLY


# ----------------------------------------------------------------------------------------------------------------------
# 1. cgv_elbo_fwd


@pytest.mark.parametrize("n_beads,F,blocks,rounds", R.KL_CASES, ids=KL_IDS)
def test_elbo_fwd_kl_path_vs_fp64(n_beads, F, blocks, rounds):
    """The KL terms and their four gradients from 1 element to 132 000: the single block's 4-deep rounds at 4095 / 4096 /
    4097 elements and its last size 16383; elbo_kl_k from 16384 (16 blocks) to its 128-block cap with the grid-stride loop
    -- and these two again with no workspace and with one 8 bytes short, where the single block takes all of it within the
    same bounds.  5 atoms, 6 bonds."""
    seed = 100 + R.KL_CASES.index((n_beads, F, blocks, rounds))
    inp, ref, bounds = _elbo_case(n_beads, F, R.KL_ATOMS, R.KL_BONDS, seed, R.GAMMA)
    d = _to_dev(inp)
    assert d["bonds"].dtype == torch.int64
    for mode in ("full",) + (("null", "short") if blocks else ()):
        o = _run_elbo(d, (n_beads, F, R.KL_ATOMS, R.KL_BONDS), R.GAMMA, mode)
        _report(f"elbo_fwd {n_beads}x{F} workspace={mode}", o.values(), ref, bounds, ELBO_NAMES)
        assert o.guards_intact()


@pytest.mark.parametrize("n_atoms,n_bonds,gamma,ws,G,blocks,chunks", R.BOND_CASES, ids=BOND_IDS)
def test_elbo_fwd_bond_path_vs_fp64(n_atoms, n_bonds, gamma, ws, G, blocks, chunks):
    """The bond-graph term and d loss / d xyz_recon: elbo_fwd's thread-group split G = 4 / 3 / 2 / 1 (two atom trips at
    1025 atoms), the pad-to-16 edge of the staged chunk at 1 / 15 / 16 / 17 bonds, a second and a third chunk; no bonds at
    all (bonds = NULL); gamma = 0 with bonds present (graph reported as an exact 0 -- its bound is 0 --, the gradient the
    reconstruction part alone); elbo_bond_k on 2, 5, 11, 17 and (through the table's 1025 atoms) more blocks over 1 .. 4
    chunks, and the shape just below its threshold.  Bond lists: elbo_restatement.make_bonds."""
    inp, ref, bounds = _elbo_case(R.BOND_BEADS, R.BOND_F, n_atoms, n_bonds, 200 + n_atoms + n_bonds, gamma)
    d = _to_dev(inp)
    o = _run_elbo(d, (R.BOND_BEADS, R.BOND_F, n_atoms, n_bonds), gamma, "full" if ws else "null")
    got = o.values()
    _report(f"elbo_fwd {n_atoms} atoms {n_bonds} bonds gamma={gamma:g} G={G} bond blocks={blocks} chunks={chunks}", got, ref, bounds, ELBO_NAMES)
    assert o.guards_intact()
    if gamma == 0.0 or n_bonds == 0:
        assert float(got["graph"]) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 2. cgv_elbo_scale


@pytest.mark.parametrize("n_beads,F,n_atoms,n_bonds", [(64, 64, 5, 6), (3, 8, 300, 360)], ids=["more-bead-elements", "more-atom-elements"])
def test_elbo_scale_vs_fp64(n_beads, F, n_atoms, n_bonds):
    """The five gradients of a cgv_elbo_fwd launch times an upstream scalar of 3.0 held on the device, with more bead
    elements than atom elements (4096 against 15) and the other way round (24 against 900): 3 x the restatement, one more
    rounding (elbo_restatement.scaled)."""
    seed = 103 if n_beads == 64 else 200 + n_atoms + n_bonds
    inp, ref, bounds = _elbo_case(n_beads, F, n_atoms, n_bonds, seed, R.GAMMA)
    o = _run_elbo(_to_dev(inp), (n_beads, F, n_atoms, n_bonds), R.GAMMA, "full")
    up = torch.tensor([UPSTREAM], device=DEV)
    _lib.call("cgv_elbo_scale", _lib.ptr(up), *o.grad_ptrs()[:4], n_beads * F, o.grad_ptrs()[4], n_atoms * 3, _lib.stream_ptr())
    got = o.values()
    ref3, bounds3 = R.scaled(ref, bounds, UPSTREAM)
    ratios = {n: R.worst_ratio(got[n], ref3[n], bounds3[n]) for n in R.GRADS}
    print(f"elbo_scale {n_beads}x{F}, {n_atoms} atoms: worst error / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert o.guards_intact()
    for n in R.SCALARS:                                                # the scalars are left alone
        assert R.worst_ratio(got[n], ref[n], bounds[n]) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 3. cgv_loss_tail


def _plan(inp, n_beads):
    """EdgePlan.from_mapping of the case's mapping; its three arrays are the bead-sorted atom order in atom order -- also
    with a bead that owns no atom."""
    plan = EdgePlan.from_mapping(inp["mapping"].to(DEV), n_beads)
    rowptr, atom_of, bead_of = R.plan_arrays(inp["mapping"], n_beads)
    n = inp["mapping"].numel()
    assert torch.equal(plan.rowptr_d.cpu(), rowptr) and torch.equal(plan.eid_d[:n].cpu(), atom_of) and torch.equal(plan.dst_d[:n].cpu(), bead_of)
    return plan


def _tail_workspace(n_beads):
    return torch.zeros(int(_lib.load().cgv_loss_tail_workspace_bytes(n_beads)), dtype=torch.uint8, device=DEV)


def _ticket(ws):
    torch.cuda.synchronize()
    return int(ws[:4].view(torch.int32).item())


def _run_tail(d, plan, dims, gamma, offset, ws):
    n_beads, F, n_atoms, n_bonds = dims
    o = Outputs(n_beads, F, n_atoms, with_tail=True)
    _lib.call("cgv_loss_tail", _lib.ptr(d["V"]), _lib.ptr(d["cg_xyz"]), _lib.ptr(plan.rowptr_d), _lib.ptr(plan.eid_d), _lib.ptr(plan.dst_d),
              _lib.ptr(d["chan"]), _lib.ptr(d["mu"]), _lib.ptr(d["sigma"]), _lib.ptr(d["prior_mu"]), _lib.ptr(d["prior_std"]),
              _lib.ptr(d["xyz"]), _lib.ptr(d["bonds"]) if n_bonds else None, n_beads, F, n_atoms, n_bonds, int(offset), R.BETA, gamma,
              _lib.ptr(o.xr), _lib.ptr(o.out4), _lib.ptr(o.loss), *o.grad_ptrs(), _lib.ptr(o.g_V), _lib.ptr(ws), ws.numel(),
              _lib.stream_ptr())
    return o


@pytest.mark.parametrize("name", list(R.TAIL_CASES))
def test_loss_tail_vs_fp64(name):
    """Decoder tail + ELBO + both backward tails in one launch, every output against the restatement (the plan from
    EdgePlan.from_mapping; unsorted mappings but for the two large cases): with and without the offset; beads of 1, 32, 33,
    64 and 65 atoms (one, two and three passes of 32 own atoms); a bead that owns no atom (zero rows of g_V, its KL terms
    counted); a second and a third bond chunk; 2050 and 3000 atoms (loops past the register slots; 3000 + 72 beads is the
    last supported size); one bead of 2050 channels; 1025 beads of one atom (the last block adds 1025 partial sums in two
    trips; more beads than bonds); gamma = 0; no bonds (bonds = NULL).  Launched twice on the same workspace without
    re-zeroing it: the same bits, and the ticket word reads 0 after each launch."""
    inp, ref, bounds, (sizes, F, n_bonds, gamma, offset) = _tail_case(name)
    n_beads, n_atoms = len(sizes), sum(sizes)
    d, plan = _to_dev(inp), _plan(inp, n_beads)
    ws = _tail_workspace(n_beads)
    first = _run_tail(d, plan, (n_beads, F, n_atoms, n_bonds), gamma, offset, ws)
    assert _ticket(ws) == 0
    got = first.values()
    _report(f"loss_tail {name}", got, ref, bounds, TAIL_NAMES)
    assert first.guards_intact()
    again = _run_tail(d, plan, (n_beads, F, n_atoms, n_bonds), gamma, offset, ws)           # replay: the workspace as it was left
    assert _ticket(ws) == 0
    for k, v in again.values().items():
        assert torch.equal(v.view(torch.int32), got[k].view(torch.int32)), (name, k)
    if gamma == 0.0 or n_bonds == 0:
        assert float(got["graph"]) == 0.0
    for b, size in enumerate(sizes):
        if size == 0:
            assert float(got["g_V"][b].abs().max()) == 0.0
            assert float(got["g_mu"][b].abs().max()) > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. through ops.elbo_loss


def _leaves(d, names):
    return {k: d[k].clone().requires_grad_() for k in names}


def test_ops_elbo_loss_on_given_coordinates_vs_fp64():
    """ops.elbo_loss on an ordinary xyz_recon tensor (cgv_elbo_fwd), bonds as int32, backward seeded with 3.0 (the
    cgv_elbo_scale path): loss, the terms and the five gradients."""
    from coarsegrainingvae_amd import ops
    n_atoms, n_bonds = 300, 360
    inp, ref, bounds = _elbo_case(R.BOND_BEADS, R.BOND_F, n_atoms, n_bonds, 200 + n_atoms + n_bonds, R.GAMMA)
    d = _to_dev(inp)
    lv = _leaves(d, ("mu", "sigma", "prior_mu", "prior_std", "xyz_recon"))
    loss, terms = ops.elbo_loss(lv["mu"], lv["sigma"], lv["prior_mu"], lv["prior_std"], d["xyz"], lv["xyz_recon"], d["bonds"].int(), R.BETA, R.GAMMA)
    (UPSTREAM * loss).backward()
    torch.cuda.synchronize()
    got = {"loss": terms[0], "kl": terms[1], "recon": terms[2], "graph": terms[3], "loss_copy": loss.detach()}
    got = {k: v.cpu() for k, v in got.items()}
    _report("ops.elbo_loss, given coordinates", got, ref, bounds, R.SCALARS)
    ref3, bounds3 = R.scaled(ref, bounds, UPSTREAM)
    grads = dict(zip(R.GRADS, (lv[k].grad for k in ("mu", "sigma", "prior_mu", "prior_std", "xyz_recon"))))
    ratios = {n: R.worst_ratio(grads[n], ref3[n], bounds3[n]) for n in R.GRADS}
    print("ops.elbo_loss, given coordinates, gradients x 3: " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name,fused", [("base-offset", True), ("atoms-3000", True), ("3073", False)])
def test_ops_elbo_loss_on_a_lazy_reconstruction_vs_fp64(name, fused):
    """ops.reconstruct(lazy=True) + ops.elbo_loss: one cgv_loss_tail launch up to n_atoms + n_beads = 3072; at 3073 the
    coordinates are materialised (cgv_reconstruct_fwd) and cgv_elbo_fwd / cgv_reconstruct_bwd run instead -- within the same
    bounds.  Bonds as int32, backward seeded with 3.0."""
    from coarsegrainingvae_amd import ops
    inp, ref, bounds, (sizes, F, n_bonds, gamma, offset) = _tail_case(name)
    n_beads, n_atoms = len(sizes), sum(sizes)
    assert bool(_lib.load().cgv_loss_tail_supported(n_beads, F, n_atoms, n_bonds)) == fused
    d, plan = _to_dev(inp), _plan(inp, n_beads)
    lv = _leaves(d, ("mu", "sigma", "prior_mu", "prior_std", "V"))
    xr = ops.reconstruct(lv["V"], d["cg_xyz"], d["chan"], plan, offset, lazy=True)
    slot = xr._cgv_tail
    assert not slot.filled
    loss, terms = ops.elbo_loss(lv["mu"], lv["sigma"], lv["prior_mu"], lv["prior_std"], d["xyz"], xr, d["bonds"].int(), R.BETA, gamma)
    assert slot.filled and (slot.g_V is not None) == fused                            # which of the two paths ran
    (UPSTREAM * loss).backward()
    torch.cuda.synchronize()
    got = {"loss": terms[0], "kl": terms[1], "recon": terms[2], "graph": terms[3], "loss_copy": loss.detach(), "xyz_recon": xr.detach()}
    got = {k: v.cpu() for k, v in got.items()}
    _report(f"ops.elbo_loss, lazy reconstruction {name}", got, ref, bounds, R.SCALARS + ("xyz_recon",))
    ref3, bounds3 = R.scaled(ref, bounds, UPSTREAM)
    names = ("g_mu", "g_sigma", "g_prior_mu", "g_prior_std", "g_V")
    grads = dict(zip(names, (lv[k].grad for k in ("mu", "sigma", "prior_mu", "prior_std", "V"))))
    ratios = {n: R.worst_ratio(grads[n], ref3[n], bounds3[n]) for n in names}
    print(f"ops.elbo_loss, lazy reconstruction {name}, gradients x 3: " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
