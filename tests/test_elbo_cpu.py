"""tests/elbo_restatement.py pinned to what csrc/elbo.hip and csrc/loss_tail.hip replace: train.KL and the tensor-op branch
of train.loss_terms (scripts/utils.py:81-86, 117-141) in fp64, through autograd; the closed-form gradients the kernels were
written from against that autograd; every bound of the restatement exercised by an fp32 evaluation of the same formulas on
the CPU; and, for every shape of tests/test_elbo_gpu.py, the host predicates that select a kernel path -- so that the GPU
test compares the kernels with the right thing on the branch it claims."""
import pytest
import torch

import elbo_restatement as R
from coarsegrainingvae_amd import _lib, train

KL_IDS = [f"{n}x{F}" for n, F, _, _ in R.KL_CASES]
BOND_IDS = [f"{a}-atoms-{m}-bonds-gamma-{g:g}-{'ws' if ws else 'no-ws'}" for a, m, g, ws, _, _, _ in R.BOND_CASES]


def _close(got, want, what, rel=1e-12):
    """fp64 rounding: ``rel`` per element, plus a hundred roundings of the tensor's largest entry for elements that cancel."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape and bool(torch.isfinite(want).all()), what
    bound = rel * want.abs() + 1e-14 * (want.abs().max() if want.numel() else 0.0)
    err = (got - want).abs()
    assert bool((err <= bound).all()), (what, float((err / bound.clamp(min=1e-300)).max()))


def _all_cases():
    """(id, inputs, gamma, offset or None) of every GPU case."""
    for i, (n, F, _, _) in enumerate(R.KL_CASES):
        yield f"kl-{n}x{F}", R.elbo_inputs(n, F, R.KL_ATOMS, R.KL_BONDS, 100 + i), R.GAMMA, None
    for i, (a, m, g, ws, _, _, _) in enumerate(R.BOND_CASES):
        if ws:                                                    # (the no-workspace runs repeat the inputs of a case that has one)
            yield f"bond-{a}-{m}-{g:g}", R.elbo_inputs(R.BOND_BEADS, R.BOND_F, a, m, 200 + a + m), g, None
    for i, (name, (sizes, F, m, g, offset, unsorted)) in enumerate(R.TAIL_CASES.items()):
        yield f"tail-{name}", R.tail_inputs(sizes, F, m, 300 + i, unsorted), g, offset
    sizes, F, m, g, offset, unsorted = R.TAIL_UNSUPPORTED
    yield "tail-3073", R.tail_inputs(sizes, F, m, 399, unsorted), g, offset


ALL = list(_all_cases())


# ----------------------------------------------------------------------------------------------------------------------
# 1. the restatement is the reference loop's loss


@pytest.mark.parametrize("n_beads,F,n_atoms,n_bonds,gamma", [(1, 1, 2, 1, 50.0), (3, 30, 17, 40, 50.0), (5, 7, 9, 12, 0.0),
                                                             (4, 6, 11, 0, 0.0), (12, 20, 60, 300, 25.0)])
def test_restatement_equals_train_loss_terms(n_beads, F, n_atoms, n_bonds, gamma):
    """All three terms, the loss and the five gradients against train.KL and train.loss_terms' tensor-op branch on fp64 CPU
    tensors; gamma == 0 and an empty bond list among the sizes.  (With an empty bond list and gamma != 0 the tensor-op
    branch takes the mean of nothing; the kernels and the restatement report 0 there: checked at the end.)"""
    inp = R.elbo_inputs(n_beads, F, n_atoms, n_bonds, seed=n_beads + F)
    beta = R.BETA
    leaves = [inp[k].double().requires_grad_() for k in ("mu", "sigma", "prior_mu", "prior_std", "xyz_recon")]
    xyz = inp["xyz"].double()
    loss, kl, recon, graph = train.loss_terms((*leaves[:4], xyz, leaves[4]), {"bond_edge_list": inp["bonds"]}, beta, gamma)
    loss.backward()
    ref = R.reference(inp, beta, gamma)
    _close(ref["kl"], train.KL(*[x.detach() for x in leaves[:4]]), "KL")
    for name, want in (("loss", loss), ("kl", kl), ("recon", recon), ("graph", graph)):
        _close(ref[name], want.detach(), name)
    for name, leaf in zip(R.GRADS, leaves):
        _close(ref[name], leaf.grad, name)
    if n_bonds == 0:
        again = R.reference(inp, beta, 50.0)
        assert float(again["graph"]) == 0.0 and torch.equal(again["g_xyz_recon"], ref["g_xyz_recon"])
        _close(again["loss"], ref["loss"], "loss without bonds")
    if gamma == 0.0:
        assert float(ref["graph"]) == 0.0


def test_tail_restatement_equals_the_indexing_of_the_decoder():
    """cgvae.py:462-481 written out with a host loop per bead: channel = rank of the atom inside its bead, the bead's mean
    taken over its own atoms, the bead centre added; the plan arrays are the bead-sorted order, stable."""
    sizes, F = [3, 0, 5, 1], 6
    inp = R.tail_inputs(sizes, F, 10, seed=5)
    mapping, V, cg = inp["mapping"], inp["V"].double(), inp["cg_xyz"].double()
    rowptr, atom_of, bead_of = R.plan_arrays(mapping, len(sizes))
    assert rowptr.tolist() == [0, 3, 3, 8, 9]
    for offset in (True, False):
        want = torch.zeros(mapping.numel(), 3, dtype=torch.float64)
        for b in range(len(sizes)):
            own = [a for a in range(mapping.numel()) if int(mapping[a]) == b]                 # in atom order
            assert atom_of[int(rowptr[b]):int(rowptr[b + 1])].tolist() == own and all(int(x) == b for x in bead_of[int(rowptr[b]):int(rowptr[b + 1])])
            rel = torch.stack([V[b, k] for k in range(len(own))]) if own else torch.zeros(0, 3, dtype=torch.float64)
            assert [int(inp["chan"][a]) for a in own] == list(range(len(own)))
            if offset and own:
                rel = rel - rel.mean(0)
            for k, a in enumerate(own):
                want[a] = rel[k] + cg[b]
        _close(R.tail(V, cg, mapping, inp["chan"], offset), want, f"tail offset={offset}")


# ----------------------------------------------------------------------------------------------------------------------
# 2. the formulas the kernels were written from


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_closed_form_gradients_equal_autograd_and_bounds_hold_in_fp32(case):
    """For every GPU case.  (a) The reference is finite everywhere, its bounds finite and positive wherever the output is
    not an exact zero.  (b) In fp64 the closed forms -- the four KL formulas, 2 (xr - x) / nr, the bond formula with
    a0 == a1 giving zero, g_xr[a] - mean_b(g_xr) -- equal autograd to 1e-12 relative.  (c) The same formulas evaluated in
    fp32 by torch on the CPU stay within the bounds: that is the reference against itself, not the kernels."""
    name, inp, gamma, offset = case
    ref = R.reference(inp, R.BETA, gamma, offset)
    bounds = R.bounds(inp, ref, R.BETA, gamma, offset)
    exact = R.closed_form(inp, R.BETA, gamma, offset, torch.float64)
    rounded = R.closed_form(inp, R.BETA, gamma, offset, torch.float32)
    outputs = R.SCALARS + R.GRADS + (R.TAIL_ONLY if offset is not None else ())
    line = []
    for out in outputs:
        want = ref[out]
        assert bool(torch.isfinite(want).all()), out
        b = torch.as_tensor(bounds[out]).double().expand_as(want)
        assert bool(torch.isfinite(b).all()) and bool((b[want != 0] > 0).all()), out
        _close(exact[out], want, (name, out), rel=1e-11 if out in ("g_xyz_recon", "g_V", "loss", "graph") else 1e-12)
        ratio = R.worst_ratio(rounded[out], want, bounds[out])
        line.append(f"{out} {ratio:.3f}")
        assert ratio <= 1.0, (name, out, ratio)
    print(f"{name}: fp32 on the CPU, worst error / bound: " + ", ".join(line))
    if inp["bonds"].shape[0] >= 64 and ref["xyz_recon"].shape[0] >= 64:
        props = R.bond_properties(inp["bonds"], ref["xyz_recon"], ref["xyz_recon"].shape[0])
        assert props["self"] >= 2 and props["repeated"] >= 1 and props["reversed"] >= 1 and props["coincident"] >= 1, props
        assert props["hub"] >= R.HUB_BONDS, props
    if gamma == 0.0:
        assert float(ref["graph"]) == 0.0 and float(bounds["graph"]) == 0.0
        _close(ref["g_xyz_recon"], 2.0 * (ref["xyz_recon"] - inp["xyz"].double()) / ref["xyz_recon"].numel(), "reconstruction part only")


def test_the_comparison_sees_a_wrong_kl_formula_and_a_dropped_bond():
    """(mu1 - mu2)^2 / std2^2 instead of / std2 moves KL and g_prior_std by far more than their bounds; so does a bond left
    out of one atom's gradient (the hub's: the loosest bound of the case)."""
    inp = R.elbo_inputs(3, 30, 300, 360, seed=1)
    ref = R.reference(inp, R.BETA, R.GAMMA)
    b = R.bounds(inp, ref, R.BETA, R.GAMMA)
    mu, sigma, pmu, pstd = (inp[k].double() for k in ("mu", "sigma", "prior_mu", "prior_std"))
    wrong_kl = 0.5 * ((sigma ** 2 / pstd ** 2 + (mu - pmu) ** 2 / pstd ** 2 + torch.log(pstd ** 2) - torch.log(sigma ** 2)).sum(-1) - 30).mean()
    assert R.worst_ratio(wrong_kl, ref["kl"], b["kl"]) > 1e3
    less = dict(inp, bonds=inp["bonds"][1:])
    hub = int(torch.bincount(inp["bonds"].flatten()).argmax())
    g_less = R.reference(less, R.BETA, R.GAMMA * 359.0 / 360.0)["g_xyz_recon"]              # (the same gamma / n_bonds)
    touched = inp["bonds"][0]
    if int(touched[0]) != int(touched[1]) and not torch.equal(ref["xyz_recon"][touched[0]], ref["xyz_recon"][touched[1]]):
        assert R.worst_ratio(g_less, ref["g_xyz_recon"], b["g_xyz_recon"]) > 1e3
    assert float(b["g_xyz_recon"][hub].max()) < 1e-3 * float(ref["g_xyz_recon"][hub].abs().max())      # loosest, and still tight


# ----------------------------------------------------------------------------------------------------------------------
# 3. the host predicates that select a path


@pytest.mark.parametrize("n_beads,F,blocks,rounds", R.KL_CASES, ids=KL_IDS)
def test_kl_cases_take_the_path_their_table_claims(n_beads, F, blocks, rounds):
    """cgv_elbo_workspace_bytes = 8 (blocks of elbo_kl_k + 1): nk >= 16384 selects the multi-block KL, capped at 128 blocks
    of 256 threads (a grid-stride loop beyond 32768 elements); below, and without a workspace, elbo_fwd's single block
    makes ceil(nk / 4096) rounds.  The case's atoms and bonds stay in the single block."""
    lib = _lib.load()
    nk = n_beads * F
    assert R.kl_blocks(n_beads, F) == blocks == (0 if nk < 16384 else min(-(-nk // 1024), 128))
    assert int(lib.cgv_elbo_workspace_bytes(n_beads, F)) == 8 * (blocks + 1)
    assert -(-nk // R.KL_ROUND) == rounds
    assert R.bond_blocks(R.KL_ATOMS, R.KL_BONDS, R.GAMMA) == 0
    if (n_beads, F) == (300, 440):
        assert blocks == 128 and nk > 128 * 256 * 4                      # every thread of elbo_kl_k loops more than once
    if (n_beads, F) == (128, 128):
        assert blocks == 16 and nk == 16384
    if (n_beads, F) == (127, 129):
        assert nk == 16383


@pytest.mark.parametrize("n_atoms,n_bonds,gamma,ws,G,blocks,chunks", R.BOND_CASES, ids=BOND_IDS)
def test_bond_cases_take_the_path_their_table_claims(n_atoms, n_bonds, gamma, ws, G, blocks, chunks):
    """n_atoms * n_bonds >= 512 * 1024 (with a workspace, gamma != 0, bonds) selects elbo_bond_k with ceil(n_atoms / 64)
    blocks; otherwise elbo_fwd scans with G = min(4, 1024 / n_atoms) thread groups (1 above 512 atoms); 2048 bonds a chunk."""
    assert int(_lib.load().cgv_elbo_workspace_bytes(R.BOND_BEADS, R.BOND_F)) == 8         # no KL blocks: one double, the bond sum
    multi = ws and gamma != 0.0 and n_bonds > 0 and n_atoms * n_bonds >= 512 * 1024
    assert R.bond_blocks(n_atoms, n_bonds, gamma, ws) == blocks == (-(-n_atoms // 64) if multi else 0)
    assert -(-n_bonds // R.CHUNK) == chunks
    if not multi:
        assert R.fwd_groups(n_atoms) == G == (min(4, 1024 // n_atoms) if 2 * n_atoms <= 1024 else 1)
    if (n_atoms, n_bonds) == (513, 1022):
        assert n_atoms * n_bonds == 512 * 1024 - 2
    if (n_atoms, n_bonds) == (65, 8066):
        assert n_atoms * n_bonds == 512 * 1024 + 2 and blocks == 2 and n_atoms - 64 == 1
    if (n_atoms, n_bonds) == (700, 750):
        assert blocks == 11


def test_bond_table_covers_every_group_split_and_chunk_count():
    single = [c for c in R.BOND_CASES if c[5] == 0]
    assert {c[4] for c in single} == {1, 2, 3, 4}
    assert {c[6] for c in single} >= {0, 1, 2, 3} and {c[6] for c in R.BOND_CASES if c[5] > 0} >= {1, 2, 3, 4}
    assert any(c[0] > 1024 for c in single)                                               # two atom trips with G = 1


@pytest.mark.parametrize("name", list(R.TAIL_CASES))
def test_tail_cases_take_the_path_their_table_claims(name):
    sizes, F, n_bonds, gamma, offset, unsorted = R.TAIL_CASES[name]
    n_beads, n_atoms = len(sizes), sum(sizes)
    lib = _lib.load()
    assert lib.cgv_loss_tail_supported(n_beads, F, n_atoms, n_bonds) == 1 and R.tail_supported(n_beads, F, n_atoms, n_bonds)
    assert int(lib.cgv_loss_tail_workspace_bytes(n_beads)) == 24 * n_beads + 16
    assert max(sizes) <= F
    claims = {
        "base-offset": n_atoms == 80 and n_beads == 8 and F == 16 and max(sizes) <= 32,
        "bead-sizes-1-32-33-64-65": sizes == [1, 32, 33, 64, 65],                       # passes of 32 own atoms: 1, 1, 2, 2, 3
        "empty-bead": 0 in sizes,
        "bonds-2049": n_bonds == R.CHUNK + 1 and n_atoms == 300,
        "bonds-4100": -(-n_bonds // R.CHUNK) == 3 and n_atoms == 300,
        "atoms-2050": n_atoms == R.LT_NP_ELEMS + 2 and n_beads == 41,
        "atoms-3000": n_atoms == 3000 and n_beads == 72 and n_atoms + n_beads == 3072 and n_bonds > R.CHUNK,
        "kl-loop-F-2050": n_beads == 1 and F == R.LT_NP_ELEMS + 2,
        "beads-1025": n_beads == 1025 and sizes == [1] * 1025 and n_bonds < n_beads,
        "gamma-0": gamma == 0.0 and n_bonds > 0,
        "no-bonds": n_bonds == 0 and gamma != 0.0,
    }
    assert claims.get(name, True), name


def test_tail_support_ends_at_3072_atoms_plus_beads():
    lib = _lib.load()
    sizes, F, n_bonds = R.TAIL_UNSUPPORTED[:3]
    assert sum(sizes) + len(sizes) == 3073 and max(sizes) <= F
    assert lib.cgv_loss_tail_supported(len(sizes), F, sum(sizes), n_bonds) == 0 and not R.tail_supported(len(sizes), F, sum(sizes), n_bonds)
    for n_beads, n_atoms, want in ((1, 3071, 1), (1, 3072, 0), (2048, 1024, 1), (2049, 1023, 0), (72, 3000, 1), (72, 3001, 0), (0, 5, 0), (5, 0, 0)):
        assert lib.cgv_loss_tail_supported(n_beads, 4, n_atoms, 7) == want == int(R.tail_supported(n_beads, 4, n_atoms, 7))
