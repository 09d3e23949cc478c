"""The graph-partition coarse-graining maps on the device (csrc/newman.hip, cgmap.py): the Girvan-Newman partition against
the fp64 restatement and against networkx in both kernel forms, the removal log, bitwise reproducibility, disconnected and
degenerate graphs, the backbone partition, and the CLI end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newman_restatement as R  # noqa: E402

from coarsegrainingvae_amd import cgmap, run_ala  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = [cgmap.RESIDENT, cgmap.STREAMED]
FORM_IDS = ["resident", "streamed"]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_partition_equals_the_restatement(options, case, form):
    """Mapping (bead numbering included) and the removal log, edge by edge, on the twenty molecule-like graphs; the form is
    forced through the ``newman_form`` option (every one of these sizes would run resident under the rule)."""
    n, _, k, _ = case
    edges = R.case_graph(case)
    want, removed, _ = R.case_partition(case)
    assert cgmap.choose_newman_form(n, len(edges)) == cgmap.RESIDENT
    options.set("newman_form", form)
    mapping, info = cgmap.partition_newman(edges, n, k)
    assert info["form"] == cgmap.FORM_NAMES[form] and info["method"] == "newman"
    assert [tuple(e) for e in info["removed_edges"]] == removed
    assert info["removals"] == len(removed) and info["launches"] >= 1 + 3 * len(removed)
    assert mapping.dtype == torch.long and mapping.tolist() == want.tolist()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_partition_equals_networkx(options, case, form):
    pytest.importorskip("networkx")
    n, _, k, _ = case
    want, flagged = R.case_networkx(case)
    assert flagged == 0
    options.set("newman_form", form)
    mapping, _ = cgmap.partition_newman(R.case_graph(case), n, k)
    assert R.as_sets(mapping) == R.as_sets(want)
    assert mapping.tolist() == want.tolist()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_betweenness_is_bit_reproducible_and_right(form):
    """Two launches give the same bits (no floating-point atomic, fixed summation orders); the two forms give the same bits
    as each other; and the sums agree with the restatement to fp64 rounding: every value is a sum of at most n^2 positive
    terms, each a quotient and a product of exactly held path counts, so 4 n^2 eps relative is a generous bound for two
    different summation orders."""
    case = (166, 8, 6, 1)
    n, edges = case[0], R.case_graph(case)
    alive = np.ones(len(edges), dtype=np.int32)
    alive[[3, 50, 120]] = 0                                    # some edges already gone: several components at once
    _, first = cgmap.edge_betweenness(edges, n, alive=alive, form=form)
    _, second = cgmap.edge_betweenness(edges, n, alive=alive, form=form)
    _, other = cgmap.edge_betweenness(edges, n, alive=alive, form=FORMS[1 - FORMS.index(form)])
    assert torch.equal(first, second) and torch.equal(first, other)
    want = R.edge_betweenness(n, edges, alive)
    got = first.cpu().numpy()
    assert (got[alive == 0] == 0).all()
    dev = float(np.abs(got - want).max() / want.max())
    print(f"BETWEENNESS {cgmap.FORM_NAMES[form]} rel dev {dev:.2e}")
    assert dev <= 4 * n * n * np.finfo(np.float64).eps


@pytest.mark.parametrize("groups", [4, 0], ids=["four_groups", "rule"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_source_ranges_that_do_not_divide_evenly(form, groups):
    """n = 23 over four workgroups: ranges of 6, 6, 6 and 5 sources (and the rule: one source each)."""
    n = 23
    edges = R.molecule_graph(n, 1, 5)
    if groups:
        assert cgmap._lib.load().cgv_newman_groups(n, groups) == 4
    _, bet = cgmap.edge_betweenness(edges, n, groups=groups, form=form)
    want = R.edge_betweenness(n, edges)
    assert float(np.abs(bet.cpu().numpy() - want).max() / want.max()) <= 4 * n * n * np.finfo(np.float64).eps
    mapping, info = cgmap.partition_newman(edges, n, 4, groups=groups, form=form)
    want_map, removed, _ = R.partition(n, edges, 4)
    assert mapping.tolist() == want_map.tolist() and [tuple(e) for e in info["removed_edges"]] == removed


def _two_molecules():
    a, b = R.molecule_graph(22, 2, 7), R.molecule_graph(17, 1, 8) + 22
    return 39, np.concatenate([a, b])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_graph_that_starts_disconnected(form):
    n, edges = _two_molecules()
    want, removed, _ = R.partition(n, edges, 5)
    mapping, info = cgmap.partition_newman(edges, n, 5, form=form)
    assert mapping.tolist() == want.tolist() and [tuple(e) for e in info["removed_edges"]] == removed
    assert len(set(mapping[:22].tolist()) & set(mapping[22:].tolist())) == 0


def test_n_cgs_equal_to_the_starting_components_removes_nothing():
    n, edges = _two_molecules()
    mapping, info = cgmap.partition_newman(edges, n, 2)
    assert info["removals"] == 0 and info["launches"] == 1 and info["removed_edges"] == []
    assert mapping.tolist() == [0] * 22 + [1] * 17
    with pytest.raises(ValueError, match="already has 2 connected components"):
        cgmap.partition_newman(edges, n, 1)
    with pytest.raises(ValueError, match="n_cgs = 40"):
        cgmap.partition_newman(edges, n, 40)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_n_cgs_equal_to_n_atoms(form):
    case = (22, 2, 3, 0)
    edges = R.case_graph(case)
    mapping, info = cgmap.partition_newman(edges, 22, 22, form=form)
    _, removed, _ = R.partition(22, edges, 22)
    assert mapping.tolist() == list(range(22))
    assert [tuple(e) for e in info["removed_edges"]] == removed and info["removals"] <= len(edges)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_single_ring_every_edge_ties(form):
    """All twelve edges have the same betweenness: the lowest (u, v) goes first, (0, 1); the ring is then a chain from 1 to
    0 whose middle edge (6, 7) goes next."""
    n = 12
    edges = R.sorted_edges([(i, (i + 1) % n) for i in range(n)])
    mapping, info = cgmap.partition_newman(edges, n, 2, form=form)
    want, removed, ties = R.partition(n, edges, 2)
    assert ties >= 1 and removed[0] == (0, 1) and removed[1] == (6, 7)
    assert [tuple(e) for e in info["removed_edges"]] == removed and mapping.tolist() == want.tolist()


# ------------------------------------------------------------------ backbone partition
def _tripeptide():
    """Three residues N(H)-CA(H)(CB)-C(=O), a leading extra H on the first N and an NH2 cap, so that the last C is an amide
    carbon too: 24 atoms, backbone N, CA, C of every residue."""
    z, bonds, backbone = [], [], []

    def atom(elem, *to):
        z.append(elem)
        bonds.extend((t, len(z) - 1) for t in to)
        return len(z) - 1
    prev_c = None
    for _ in range(3):
        N = atom(7, *([prev_c] if prev_c is not None else []))
        atom(1, N)
        CA = atom(6, N)
        atom(1, CA)
        atom(6, CA)
        C = atom(6, CA)
        atom(8, C)
        backbone += [N, CA, C]
        prev_c = C
    atom(1, 0)
    cap = atom(7, prev_c)
    atom(1, cap)
    atom(1, cap)
    return np.array(z), np.array(bonds), np.array(backbone)


def test_backbone_partition_on_a_small_peptide():
    from coarsegrainingvae_amd import tica
    z, bonds, backbone = _tripeptide()
    assert tica.backbone_atoms(z, bonds).tolist() == sorted(backbone.tolist())
    n, T, k, seed, skip = len(z), 30, 3, 11, 4
    rng = np.random.default_rng(2)
    base = np.cumsum(rng.standard_normal((n, 3)) * 1.2, axis=0)
    xyz = (base[None] + 0.2 * rng.standard_normal((T, n, 3))).astype(np.float32)
    mapping, info = cgmap.partition_backbone(xyz, z, bonds, k, seed, skip=skip)
    again, _ = cgmap.partition_backbone(xyz, z, bonds, k, seed, skip=skip)
    assert info["method"] == "backbonepartition" and info["n_backbone"] == 9 and torch.equal(mapping, again)
    # numpy restatement: the same cut points (the function's documented draw), fp64 centroids and mean distances
    bb = np.sort(backbone)
    segment = cgmap._cut_points(len(bb), k, np.random.default_rng([seed, 2]))
    assert sorted(set(segment.tolist())) == [0, 1, 2]
    fr = xyz[::skip].astype(np.float64)
    cen = np.stack([fr[:, bb[segment == s]].mean(1) for s in range(k)], axis=1)                   # [T', k, 3]
    dist = np.sqrt(((fr[:, :, None, :] - cen[:, None, :, :]) ** 2).sum(-1)).mean(0)               # [n, k]
    want = dist.argmin(-1)
    want[bb] = segment
    assert mapping.tolist() == want.tolist()
    assert sorted(set(mapping.tolist())) == [0, 1, 2]
    assert mapping[bb].tolist() == segment.tolist()
    with pytest.raises(ValueError, match="N_backbone = 9"):
        cgmap.partition_backbone(xyz, z, bonds, 10, seed)


# ------------------------------------------------------------------ the CLI
CLI = ("-logdir run -device 0 -traj {traj} -cg_method newman -n_cgs 3 -batch_size 8 -ndata 40 -nepochs 2 -atom_cutoff 8.5 "
       "-cg_cutoff 9.5 -beta 0.05 -gamma 25.0 -dec_nconv 2 -enc_nconv 2 -lr 0.001 -n_basis 32 -n_rbf 8 -edgeorder 2")


def _molecule_file(tmp_path):
    case = (22, 2, 3, 0)
    n, T = 22, 40
    rng = np.random.default_rng(1)
    base = np.cumsum(rng.standard_normal((n, 3)) * 0.9, axis=0)
    xyz = (base[None] + 0.15 * rng.standard_normal((T, n, 3))).astype(np.float32)
    np.savez(tmp_path / "traj.npz", xyz=xyz, z=rng.integers(1, 9, n), bonds=R.case_graph(case))
    return case


def test_cli_partitions_the_bond_graph_and_trains(tmp_path, capsys, monkeypatch):
    """A 22-atom trajectory file WITHOUT a mapping, ``-cg_method newman -n_cgs 3``: two epochs, and the stored mapping is
    the restatement's -- not the contiguous equal blocks every method but cgae used to fall through to."""
    case = _molecule_file(tmp_path)
    monkeypatch.chdir(tmp_path)
    run_ala.main(CLI.format(traj=tmp_path / "traj.npz").split())
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want, removed, _ = R.case_partition(case)
    cg = summary["cg_mapping"]
    assert cg["method"] == "newman" and cg["removals"] == len(removed) and cg["form"] == "resident"
    assert "loss_recon" not in cg and "removed_edges" not in cg
    stored = json.loads(next(tmp_path.glob("run_*_N3/modelparams.json")).read_text())
    assert stored["mapping"] == want.tolist()
    assert stored["mapping"] != ((np.arange(22) * 3) // 22).tolist()
    assert summary["epochs"] == 2 and not summary["failed"]


def test_cli_mapshuffle_changes_the_mapping_reproducibly(tmp_path, capsys, monkeypatch):
    case = _molecule_file(tmp_path)
    monkeypatch.chdir(tmp_path)
    params = vars(run_ala.build_parser().parse_args((CLI.format(traj=tmp_path / "traj.npz") + " -mapshuffle 0.5").split()))
    first = run_ala.load_trajectory_dataset(dict(params), torch.device("cuda", 0))
    second = run_ala.load_trajectory_dataset(dict(params), torch.device("cuda", 0))
    want, _, _ = R.case_partition(case)
    assert first[1].tolist() == second[1].tolist() == cgmap.shuffle_mapping(want, 0.5, 123).tolist()
    assert first[1].tolist() != want.tolist() and sorted(first[1].tolist()) == sorted(want.tolist())
    assert first[2]["mapshuffle"] == 0.5 and first[2]["method"] == "newman"
