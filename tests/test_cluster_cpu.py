"""RMSD clustering without a device: the numpy restatement against hand-worked graphs, the host half of ``cluster``
(``compare_from_labels``, ``summary_of``), and every refusal of ``cluster``, ``compare`` and the command line -- all of
which happen before a device is touched."""
import json

import numpy as np
import pytest

from coarsegrainingvae_amd import _lib, cluster
import cluster_restatement as R


def _graph(S, edges, bad=()):
    adj = np.eye(S, dtype=bool)
    for p, q in edges:
        adj[p, q] = adj[q, p] = True
    for b in bad:
        adj[b, :] = adj[:, b] = False
    return adj


# ----------------------------------------------------------------------------- the restatement against hand-worked graphs
def test_one_clique_is_one_cluster_with_the_lowest_index_as_centre():
    label, centres, sizes = R.gromos(np.ones((5, 5), dtype=bool))
    assert label.tolist() == [0] * 5 and centres.tolist() == [0] and sizes.tolist() == [5]


def test_two_cliques_of_equal_size_the_lower_index_wins():
    adj = _graph(6, [(1, 3), (3, 5), (1, 5), (0, 2), (2, 4), (0, 4)])       # {1, 3, 5} and {0, 2, 4}
    label, centres, sizes = R.gromos(adj)
    assert centres.tolist() == [0, 1] and sizes.tolist() == [3, 3] and label.tolist() == [0, 1, 0, 1, 0, 1]


def test_a_path_of_seven():
    adj = _graph(7, [(i, i + 1) for i in range(6)])
    label, centres, sizes = R.gromos(adj)
    assert label.tolist() == [0, 0, 0, 1, 1, 1, 2] and centres.tolist() == [1, 4, 6] and sizes.tolist() == [3, 3, 1]


def test_an_isolated_bad_structure_has_no_label():
    adj = _graph(4, [(0, 1), (1, 2), (2, 3)], bad=[2])
    label, centres, sizes = R.gromos(adj)
    assert label.tolist() == [0, 0, -1, 1] and centres.tolist() == [0, 3] and sizes.tolist() == [2, 1]
    assert R.gromos(np.zeros((3, 3), dtype=bool))[0].tolist() == [-1, -1, -1]


def test_the_centre_is_a_member_whatever_its_diagonal_bit_says():
    adj = _graph(3, [(0, 1)])
    adj[0, 0] = adj[2, 2] = False
    label, centres, sizes = R.gromos(adj, good=[True, True, True])
    assert label.tolist() == [0, 0, 1] and centres.tolist() == [1, 2] and sizes.tolist() == [2, 1]


def test_pack_takes_the_upper_triangle_and_nan_compares_false():
    nan = float("nan")
    c2 = 0.25
    D = np.array([[0.0, c2, np.nextafter(c2, np.inf), nan],
                  [9.0, 1e-30, np.nextafter(c2, -np.inf), nan],
                  [0.0, 9.0, 0.0, nan],
                  [nan, nan, nan, nan]])
    adj = R.pack(D, c2)
    assert adj.astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    assert np.array_equal(adj, adj.T)
    w = R.words(adj)
    assert w.shape == (4, 1) and w[:, 0].tolist() == [0b0011, 0b0111, 0b0110, 0]
    assert R.words(np.ones((65, 65), dtype=bool))[0].tolist() == [2 ** 64 - 1, 1]
    assert np.array_equal(cluster.pack_mask([True, False, True], 3).view(np.uint64), [0b101])


def test_assign_restated():
    dense = np.array([[0.3, 0.1, 0.1], [2.0, 3.0, np.nan], [np.nan, np.nan, np.nan]])
    state, rmsd = R.assign(dense, 0.25)
    assert state.tolist() == [1, -1, -1] and rmsd[0] == np.sqrt(0.1) and rmsd[1] == np.sqrt(2.0) and np.isinf(rmsd[2])


# ----------------------------------------------------------------------------- compare_from_labels
def _set(states, rmsd=None):
    s = np.asarray(states, dtype=np.int64)
    return s, (np.full(s.shape, 0.5) if rmsd is None else np.asarray(rmsd, dtype=np.float64))


def test_identical_populations_have_no_divergence_and_the_keys_are_the_documented_ones():
    even, odd, gen = _set([0, 0, 1, 2]), _set([0, 0, 1, 2]), _set([0, 1, 2, 0, 0, 1, 2, 0])
    stats = cluster.compare_from_labels(even, odd, gen, centres=[4, 9, 2], sizes=[4, 2, 2], params={"cutoff": 1.0})
    assert tuple(stats) == cluster.CLUSTER_STATS_KEYS
    assert stats["jsd"] == 0.0 and stats["floor"] == 0.0
    assert stats["pop_ref"] == [4, 2, 2] and stats["pop_gen"] == [4, 2, 2] and stats["n_clusters"] == 3
    assert stats["centres"] == [4, 9, 2] and stats["sizes"] == [4, 2, 2]
    assert stats["unassigned_ref"] == 0 and stats["unassigned_gen"] == 0 and stats["missing_states"] == []
    assert stats["spread_ref"] == [0.5, 0.5, 0.5] and stats["params"] == {"cutoff": 1.0, "min_population": 0.01}
    back = json.loads(json.dumps(stats))
    assert back["pop_ref"] == [4, 2, 2]
    short = cluster.summary_of(stats)
    assert "pop_ref" not in short and "centres" not in short and "spread_gen" not in short and short["jsd"] == 0.0
    json.dumps(short)


def test_disjoint_populations_have_divergence_one():
    stats = cluster.compare_from_labels(_set([0, 0]), _set([0, 0]), _set([1, 1, 1]), [0, 1], [4, 0])
    assert stats["jsd"] == 1.0 and stats["missing_states"] == [0]
    assert stats["top_states"][0]["p_ref"] == 1.0 and stats["top_states"][0]["p_gen"] == 0.0
    assert stats["spread_gen"] == [None, 0.5] and stats["spread_ref"] == [0.5, None]


def test_states_90_missing_states_and_the_unassigned_bin():
    ref_states = [0] * 50 + [1] * 30 + [2] * 11 + [3] * 8 + [4] * 1 + [-1] * 10 + [0]          # 111, the last one bad
    rmsd = [0.25] * 110 + [np.inf]
    even = _set(ref_states[0::2], rmsd[0::2])
    odd = _set(ref_states[1::2], rmsd[1::2])
    gen = _set([0] * 6 + [1] * 2 + [-1] * 2 + [4], [0.1] * 10 + [np.inf])
    stats = cluster.compare_from_labels(even, odd, gen, [0, 1, 2, 3, 4], [50, 30, 11, 8, 1], min_population=0.05)
    assert stats["n_ref"] == 111 and stats["n_bad_ref"] == 1 and stats["n_gen"] == 11 and stats["n_bad_gen"] == 1
    assert stats["pop_ref"] == [50, 30, 11, 8, 1] and stats["unassigned_ref"] == 10
    assert stats["pop_gen"] == [6, 2, 0, 0, 0] and stats["unassigned_gen"] == 2
    assert stats["states_90"] == 3                            # 50 + 30 = 80 < 90 <= 91 of the 100 assigned
    assert stats["missing_states"] == [2, 3]                  # 11 and 8 of 110 are above 5 %, 1 of 110 is not
    assert 0.0 < stats["floor"] < 0.05
    assert stats["top_states"][0]["state"] == 0 and len(stats["top_states"]) == 5
    one = _set([0, 0])                                        # the unassigned are a bin of their own
    only = cluster.compare_from_labels(one, one, _set([0] * 4), [7], [4])
    some = cluster.compare_from_labels(one, one, _set([0] * 4 + [-1] * 4), [7], [4])
    assert only["jsd"] == 0.0 and some["jsd"] > 0.3 and some["unassigned_gen"] == 4 and some["pop_gen"] == [4]


def test_an_empty_generated_set():
    stats = cluster.compare_from_labels(_set([0, 1]), _set([0, 1]), _set([]), [0, 1], [2, 2])
    assert stats["n_gen"] == 0 and stats["jsd"] is None and stats["floor"] == 0.0 and stats["top_states"] == []
    assert stats["pop_gen"] == [0, 0] and stats["missing_states"] == [0, 1] and stats["spread_gen"] == [None, None]
    json.dumps(stats)
    none = cluster.compare_from_labels(_set([-1]), _set([-1]), _set([-1]), [], [])
    assert none["n_clusters"] == 0 and none["states_90"] == 0 and none["jsd"] == 0.0 and none["unassigned_ref"] == 2


def test_compare_from_labels_refuses_states_that_do_not_exist():
    with pytest.raises(ValueError, match="state outside"):
        cluster.compare_from_labels(_set([0, 2]), _set([0]), _set([0]), [0, 1], [1, 1])
    with pytest.raises(ValueError, match="sizes"):
        cluster.compare_from_labels(_set([0]), _set([0]), _set([0]), [0, 1], [1])
    with pytest.raises(ValueError, match="min_population"):
        cluster.compare_from_labels(_set([0]), _set([0]), _set([0]), [0], [1], min_population=2.0)


# ----------------------------------------------------------------------------- refusals before a device is touched
@pytest.fixture
def no_device(monkeypatch):
    """Any launch, and any tensor that is sent to a device, fails the test."""
    import torch

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(torch.Tensor, "to", touched)
    monkeypatch.setattr(torch, "empty", touched)
    monkeypatch.setattr(torch, "zeros", touched)


def test_cluster_refuses_before_any_launch(no_device):
    z = np.array([6, 1, 8, 1])
    x = np.zeros((5, 4, 3), np.float32)
    lim = cluster.limits()["structures"]
    assert lim == 32768
    with pytest.raises(ValueError, match="stride"):
        cluster.cluster(np.zeros((lim + 1, 4, 3), np.float32), z)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cutoff"):
            cluster.cluster(x, z, cutoff=bad)
    with pytest.raises(ValueError, match="empty"):
        cluster.cluster(x, np.array([1, 1, 1, 1]))            # no heavy atom
    with pytest.raises(ValueError, match="names atom 4"):
        cluster.cluster(x, z, atoms=[0, 4])
    with pytest.raises(ValueError, match="z lists 3 atoms"):
        cluster.cluster(x, z[:3])
    with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
        cluster.cluster(np.zeros((5, 4), np.float32), z)
    with pytest.raises(ValueError, match="'heavy', 'all'"):
        cluster.cluster(x, z, atoms="backbone")
    with pytest.raises(ValueError, match="stride"):
        cluster.adjacency(np.zeros((lim + 1, 4, 3), np.float32))
    with pytest.raises(ValueError, match="stride"):
        cluster.gromos(None, lim + 1)
    with pytest.raises(ValueError, match="cutoff"):
        cluster.assign(x, x[:2], None, cutoff=-1.0)
    with pytest.raises(ValueError, match="mismatched n"):
        cluster.assign(x, np.zeros((2, 5, 3), np.float32))


def test_compare_refuses_before_any_launch(no_device):
    z = np.array([6, 1, 8, 1])
    ref, gen = np.zeros((6, 4, 3), np.float32), np.zeros((3, 4, 3), np.float32)
    with pytest.raises(ValueError, match="at least two reference frames"):
        cluster.compare(ref[:1], gen, z)
    with pytest.raises(ValueError, match="z lists 4 atoms"):
        cluster.compare(ref, np.zeros((3, 5, 3), np.float32), z)
    with pytest.raises(ValueError, match="stride"):
        cluster.compare(ref, gen, z, stride=0)
    with pytest.raises(ValueError, match="min_population"):
        cluster.compare(ref, gen, z, min_population=-0.1)
    with pytest.raises(ValueError, match="cutoff"):
        cluster.compare(ref, gen, z, cutoff=float("nan"))
    with pytest.raises(ValueError, match="empty"):
        cluster.compare(ref, gen, np.array([1, 1, 1, 1]))
    lim = cluster.limits()["structures"]
    with pytest.raises(ValueError, match="stride"):
        cluster.compare(np.zeros((2 * lim + 1, 4, 3), np.float32), gen, z, stride=2)


# ----------------------------------------------------------------------------- command line
def _files(tmp_path, n_ref=4):
    z = np.array([6, 6, 8, 7, 1])
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "ref.npz", xyz=rng.normal(0, 2, (n_ref, 5, 3)).astype(np.float32), z=z)
    np.savez(tmp_path / "gen.npz", xyz=rng.normal(0, 2, (2, 3, 5, 3)).astype(np.float32))
    return f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'}"


def test_the_parser_and_read_inputs(tmp_path, no_device):
    base = _files(tmp_path)
    args = cluster.parser().parse_args(base.split())
    assert (args.cluster_cutoff, args.cluster_atoms, args.cluster_stride, args.labels, args.out, args.top) == \
        (1.0, "heavy", 1, None, "cluster_stats.json", None)
    inp = cluster.read_inputs(args)
    assert inp["ref_xyz"].shape == (4, 5, 3) and inp["gen_xyz"].shape == (6, 5, 3) and inp["z"].tolist() == [6, 6, 8, 7, 1]
    args = cluster.parser().parse_args((base + " -cluster_cutoff 2.5 -cluster_atoms all -cluster_stride 3 -labels l.npz -out x.json").split())
    assert (args.cluster_cutoff, args.cluster_atoms, args.cluster_stride, args.labels, args.out) == (2.5, "all", 3, "l.npz", "x.json")


def test_the_command_line_refuses_before_any_launch(tmp_path, no_device):
    base = _files(tmp_path)

    def refused(extra, match):
        with pytest.raises(SystemExit, match=match):
            cluster.read_inputs(cluster.parser().parse_args((base + " " + extra).split()))
    refused("-cluster_cutoff -1", "-cluster_cutoff")
    refused("-cluster_cutoff nan", "-cluster_cutoff")
    refused("-cluster_stride 0", "-cluster_stride")
    refused(f"-top {tmp_path / 'nothing.npz'}", "no such file")
    np.savez(tmp_path / "other.npz", z=[6, 6])
    refused(f"-top {tmp_path / 'other.npz'}", "the topology has 2 atoms")
    np.savez(tmp_path / "hydrogen.npz", z=[1, 1, 1, 1, 1])
    refused(f"-top {tmp_path / 'hydrogen.npz'}", "no heavy atoms")
    np.savez(tmp_path / "bare.npz", xyz=np.zeros((4, 5, 3), np.float32))
    with pytest.raises(SystemExit, match="missing z"):
        cluster.read_inputs(cluster.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'bare.npz'}".split()))
    np.savez(tmp_path / "short.npz", xyz=np.zeros((1, 5, 3), np.float32), z=[6, 6, 8, 7, 1])
    with pytest.raises(SystemExit, match="at least two"):
        cluster.read_inputs(cluster.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'short.npz'}".split()))
    np.savez(tmp_path / "wide.npz", xyz=np.zeros((3, 6, 3), np.float32))
    with pytest.raises(SystemExit, match="wide.npz: xyz is"):
        cluster.read_inputs(cluster.parser().parse_args(f"-gen {tmp_path / 'wide.npz'} -ref {tmp_path / 'ref.npz'}".split()))
    lim = cluster.limits()["structures"]
    np.savez(tmp_path / "long.npz", xyz=np.zeros((2 * lim + 2, 5, 3), np.float32), z=[6, 6, 8, 7, 1])
    with pytest.raises(SystemExit, match="-cluster_stride 3"):
        cluster.read_inputs(cluster.parser().parse_args(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'long.npz'} -cluster_stride 2".split()))
    with pytest.raises(SystemExit):
        cluster.parser().parse_args(["-gen", "a.npz"])                         # -ref is required


# ----------------------------------------------------------------------------- library
def test_the_library_declares_binds_and_exports_the_clustering_kernels():
    names = {"cgv_cluster_max_structures", "cgv_cluster_workspace_bytes", "cgv_cluster_pack", "cgv_cluster_gromos"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.cgv_cluster_max_structures() == 32768
    assert lib.cgv_cluster_workspace_bytes(200, 64) == 200 * 4 * 8 + 64 * 64 * 8
    assert lib.cgv_cluster_workspace_bytes(32768, 4096) == (128 << 20) + (128 << 20)
    assert lib.cgv_cluster_workspace_bytes(32769, 64) == 0 and lib.cgv_cluster_workspace_bytes(10, 0) == 0
