"""RMSD clustering on the device: K24 (csrc/cluster.hip) against the numpy restatement and against graphs whose clusters
are known in closed form.  The neighbour criterion is an exact comparison of doubles that K17 wrote, the loop is integer
and ordered: every comparison here is integer EQUALITY."""
import functools

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import _lib, cluster, coverage
import cluster_restatement as R
import superpose_restatement as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIMIT = 32768


# ----------------------------------------------------------------------------- helpers
def _to_device(adj):
    return torch.from_numpy(np.ascontiguousarray(R.words(adj)).view(np.int64)).to(DEV)


def _pack(dense, c2, chunk):
    """``cgv_cluster_pack`` over every pair of chunks ``oa <= ob`` of a full dense matrix the test wrote."""
    S = dense.shape[0]
    W = (S + 63) // 64
    d = torch.from_numpy(np.array(dense)).to(DEV)
    bits = torch.full((S, W), 0x5555555555555555, dtype=torch.int64, device=DEV)      # every word must be overwritten
    for oa in range(0, S, chunk):
        for ob in range(oa, S, chunk):
            piece = d[oa:oa + chunk, ob:ob + chunk].contiguous()
            _lib.call("cgv_cluster_pack", _lib.ptr(piece), int(piece.shape[0]), int(piece.shape[1]), oa, ob, S, float(c2),
                      _lib.ptr(bits), _lib.stream_ptr())
    return bits.cpu().numpy().view(np.uint64)


def _bits_from_pairs(S, p, q):
    """A device bit matrix with the bits (p[e], q[e]) set; the pairs are distinct, so adding the powers of two sets them."""
    W = (S + 63) // 64
    flat = torch.zeros(S * W, dtype=torch.int64, device=DEV)
    flat.index_put_((p * W + (q >> 6),), torch.ones_like(q) << (q & 63), accumulate=True)
    return flat.view(S, W)


def _bits_of_groups(group):
    """The device bit matrix of adj(p, q) = (group[p] == group[q]), built in blocks of rows."""
    S = int(group.shape[0])
    W = (S + 63) // 64
    g = torch.from_numpy(group.astype(np.int64)).to(DEV)
    wide = torch.full((64 * W,), -1, dtype=torch.int64, device=DEV)
    wide[:S] = g
    weight = torch.ones(64, dtype=torch.int64, device=DEV) << torch.arange(64, device=DEV)
    bits = torch.empty(S, W, dtype=torch.int64, device=DEV)
    for r0 in range(0, S, 1024):
        same = (g[r0:r0 + 1024, None] == wide[None, :]).view(-1, W, 64)
        bits[r0:r0 + 1024] = (same.to(torch.int64) * weight).sum(dim=2)
    return bits


def _same(got, want, what=""):
    for a, b, name in zip(got, want, ("label", "centres", "sizes")):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)


# ----------------------------------------------------------------------------- pack alone
@functools.lru_cache(maxsize=None)
def _synthetic(S):
    """A dense matrix on and around the threshold: the upper triangle decides, the lower one contradicts it."""
    rng = np.random.default_rng(S)
    c2 = 0.7 * 0.7
    values = np.array([c2, np.nextafter(c2, np.inf), np.nextafter(c2, -np.inf), 0.0, np.inf, 2.0 * c2, 0.25 * c2])
    D = values[rng.integers(0, len(values), (S, S))]
    upper = np.triu(D <= c2, 1)
    D = np.where(np.tri(S, k=-1, dtype=bool), np.where(upper.T, np.inf, 0.0), D)       # the lower triangle lies
    D[np.diag_indices(S)] = np.where(rng.random(S) < 0.5, 0.0, 5.0 * c2)               # a good diagonal may exceed c2
    bad = rng.random(S) < 0.1 if S > 2 else np.zeros(S, bool)
    D[bad, :] = np.nan
    D[:, bad] = np.nan
    D.setflags(write=False)
    want = R.words(R.pack(D, c2))
    want.setflags(write=False)
    return D, c2, bad, want


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 200])
def test_pack_on_the_threshold_with_a_lying_lower_triangle_in_every_chunking(S):
    D, c2, bad, want = _synthetic(S)
    one = _pack(D, c2, (S + 63) // 64 * 64)
    assert one.shape == want.shape and np.array_equal(one, want)
    assert np.array_equal(_pack(D, c2, 64), want) and np.array_equal(_pack(D, c2, 128), want)
    if S % 64:
        assert not (one[:, -1] >> np.uint64(S % 64)).any()                             # bits at columns >= S
    rows = np.unpackbits(one.view(np.uint8), axis=1, bitorder="little")[:, :S].astype(bool)
    assert np.array_equal(rows, rows.T) and not rows[bad].any() and rows[~bad, ~bad].all()


def test_pack_refuses_offsets_it_cannot_own():
    d = torch.zeros(64, 64, dtype=torch.float64, device=DEV)
    bits = torch.zeros(128, 2, dtype=torch.int64, device=DEV)
    for sa, sb, oa, ob in ((64, 64, 64, 0), (64, 64, 32, 64), (64, 64, 64, 128), (32, 64, 0, 64), (64, 32, 0, 0)):
        with pytest.raises(RuntimeError, match="cgv_cluster_pack"):
            _lib.call("cgv_cluster_pack", _lib.ptr(d), sa, sb, oa, ob, 128, 1.0, _lib.ptr(bits), _lib.stream_ptr())


# ----------------------------------------------------------------------------- gromos alone, against the restatement
@functools.lru_cache(maxsize=None)
def _random_graph(S, density):
    rng = np.random.default_rng(1000 * S + int(100 * density))
    upper = np.triu(rng.random((S, S)) < density, 1)
    adj = upper | upper.T | np.eye(S, dtype=bool)
    bad = rng.random(S) < 0.05 if S > 2 else np.zeros(S, bool)
    adj[bad, :] = False
    adj[:, bad] = False
    adj.setflags(write=False)
    return adj, R.gromos(adj)


@pytest.mark.parametrize("density", [0.02, 0.3])
@pytest.mark.parametrize("S", [1, 2, 64, 65, 257, 1000])
def test_gromos_on_random_symmetric_graphs(S, density):
    adj, want = _random_graph(S, density)
    got = cluster.gromos(_to_device(adj), S)
    _same(got, want, (S, density))
    assert got[2].sum() == (got[0] >= 0).sum() and (got[0][got[1]] == np.arange(len(got[1]))).all()


def test_the_centre_is_a_member_whatever_its_diagonal_bit_says():
    adj = np.array(_random_graph(257, 0.02)[0])
    good = adj.diagonal().copy()
    cleared = np.flatnonzero(good)[::3]
    adj[cleared, cleared] = False
    want = R.gromos(adj, good)
    got = cluster.gromos(_to_device(adj), 257, good=good)
    _same(got, want)
    assert (got[0][cleared] >= 0).all() and np.isin(got[1], cleared).any()
    _same(cluster.gromos(_to_device(adj), 257), R.gromos(adj))                         # the diagonal decides who is good


def test_all_bad_input_has_no_cluster():
    for S in (1, 65, 300):
        label, centres, sizes = cluster.gromos(torch.zeros(S, (S + 63) // 64, dtype=torch.int64, device=DEV), S)
        assert label.tolist() == [-1] * S and centres.shape == (0,) and sizes.shape == (0,)


# ----------------------------------------------------------------------------- gromos alone, closed forms
def test_the_identity_at_the_limit():
    i = torch.arange(LIMIT, device=DEV)
    label, centres, sizes = cluster.gromos(_bits_from_pairs(LIMIT, i, i), LIMIT)
    assert np.array_equal(label, np.arange(LIMIT)) and np.array_equal(centres, np.arange(LIMIT)) and (sizes == 1).all()


@pytest.mark.parametrize("k", [90, 255])
def test_cliques_of_descending_size_in_shuffled_order(k):
    """Cliques of k, k - 1, ..., 1 structures (4095 structures, and 32640: the limit's LDS): cluster j is the clique of
    size k - j, its centre the clique's lowest index."""
    S = k * (k + 1) // 2
    rng = np.random.default_rng(k)
    group = rng.permutation(np.repeat(np.arange(k), np.arange(k, 0, -1)))              # group j has k - j members
    label, centres, sizes = cluster.gromos(_bits_of_groups(group), S)
    assert np.array_equal(label, group) and np.array_equal(sizes, np.arange(k, 0, -1))
    first = np.full(k, S)
    np.minimum.at(first, group, np.arange(S))
    assert np.array_equal(centres, first)


def test_a_path_graph():
    """0 - 1 - ... - 4096: {0, 1, 2}, {3, 4, 5}, ... with the middle one as centre, and the last two with 4095."""
    S = 4097
    i = torch.arange(S, device=DEV)
    p = torch.cat([i, i[:-1], i[1:]])
    q = torch.cat([i, i[1:], i[:-1]])
    label, centres, sizes = cluster.gromos(_bits_from_pairs(S, p, q), S)
    assert np.array_equal(label, np.arange(S) // 3)
    assert np.array_equal(centres, np.append(3 * np.arange(1365) + 1, 4095)) and sizes.tolist() == [3] * 1365 + [2]


# ----------------------------------------------------------------------------- end to end
def _copies(templates, sizes, seed, noise=0.05):
    """Randomly rotated and translated noisy copies of the templates, shuffled; which template a frame came from."""
    rng = np.random.default_rng(seed)
    frames, source = [], []
    for t, count in enumerate(sizes):
        for _ in range(count):
            x = templates[t] @ SR.random_rotation(rng).T + rng.normal(0, 5.0, 3) + rng.normal(0, noise, templates[t].shape)
            frames.append(x)
            source.append(t)
    order = rng.permutation(len(frames))
    return np.stack(frames)[order].astype(np.float32), np.array(source)[order]


@functools.lru_cache(maxsize=None)
def _margin_case(m, sizes):
    rng = np.random.default_rng(100 * m + len(sizes))
    templates = rng.normal(0, 2.0, (len(sizes), m, 3))
    xyz, source = _copies(templates, sizes, seed=m)
    d2 = SR.rmsd2_matrix(xyz, xyz)
    xyz.setflags(write=False)
    d2.setflags(write=False)
    return templates, xyz, source, d2


CASES = [(8, (40, 25, 25, 7, 1)), (22, (70, 33, 20, 5)), (5, (33, 31))]
CUTOFF = 0.5


@pytest.mark.parametrize("m,sizes", CASES)
def test_noisy_copies_of_templates_cluster_by_template(m, sizes):
    _, xyz, source, d2 = _margin_case(m, sizes)
    c2 = CUTOFF * CUTOFF
    margin = np.abs(d2 / c2 - 1.0).min()
    print("nearest pair to the threshold, relative:", margin)
    assert margin > 1e-6
    want = R.gromos(R.pack(d2, c2))
    z = np.full(m, 6)
    got = cluster.cluster(xyz, z, cutoff=CUTOFF, device=DEV)
    _same((got["label"], got["centres"], got["sizes"]), want)
    assert got["sizes"].tolist() == sorted(sizes, reverse=True) and got["n_bad"] == 0 and got["atoms"] == list(range(m))
    for k in range(len(sizes)):
        assert len(set(source[got["label"] == k])) == 1
    small = cluster.cluster(xyz, z, cutoff=CUTOFF, structures_per_launch=64, device=DEV)
    _same((small["label"], small["centres"], small["sizes"]), want)
    bits = cluster.adjacency(xyz, None, CUTOFF, device=DEV)
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), R.words(R.pack(d2, c2)))
    assert torch.equal(bits, cluster.adjacency(xyz, None, CUTOFF, structures_per_launch=64, device=DEV))


def test_a_frame_with_a_nan_coordinate_is_bad_and_has_no_label():
    m, sizes = CASES[0]
    _, xyz, source, _ = _margin_case(m, sizes)
    xyz = xyz.copy()
    victim = int(np.flatnonzero(source == 0)[3])
    xyz[victim, 2, 1] = np.nan
    d2 = SR.rmsd2_matrix(xyz, xyz)
    want = R.gromos(R.pack(d2, CUTOFF * CUTOFF))
    for spl in (4096, 64):
        got = cluster.cluster(xyz, np.full(m, 6), cutoff=CUTOFF, structures_per_launch=spl, device=DEV)
        _same((got["label"], got["centres"], got["sizes"]), want)
        assert got["label"][victim] == -1 and got["n_bad"] == 1 and got["sizes"].tolist() == [39, 25, 25, 7, 1]


def test_random_walk_chains_at_the_median_rmsd():
    """200 chains of 12 atoms with the cutoff at the median pairwise RMSD: one large cluster and a few small ones, many
    pairs near the threshold.  The expected labels are the restatement's on the dense matrix K17 itself wrote, so no
    margin is needed."""
    rng = np.random.default_rng(12)
    xyz = np.cumsum(rng.normal(0, 1.0, (200, 12, 3)), axis=1).astype(np.float32)
    x = torch.from_numpy(xyz).to(DEV)
    dense = torch.empty(200, 200, dtype=torch.float64, device=DEV)
    coverage.superpose_launch(x, x, torch.arange(12, dtype=torch.int32, device=DEV), **coverage.new_state(200, 200, DEV), dense=dense)
    d2 = dense.cpu().numpy()
    cutoff = float(np.sqrt(np.median(d2[np.triu_indices(200, 1)])))
    want = R.gromos(R.pack(d2, cutoff * cutoff))
    print("clusters:", len(want[1]), "largest:", want[2].max())
    assert 2 <= len(want[1]) < 100 and want[2].max() > 50
    for spl in (4096, 64, 128):
        got = cluster.cluster(xyz, np.full(12, 6), cutoff=cutoff, structures_per_launch=spl, device=DEV)
        _same((got["label"], got["centres"], got["sizes"]), want, spl)


# ----------------------------------------------------------------------------- assign / compare
@functools.lru_cache(maxsize=None)
def _four_states():
    rng = np.random.default_rng(4)
    templates = rng.normal(0, 2.0, (4, 9, 3))
    ref, ref_source = _copies(templates, (30, 20, 12, 8), seed=1)
    gen, gen_source = _copies(templates, (15, 0, 10, 0), seed=2)
    far, _ = _copies(rng.normal(0, 2.0, (3, 9, 3)), (5, 5, 5), seed=3)
    for a in (ref, gen, far):
        a.setflags(write=False)
    return ref, ref_source, gen, gen_source, far


def test_assign_finds_the_cluster_of_every_clustered_frame():
    ref, source, gen, _, far = _four_states()
    z = np.full(9, 6)
    found = cluster.cluster(ref, z, cutoff=CUTOFF, device=DEV)
    assert found["sizes"].tolist() == [30, 20, 12, 8]
    centre_xyz = ref[found["centres"]]
    d2 = SR.rmsd2_matrix(ref, centre_xyz)
    assert np.abs(d2 / (CUTOFF * CUTOFF) - 1.0).min() > 1e-6
    want_state, want_rmsd = R.assign(d2, CUTOFF * CUTOFF)
    for spl in (4096, 16):
        state, rmsd = cluster.assign(ref, centre_xyz, None, CUTOFF, structures_per_launch=spl, device=DEV)
        assert np.array_equal(state, want_state) and np.array_equal(state, found["label"]) and (state >= 0).all()
        assert np.allclose(rmsd, want_rmsd, rtol=0, atol=5e-6)      # sqrt of two fp64 routes to a d2 that may be 0
    state, rmsd = cluster.assign(far, centre_xyz, None, CUTOFF, device=DEV)
    assert (state == -1).all() and np.isfinite(rmsd).all() and (rmsd > CUTOFF).all()
    broken = np.array(gen[:3])
    broken[1, 0, 0] = np.inf
    state, rmsd = cluster.assign(broken, centre_xyz, None, CUTOFF, device=DEV)
    assert state[1] == -1 and np.isinf(rmsd[1]) and (state[[0, 2]] >= 0).all()


def test_compare_reports_populations_missing_states_and_is_reproducible():
    ref, source, gen, gen_source, far = _four_states()
    z = np.full(9, 6)
    same = cluster.compare(ref, ref, z, cutoff=CUTOFF, device=DEV)
    assert tuple(same) == cluster.CLUSTER_STATS_KEYS
    assert same["jsd"] == 0.0 and same["pop_ref"] == same["pop_gen"] == [30, 20, 12, 8] and same["missing_states"] == []
    assert same["unassigned_ref"] == 0 and same["n_clusters"] == 4 and same["sizes"] == [30, 20, 12, 8]
    assert [int(source[c]) for c in same["centres"]] == [0, 1, 2, 3] and same["states_90"] == 4
    stats = cluster.compare(ref, gen, z, cutoff=CUTOFF, device=DEV)
    assert stats["pop_gen"] == [15, 0, 10, 0] and stats["missing_states"] == [1, 3] and stats["unassigned_gen"] == 0
    assert 0.0 < stats["jsd"] < 1.0 and stats["floor"] < stats["jsd"]
    assert stats["spread_gen"][1] is None and 0.0 < stats["spread_gen"][0] < CUTOFF
    assert stats == cluster.compare(ref, gen, z, cutoff=CUTOFF, structures_per_launch=64, device=DEV)
    lost = cluster.compare(ref, far, z, cutoff=CUTOFF, device=DEV)
    assert lost["unassigned_gen"] == 15 and lost["pop_gen"] == [0, 0, 0, 0] and lost["jsd"] == 1.0
    strided = cluster.compare(ref, gen, z, cutoff=CUTOFF, stride=2, device=DEV)
    assert sorted(strided["pop_ref"]) == [8, 12, 20, 30] and sum(strided["sizes"]) == 35 and all(c % 2 == 0 for c in strided["centres"])


def test_the_command_line_end_to_end(tmp_path, capsys):
    import json
    ref, _, gen, _, _ = _four_states()
    np.savez(tmp_path / "ref.npz", xyz=ref, z=np.full(9, 6))
    np.savez(tmp_path / "gen.npz", xyz=gen.reshape(5, 5, 9, 3))
    out, labels = tmp_path / "stats.json", tmp_path / "labels.npz"
    stats = cluster.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -cluster_cutoff 0.5 -labels {labels} -out {out}".split())
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["cluster_stats"]["missing_states"] == [1, 3] and "pop_ref" not in line["cluster_stats"]
    assert json.load(open(out)) == json.loads(json.dumps(stats))
    with np.load(labels) as f:
        assert f["ref_state"].shape == (70,) and f["gen_state"].shape == (25,) and f["centres"].tolist() == stats["centres"]
