"""The relaxation on the device: K32 (csrc/relax.hip) against the numpy.float32 restatement.  Both sides round every
operation identically: ``xyz``, ``clashes``, ``disp2`` and ``bad`` are compared for EQUALITY of bits; ``energy`` within
``N_terms * 2^-52`` relative of ``math.fsum`` of the same fp64 terms."""
import functools
import json

import numpy as np
import pytest
import torch

from coarsegrainingvae_amd import lddt, relax
import relax_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


@functools.lru_cache(maxsize=None)
def _case(n, S, seed=0, sigma=0.3):
    z, bonds, ref, gen = R.case(n, S, seed, sigma=sigma)
    return z, bonds, ref, gen, relax.restraints(z, bonds, ref)


@functools.lru_cache(maxsize=None)
def _want(n, S, steps, seed=0):
    z, bonds, _, gen, tab = _case(n, S, seed)
    probe = relax.relax(gen[:0], tab, z, bonds, device="cpu")          # no structures: the tables relax makes, no launch
    return R.relax32(gen, tab, probe["radii"], probe["excl"], steps)


def _same(got, want, what=""):
    assert got["xyz"].dtype == F and np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)), what
    assert got["clashes"].dtype == np.int32 and np.array_equal(got["clashes"], want["clashes"]), what
    assert np.array_equal(got["disp2"].view(np.uint32), want["disp2"].view(np.uint32)), what
    assert np.array_equal(got["bad"], want["bad"]), what
    assert got["energy"].dtype == np.float64
    tol = want["n_terms"] * 2.0 ** -52 * np.abs(want["energy"])
    assert (np.abs(got["energy"] - want["energy"]) <= tol).all(), (what, got["energy"], want["energy"])


def _bits(res):
    return [res[k].tobytes() for k in ("xyz", "clashes", "energy", "disp2", "bad")]


# ----------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", [5, 22, 31, 32, 33, 65])
def test_atoms_at_the_word_edges_and_the_wave_edge(n):
    z, bonds, _, gen, tab = _case(n, 3)
    got = relax.relax(gen, tab, z, bonds, steps=2, device=DEV)
    _same(got, _want(n, 3, 2), f"n = {n}")
    assert not got["bad"].any() and (n <= 22 or got["clashes"][:, 0].sum() > 0)


def test_more_atoms_than_threads():
    z, bonds, _, gen, tab = _case(300, 2)
    assert relax.pack_of(300) == 1
    got = relax.relax(gen, tab, z, bonds, steps=3, device=DEV)
    _same(got, _want(300, 2, 3), "n = 300")
    assert got["clashes"].min() > 0


@pytest.mark.parametrize("S", [1, 3, 4, 5, 65])
def test_structures_at_the_packing_factor_and_beyond(S):
    assert relax.pack_of(22) == 4 and relax.pack_of(65) == 2
    z, bonds, _, gen, tab = _case(22, S)
    _same(relax.relax(gen, tab, z, bonds, steps=2, device=DEV), _want(22, S, 2), f"S = {S}")
    if S in (1, 3):                                                   # two structures per block: S = pack - 1, pack + 1
        z, bonds, _, gen, tab = _case(65, S)
        _same(relax.relax(gen, tab, z, bonds, steps=2, device=DEV), _want(65, S, 2), f"n = 65, S = {S}")


@pytest.mark.parametrize("steps", [0, 1, 2, 25])
def test_the_number_of_steps(steps):
    z, bonds, _, gen, tab = _case(33, 2)
    got = relax.relax(gen, tab, z, bonds, steps=steps, device=DEV)
    _same(got, _want(33, 2, steps), f"steps = {steps}")
    if steps == 0:
        assert np.array_equal(got["xyz"], gen) and np.array_equal(got["clashes"][:, 0], got["clashes"][:, 1])
        assert np.array_equal(got["energy"][:, 0], got["energy"][:, 1]) and not got["disp2"].any()
    else:
        assert (got["energy"][:, 1] < got["energy"][:, 0]).all()


# ----------------------------------------------------------------------------- state, chunks, repeats
def test_ten_steps_are_four_and_then_six_from_the_same_anchor():
    z, bonds, _, gen, tab = _case(33, 3)
    whole = relax.relax(gen, tab, z, bonds, steps=10, device=DEV)
    first = relax.relax(gen, tab, z, bonds, steps=4, device=DEV)
    second = relax.relax(first["xyz"], tab, z, bonds, steps=6, anchor=gen, device=DEV)
    assert np.array_equal(whole["xyz"].view(np.uint32), second["xyz"].view(np.uint32))
    assert np.array_equal(whole["clashes"][:, 1], second["clashes"][:, 1]) and np.array_equal(whole["clashes"][:, 0], first["clashes"][:, 0])
    assert np.array_equal(whole["energy"][:, 1], second["energy"][:, 1]) and np.array_equal(whole["disp2"], second["disp2"])
    assert np.array_equal(first["energy"][:, 1], second["energy"][:, 0])


def test_chunks_and_repeats_give_the_same_bits():
    z, bonds, _, gen, tab = _case(22, 5)
    base = relax.relax(gen, tab, z, bonds, steps=3, device=DEV)
    for chunk in (1, 2, 5):
        assert _bits(relax.relax(gen, tab, z, bonds, steps=3, chunk=chunk, device=DEV)) == _bits(base), chunk
    assert _bits(relax.relax(gen, tab, z, bonds, steps=3, device=DEV)) == _bits(base)
    kept = relax.relax(torch.from_numpy(gen).to(DEV), tab, z, bonds, steps=3, keep_on_device=True)
    assert kept["xyz"].is_cuda and np.array_equal(kept["xyz"].cpu().numpy(), base["xyz"])


# ----------------------------------------------------------------------------- special inputs
def test_a_structure_with_a_nan_comes_back_unchanged_and_alone():
    z, bonds, _, gen, tab = _case(22, 5)
    base = relax.relax(gen, tab, z, bonds, steps=3, device=DEV)
    marked = gen.copy()
    marked[1, 7, 2], marked[4, 0, 0] = np.nan, np.inf
    got = relax.relax(marked, tab, z, bonds, steps=3, device=DEV)
    assert got["bad"].tolist() == [False, True, False, False, True] and got["n_good"] == 3
    assert np.array_equal(got["xyz"].view(np.uint32), np.where(got["bad"][:, None, None], marked, base["xyz"]).view(np.uint32))
    for k in ("clashes", "energy", "disp2"):
        assert not got[k][got["bad"]].any() and np.array_equal(got[k][~got["bad"]], base[k][~got["bad"]])
    probe = relax.relax(gen[:0], tab, z, bonds, device="cpu")
    _same(got, R.relax32(marked, tab, probe["radii"], probe["excl"], 3), "bad structures")
    held = gen.copy()
    held[2, 3, 1] = np.nan                                            # a non-finite anchor is as bad
    assert relax.relax(gen, tab, z, bonds, steps=1, anchor=held, device=DEV)["bad"].tolist() == [False, False, True, False, False]


def test_an_empty_table_no_clash_at_all_and_everything_excluded():
    z, bonds, _, gen, tab = _case(33, 3)
    n = 33
    probe = relax.relax(gen[:0], tab, z, bonds, device="cpu")
    empty = relax.table_of(np.zeros((0, 2), int), [], [], n)
    _same(relax.relax(gen, empty, z, bonds, steps=3, device=DEV), R.relax32(gen, empty, probe["radii"], probe["excl"], 3), "empty table")
    far = relax.relax(gen, tab, z, bonds, steps=3, tol=3.5, device=DEV)    # c = 3.4 - 3.5 < 0: nothing can clash
    _same(far, R.relax32(gen, tab, probe["radii"], probe["excl"], 3, tol=3.5), "no clash")
    assert not far["clashes"].any()
    shut = relax.relax(gen, tab, z, bonds, steps=3, exclude=n, device=DEV)
    assert shut["excl"].all() and not shut["clashes"].any()
    _same(shut, R.relax32(gen, tab, probe["radii"], np.ones((n, n), bool), 3), "all excluded")
    alone = relax.relax(gen, empty, z, bonds, steps=3, k_pos=0.0, exclude=n, device=DEV)     # h = 0 everywhere
    assert np.array_equal(alone["xyz"], gen) and not alone["energy"].any()


# ----------------------------------------------------------------------------- behaviour
def test_fifty_default_steps_repair_dipeptide_sized_samples():
    c = R.behaviour_case()
    got = relax.relax(c["gen"], c["tab"], c["z"], c["bonds"], steps=50, device=DEV)
    assert np.array_equal(got["radii"], c["radii"]) and np.array_equal(got["excl"], c["excl"])
    R.check_behaviour(c, got["xyz"], got["clashes"], got["disp2"], lambda b, a, exp: relax.stereo_changes(b, a, exp, device=DEV))
    assert np.array_equal(relax.stereo_changes(c["gen"], got["xyz"], c["exp"], device=DEV), R.stereo_changes_host(c["gen"], got["xyz"], c["exp"]))
    ref = lddt.lddt_counts(got["xyz"], c["ref"][:1], c["z"], c["bonds"], ref_index=np.zeros(6, int), atoms="all", device=DEV)
    assert np.array_equal(ref["struct_counts"][:, 5], got["clashes"][:, 1])          # the count lddt reports


# ----------------------------------------------------------------------------- command line
def test_the_command_line_end_to_end(tmp_path, capsys):
    c = R.behaviour_case()
    gen = c["gen"].reshape(3, 2, 34, 3)
    np.savez(tmp_path / "ref.npz", xyz=c["ref"][:3], z=c["z"], bonds=c["bonds"])
    np.savez(tmp_path / "gen.npz", xyz=gen)
    stats = relax.main(f"-gen {tmp_path / 'gen.npz'} -ref {tmp_path / 'ref.npz'} -relax_steps 20 -relaxed {tmp_path / 'relaxed.npz'} "
                       f"-out {tmp_path / 'stats.json'}".split())
    assert tuple(stats) == relax.RELAX_STATS_KEYS
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(line) == {"relax_stats", "out"} and set(line["relax_stats"]) == set(relax.RELAX_STATS_KEYS) - {"params"}
    with open(tmp_path / "stats.json") as f:
        assert json.load(f) == json.loads(json.dumps(stats))
    assert stats["n_gen"] == 6 and stats["params"]["steps"] == 20 and stats["clashes"]["after"]["mean"] < stats["clashes"]["before"]["mean"]
    assert stats["bonds"]["after"] < stats["bonds"]["before"] and stats["bonds"]["ref_even"] < stats["bonds"]["before"]
    assert stats["stereo"]["structures_changed"] == 0 and stats["stereo"]["n_omega"] == 2
    with np.load(tmp_path / "relaxed.npz") as f:
        assert f["xyz"].shape == gen.shape and f["xyz"].dtype == F and f["bad"].shape == (3, 2)
    args = lddt.parser().parse_args(f"-gen {tmp_path / 'relaxed.npz'} -ref {tmp_path / 'ref.npz'}".split())
    inp = lddt.read_inputs(args)                                      # every other tool reads it
    assert inp["gen_xyz"].shape == (6, 34, 3) and inp["ref_index"].tolist() == [0, 0, 1, 1, 2, 2]
