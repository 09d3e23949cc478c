"""The front end the stand-alone command lines share (``compare_cli``): every refusal of ``read_npz`` / ``read_sets`` with
its message, what ``read_sets`` hands back, and how a tool ends; no GPU."""
import argparse
import json
import re

import numpy as np
import pytest

from coarsegrainingvae_amd import compare_cli

Z, BONDS = np.array([6, 6, 8, 7, 1]), np.array([[0, 1], [1, 2], [1, 3], [3, 4]])


def _save(tmp_path, name, **arrays):
    np.savez(tmp_path / name, **arrays)
    return str(tmp_path / name)


def _args(gen, ref, top=None):
    return argparse.Namespace(gen=gen, ref=ref, top=top)


def _refused(message, *a, **kw):
    with pytest.raises(SystemExit, match="^" + re.escape(message) + "$"):
        compare_cli.read_sets(*a, **kw)


@pytest.fixture
def files(tmp_path):
    rng = np.random.default_rng(0)
    return {"ref": _save(tmp_path, "ref.npz", xyz=rng.normal(0, 2, (4, 5, 3)), z=Z, bonds=BONDS, mapping=[0, 0, 1, 1, 1]),
            "gen": _save(tmp_path, "gen.npz", xyz=rng.normal(0, 2, (2, 3, 5, 3)).astype(np.float32)),
            "bare": _save(tmp_path, "bare.npz", xyz=np.zeros((4, 5, 3), np.float32)),
            "z_only": _save(tmp_path, "z_only.npz", xyz=np.zeros((4, 5, 3), np.float32), z=Z)}


def test_read_npz_loads_every_array_and_refuses_a_missing_file_or_key(tmp_path, files):
    got = compare_cli.read_npz(files["ref"], ["xyz", "z"])
    assert sorted(got) == ["bonds", "mapping", "xyz", "z"] and got["z"].tolist() == Z.tolist()
    nothing = str(tmp_path / "nothing.npz")
    with pytest.raises(SystemExit, match="^" + re.escape(f"{nothing}: no such file") + "$"):
        compare_cli.read_npz(nothing, ["xyz"])
    with pytest.raises(SystemExit, match="^" + re.escape(f"{files['bare']}: missing ['bonds', 'z']") + "$"):
        compare_cli.read_npz(files["bare"], ["z", "xyz", "bonds"])


def test_read_sets_refuses_with_the_message_of_the_tools(tmp_path, files):
    gen, ref, bare = files["gen"], files["ref"], files["bare"]
    nothing = str(tmp_path / "nothing.npz")
    _refused(f"{nothing}: no such file", _args(gen, nothing))
    _refused(f"{nothing}: no such file", _args(gen, ref, nothing))
    _refused(f"{nothing}: no such file", _args(nothing, ref))
    _refused(f"{files['z_only']}: missing ['bonds']", _args(gen, ref, files["z_only"]))          # a -top file names itself
    # the topology comes from -ref and is not there: the message names what is needed
    _refused(f"{bare}: missing z (or pass -top)", _args(gen, bare), need=("z",))
    _refused(f"{bare}: missing z / bonds (or pass -top)", _args(gen, bare))
    _refused(f"{files['z_only']}: missing z / bonds (or pass -top)", _args(gen, files["z_only"]))
    compare_cli.read_sets(_args(gen, files["z_only"]), need=("z",))
    # xyz of the wrong width, for -ref and for -gen; a -gen of the wrong rank
    other = _save(tmp_path, "other.npz", z=[6, 6], bonds=[[0, 1]])
    _refused(f"{ref}: xyz is (4, 5, 3), the topology has 2 atoms", _args(gen, ref, other))
    wide = _save(tmp_path, "wide.npz", xyz=np.zeros((3, 6, 3), np.float32))
    _refused(f"{wide}: xyz is (3, 6, 3), the topology has 5 atoms", _args(wide, ref))
    flat = _save(tmp_path, "flat.npz", xyz=np.zeros((5, 3), np.float32))
    _refused(f"{flat}: xyz is (5, 3), the topology has 5 atoms", _args(flat, ref))
    _refused(f"{flat}: xyz is (5, 3), the topology has 5 atoms", _args(gen, flat, ref))
    no_xyz = _save(tmp_path, "no_xyz.npz", z=Z)
    _refused(f"{no_xyz}: missing ['xyz']", _args(no_xyz, ref))
    # one reference frame; the reference is looked at before -gen is opened
    short = _save(tmp_path, "short.npz", xyz=np.zeros((1, 5, 3), np.float32), z=Z, bonds=BONDS)
    _refused(f"{short}: at least two reference frames are needed", _args(gen, short))
    _refused(f"{short}: at least two reference frames are needed", _args(nothing, short))


def test_read_sets_flattens_and_takes_the_topology_from_top_first(tmp_path, files):
    ref_xyz, gen_xyz, z, top, ref = compare_cli.read_sets(_args(files["gen"], files["ref"]))
    assert top is ref and ref_xyz.shape == (4, 5, 3) and ref_xyz.dtype == np.float32          # the file holds float64
    assert z.dtype == np.int64 and z.tolist() == Z.tolist()
    with np.load(files["gen"]) as f:
        want = f["xyz"]
    assert gen_xyz.shape == (6, 5, 3) and gen_xyz.dtype == np.float32 and np.array_equal(gen_xyz, want.reshape(6, 5, 3))
    assert np.array_equal(gen_xyz[4], want[1, 1])                              # [T, K] flattened to T * K, frame-major
    rank3 = _save(tmp_path, "rank3.npz", xyz=want[0])
    assert np.array_equal(compare_cli.read_sets(_args(rank3, files["ref"]))[1], want[0])
    # -top overrides -ref; mapping is found in either
    topf = _save(tmp_path, "top.npz", z=[6, 6, 8, 7, 9], bonds=[[0, 1]])
    _, _, z, top, ref = compare_cli.read_sets(_args(files["gen"], files["ref"], topf))
    assert z.tolist() == [6, 6, 8, 7, 9] and top["bonds"].tolist() == [[0, 1]] and ref["bonds"].tolist() == BONDS.tolist()
    assert "mapping" not in top and top.get("mapping", ref.get("mapping")).tolist() == [0, 0, 1, 1, 1]
    topm = _save(tmp_path, "topm.npz", z=Z, bonds=BONDS, mapping=[0, 1, 2, 3, 4])
    _, _, _, top, ref = compare_cli.read_sets(_args(files["gen"], files["ref"], topm))
    assert top.get("mapping", ref.get("mapping")).tolist() == [0, 1, 2, 3, 4]
    _, _, _, top, ref = compare_cli.read_sets(_args(files["gen"], files["z_only"]), need=("z",))
    assert top.get("mapping", ref.get("mapping")) is None


def test_the_parser_has_the_shared_options_around_a_tools_own():
    p = compare_cli.base_parser("python -m tool", "what it does", top_help="npz with z")
    p.add_argument("-own", type=int, default=3)
    p = compare_cli.finish_parser(p, "tool_stats.json")
    assert [a.dest for a in p._actions] == ["help", "gen", "ref", "top", "own", "out", "device"]
    args = p.parse_args("-gen g.npz -ref r.npz".split())
    assert (args.gen, args.ref, args.top, args.own, args.out, args.device) == ("g.npz", "r.npz", None, 3, "tool_stats.json", "cuda")
    assert "(tool_stats.json)" in p.format_help() and p.prog == "python -m tool"
    with pytest.raises(SystemExit):
        p.parse_args(["-gen", "g.npz"])                                        # -ref is required


def test_refusing_turns_a_value_error_into_the_exit_message():
    with pytest.raises(SystemExit, match="^-groups bead: no mapping$"):
        with compare_cli.refusing("-groups bead: "):
            raise ValueError("no mapping")
    with pytest.raises(SystemExit, match="^no mapping$"):
        with compare_cli.refusing():
            raise ValueError("no mapping")
    with pytest.raises(KeyError):                                              # nothing else is caught
        with compare_cli.refusing():
            raise KeyError("z")
    with compare_cli.refusing():
        kept = 1
    assert kept == 1


def test_finish_writes_the_file_and_prints_one_line(tmp_path, capsys):
    out = str(tmp_path / "tool_stats.json")
    stats = {"n_ref": 4, "profile": [0.5, None], "params": {"probe": 1.4}}
    assert compare_cli.finish("tool", stats, {"n_ref": 4}, out) is None
    with open(out) as f:
        assert json.load(f) == stats
    printed = capsys.readouterr().out
    assert printed.endswith("\n") and printed.count("\n") == 1
    line = json.loads(printed)
    assert list(line) == ["tool_stats", "out"] and line == {"tool_stats": {"n_ref": 4}, "out": out}
