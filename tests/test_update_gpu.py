"""The UpdateBlock kernels (K5) called directly and through ops.update_block, against tests/update_restatement.py in fp64:
the six element-wise launches of csrc/update.hip at ld = F and ld = 2 F, the NormStackOut store epilogue of tile_bwd_input_k
(cgv_tile_linear_bwd_input_norm_stack) on every register-tile variant, and the block end to end on the composition path and
on every route of the fused node.  Every comparison is element by element within the a-priori bound the restatement returns
beside the value (operation counts x 2^-24 x the terms' magnitudes; tests/test_update_cpu.py pins that file); every output
sits between 64-float canaries on either side.  Each check prints its largest error / bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
import update_restatement as R
from coarsegrainingvae_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0x7FC0BEEF           # a quiet NaN with a payload: an element left unwritten fails its comparison too
PAD = 64


class Padded:
    """a float32 tensor of ``shape`` with PAD canary floats on either side of it, itself canary-filled"""

    def __init__(self, *shape, init=None):
        numel = int(np.prod(shape))
        self.full = torch.full((numel + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
        self.t = self.full[PAD:PAD + numel].view(torch.float32).view(*shape)
        if init is not None:
            self.t.copy_(dev(init).view(*shape))

    def intact(self):
        return bool((self.full[:PAD] == CANARY).all()) and bool((self.full[-PAD:] == CANARY).all())

    def np(self):
        assert self.intact(), "canary overwritten"
        return self.t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(got, ref, what):
    """element by element inside the bound (a zero bound: equality); prints the largest error / bound"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    got = got.astype(np.float64).reshape(ref.val.shape)
    err = np.abs(got - ref.val)
    ratio = float((err[ref.err > 0] / ref.err[ref.err > 0]).max()) if (ref.err > 0).any() else 0.0
    print(f"ratio {what}: {ratio:.3f}")
    bad = ~(err <= ref.err)                                      # (a NaN is bad)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside their bound, worst {ratio:.3g} x the bound"


def within_two_bounds(a, b, ref, what):
    a, b = (t.detach().cpu().double().numpy().reshape(ref.val.shape) for t in (a, b))
    assert (np.abs(a - b) <= 2 * ref.err).all(), what


def call(name, *args):
    _lib.call(name, *args, _lib.stream_ptr())


P = _lib.ptr


# ------------------------------------------------------------------------------------------------ element-wise kernels
def _strided(U, Vv, n, F, ld):
    """device operands at row stride ld: (U pointer, Vv pointer, the host buffers and columns the restatement reads)"""
    Ub, uc, Vb, vc = R.as_buffers(U, Vv, n, F, ld)
    if ld == F:
        tu, tv = dev(Ub), dev(Vb)
        return (tu, tv), tu.data_ptr(), tv.data_ptr(), Ub, uc, Vb, vc
    t = dev(Ub)
    return (t,), t.data_ptr(), t.data_ptr() + 4 * F, Ub, uc, Vb, vc


def _out_pair(n, F, ld, init_u=None, init_v=None):
    """gU / gVv outputs at row stride ld: two padded buffers, or the halves of one.  Returns (buffers, gU ptr, gVv ptr, read)"""
    if ld == F:
        bu, bv = Padded(3 * n, F, init=init_u), Padded(3 * n, F, init=init_v)
        return (bu, bv), bu.t.data_ptr(), bv.t.data_ptr(), lambda: (bu.np().reshape(n, 3, F), bv.np().reshape(n, 3, F))
    init = None if init_u is None else np.concatenate([init_u.reshape(n, 3, F), init_v.reshape(n, 3, F)], 2)
    b = Padded(3 * n, 2 * F, init=init)

    def read():
        x = b.np().reshape(n, 3, 2 * F)
        return x[:, :, :F], x[:, :, F:]
    return (b,), b.t.data_ptr(), b.t.data_ptr() + 4 * F, read


@pytest.mark.parametrize("wide", [False, True], ids=["ld=F", "ld=2F"])
@pytest.mark.parametrize("n,F", R.ELEMENTWISE_SHAPES)
def test_elementwise_launches_vs_fp64(n, F, wide):
    ld = 2 * F if wide else F
    d = R.elementwise_inputs(n, F)
    keep, pU, pV, Ub, uc, Vb, vc = _strided(d["U"], d["Vv"], n, F, ld)
    t = {k: dev(x) for k, x in d.items()}
    # rows_from_vec, vec_from_rows: copies, and their round trip returns the input bits
    rows, back, vec = Padded(3 * n, F), Padded(n, F, 3), Padded(n, F, 3)
    call("cgv_update_rows_from_vec", P(t["v"]), P(rows.t), n, F)
    call("cgv_update_vec_from_rows", P(rows.t), None, P(back.t), n, F)
    assert np.array_equal(rows.np().view(np.int32), R.rows_from_vec(d["v"], n, F).val.astype(np.float32).view(np.int32))
    assert np.array_equal(back.np().view(np.int32), d["v"].view(np.int32))
    call("cgv_update_vec_from_rows", P(t["old"]), P(t["v"]), P(vec.t), n, F)
    check(vec.np(), R.vec_from_rows(d["old"].reshape(3 * n, F), n, F, d["v"]), "vec_from_rows")
    # norm_stack_fwd
    stack = Padded(n, 2 * F)
    call("cgv_update_norm_stack_fwd", P(t["s"]), pV, P(stack.t), n, F, ld)
    stack_h = stack.np()
    check(stack_h, R.norm_stack_fwd(d["s"], Vb, n, F, ld, vc), "norm_stack_fwd")
    assert np.array_equal(stack_h[:, :F], d["s"])
    # norm_stack_bwd: the U half of an interleaved buffer survives, with and without accumulation
    u_old = d["U"][::-1].copy()
    oldb = R.as_buffers(u_old, d["old"], n, F, ld)[2]
    for g_res in (None, "g_res"):
        for acc in (0, 1):
            g_s = Padded(n, F)
            bufs, pgU, pgV, read = _out_pair(n, F, ld, u_old, d["old"])
            call("cgv_update_norm_stack_bwd", P(t["gstack"]), pV, P(stack.t), P(t[g_res]) if g_res else None, P(g_s.t), pgV, n, F, ld, acc)
            ref_s, ref_v = R.norm_stack_bwd(d["gstack"], Vb, stack_h, n, F, ld, vc, d[g_res] if g_res else None, oldb, acc)
            gU_after, gVv = read()
            check(g_s.np(), ref_s, f"norm_stack_bwd g_s res={g_res is not None}")
            check(gVv, ref_v, f"norm_stack_bwd gVv acc={acc}")
            assert np.array_equal(gU_after.view(np.int32), u_old.view(np.int32)), "the other half / buffer was written"
    # gate_fwd with and without the residual
    for res in (False, True):
        ds, dv = Padded(n, F), Padded(n, F, 3)
        call("cgv_update_gate_fwd", pU, pV, P(t["a"]), P(t["s"]) if res else None, P(t["v"]) if res else None, P(ds.t), P(dv.t), n, F, ld)
        ref_ds, ref_dv = R.gate_fwd(Ub, Vb, d["a"], n, F, ld, uc, vc, d["s"] if res else None, d["v"] if res else None)
        check(ds.np(), ref_ds, f"gate_fwd ds res={res}")
        check(dv.np(), ref_dv, f"gate_fwd dv res={res}")
    # gate_bwd with either or both upstream gradients absent
    for g_ds, g_dv in (("g_ds", "g_dv"), (None, "g_dv"), ("g_ds", None), (None, None)):
        ga = Padded(n, 3 * F)
        bufs, pgU, pgV, read = _out_pair(n, F, ld)
        call("cgv_update_gate_bwd", pU, pV, P(t["a"]), P(t[g_ds]) if g_ds else None, P(t[g_dv]) if g_dv else None, pgU, pgV, P(ga.t), n, F, ld)
        refs = R.gate_bwd(Ub, Vb, d["a"], n, F, ld, uc, vc, d[g_ds] if g_ds else None, d[g_dv] if g_dv else None)
        gU, gVv = read()
        for got, ref, name in zip((gU, gVv, ga.np()), refs, ("gU", "gVv", "ga")):
            check(got, ref, f"gate_bwd {name} g_ds={g_ds is not None} g_dv={g_dv is not None}")
        if g_ds is None:                                         # everything that carries g_ds is exactly zero
            assert not gVv.any() and not ga.np()[:, F:].any()
            if g_dv is None:
                assert not gU.any() and not ga.np().any()
        # ... then the norm / stack backward on top of what the gate left (the fused node's order)
        if g_ds and g_dv:
            gate_h = np.concatenate([gU, gVv], 2).reshape(3 * n, 2 * F).copy() if wide else gVv.reshape(3 * n, F).copy()
            gU_before = gU.copy()
            g_s = Padded(n, F)
            call("cgv_update_norm_stack_bwd", P(t["gstack"]), pV, P(stack.t), None, P(g_s.t), pgV, n, F, ld, 1)
            _, ref_v = R.norm_stack_bwd(d["gstack"], Vb, stack_h, n, F, ld, vc, None, gate_h, 1)
            gU2, gVv2 = read()
            assert np.array_equal(gU2.view(np.int32), gU_before.view(np.int32)), "gU changed under the norm / stack backward"
            check(gVv2, ref_v, "gate_bwd + norm_stack_bwd accumulate=1")
            call("cgv_update_norm_stack_bwd", P(t["gstack"]), pV, P(stack.t), None, P(g_s.t), pgV, n, F, ld, 0)
            _, ref_v = R.norm_stack_bwd(d["gstack"], Vb, stack_h, n, F, ld, vc, None, None, 0)
            gU3, gVv3 = read()
            assert np.array_equal(gU3.view(np.int32), gU_before.view(np.int32))
            check(gVv3, ref_v, "gate_bwd + norm_stack_bwd accumulate=0")
    torch.cuda.synchronize()
    del keep


def test_gate_fwd_refuses_one_residual_pointer_without_the_other():
    n, F = 3, 20
    d = {k: dev(x) for k, x in R.elementwise_inputs(n, F).items()}
    ds, dv = Padded(n, F), Padded(n, F, 3)
    lib = _lib.load()
    for s_res, v_res in ((P(d["s"]), None), (None, P(d["v"]))):
        rc = lib.cgv_update_gate_fwd(P(d["U"]), P(d["Vv"]), P(d["a"]), s_res, v_res, P(ds.t), P(dv.t), n, F, F, _lib.stream_ptr())
        assert rc != 0 and b"s_res and v_res go together" in lib.cgv_last_error_string()
    torch.cuda.synchronize()
    assert bool((ds.full == CANARY).all()) and bool((dv.full == CANARY).all()), "something was launched"


# ------------------------------------------------------------------------------------------------ fused epilogue
def _plan(M, N, K):
    shares, sk = C.c_int(0), C.c_int(0)
    assert _lib.load().cgv_tile_bwd_input_plan(M, N, K, 1, C.byref(shares), C.byref(sk)) == 0
    return shares.value, sk.value


def _epilogue_case(M, F, direct):
    """every (act, g_res, accumulate) at ld = 2 F: the fused launch against fp64, and against product + element-wise launch.
    ``direct``: call the library itself (the caller has set the calling thread's workspace registration), else _lib.call."""
    N, K = F, 2 * F
    d = R.epilogue_inputs(M, F)
    t = {k: dev(x) for k, x in d.items()}
    both_h = np.concatenate([d["U"], d["Vv"]], 2).reshape(3 * M, K)
    old_h = np.concatenate([d["U"][::-1], d["old"]], 2).reshape(3 * M, K)
    both = dev(both_h)
    pV = both.data_ptr() + 4 * F
    stack = dev(d["stack"])
    lib, st = _lib.load(), _lib.stream_ptr()

    def run(name, *args):
        if direct:
            assert getattr(lib, name)(*args, st) == 0, lib.cgv_last_error_string()
        else:
            _lib.call(name, *args, st)

    first = None
    for act in (0, 1):
        z = P(t["z"]) if act else None
        for g_res in (None, t["g_res"]):
            for acc in (0, 1):
                what = f"M={M} F={F} act={act} g_res={g_res is not None} acc={acc}"
                g_s, gUV = Padded(M, F), Padded(3 * M, K, init=old_h)
                run("cgv_tile_linear_bwd_input_norm_stack", P(t["gy"]), z, P(t["W"]), M, N, K, act, P(stack), pV, P(g_res), P(g_s.t),
                    gUV.t.data_ptr() + 4 * F, K, acc)
                ref_s, ref_v = R.bwd_input_norm_stack(d["gy"], d["z"] if act else None, d["W"], d["stack"], both_h, M, F, K, F,
                                                      None if g_res is None else d["g_res"], old_h, acc)
                out = gUV.np().reshape(M, 3, K)
                check(g_s.np(), ref_s, "epilogue g_s " + what)
                check(out[:, :, F:], ref_v, "epilogue gVv " + what)
                assert np.array_equal(out[:, :, :F].view(np.int32), d["U"][::-1].view(np.int32)), "the gU half was written"
                # the same through the product and the element-wise launch
                g_stack, g_s2, gUV2 = Padded(M, K), Padded(M, F), Padded(3 * M, K, init=old_h)
                if act:
                    run("cgv_tile_linear_bwd_input_act", P(t["gy"]), z, P(t["W"]), P(g_stack.t), M, N, K, act)
                else:
                    run("cgv_tile_linear_bwd_input", P(t["gy"]), P(t["W"]), P(g_stack.t), M, N, K)
                _lib.call("cgv_update_norm_stack_bwd", P(g_stack.t), pV, P(stack), P(g_res), P(g_s2.t), gUV2.t.data_ptr() + 4 * F, M, F, K,
                          acc, st)
                assert g_stack.intact()
                check(g_s2.np(), ref_s, "separate g_s " + what)
                check(gUV2.np().reshape(M, 3, K)[:, :, F:], ref_v, "separate gVv " + what)
                within_two_bounds(g_s.t, g_s2.t, ref_s, "fused against separate g_s " + what)
                within_two_bounds(gUV.t.view(M, 3, K)[:, :, F:], gUV2.t.view(M, 3, K)[:, :, F:], ref_v, "fused against separate gVv " + what)
                if first is None:
                    first = (g_s.t.clone(), gUV.t.clone())
    # the first case once more: bit-identical (a split reduction adds its shares in share order; tickets reset themselves)
    g_s, gUV = Padded(M, F), Padded(3 * M, K, init=old_h)
    run("cgv_tile_linear_bwd_input_norm_stack", P(t["gy"]), None, P(t["W"]), M, N, K, 0, P(stack), pV, None, P(g_s.t),
        gUV.t.data_ptr() + 4 * F, K, 0)
    assert torch.equal(g_s.t, first[0]) and torch.equal(gUV.t.view(torch.int32), first[1].view(torch.int32))
    torch.cuda.synchronize()


@pytest.mark.parametrize("tag,M,F", R.EPILOGUE_SHAPES[:-1], ids=[s[0] for s in R.EPILOGUE_SHAPES[:-1]])
def test_norm_stack_epilogue_vs_fp64_on_the_8_and_4_wave_tiles(tag, M, F):
    """BWD_R16_W8 with row tails mod 16 and a 64-column tile across column F (F = 36), BWD_R32_W8 (200 .. 511 32-row tiles)
    and BWD_R32_W4 (>= 512) with a row tail mod 32; the plan reports neither a split nor the stream-K kernel for them."""
    assert _plan(M, F, 2 * F) == (1, 0)
    _epilogue_case(M, F, direct=False)


@pytest.mark.parametrize("workspace", [False, True], ids=["no-workspace", "split"])
def test_norm_stack_epilogue_vs_fp64_on_the_16_wave_tile(workspace):
    """BWD_R16_W16 (96 output tiles, a 1024-deep reduction): unsplit without a registered workspace; with one the plan
    reports more than one share, SplitN feeds the epilogue, and the tickets are zero again afterwards."""
    _, M, F = R.EPILOGUE_SHAPES[-1]
    lib, st = _lib.load(), _lib.stream_ptr()
    ws = torch.zeros(64 * 1024 + 8 * 1024 * 1024, dtype=torch.uint8, device=DEV)
    try:
        assert lib.cgv_tile_bwd_input_split(ws.data_ptr() if workspace else None, ws.numel() if workspace else 0, st) == 0
        _lib._SPLIT_TLS.cur = None                               # (this thread's registration was replaced just above)
        if workspace:
            shares, sk = _plan(M, F, 2 * F)
            assert shares > 1 and sk == 0
        _epilogue_case(M, F, direct=True)
        torch.cuda.synchronize()
        assert not ws[:64 * 1024].any(), "tickets not reset"
        assert bool(ws[64 * 1024:].any()) == workspace, "partial tiles written exactly when the reduction is split"
    finally:
        lib.cgv_tile_bwd_input_split(None, 0, st)
        _lib._SPLIT_TLS.cur = None


def test_norm_stack_epilogue_refuses_misaligned_vv_and_odd_halves():
    M, F = 17, 36
    d = {k: dev(x) for k, x in R.epilogue_inputs(M, F).items()}
    both = torch.zeros(3 * M * 2 * F + 8, device=DEV)
    g_s, gUV = Padded(M, F), Padded(3 * M, 2 * F)
    lib, st = _lib.load(), _lib.stream_ptr()
    rc = lib.cgv_tile_linear_bwd_input_norm_stack(P(d["gy"]), None, P(d["W"]), M, F, 2 * F, 0, P(d["stack"]), both.data_ptr() + 4, None,
                                                  P(g_s.t), gUV.t.data_ptr() + 4 * F, 2 * F, 0, st)
    assert rc != 0 and b"16-byte aligned" in lib.cgv_last_error_string()
    # K = 36 = 2 x 18: a multiple of 4 (a shape the tile kernels take) whose halves are not
    rc = lib.cgv_tile_linear_bwd_input_norm_stack(P(d["gy"]), None, P(d["W"]), M, F, 36, 0, P(d["stack"]), both.data_ptr(), None,
                                                  P(g_s.t), gUV.t.data_ptr(), 36, 0, st)
    assert rc != 0 and b"unsupported shape" in lib.cgv_last_error_string()
    torch.cuda.synchronize()
    assert bool((g_s.full == CANARY).all()) and bool((gUV.full == CANARY).all()), "something was launched"


# ------------------------------------------------------------------------------------------------ ops.update_block end to end
GRADS = ("g_u", "g_vw", "g_W0", "g_b0", "g_W1", "g_b1")


def _block(F, seed):
    torch.manual_seed(seed)
    blk = cg.UpdateBlock(F, "swish", 0.0).to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.2)
    return blk


def _params(blk):
    ps = (blk.u_mat.weight, blk.v_mat.weight, blk.s_dense[0].weight, blk.s_dense[0].bias, blk.s_dense[1].weight, blk.s_dense[1].bias)
    return ps, {k: p.detach().cpu().double().numpy() for k, p in zip(R.PARAMS, ps)}


def _block_inputs(n, F):
    g = np.random.default_rng(n * 131 + F)
    rnd = lambda *sh: g.standard_normal(sh).astype(np.float32)
    v = rnd(n, F, 3)
    v[0] = 0.0                                                   # ||Vv||_eps = sqrt(3e-10): the backward divides by it
    v[1] *= np.float32(1e-6)
    return rnd(n, F), v, rnd(n, F), rnd(n, F, 3)


def _run(blk, s, v, gs, gv, residual, drive, arena=None, rows=None):
    ps, _ = _params(blk)
    if arena is None:
        for p in ps:
            p.grad = None
    else:
        arena.g.fill_(float("nan"))
        for p in ps:
            p.grad.fill_(float("nan"))
        arena.zero_grad()
    s1, v1 = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
    if rows is not None:
        v1._cgv_rows = rows
    ds, dv = blk(s1, v1, residual=residual)
    loss = 0.0
    if drive != "vector":
        loss = loss + (ds * gs).sum()
    if drive != "scalar":
        loss = loss + (dv * gv).sum()                            # "scalar": dv unused, g_dv is None in the node's backward
    loss.backward()
    out = {"ds": ds.detach(), "dv": dv.detach(), "g_s": s1.grad, "g_v": v1.grad}
    out.update({k: p.grad.clone() for k, p in zip(GRADS, ps)})
    return out


def _check_block(got, ref, what):
    for k, r in ref.items():
        check(got[k], r, f"block {k} {what}")


DRIVES = ("both", "scalar", "vector")


@pytest.mark.parametrize("F", [8, 52])
def test_update_block_composition_path_vs_fp64(F):
    """parameters outside an arena: tensor-op composition around _UpdateNormStack / _UpdateGate (ld = F)"""
    from coarsegrainingvae_amd.ops import _UpdateBlockFused
    n = 13
    blk = _block(F, 5)
    ps, params = _params(blk)
    sh, vh, gsh, gvh = _block_inputs(n, F)
    s, v, gs, gv = (dev(x) for x in (sh, vh, gsh, gvh))
    assert not _UpdateBlockFused.usable(s, v, ps[0], ps[1], blk.s_dense[0], blk.s_dense[1])
    for residual in (False, True):
        for drive in DRIVES:
            ref = R.block(sh, vh, params, residual, gsh if drive != "vector" else None, gvh if drive != "scalar" else None)
            _check_block(_run(blk, s, v, gs, gv, residual, drive), ref, f"composition F={F} residual={residual} {drive}")


def _arena(blk):
    """ParamArena over the block; where F x F is no multiple of the arena's 64-float alignment (F = 36) the [u_mat; v_mat]
    pair, which the fused node needs back to back, is packed by hand in a buffer of its own"""
    from coarsegrainingvae_amd.ops import _adjacent
    from coarsegrainingvae_amd.trainer import ParamArena
    params = list(blk.parameters())
    arena = ParamArena(params)
    u, vw = blk.u_mat.weight, blk.v_mat.weight
    if not _adjacent(u, vw):
        m = u.numel()
        arena.pair = (torch.zeros(2 * m, device=DEV), torch.zeros(2 * m, device=DEV))
        for i, p in enumerate((u, vw)):
            arena.pair[0][i * m:(i + 1) * m].copy_(p.data.reshape(-1))
            p.data = arena.pair[0][i * m:(i + 1) * m].view_as(p)
            p.grad = arena.pair[1][i * m:(i + 1) * m].view_as(p)
            arena.grad_views[[j for j, x in enumerate(params) if x is p][0]] = p.grad
    return arena


@pytest.mark.parametrize("F", [36, 128])
@pytest.mark.parametrize("n,split_ready", [(12, True), (40, True), (40, False), (96, True)],
                         ids=["12-skinny", "40-epilogue", "40-separate", "96-tile"])
def test_fused_update_block_vs_fp64(n, split_ready, F, options):
    """_UpdateBlockFused on its routes: 12 beads the skinny kernels and the element-wise norm / stack backward, 40 the epilogue
    where the split workspace is ready and product + launch where it is not, 96 the tile kernels and the epilogue; residual
    on / off, three backward drives, update_fused_bwd on / off; a ``_cgv_rows`` hint changes no bit."""
    from coarsegrainingvae_amd.ops import _UpdateBlockFused
    blk = _block(F, 7)
    sh, vh, gsh, gvh = _block_inputs(n, F)
    s, v, gs, gv = (dev(x) for x in (sh, vh, gsh, gvh))
    _run(blk, s, v, gs, gv, False, "both")                       # the composition once: its backward marks the direct-write parameters
    arena = _arena(blk)
    ps, params = _params(blk)
    assert _UpdateBlockFused.usable(s, v, ps[0], ps[1], blk.s_dense[0], blk.s_dense[1])
    if not split_ready:
        options.set("bwd_input_split", 1)
    assert _lib.split_workspace_ready() == split_ready
    for residual in (False, True):
        for drive in DRIVES:
            ref = R.block(sh, vh, params, residual, gsh if drive != "vector" else None, gvh if drive != "scalar" else None)
            got = {}
            for fused_bwd in (1, 0):
                options.set("update_fused_bwd", fused_bwd)
                got[fused_bwd] = _run(blk, s, v, gs, gv, residual, drive, arena)
                _check_block(got[fused_bwd], ref, f"fused n={n} F={F} residual={residual} {drive} update_fused_bwd={fused_bwd}")
            for k, r in ref.items():
                within_two_bounds(got[1][k], got[0][k], r, f"update_fused_bwd on against off: {k}")
    options.set("update_fused_bwd", 1)
    plain = _run(blk, s, v, gs, gv, True, "both", arena)
    exact = v.transpose(1, 2).reshape(3 * n, F).contiguous()
    for rows in (exact, exact[:-1], torch.zeros(3 * n, F + 4, device=DEV)):     # the transposition; two wrong shapes: ignored
        hinted = _run(blk, s, v, gs, gv, True, "both", arena, rows=rows)
        for k, x in plain.items():
            assert torch.equal(x.view(torch.int32), hinted[k].view(torch.int32)), f"_cgv_rows {tuple(rows.shape)}: {k}"
    torch.cuda.synchronize()
