"""tests/update_restatement.py pinned without a GPU: its forward to oracle.cgvae_oracle.update_block in fp64, its hand-written
backward to torch autograd of that oracle, and its a-priori fp32 bounds to the kernels' formulas executed in numpy.float32
in the kernels' operation order -- inside the bounds on every input tests/test_update_gpu.py uses, and not vacuously so."""
import numpy as np
import pytest
import torch

import update_restatement as R
from oracle import cgvae_oracle as O


def _block_inputs(n, F, seed, zero_rows=False):
    g = np.random.default_rng(seed)
    rnd = lambda *sh: g.standard_normal(sh)
    params = {"u": rnd(F, F) / F ** 0.5, "vw": rnd(F, F) / F ** 0.5, "W0": rnd(F, 2 * F) / (2 * F) ** 0.5, "b0": 0.2 * rnd(F),
              "W1": rnd(3 * F, F) / F ** 0.5, "b1": 0.2 * rnd(3 * F)}
    s, v = rnd(n, F), rnd(n, F, 3)
    if zero_rows:
        v[0] = 0.0
        v[n - 1] = 0.0
    return s, v, params, rnd(n, F), rnd(n, F, 3)


def _oracle(s, v, params, residual):
    P = {"b.u_mat.weight": params["u"], "b.v_mat.weight": params["vw"], "b.s_dense.0.weight": params["W0"],
         "b.s_dense.0.bias": params["b0"], "b.s_dense.1.weight": params["W1"], "b.s_dense.1.bias": params["b1"]}
    P = {k: torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True) for k, x in P.items()}
    st, vt = torch.from_numpy(s).requires_grad_(True), torch.from_numpy(v).requires_grad_(True)
    ds, dv = O.update_block(st, vt, P, "b", O.swish)
    if residual:
        ds, dv = st + ds, vt + dv                                # cgvae.py:122-123
    return st, vt, P, ds, dv


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n,F", [(1, 4), (5, 7), (13, 36)])
def test_restatement_forward_equals_the_oracle(n, F, residual):
    s, v, params, _, _ = _block_inputs(n, F, 11 * n + F, zero_rows=n > 1)
    _, _, _, ds, dv = _oracle(s, v, params, residual)
    out = R.block(s, v, params, residual, backward=False)
    assert _rel(out["ds"].val, ds.detach().numpy()) <= 1e-13
    assert _rel(out["dv"].val, dv.detach().numpy()) <= 1e-13


@pytest.mark.parametrize("zero_rows", [False, True], ids=["normal", "zero-v-rows"])
@pytest.mark.parametrize("drive", ["both", "scalar", "vector"])
@pytest.mark.parametrize("residual", [False, True])
def test_restatement_backward_equals_autograd_of_the_oracle(residual, drive, zero_rows):
    n, F = 6, 8
    s, v, params, g_ds, g_dv = _block_inputs(n, F, 5, zero_rows)
    g_ds, g_dv = (g_ds if drive != "vector" else None), (g_dv if drive != "scalar" else None)
    st, vt, P, ds, dv = _oracle(s, v, params, residual)
    loss = 0.0
    if g_ds is not None:
        loss = loss + (ds * torch.from_numpy(g_ds)).sum()
    if g_dv is not None:
        loss = loss + (dv * torch.from_numpy(g_dv)).sum()
    loss.backward()
    out = R.block(s, v, params, residual, g_ds, g_dv)
    want = {"g_s": st.grad, "g_v": vt.grad, "g_u": P["b.u_mat.weight"].grad, "g_vw": P["b.v_mat.weight"].grad,
            "g_W0": P["b.s_dense.0.weight"].grad, "g_b0": P["b.s_dense.0.bias"].grad, "g_W1": P["b.s_dense.1.weight"].grad,
            "g_b1": P["b.s_dense.1.bias"].grad}
    for k, ref in want.items():
        assert _rel(out[k].val, ref.numpy()) <= 1e-12, k
    if zero_rows:
        assert np.isfinite(out["g_v"].val).all()


# ------------------------------------------------------------------------------------------------ the bounds
def _ratio(got32, ref, what, worst):
    """got32 inside ref's bound element by element (a zero bound: equality); records the largest error / bound"""
    err = np.abs(got32.astype(np.float64) - ref.val)
    assert err.shape == ref.err.shape, what
    bad = err > ref.err
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside their bound, worst {float((err / np.maximum(ref.err, 1e-300)).max()):.3g} x"
    nz = ref.err > 0
    if nz.any():
        worst[what] = max(worst.get(what, 0.0), float((err[nz] / ref.err[nz]).max()))


def _elementwise_fp32(n, F, ld, worst):
    d = R.elementwise_inputs(n, F)
    Ub, uc, Vb, vc = R.as_buffers(d["U"], d["Vv"], n, F, ld)
    stack32 = R.norm_stack_fwd_fp32(d["s"], d["Vv"])
    _ratio(stack32, R.norm_stack_fwd(d["s"], Vb, n, F, ld, vc), "norm_stack_fwd", worst)
    oldb = R.as_buffers(d["old"], d["old"], n, F, ld)[2]
    for g_res in (None, d["g_res"]):
        for acc in (0, 1):
            gs32, gv32 = R.norm_stack_bwd_fp32(d["gstack"], d["Vv"], stack32, g_res, d["old"] if acc else None)
            g_s, gVv = R.norm_stack_bwd(d["gstack"], Vb, stack32, n, F, ld, vc, g_res, oldb, acc)
            _ratio(gs32, g_s, "norm_stack_bwd g_s", worst)
            _ratio(gv32, gVv, "norm_stack_bwd gVv", worst)
    for res in (False, True):
        ds32, dv32 = R.gate_fwd_fp32(d["U"], d["Vv"], d["a"], d["s"] if res else None, d["v"] if res else None)
        ds, dv = R.gate_fwd(Ub, Vb, d["a"], n, F, ld, uc, vc, d["s"] if res else None, d["v"] if res else None)
        _ratio(ds32, ds, "gate_fwd ds", worst)
        _ratio(dv32, dv, "gate_fwd dv", worst)
    for g_ds, g_dv in ((d["g_ds"], d["g_dv"]), (None, d["g_dv"]), (d["g_ds"], None), (None, None)):
        got = R.gate_bwd_fp32(d["U"], d["Vv"], d["a"], g_ds, g_dv)
        ref = R.gate_bwd(Ub, Vb, d["a"], n, F, ld, uc, vc, g_ds, g_dv)
        for g32, r, name in zip(got, ref, ("gU", "gVv", "ga")):
            _ratio(g32, r, "gate_bwd " + name, worst)
    rows = R.rows_from_vec(d["v"], n, F)
    assert not rows.err.any() and np.array_equal(R.vec_from_rows(rows, n, F).val, d["v"].astype(np.float64))
    vec32 = d["old"].transpose(0, 2, 1) + d["v"]
    _ratio(vec32, R.vec_from_rows(d["old"].reshape(3 * n, F), n, F, d["v"]), "vec_from_rows", worst)


def test_kernel_formulas_in_float32_stay_inside_the_bounds_and_the_bounds_are_not_vacuous():
    """Every element-wise launch on every (shape, ld) of the GPU test, in numpy.float32 in the kernels' operation order:
    inside its bound, and the largest error / bound per output above 1/64 -- a condition on the bounds' tightness (a count
    inflated a thousandfold fails it), not a measurement."""
    worst = {}
    for n, F in R.ELEMENTWISE_SHAPES:
        for ld in (F, 2 * F):
            _elementwise_fp32(n, F, ld, worst)
    print({k: round(x, 3) for k, x in worst.items()})
    assert len(worst) == 9
    for what, x in worst.items():
        assert 1.0 / 64 < x <= 1.0, (what, x)


@pytest.mark.parametrize("tag,M,F", R.EPILOGUE_SHAPES, ids=[t for t, _, _ in R.EPILOGUE_SHAPES])
def test_epilogue_formulas_in_float32_stay_inside_the_bounds(tag, M, F):
    """The fused epilogue's inputs: the product in float32 (numpy's own summation order: the bound is the any-order one),
    Swish' and the norm / stack backward in the kernel's order."""
    d = R.epilogue_inputs(M, F)
    both = np.concatenate([d["U"], d["Vv"]], 2).reshape(3 * M, 2 * F)
    oldb = np.concatenate([d["U"], d["old"]], 2).reshape(3 * M, 2 * F)
    worst = {}
    for act in (0, 1):
        g32 = d["gy"] * R.swish_prime_fp32(d["z"]) if act else d["gy"]
        gstack32 = g32 @ d["W"]
        for g_res in (None, d["g_res"]):
            for acc in (0, 1):
                gs32, gv32 = R.norm_stack_bwd_fp32(gstack32, d["Vv"], d["stack"], g_res, d["old"] if acc else None)
                g_s, gVv = R.bwd_input_norm_stack(d["gy"], d["z"] if act else None, d["W"], d["stack"], both, M, F, 2 * F, F, g_res,
                                                  oldb, acc)
                _ratio(gs32, g_s, "g_s", worst)
                _ratio(gv32, gVv, "gVv", worst)
    print(tag, worst)
    # the any-order bound grows with N where random roundings grow with sqrt(N): the tightness condition is asked of the
    # short reductions only
    if F == 36:
        assert max(worst.values()) > 1.0 / 64


def test_block_bounds_cover_a_float32_run_of_the_oracle():
    """The composed bounds of ``block`` against the oracle run in torch.float32 (another operation order, the same count
    class), outputs and every gradient, with zero and tiny rows of v."""
    n, F = 13, 36
    s, v, params, g_ds, g_dv = _block_inputs(n, F, 3)
    v[0], v[1] = 0.0, v[1] * 1e-6
    s, v, g_ds, g_dv = (x.astype(np.float32) for x in (s, v, g_ds, g_dv))
    params = {k: x.astype(np.float32) for k, x in params.items()}
    for residual in (False, True):
        out = R.block(s.astype(np.float64), v.astype(np.float64), params, residual, g_ds, g_dv)
        P = {"b.u_mat.weight": params["u"], "b.v_mat.weight": params["vw"], "b.s_dense.0.weight": params["W0"],
             "b.s_dense.0.bias": params["b0"], "b.s_dense.1.weight": params["W1"], "b.s_dense.1.bias": params["b1"]}
        P = {k: torch.from_numpy(x).requires_grad_(True) for k, x in P.items()}
        st, vt = torch.from_numpy(s).requires_grad_(True), torch.from_numpy(v).requires_grad_(True)
        ds, dv = O.update_block(st, vt, P, "b", O.swish)
        if residual:
            ds, dv = st + ds, vt + dv
        ((ds * torch.from_numpy(g_ds)).sum() + (dv * torch.from_numpy(g_dv)).sum()).backward()
        got = {"ds": ds, "dv": dv, "g_s": st.grad, "g_v": vt.grad, "g_u": P["b.u_mat.weight"].grad, "g_vw": P["b.v_mat.weight"].grad,
               "g_W0": P["b.s_dense.0.weight"].grad, "g_b0": P["b.s_dense.0.bias"].grad, "g_W1": P["b.s_dense.1.weight"].grad,
               "g_b1": P["b.s_dense.1.bias"].grad}
        worst = {}
        for k, t in got.items():
            _ratio(t.detach().numpy(), out[k], k, worst)
