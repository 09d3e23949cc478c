"""The fp64 reference of the pseudo-vector decoder loop (tests/decoder_loop_reference.py) and the inputs that keep every
term of the message alive -- no GPU needed.

Under the product's initial state (V = Vbar = 0, Sbar = 0; cgvae.py:100-103) most of EquiMessagePsuedo (conv.py:199-217)
multiplies zeros in the first two layers, and the last layer's Vbar terms get no upstream gradient: a step-level test
never runs the backward of those terms on non-zero values.  ``test_product_state_leaves_filters_dead`` writes that down;
``test_dense_state_keeps_every_term_alive`` shows that the inputs of tests/test_decoder_loop_fp64.py do not."""
import numpy as np
import pytest
import torch
from torch.overrides import TorchFunctionMode

import decoder_loop_reference as R
from oracle import cgvae_oracle as O


class _NoFloat32(TorchFunctionMode):
    """Records every torch call that returns a float32 tensor of one or more dimensions (0-dim constants such as
    ``torch.tensor(1.0)`` never take part in type promotion and are let through)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if torch.is_tensor(t) and t.dtype in (torch.float32, torch.float16, torch.bfloat16) and t.dim() >= 1:
                self.seen.append(getattr(func, "__name__", str(func)))
        return out


def _case(n=6, F=16, n_rbf=8, layers=3, seed=0, dtype=torch.float64):
    xyz, nbrs = R.bead_graph(n, "dense", seed)
    return xyz, nbrs, R.dense_inputs(n, F, seed), R.decoder_params(F, n_rbf, layers, dtype=dtype)


def test_reference_stays_in_float64():
    xyz, nbrs, inp, P = _case()
    V0 = inp["V0"].double()
    with _NoFloat32() as watch:
        S_out, V_out = R.decoder_loop(xyz.double(), nbrs, inp["S"].double(), inp["Sbar0"].double(), V0, V0, P, 3, 8, 9.5)
    assert S_out.dtype == torch.float64 and V_out.dtype == torch.float64
    assert watch.seen == [], f"float32 intermediates in the fp64 reference: {sorted(set(watch.seen))}"


def test_oracle_pieces_keep_float64_precision():
    """The three places where a constant could silently be fp32: the radial basis' ``n pi / cutoff`` (modules.py:148-172),
    the envelope (modules.py:52-58) and the 1e-10 inside the update block's norm (conv.py:600)."""
    cutoff, n_rbf = 9.5, 10
    d = torch.tensor([0.37, 1.0, 2.5, 7.123456789, 9.4], dtype=torch.float64)
    rbf = O.painn_rbf(d, n_rbf, cutoff)
    env = O.cosine_envelope(d, cutoff)
    assert rbf.dtype == torch.float64 and env.dtype == torch.float64
    k = np.arange(1, n_rbf + 1, dtype=np.float64)
    want = np.sin(k[None, :] * np.pi / cutoff * d.numpy()[:, None]) / d.numpy()[:, None]
    assert np.abs(rbf.numpy() - want).max() <= 1e-14           # an fp32 coefficient would be off by ~1e-6 here
    assert np.abs(env.numpy() - 0.5 * (np.cos(np.pi * d.numpy() / cutoff) + 1)).max() <= 1e-15
    # the norm's epsilon: v = 0 and identity gates route ||Vv||_eps = sqrt(3e-10) straight into ds
    F = 4
    eye, zero = torch.eye(F, dtype=torch.float64), torch.zeros(F, F, dtype=torch.float64)
    P = {"u.u_mat.weight": eye, "u.v_mat.weight": eye,
         "u.s_dense.0.weight": torch.cat([zero, eye], dim=1), "u.s_dense.0.bias": torch.zeros(F, dtype=torch.float64),
         "u.s_dense.1.weight": torch.cat([zero, zero, eye], dim=0), "u.s_dense.1.bias": torch.zeros(3 * F, dtype=torch.float64)}
    ds, dv = O.update_block(torch.zeros(2, F, dtype=torch.float64), torch.zeros(2, F, 3, dtype=torch.float64), P, "u", lambda x: x)
    assert ds.dtype == torch.float64 and dv.dtype == torch.float64
    assert float((ds - np.sqrt(3e-10)).abs().max()) <= 1e-20     # fp32's 1e-10 is 1.00000001e-10: off by 6e-14


def test_float32_loop_is_the_oracle_loop_bit_for_bit():
    """From the product's initial state, in fp32, the helper IS ``pseudo_decoder_forward`` (both values of breaksym)."""
    n, F, n_rbf, layers = 6, 16, 8, 3
    xyz, nbrs, inp, P = _case(n, F, n_rbf, layers, dtype=torch.float32)
    for n_cgs in (6, 3):
        hp = O.Hyper(F, n_rbf, 9.5, 25.0, 1, layers, n_cgs)
        want = O.pseudo_decoder_forward(xyz, nbrs, inp["S"], P, hp)
        Sbar, V, Vbar = R.product_state(inp["S"], hp.breaksym)
        got = R.decoder_loop(xyz, nbrs, inp["S"], Sbar, V, Vbar, P, layers, n_rbf, hp.atom_cutoff)
        assert got[0].dtype == torch.float32
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("breaksym", [False, True])
def test_product_state_leaves_filters_dead(breaksym):
    """The gap: product initial state, 3 layers, the product's loss (cg_v[mapping, chan, :] only, cgvae.py:462-484).  The
    rows of inv_dense.1 that feed q3, q4, q5, q8 get an exactly zero gradient in layers 0 and 1, those of q5..q8 in the
    last layer; q3 first comes alive in the third layer.  q4 multiplies sbar_i * vbar_j: with Sbar0 = 1 (n_cgs == 3) it
    comes alive there too, with Sbar0 = 0 it stays dead even in the third layer (Sbar is still 0 on entry: its first
    non-zero increment v_i . vbar_j is the third layer's own) -- it would take a fourth."""
    n, F, n_rbf, layers = 6, 16, 8, 3
    xyz, nbrs, inp, P = _case(n, F, n_rbf, layers)
    P = {k: v.requires_grad_(True) for k, v in P.items()}
    S = inp["S"].double().requires_grad_(True)
    Sbar, V, Vbar = R.product_state(S, breaksym)
    _, V_out = R.decoder_loop(xyz.double(), nbrs, S, Sbar, V, Vbar, P, layers, n_rbf, 9.5)
    mapping = torch.arange(n).repeat_interleave(3)                # three atoms per bead: channels 0..2 reach the loss
    chan = O.channel_index(mapping)
    up = torch.randn(mapping.shape[0], 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (V_out[mapping, chan, :] * up).sum().backward()
    blocks = [R.row_block_max(P[R.layer_keys(l)[R.W2]].grad, F) for l in range(layers)]
    for l in (0, 1):
        for k in (3, 4, 5, 8):
            assert blocks[l][k] == 0.0, (l, k, blocks[l])
    for k in (5, 6, 7, 8):
        assert blocks[layers - 1][k] == 0.0, (k, blocks[layers - 1])
    assert blocks[layers - 1][3] > 0.0, blocks[layers - 1]
    if breaksym:
        assert blocks[layers - 1][4] > 0.0, blocks[layers - 1]
    else:
        assert blocks[layers - 1][4] == 0.0, blocks[layers - 1]
    for k in (0, 1):                                              # what every layer does exercise
        assert all(blocks[l][k] > 0.0 for l in range(layers))


@pytest.mark.parametrize("layers,use_uS,use_uV", [(2, True, True), (2, False, True), (2, True, False), (4, True, True)])
def test_dense_state_keeps_every_term_alive(layers, use_uS, use_uV):
    """The cure: dense random S, Sbar0, V0 = Vbar0 and dense upstream weights on S and V (or one of them) -- all nine
    filters live in every layer but the last, q0..q4 in the last, no parameter without a gradient."""
    n, F, n_rbf = 6, 16, 8
    xyz, nbrs, inp, P = _case(n, F, n_rbf, layers)
    ref = R.run_reference(xyz, nbrs, inp, P, layers, n_rbf, 9.5, use_uS, use_uV)
    R.assert_every_term_live(ref, F, layers, "dense inputs")
    assert all(g.dtype == torch.float64 for g in ref["grads"].values())
    last = R.row_block_max(ref["grads"][R.layer_keys(layers - 1)[R.W2]], F)
    assert last[5:] == [0.0] * 4                                  # Vbar leaves the loop unused (cgvae.py:125)
