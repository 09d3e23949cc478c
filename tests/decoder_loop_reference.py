"""High-precision reference of the pseudo-vector decoder loop (cgvae.py:100-123) for tests.  NOT a restatement: every
formula comes from ``oracle.cgvae_oracle`` (``equi_message_pseudo`` + ``update_block``), looped exactly as
``pseudo_decoder_forward`` loops them -- but with the initial ``Sbar`` / ``V`` / ``Vbar`` as arguments and in whatever
dtype the inputs and the parameter dict carry (``pseudo_decoder_forward`` creates fp32 zeros itself).

Shared by tests/test_decoder_loop_cpu.py (no GPU) and tests/test_decoder_loop_fp64.py (the channel-group kernels of
csrc/decoder_layer.hip against this reference in float64).
"""
from __future__ import annotations

from typing import Dict

import torch

from oracle import cgvae_oracle as O

PREFIX = "equivaraintconv"
W2 = 2            # position of inv_message.inv_dense.1.weight [9F, F] in layer_keys: row block k = filter q_k (conv.py:199-217)


def layer_keys(layer: int, prefix: str = PREFIX):
    """Oracle names of the 12 tensors per layer, in ``decoder_fused.layer_params`` order
    (W1 b1 W2 b2 Wd bd Wu Wv W0 b0 W1' b1')."""
    m, u = f"{prefix}.message_blocks.{layer}.inv_message", f"{prefix}.update_blocks.{layer}"
    return [m + ".inv_dense.0.weight", m + ".inv_dense.0.bias", m + ".inv_dense.1.weight", m + ".inv_dense.1.bias",
            m + ".dist_embed.block.1.weight", m + ".dist_embed.block.1.bias", u + ".u_mat.weight", u + ".v_mat.weight",
            u + ".s_dense.0.weight", u + ".s_dense.0.bias", u + ".s_dense.1.weight", u + ".s_dense.1.bias"]


def decoder_loop(cg_xyz, cg_nbr_list, S, Sbar, V, Vbar, P, n_layers, n_rbf, cutoff, act=O.swish, prefix=PREFIX):
    """(S, V) after ``n_layers`` layers from the given initial state; dtype = that of the inputs and of ``P``."""
    cg_nbr_list, _ = O.make_directed(cg_nbr_list)
    r_ij = cg_xyz[cg_nbr_list[:, 1]] - cg_xyz[cg_nbr_list[:, 0]]
    for k in range(n_layers):
        dS, dSbar, dV, dVbar = O.equi_message_pseudo(S, Sbar, V, Vbar, r_ij, cg_nbr_list, P, f"{prefix}.message_blocks.{k}",
                                                     act, n_rbf, cutoff)
        S = S + dS
        Sbar = Sbar + dSbar
        V = V + dV
        Vbar = Vbar + dVbar
        dS_u, dV_u = O.update_block(S, V, P, f"{prefix}.update_blocks.{k}", act)
        S = S + dS_u
        V = V + dV_u
    return S, V


def product_state(S, breaksym: bool = False):
    """The state the product enters the loop with (cgvae.py:100-103): Sbar = 0 (1 for n_cgs == 3), V = Vbar = 0."""
    n, F = S.shape
    Sbar = torch.ones(n, F, dtype=S.dtype) if breaksym else torch.zeros(n, F, dtype=S.dtype)
    return Sbar, torch.zeros(n, F, 3, dtype=S.dtype), torch.zeros(n, F, 3, dtype=S.dtype)


def decoder_params(F, R, n_layers, seed=11, dtype=torch.float64, bias_std=0.1) -> Dict[str, torch.Tensor]:
    """Fresh parameters of the loop under the oracle's names; the (zero-initialised) biases are drawn too, so that no
    bias path is fed zeros."""
    hp = O.Hyper(F, R, 5.0, 9.5, 1, n_layers, 6)
    P = {k: v for k, v in O.init_params(hp, seed=seed).items() if k.startswith(PREFIX + ".")}
    gen = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith(".bias"):
            P[k] = torch.randn(P[k].shape, generator=gen) * bias_std
    return {k: v.to(dtype) for k, v in P.items()}


def bead_graph(n: int, kind: str = "dense", seed: int = 0):
    """(xyz fp32 [n, 3], directed neighbour list [E, 2]).  ``dense``: random beads in a 6 A box, every ordered pair an
    edge.  ``sparse`` (n >= 6): a fully connected cluster, a pair that sees only each other (one incoming edge each) and
    one bead out of everybody's reach (no edge at all) under a 4 A neighbour cutoff."""
    gen = torch.Generator().manual_seed(1000 + seed)
    if kind == "dense":
        xyz = torch.rand(n, 3, generator=gen) * 6.0
        und = O.get_neighbor_list(xyz, 25.0, True)
    elif kind == "sparse":
        xyz = torch.rand(n, 3, generator=gen) * 2.0
        xyz[n - 3] = torch.tensor([10.0, 0.5, 0.0])
        xyz[n - 2] = torch.tensor([11.0, 0.0, 0.7])
        xyz[n - 1] = torch.tensor([30.0, 1.0, 1.0])
        und = O.get_neighbor_list(xyz, 4.0, True)
    else:
        raise ValueError(kind)
    nbrs, _ = O.make_directed(und)
    return xyz, nbrs


def dense_inputs(n: int, F: int, seed: int = 0):
    """Random dense S, Sbar0, V0 (= Vbar0, as the fused entry point takes it) and upstream weights uS, uV (fp32).
    V0 has standard deviation 0.3, about what the message blocks add to V per layer: the cross and sbar * vbar terms are
    quadratic in the state, so unit-size vectors grow without bound over a few layers (1e22 after four at F = 128) and the
    comparison would measure the conditioning of the inputs; at 0.3 all nine filter gradients stay within two decades."""
    gen = torch.Generator().manual_seed(2000 + seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(S=r(n, F), Sbar0=r(n, F), V0=0.3 * r(n, F, 3), uS=r(n, F), uV=r(n, F, 3))


def run_reference(xyz, nbrs, inp, P, n_layers, R, cutoff, use_uS=True, use_uV=True, dtype=torch.float64):
    """Forward + backward of ``(S_out * uS).sum() + (V_out * uV).sum()`` (either term optional) in ``dtype``:
    {"S_out", "V_out", "gS", "grads": {oracle key: gradient}}."""
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
    S = inp["S"].to(dtype).requires_grad_(True)
    V0 = inp["V0"].to(dtype)
    S_out, V_out = decoder_loop(xyz.to(dtype), nbrs, S, inp["Sbar0"].to(dtype), V0, V0, P, n_layers, R, cutoff)
    loss = 0.0
    if use_uS:
        loss = loss + (S_out * inp["uS"].to(dtype)).sum()
    if use_uV:
        loss = loss + (V_out * inp["uV"].to(dtype)).sum()
    loss.backward()
    keys = [k for l in range(n_layers) for k in layer_keys(l)]
    return dict(S_out=S_out.detach(), V_out=V_out.detach(), gS=S.grad,
                grads={k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in keys})


def row_block_max(g: torch.Tensor, F: int):
    """max |.| of each of the nine row blocks [kF, (k+1)F) of an ``inv_dense.1.weight`` gradient."""
    assert g.shape[0] == 9 * F
    return [float(g[k * F:(k + 1) * F].abs().max()) for k in range(9)]


def assert_every_term_live(ref, F: int, n_layers: int, what: str = "") -> None:
    """The condition on the INPUTS of a dense case: in every layer but the last all nine filters q0..q8 receive a non-zero
    gradient, in the last one q0..q4 (q5..q8 feed only Vbar, which leaves the loop unused; S and V both pass through the
    last update block, so either upstream gradient reaches q0..q4), and every parameter of every layer has a non-zero
    gradient.  A case that leaves a term dead would pass trivially: it fails here instead."""
    for l in range(n_layers):
        keys = layer_keys(l)
        blocks = row_block_max(ref["grads"][keys[W2]], F)
        last = l == n_layers - 1
        need = range(5) if last else range(9)
        for k in need:
            assert blocks[k] > 0.0, f"{what}: layer {l}: filter q{k} is dead ({blocks})"
        for key in keys:
            assert float(ref["grads"][key].abs().max()) > 0.0, f"{what}: {key} has a zero gradient"
    assert float(ref["gS"].abs().max()) > 0.0
