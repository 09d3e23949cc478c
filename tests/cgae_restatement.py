"""Test-side restatement of the mapping learner's step (reference: CoarseGrainingVAE/cgae.py:21-33, datasets.py:217-239)
in fp64 torch, and of the kernels' noise generator in numpy.  It lives in the tests only: nothing on the product path
imports it, and it is no fallback for a missing kernel.

    M = softmax(W + g)             g = -log(E), E ~ Exp(1)  (F.gumbel_softmax at its default tau = 1: the ``tau`` that
                                   learn_map decrements never reaches it, cgae.py:27)
    M_norm = M / colsum(M)
    cg = M_norm^T X                recon = D^T cg            lift = M cg
    loss_recon = mean((X - recon)^2)        loss_reg = mean_{b,i} sum_xyz (X - lift)^2
    loss = loss_recon + reg_weight * loss_reg               then torch.optim.Adam(lr) on (W, D)
"""
import numpy as np
import torch

F64 = torch.float64


def _t(x, dtype=F64):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def forward(W, D, X, g, reg_weight):
    """All tensors fp64; X [B, n, 3] already centred per frame; g [n, K] or None (noise free)."""
    M = torch.softmax(W if g is None else W + g, dim=-1)
    M_norm = M / M.sum(-2, keepdim=True)
    cg = torch.einsum("bij,in->bnj", X, M_norm)
    recon = torch.einsum("bnj,ni->bij", cg, D)
    lift = torch.einsum("bij,ni->bnj", cg, M)
    loss_reg = (X - lift).pow(2).sum(-1).mean()
    loss_recon = (X - recon).pow(2).mean()
    return {"M": M, "cg_xyz": cg, "recon": recon, "lift": lift, "loss_recon": loss_recon, "loss_reg": loss_reg,
            "loss": loss_recon + reg_weight * loss_reg}


def step_outputs(W, D, X, g, reg_weight, dtype=F64):
    """Forward quantities and both gradients as numpy arrays.  ``dtype=torch.float32`` is the reference's own arithmetic
    (the same tensor ops in its precision): what the deviation of an fp32 implementation from fp64 looks like at a size
    no stored fixture covers."""
    W, D = _t(W, dtype).clone().requires_grad_(True), _t(D, dtype).clone().requires_grad_(True)
    out = forward(W, D, _t(X, dtype), _t(g, dtype), float(reg_weight))
    out["loss"].backward()
    res = {k: v.detach().numpy() for k, v in out.items()}
    res["dW"], res["dD"] = W.grad.numpy(), D.grad.numpy()
    return res


def adam_steps(W, D, X, noise, reg_weight, lr=4e-3, dtype=F64):
    """``len(noise)`` optimiser steps on the same batch X with the given noise per step; returns (W, D) as numpy."""
    W, D = _t(W, dtype).clone().requires_grad_(True), _t(D, dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([W, D], lr=lr)
    X = _t(X, dtype)
    for g in noise:
        opt.zero_grad()
        forward(W, D, X, _t(g, dtype), float(reg_weight))["loss"].backward()
        opt.step()
    return W.detach().numpy(), D.detach().numpy()


STEP_FIXTURES = ("g13_cgae_step_n22_k3_b32", "g13_cgae_step_n22_k3_b4", "g13_cgae_step_n166_k6_b8")
QUANTITIES = ("M", "cg_xyz", "loss_recon", "loss_reg", "dW", "dD", "W_after1", "D_after1", "W_after10", "D_after10")


def restate_fixture(f):
    """Every checked quantity of a step fixture from its stored inputs, fp64."""
    reg = float(f["reg_weight"])
    res = step_outputs(f["W"], f["D"], f["X"], f["noise"][0], reg)
    for k in (1, 10):
        res[f"W_after{k}"], res[f"D_after{k}"] = adam_steps(f["W"], f["D"], f["X"], f["noise"][:k], reg, lr=float(f["lr"]))
    return res


def rel_dev(got, want):
    """max |got - want| / max |want|: the deviation measure of every parity check of the learner."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


def reference_deviation(fixtures):
    """Per quantity: the largest rel_dev, over the loaded step fixtures, of the REFERENCE's fp32 output from the fp64
    restatement -- what fp32 arithmetic costs on this computation.  The kernels are allowed four times that."""
    dev = {q: 0.0 for q in QUANTITIES}
    for f in fixtures:
        r = restate_fixture(f)
        for q in QUANTITIES:
            dev[q] = max(dev[q], rel_dev(f[q], r[q]))
    return dev


def noise_free_objective(W, D, frames, reg=0.25):
    """loss_recon + reg * loss_reg at g = 0 over ``frames`` [T, n, 3] (centred here), fp64."""
    X = _t(frames)
    X = X - X.mean(1, keepdim=True)
    with torch.no_grad():
        out = forward(_t(W), _t(D), X, None, reg)
    return float(out["loss_recon"] + reg * out["loss_reg"])


# ------------------------------------------------------------------ the kernels' noise generator (csrc/cgae.hip)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays; returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) & _LOW for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & _LOW, n2, p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def gumbel_noise(seed, step, n, K):
    """The [n, K] fp32 noise matrix of optimiser step ``step`` (0-based, counted over the whole schedule).

    Element (i, k) takes word k % 4 of Philox(counter = (i, k // 4, step low, step high), key = (seed low, seed high)).
    The word's top 23 bits b give u = (b + 0.5) / 2^23, exactly representable and inside the OPEN interval (0, 1);
    g = -log(-log(u)) is evaluated in fp64 and rounded to fp32 once."""
    i = np.arange(n, dtype=np.uint32)[:, None]
    q = np.arange((K + 3) // 4, dtype=np.uint32)[None, :]
    words = philox4x32_10(i, q, np.uint32(step & 0xFFFFFFFF), np.uint32((step >> 32) & 0xFFFFFFFF),
                          seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    bits = np.stack(words, axis=-1).reshape(n, -1)[:, :K]
    u = ((bits >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0
    return (-np.log(-np.log(u))).astype(np.float32)
