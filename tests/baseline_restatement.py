"""Test-side restatement of the baseline models (reference: CoarseGrainingVAE/baseline.py:8-36, 109-147, 387-443 under the
fixed pooler of diffpoolvae.py:105-195; losses scripts/run_baseline.py:86-92, 147-149) in fp64 torch.  It lives in the tests
only: nothing on the product path imports it, and it is no fallback for a missing kernel.

    cg[b,k]  = mean of xyz[b,a] over the atoms a of bead k
    linear      shift = mean_a xyz[b,a];  recon[b,a] = sum_c B[c,a] (cg[b,c] - shift);  target = xyz - shift
    equilinear  U[b, i knn + (c-1)] = cg[b,c] - cg[b,i]  (i = 0..K-1, c = 1..knn: c is a bead index)
                dx[b,a] = sum_j B[a,j] U[b,j];  off[b,k] = mean of dx[b,a] over bead k
                recon[b,a] = cg[b,m(a)] - off[b,m(a)] + dx[b,a];  target = xyz
    mlp         recon = Linear_out(act(Linear_hid(... act(Linear_in(cg.reshape(b, 3K)))))) with ONE hidden layer applied
                ``depth`` times;  target = xyz
    loss_recon = mean((recon - target)^2);  loss_dist = mean over (b, e = (i, j)) of (|recon_i - recon_j| - |x_i - x_j|)^2,
    0 for an empty edge list; a pair whose reconstructed length is exactly 0 gets no gradient
    loss = loss_recon + gamma loss_dist, then torch.optim.Adam(lr)
"""
import numpy as np
import torch

F64 = torch.float64
LINEAR_KINDS = ("linear", "equilinear")


def _t(x, dtype=F64):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def bead_means(xyz, mapping, K):
    mapping = torch.as_tensor(np.asarray(mapping)).long()
    sums = torch.zeros(xyz.shape[0], K, 3, dtype=xyz.dtype).index_add_(1, mapping, xyz)
    return sums / torch.bincount(mapping, minlength=K).to(xyz.dtype)[None, :, None]


def features(cg, knn):
    K = cg.shape[1]
    return torch.stack([cg[:, c] - cg[:, i] for i in range(K) for c in range(1, knn + 1)], dim=1)


def forward_linear(B, xyz, mapping):
    K = B.shape[0]
    shift = xyz.mean(1, keepdim=True)
    cg = bead_means(xyz, mapping, K) - shift
    return xyz - shift, torch.einsum("bce,ca->bae", cg, B)


def forward_equilinear(B, xyz, mapping, K, knn):
    mapping = torch.as_tensor(np.asarray(mapping)).long()
    cg = bead_means(xyz, mapping, K)
    dx = torch.einsum("bje,nj->bne", features(cg, knn), B)
    off = bead_means(dx, mapping, K)
    return xyz, cg[:, mapping] - off[:, mapping] + dx


def forward_mlp(weights, xyz, mapping, K, depth, act=torch.relu):
    """``weights`` = (W_in, b_in, W_hid, b_hid, W_out, b_out); the hidden layer runs ``depth`` times."""
    W0, b0, W1, b1, W2, b2 = weights
    x = bead_means(xyz, mapping, K).reshape(xyz.shape[0], 3 * K) @ W0.t() + b0
    for _ in range(depth):
        x = act(x) @ W1.t() + b1
    x = act(x) @ W2.t() + b2
    return xyz, x.reshape(xyz.shape[0], -1, 3)


def losses(recon, target, edges):
    """(loss_recon, loss_dist).  The hyperedge distances of the target equal those of xyz (a shift cancels)."""
    loss_recon = (recon - target).pow(2).mean()
    edges = torch.as_tensor(np.asarray(edges)).long().reshape(-1, 2)
    if edges.shape[0] == 0:
        return loss_recon, torch.zeros((), dtype=recon.dtype)
    d = recon[:, edges[:, 0]] - recon[:, edges[:, 1]]
    sq = d.pow(2).sum(-1)
    zero = sq == 0
    gen = torch.where(zero, torch.zeros_like(sq), torch.where(zero, torch.ones_like(sq), sq).sqrt())    # no gradient at 0
    data = (target[:, edges[:, 0]] - target[:, edges[:, 1]]).pow(2).sum(-1).sqrt()
    return loss_recon, (gen - data).pow(2).mean()


def model_forward(kind, params, xyz, mapping, K, knn=0, depth=1):
    if kind == "linear":
        return forward_linear(params[0], xyz, mapping)
    if kind == "equilinear":
        return forward_equilinear(params[0], xyz, mapping, K, knn)
    return forward_mlp(params, xyz, mapping, K, depth)


def step_outputs(kind, params, xyz, mapping, edges, gamma, K, knn=0, depth=1, dtype=F64):
    """Forward, both losses and the parameter gradients as numpy arrays (``dtype=torch.float32``: the reference's own
    arithmetic, for sizes no stored fixture covers)."""
    params = [_t(p, dtype).clone().requires_grad_(True) for p in params]
    target, recon = model_forward(kind, params, _t(xyz, dtype), mapping, K, knn, depth)
    recon.retain_grad()
    l_recon, l_dist = losses(recon, target, edges)
    (l_recon + float(gamma) * l_dist).backward()
    return {"xyz_recon": recon.detach().numpy(), "target": target.detach().numpy(), "loss_recon": float(l_recon.detach()),
            "loss_dist": float(l_dist.detach()), "grads": [p.grad.numpy() for p in params], "grad_recon": recon.grad.numpy()}


def adam_steps(kind, params, batches, mapping, edges, gamma, K, knn=0, depth=1, lr=1e-3, dtype=F64):
    """One optimiser step per entry of ``batches`` (each [b, n, 3]); returns the parameters as numpy arrays and the
    [steps, 2] loss log."""
    params = [_t(p, dtype).clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(params, lr=lr)
    log = []
    for xyz in batches:
        opt.zero_grad()
        target, recon = model_forward(kind, params, _t(xyz, dtype), mapping, K, knn, depth)
        l_recon, l_dist = losses(recon, target, edges)
        (l_recon + float(gamma) * l_dist).backward()
        opt.step()
        log.append((float(l_recon.detach()), float(l_dist.detach())))
    return [p.detach().numpy() for p in params], np.array(log)


# ------------------------------------------------------------------ the stored fixtures (tests/golden/make_golden_baseline.py)
LINEAR_CASES = (("n22_k3_knn2", 22, 3, 2, 4), ("n166_k6_knn5", 166, 6, 5, 8), ("n22_k3_knn1", 22, 3, 1, 4))
GAMMAS = (0.0, 0.5)
STEP_FIXTURES = tuple(f"g19_baseline_step_{kind}_{tag}_g{str(g).replace('.', '')}"
                      for kind in LINEAR_KINDS for tag, *_ in LINEAR_CASES for g in GAMMAS)
TRAJ_FIXTURES = tuple(f"g19_baseline_traj_{kind}" for kind in LINEAR_KINDS)
MLP_FIXTURES = tuple(f"g19_baseline_mlp_w1_d{d}_g{str(g).replace('.', '')}" for d in (1, 2) for g in GAMMAS)
QUANTITIES = ("xyz_recon", "loss_recon", "loss_dist", "grad", "B_after1", "B_after10")


def rel_dev(got, want):
    """max |got - want| / max |want| (a zero reference: the absolute deviation)."""
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (scale if scale > 0 else 1.0))


def restate_step_fixture(f):
    """Every checked quantity of a linear-kind step fixture from its stored inputs, fp64.  The first Adam step runs on the
    fixture's first batch (the full one), steps 2..10 on the same batch again -- as the generator did."""
    kind, K, knn = str(f["kind"]), int(f["K"]), int(f["knn"])
    args = dict(mapping=f["mapping"], edges=f["edges"], gamma=float(f["gamma"]), K=K, knn=knn)
    out = step_outputs(kind, [f["B"]], f["xyz"], **args)
    res = {"xyz_recon": out["xyz_recon"], "loss_recon": out["loss_recon"], "loss_dist": out["loss_dist"], "grad": out["grads"][0]}
    for k in (1, 10):
        res[f"B_after{k}"] = adam_steps(kind, [f["B"]], [f["xyz"]] * k, lr=float(f["lr"]), **args)[0][0]
    if "xyz_partial" in f:
        part = step_outputs(kind, [f["B"]], f["xyz_partial"], **args)
        res.update(partial_xyz_recon=part["xyz_recon"], partial_loss_recon=part["loss_recon"],
                   partial_loss_dist=part["loss_dist"], partial_grad=part["grads"][0])
    return res
