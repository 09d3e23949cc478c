"""csrc/elbo.hip and csrc/loss_tail.hip restated in plain fp64 torch: the loss of scripts/utils.py:81-86, 117-141 (its
``(mu1 - mu2)^2 / std2`` included: std2, not std2^2), the decoder tail in front of it (cgvae.py:462-481), their gradients
by fp64 autograd -- and the error bounds the fp32 kernels are held to (tests/test_elbo_gpu.py; tests/test_elbo_cpu.py pins
this file to train.KL / train.loss_terms and to the closed-form gradients the kernels were written from).

    KL     = 0.5 * mean_beads[ sum_f ( s1^2/s2^2 + dm^2/s2 + log s2^2 - log s1^2 ) - F ],      dm = mu - prior_mu
    recon  = mean( (xr - x)^2 )
    graph  = mean_bonds( (lg - ld)^2 ),   lg = |xr_a0 - xr_a1|_eps,  ld = |x_a0 - x_a1|_eps,  |d|_eps = sqrt(d.d + 1e-6)
    loss   = recon + beta KL + gamma graph;  the REPORTED graph term is 0 when gamma == 0 or there are no bonds
    tail:    xyz_rel[a] = V[bead(a), chan[a]];  minus the bead's mean (offset);  plus cg_xyz[bead(a)]

Everything runs on fp64 copies of the kernels' fp32 inputs; beta and gamma enter as the fp32 values the C ABI receives.

ERROR BOUNDS.  Each output has a MAGNITUDE: its own expression with every subtraction that can cancel replaced by the sum
of the magnitudes (``magnitudes``), and a count K of fp32 roundings (U = 2^-24 each; divide and sqrtf are correctly rounded,
-ffast-math is not used, a contraction into an fma only removes a rounding) on the longest chain that leads to it in the
kernels.  The bound is K U magnitude, times SLACK for the terms of second order, plus TINY for results that underflow.
The kernels compute every TERM of the three scalars in fp32 and add the terms in double (block_sum, the per-block partial
sums, the last block): the scalars' bounds are sums of per-term bounds and do not grow with the number of terms; the double
additions are counted at 2^-53 per term (F64).  The counts, expression by expression (the same text in both kernel files):

  ck = 0.5f * beta / (float)n_beads            1   (0.5 beta and the conversion are exact)
  dm = m1 - m2                                 1   relative to |dm|: the operands are inputs
  g_mu = ck * (2.f * dm / s2)                  dm 1, divide 1, ck 1, product 1                                  K_GMU  = 4
  g_prior_mu = -ck * (...)                     the same (negation is exact)
  g_sigma = ck * (2 s1 / s2s - 2 / s1)         A = 2 s1 / s2s: s2s 1, divide 1;  B = 2 / s1: 1;  A - B: 1 on |A| + |B|;
                                               ck 1, product 1: the A chain 2 + 1 + 2                           K_GSIG = 5
  g_prior_std = ck * (-2 s1s / (s2s s2) - dm dm / s2s + 2 / s2)
                                               T2 = dm dm / s2s: dm 2 (twice), product 1, s2s 1, divide 1 = 5 (T1: 4, T3: 1);
                                               two sums 2, ck 1, product 1                                      K_GPST = 9
  KL term = s1s / s2s + dm dm / s2 + logf(s2s) - logf(s1s)
                                               t2 = dm dm / s2: 2 + 1 + 1 = 4 (t1: 3);  three sums 3            K_KL   = 7
                                               each logf: its argument carries 1 rounding = U ABSOLUTE on the logarithm
                                               (magnitude 1 per logarithm: ``kl_arg``), and the function itself LOGF_ULP
                                               ulp = 2 LOGF_ULP U relative to |log| (``kl_log``)
  recon term = d * d, d = xr - x               d 1 (twice), product 1                                           K_RECON = 3
  |e|_eps = sqrtf(1e-6f + ex ex + ey ey + ez ez)
                                               ex 1 (twice), square 1, three sums 3: 6 on the radicand (the constant: its
                                               own rounding 1 + 3 sums); the root halves it, sqrtf 1            K_LEN  = 4
  graph term = diff * diff, diff = lg - ld     |delta diff| <= K_LEN U (lg + ld) + U |diff|;  the square doubles it, product 1:
                                               U (8 |diff| (lg + ld) + 3 diff^2) <= 11 U |diff| (lg + ld)       K_GRAPH = 11
                                               magnitude |diff| (lg + ld) -- plus the square of delta diff, (5 U (lg + ld))^2,
                                               which is not of second order where diff itself vanishes (``graph2``)
  bond gradient c e_j, c = cg * diff / lg, cg = gamma * 2.f / (float)n_bonds
                                               cg 1, product 1, divide 1, e_j 1, product 1, lg K_LEN = 9 relative to |c e_j|,
                                               plus |cg e_j| / lg x delta diff: U |cg e_j| / lg x (4 (lg + ld) + 10 |diff|)
                                               <= 14 U |cg e_j| (lg + ld) / lg                                  K_BOND = 14
                                               ABSOLUTE and conditioning-aware: the magnitude is |cg e_j| (lg + ld) / lg, not
                                               |c e_j| -- relative to the latter the bound would be unbounded where lg ~ ld
  g_xyz_recon[a] = sc * (xr - x) + sum over the bonds of a
                                               sc = 2.f / nr 1, difference 1, product 1                         K_RP   = 3
                                               the sum: a chain of fmaf(w, c e_j, g) with w = 0 for every bond that does not
                                               touch a (exact), split over thread groups / waves / chunks whose partial sums
                                               are added in order: a term passes at most deg(a) roundings, and 1 more when
                                               the reconstruction part joins: K_BOND + deg(a) + 1 on the bond terms and
                                               K_RP + deg(a) + 1 on the reconstruction part (deg = 0: K_RP alone)
  tail: mean = (sum over the bead) * (1 / n)   a lane adds ceil(n / 64) values (the first add to 0 is exact), 6 butterfly
                                               levels, 1 / n 1, product 1: ceil(n / 64) + 7 on mean|v|
        xr = (v - mean) + cg                   2 more                                                           K_XR = ceil(n / 64) + 9
                                               on |v| + mean|v| + |cg|; without the offset the mean is an exact 0: K = 1
        g_V = g_xr[a] - (gsum * (1 / n))       gsum: n - 1 sequential adds, 1 / n 1, product 1, difference 1    K_GV = n + 2
                                               on |g_xr[a]| + mean|g_xr|; zero elsewhere, exactly
  a scalar's cast to fp32: 1 on the scalar itself (``cast``); the loss: the three terms' bounds without their casts,
  weighted by 1, beta, gamma, and its own cast.

The fused tail computes the loss from ITS fp32 xyz_recon; this file from the fp64 one.  What the error allowed on xyz_recon
(``e_xr``) does to each later output is carried through to first order (the ``carry`` of each output: its sensitivity to
xyz_recon times e_xr) and added to K U (magnitude + carry).  For cgv_elbo_fwd, which is GIVEN xyz_recon, the carry is zero.

LOGF_ULP: no ROCm document installed next to the compiler states an error for device logf; the value is the one the HIP
programming guide's table of single-precision device functions gives for logf (2 ulp; CUDA's guide states 1 for its own).

No GPU, no library call, nothing imported from the package: importable anywhere."""
import math

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest): |fl(x) - x| <= U |x|
TINY = 2.0 ** -149                   # the smallest fp32 step (results that underflow)
SLACK = 1.0 + 2.0 ** -10             # the terms of second order in U that the first-order counts leave out
F64 = 2.0 ** -53                     # one double addition, counted per term of a scalar
LOGF_ULP = 2.0                       # device logf (see above)
BOND_EPS = 1e-6                      # scripts/utils.py:15
K_GMU, K_GSIG, K_GPST, K_KL, K_RECON, K_LEN, K_GRAPH, K_BOND, K_RP = 4, 5, 9, 7, 3, 4, 11, 14, 3
F64T = torch.float64

SCALARS = ("loss", "kl", "recon", "graph")
GRADS = ("g_mu", "g_sigma", "g_prior_mu", "g_prior_std", "g_xyz_recon")
TAIL_ONLY = ("xyz_recon", "g_V")


def f32(x):
    """The double a float argument of the C ABI carries."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------------------------------------------------
# the loss and the tail


def bond_lengths(x, bonds):
    d = x[bonds[:, 0]] - x[bonds[:, 1]]
    return (d.pow(2).sum(-1) + BOND_EPS).sqrt()


def kl_term(mu, sigma, pmu, pstd):
    F = mu.shape[-1]
    per_bead = (sigma.pow(2) / pstd.pow(2) + (mu - pmu).pow(2) / pstd + torch.log(pstd.pow(2)) - torch.log(sigma.pow(2))).sum(-1)
    return 0.5 * (per_bead - F).mean()


def loss_terms(mu, sigma, pmu, pstd, xyz, xr, bonds, beta, gamma):
    """(loss, KL, recon, graph as reported): differentiable tensors, in the dtype of the inputs."""
    kl = kl_term(mu, sigma, pmu, pstd)
    recon = (xr - xyz).pow(2).mean()
    if bonds.shape[0] > 0:
        graph = (bond_lengths(xr, bonds) - bond_lengths(xyz, bonds)).pow(2).mean()
    else:
        graph = xr.new_zeros(())
    loss = recon + beta * kl + gamma * graph
    return loss, kl, recon, (graph if gamma != 0.0 else xr.new_zeros(()))


def channel_index(mapping):
    """Rank of each atom among the atoms of its bead, in atom order (cgvae.py:451-460)."""
    rowptr, atom_of, bead_of = plan_arrays(mapping, int(mapping.max()) + 1)
    chan = torch.empty_like(mapping)
    chan[atom_of.long()] = torch.arange(mapping.numel()) - rowptr[bead_of.long()].long()
    return chan


def plan_arrays(mapping, n_beads):
    """(rowptr[n_beads + 1], atom_of[n_atoms], bead_of[n_atoms]) of the bead-sorted atom order, int32: what
    EdgePlan.from_mapping builds on the device (stable: atoms of a bead in atom order)."""
    order = torch.argsort(mapping, stable=True)
    counts = torch.bincount(mapping, minlength=n_beads)
    rowptr = torch.zeros(n_beads + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr.int(), order.int(), mapping[order].int()


def _bead_mean(x, mapping, n_beads):
    sums = torch.zeros((n_beads,) + x.shape[1:], dtype=x.dtype).index_add(0, mapping, x)
    counts = torch.bincount(mapping, minlength=n_beads).clamp(min=1).to(x.dtype)
    return sums / counts.view(-1, *[1] * (x.dim() - 1))


def tail(V, cg_xyz, mapping, chan, offset):
    rel = V[mapping, chan]
    if offset:
        rel = rel - _bead_mean(rel, mapping, V.shape[0])[mapping]
    return rel + cg_xyz[mapping]


def reference(inp, beta, gamma, offset=None):
    """All outputs of one launch in fp64, from the fp32 tensors of ``inp`` (dict: mu, sigma, prior_mu, prior_std, xyz,
    bonds, and either xyz_recon, or V, cg_xyz, mapping, chan with ``offset`` given: the fused tail)."""
    lv = {k: inp[k].double().requires_grad_() for k in ("mu", "sigma", "prior_mu", "prior_std")}
    xyz, bonds = inp["xyz"].double(), inp["bonds"].long()
    if offset is None:
        xr = inp["xyz_recon"].double().requires_grad_()
        V = None
    else:
        V = inp["V"].double().requires_grad_()
        xr = tail(V, inp["cg_xyz"].double(), inp["mapping"], inp["chan"], offset)
        xr.retain_grad()
    loss, kl, recon, graph = loss_terms(lv["mu"], lv["sigma"], lv["prior_mu"], lv["prior_std"], xyz, xr, bonds, beta, gamma)
    loss.backward()
    out = {"loss": loss.detach(), "kl": kl.detach(), "recon": recon.detach(), "graph": graph.detach(),
           "g_mu": lv["mu"].grad, "g_sigma": lv["sigma"].grad, "g_prior_mu": lv["prior_mu"].grad,
           "g_prior_std": lv["prior_std"].grad, "g_xyz_recon": xr.grad, "xyz_recon": xr.detach()}
    if V is not None:
        out["g_V"] = V.grad
    return out


def closed_form(inp, beta, gamma, offset=None, dtype=F64T):
    """The formulas the kernels implement, term by term in ``dtype`` with the scalars' terms added in double as the
    kernels add them: in fp64 they must equal ``reference`` (the formulas, apart from any rounding); in fp32 they exercise
    the bounds below on the CPU."""
    c = lambda k: inp[k].to(dtype)
    mu, sigma, pmu, pstd, xyz, bonds = c("mu"), c("sigma"), c("prior_mu"), c("prior_std"), c("xyz"), inp["bonds"].long()
    n_beads, F = mu.shape
    out = {}
    if offset is None:
        xr = c("xyz_recon")
    else:
        xr = tail(c("V"), c("cg_xyz"), inp["mapping"], inp["chan"], offset)
    out["xyz_recon"] = xr
    n_atoms, nb = xr.shape[0], bonds.shape[0]
    nr = 3 * n_atoms
    ck = torch.tensor(0.5 * beta, dtype=dtype) / torch.tensor(float(n_beads), dtype=dtype)
    s1s, s2s, dm = sigma * sigma, pstd * pstd, mu - pmu
    kl_sum = (s1s / s2s + dm * dm / pstd + torch.log(s2s) - torch.log(s1s)).double().sum()
    out["g_mu"] = ck * (2.0 * dm / pstd)
    out["g_prior_mu"] = -ck * (2.0 * dm / pstd)
    out["g_sigma"] = ck * (2.0 * sigma / s2s - 2.0 / sigma)
    out["g_prior_std"] = ck * (-2.0 * s1s / (s2s * pstd) - dm * dm / s2s + 2.0 / pstd)
    d = xr - xyz
    rec_sum = (d * d).double().sum()
    g = (torch.tensor(2.0, dtype=dtype) / torch.tensor(float(nr), dtype=dtype)) * d
    gr_sum = torch.zeros((), dtype=F64T)
    if nb > 0:
        a0, a1 = bonds[:, 0], bonds[:, 1]
        e, f = xr[a0] - xr[a1], xyz[a0] - xyz[a1]
        eps = torch.tensor(BOND_EPS, dtype=dtype)
        lg, ld = (eps + (e * e).sum(-1)).sqrt(), (eps + (f * f).sum(-1)).sqrt()
        diff = lg - ld
        gr_sum = (diff * diff).double().sum()
        if gamma != 0.0:
            cg = torch.tensor(gamma * 2.0, dtype=dtype) / torch.tensor(float(nb), dtype=dtype)
            coef = torch.where(a0 == a1, torch.zeros_like(diff), cg * diff / lg)           # a0 == a1: zero
            term = coef[:, None] * e
            g = g + torch.zeros_like(g).index_add_(0, a0, term).index_add_(0, a1, -term)
    out["g_xyz_recon"] = g
    kl = 0.5 * (kl_sum / n_beads - F)
    recon = rec_sum / nr
    graph = gr_sum / nb if nb > 0 else gr_sum
    out["loss"] = (recon + beta * kl + gamma * graph).to(dtype)
    out["kl"], out["recon"] = kl.to(dtype), recon.to(dtype)
    out["graph"] = graph.to(dtype) if gamma != 0.0 else torch.zeros((), dtype=dtype)
    if offset is not None:
        mapping, chan = inp["mapping"], inp["chan"]
        gv = g - _bead_mean(g, mapping, n_beads)[mapping] if offset else g                   # g_xr[a] - mean_b(g_xr)
        out["g_V"] = torch.zeros(n_beads, F, 3, dtype=dtype).index_put_((mapping, chan), gv)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# magnitudes and bounds (module docstring)


def _scatter2(n, a0, a1, val):
    return torch.zeros((n,) + val.shape[1:], dtype=F64T).index_add_(0, a0, val).index_add_(0, a1, val)


def tail_roundings(n_own):
    """K_XR of a bead of n_own atoms (module docstring)."""
    return (n_own + 63) // 64 + 9


def tail_analysis(inp, offset):
    """(magnitude, bound) of the fused tail's xyz_recon, [n_atoms, 3] each."""
    V, cg, mapping, chan = inp["V"].double(), inp["cg_xyz"].double(), inp["mapping"], inp["chan"]
    v = V[mapping, chan]
    if not offset:
        mag = (v + cg[mapping]).abs()                            # one rounding, on the result
        return mag, SLACK * U * mag + TINY
    n_own = torch.bincount(mapping, minlength=V.shape[0])
    mag = v.abs() + _bead_mean(v.abs(), mapping, V.shape[0])[mapping] + cg[mapping].abs()
    k = tail_roundings(n_own)[mapping].double()[:, None]
    return mag, SLACK * U * k * mag + TINY


def magnitudes(inp, beta, gamma, offset=None):
    """(M, C, deg): the magnitude of every output, its carry of the error allowed on the fused tail's xyz_recon (zero for
    cgv_elbo_fwd), and the number of bond ends at each atom that carry a gradient (self bonds carry none)."""
    mu, sigma, pmu, pstd = (inp[k].double() for k in ("mu", "sigma", "prior_mu", "prior_std"))
    xyz, bonds = inp["xyz"].double(), inp["bonds"].long()
    n_beads, F = mu.shape
    M, C = {}, {}
    if offset is None:
        xr = inp["xyz_recon"].double()
        e_xr = torch.zeros_like(xr)
    else:
        xr = tail(inp["V"].double(), inp["cg_xyz"].double(), inp["mapping"], inp["chan"], offset)
        M["xyz_recon"], e_xr = tail_analysis(inp, offset)
    n_atoms, nb = xr.shape[0], bonds.shape[0]
    nr = 3 * n_atoms
    ck = 0.5 * beta / n_beads
    s1s, s2s, dm = sigma * sigma, pstd * pstd, mu - pmu
    l1, l2 = torch.log(s1s).abs(), torch.log(s2s).abs()
    M["kl"] = 0.5 * float((s1s / s2s + dm * dm / pstd + l1 + l2).sum()) / n_beads
    M["kl_log"] = 0.5 * float((l1 + l2).sum()) / n_beads
    M["kl_arg"] = float(F)                                       # 0.5 * mean over the beads of sum_f (1 + 1)
    M["g_mu"] = M["g_prior_mu"] = abs(ck) * (2.0 * dm / pstd).abs()
    M["g_sigma"] = abs(ck) * (2.0 * sigma / s2s + 2.0 / sigma)
    M["g_prior_std"] = abs(ck) * (2.0 * s1s / (s2s * pstd) + dm * dm / s2s + 2.0 / pstd)
    d = xr - xyz
    M["recon"] = float((d * d).mean())
    C["recon"] = float((2.0 * d.abs() * e_xr + e_xr * e_xr).mean())
    M["rp"], C["rp"] = (2.0 * d / nr).abs(), 2.0 * e_xr / nr
    M["bond"], C["bond"] = torch.zeros_like(xr), torch.zeros_like(xr)
    M["graph"] = M["graph2"] = C["graph"] = 0.0
    deg = torch.zeros(n_atoms, dtype=F64T)
    if nb > 0:
        a0, a1 = bonds[:, 0], bonds[:, 1]
        live = (a0 != a1).double()
        e = xr[a0] - xr[a1]
        de = (e_xr[a0] + e_xr[a1]) * live[:, None]               # a self bond: both kernels subtract a value from itself
        lg, ld = bond_lengths(xr, bonds), bond_lengths(xyz, bonds)
        diff = (lg - ld).abs()
        dq = (2.0 * e.abs() * de + de * de).sum(-1)
        lg_lo = (lg * lg - (2.0 * e.abs() * de).sum(-1)).clamp(min=BOND_EPS).sqrt()      # the shortest the kernel's lg can be
        dlg = dq / (2.0 * lg_lo)
        M["graph"] = float((diff * (lg + ld)).mean())
        M["graph2"] = float(((lg + ld) ** 2).mean())
        C["graph"] = float((2.0 * diff * dlg + dlg * dlg).mean())
        if gamma != 0.0:
            cg = abs(gamma) * 2.0 / nb
            mterm = (cg * (lg + ld) / lg_lo * live)[:, None] * (e.abs() + de)
            cterm = cg * live[:, None] * ((dlg / lg_lo)[:, None] * e.abs() + (diff / lg_lo)[:, None] * de
                                          + (diff * dlg / (lg * lg_lo))[:, None] * e.abs())
            M["bond"], C["bond"] = _scatter2(n_atoms, a0, a1, mterm), _scatter2(n_atoms, a0, a1, cterm)
            deg = _scatter2(n_atoms, a0, a1, live)
    M["g_xyz_recon"], C["g_xyz_recon"] = M["rp"] + M["bond"], C["rp"] + C["bond"]
    return M, C, deg


def bounds(inp, ref, beta, gamma, offset=None):
    """{output: bound on |kernel - reference|}: a float for the four scalars, a tensor of the output's shape otherwise."""
    M, C, deg = magnitudes(inp, beta, gamma, offset)
    n_beads, F = inp["mu"].shape
    n_atoms, nb = ref["xyz_recon"].shape[0], inp["bonds"].shape[0]
    b = {}
    for name, k in (("g_mu", K_GMU), ("g_prior_mu", K_GMU), ("g_sigma", K_GSIG), ("g_prior_std", K_GPST)):
        b[name] = SLACK * k * U * M[name] + TINY
    kl = SLACK * (U * (K_KL * M["kl"] + 2.0 * LOGF_ULP * M["kl_log"] + M["kl_arg"]) + F64 * n_beads * F * M["kl"])
    recon = SLACK * ((K_RECON * U + F64 * 3 * n_atoms) * (M["recon"] + C["recon"]) + C["recon"])
    graph = SLACK * ((K_GRAPH * U + F64 * nb) * (M["graph"] + C["graph"]) + (5.0 * U) ** 2 * M["graph2"] + C["graph"])
    cast = lambda name: U * abs(float(ref[name])) + TINY
    b["kl"], b["recon"] = kl + cast("kl"), recon + cast("recon")
    b["graph"] = graph + cast("graph") if gamma != 0.0 else 0.0                    # reported as an exact 0
    b["loss"] = recon + abs(beta) * kl + abs(gamma) * graph + cast("loss")
    joins = torch.where(deg > 0, deg + 1.0, torch.zeros_like(deg))[:, None]       # roundings of the sum over an atom's bonds
    b["g_xyz_recon"] = SLACK * (U * ((K_RP + joins) * (M["rp"] + C["rp"]) + (K_BOND + joins) * (M["bond"] + C["bond"]))
                                + C["g_xyz_recon"]) + TINY
    if offset is not None:
        b["xyz_recon"] = tail_analysis(inp, offset)[1]
        mapping, chan = inp["mapping"], inp["chan"]
        g, bg = ref["g_xyz_recon"], b["g_xyz_recon"]
        if offset:
            n_own = torch.bincount(mapping, minlength=n_beads)[mapping].double()[:, None]
            mean_abs, mean_b = _bead_mean(g.abs(), mapping, n_beads)[mapping], _bead_mean(bg, mapping, n_beads)[mapping]
            per_atom = SLACK * ((n_own + 2.0) * U * (g.abs() + mean_abs + bg + mean_b) + bg + mean_b) + TINY
        else:
            per_atom = bg                                                           # g_xr[a] - 0: exact
        b["g_V"] = torch.zeros(n_beads, F, 3, dtype=F64T).index_put_((mapping, chan), per_atom)        # zero elsewhere
    return b


def scaled(ref, b, s):
    """Reference and bounds of the five gradients after cgv_elbo_scale with the upstream scalar ``s`` (and of g_V after the
    same product): one more rounding, on the product."""
    names = [n for n in GRADS + ("g_V",) if n in ref]
    r2 = {n: s * ref[n] for n in names}
    b2 = {n: abs(s) * b[n] + U * (r2[n].abs() + abs(s) * b[n]) * (b[n] > 0) for n in names}
    return r2, b2


def worst_ratio(got, want, bound):
    """max |got - want| / bound over ALL elements (nothing masked: got must be finite wherever it is compared); where the
    bound is zero the values must be equal."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = torch.as_tensor(bound).double().expand_as(want)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(bound).all())
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# Inputs shared by the GPU test and the CPU test (same recipe; fp32 CPU tensors, moved by the GPU test)

BETA, GAMMA = f32(0.05), f32(50.0)
HUB_BONDS = 40


def make_bonds(n_atoms, n_bonds, gen, pair=None):
    """int64 [n_bonds, 2]: a pair of distinct atoms whose reconstructed coordinates the caller makes coincide (``pair``,
    default (0, 1) -> lg = 1e-3), two self bonds, a reversed and a repeated bond, HUB_BONDS bonds of one hub atom (the last
    atom), the chain, random extra pairs -- in that order of precedence when n_bonds is small -- then shuffled, so the special
    bonds land in any chunk."""
    if n_bonds == 0:
        return torch.zeros(0, 2, dtype=torch.int64)
    p, q = pair if pair is not None else (0, min(1, n_atoms - 1))
    last = n_atoms - 1
    mid = n_atoms // 2
    rows = [(p, q), (mid, mid), (last, last), (min(2, last), min(1, last)), (min(1, last), min(2, last)), (min(1, last), min(2, last))]
    if last > 0:
        others = torch.randperm(last, generator=gen).tolist()                       # partners of the hub: atoms 0 .. last - 1
        rows += [(last, others[i % last]) if i % 2 else (others[i % last], last) for i in range(HUB_BONDS)]
    rows += [(i, i + 1) for i in range(n_atoms - 1)]
    rows = rows[:n_bonds]
    if len(rows) < n_bonds:
        extra = torch.randint(0, n_atoms, (n_bonds - len(rows), 2), generator=gen)
        rows += [tuple(r) for r in extra.tolist()]
    bonds = torch.tensor(rows, dtype=torch.int64)
    return bonds[torch.randperm(n_bonds, generator=gen)]


def bond_properties(bonds, xr, n_atoms):
    """What the bond list of a case holds: counted by the tests, required where the case is large enough."""
    a0, a1 = bonds[:, 0], bonds[:, 1]
    keys = (a0 * n_atoms + a1).tolist()
    seen = set(keys)
    coincide = (a0 != a1) & (xr[a0] == xr[a1]).all(-1)
    ends = torch.bincount(torch.cat([a0[a0 != a1], a1[a0 != a1]]), minlength=n_atoms)
    return {"self": int((a0 == a1).sum()), "repeated": len(keys) - len(seen),
            "reversed": sum(1 for x, y in zip(a0.tolist(), a1.tolist()) if x != y and y * n_atoms + x in seen) // 2,
            "coincident": int(coincide.sum()), "hub": int(ends.max()) if bonds.shape[0] else 0}


def _bead_inputs(n_beads, F, gen):
    mu, pmu = torch.randn(n_beads, F, generator=gen), torch.randn(n_beads, F, generator=gen)
    sigma, pstd = 0.5 + torch.rand(n_beads, F, generator=gen), 0.5 + torch.rand(n_beads, F, generator=gen)      # [0.5, 1.5]
    return {"mu": mu, "sigma": sigma, "prior_mu": pmu, "prior_std": pstd}


def elbo_inputs(n_beads, F, n_atoms, n_bonds, seed):
    """fp32 inputs of cgv_elbo_fwd: coordinates scaled by 4, xyz_recon of atoms 0 and 1 equal."""
    gen = torch.Generator().manual_seed(seed)
    inp = _bead_inputs(n_beads, F, gen)
    inp["xyz"], inp["xyz_recon"] = 4.0 * torch.randn(n_atoms, 3, generator=gen), 4.0 * torch.randn(n_atoms, 3, generator=gen)
    if n_atoms > 1:
        inp["xyz_recon"][1] = inp["xyz_recon"][0]
    inp["bonds"] = make_bonds(n_atoms, n_bonds, gen)
    return inp


def mapping_from_sizes(sizes, gen=None):
    """Atom -> bead index with ``sizes[b]`` atoms in bead b; shuffled (an unsorted mapping) when ``gen`` is given."""
    mapping = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return mapping[torch.randperm(mapping.numel(), generator=gen)] if gen is not None else mapping


def tail_inputs(sizes, F, n_bonds, seed, unsorted=True):
    """fp32 inputs of cgv_loss_tail for beads of the given sizes (<= F each).  The coinciding pair: the first two atoms of
    the first bead that owns two (equal rows of V); with one atom per bead, the atoms of beads 0 and 1 (equal rows of V and
    equal bead centres)."""
    gen = torch.Generator().manual_seed(seed)
    n_beads = len(sizes)
    assert max(sizes) <= F
    mapping = mapping_from_sizes(sizes, gen if unsorted else None)
    n_atoms = mapping.numel()
    inp = _bead_inputs(n_beads, F, gen)
    inp["mapping"], inp["chan"] = mapping, channel_index(mapping) if n_atoms else mapping
    inp["xyz"], inp["cg_xyz"] = 4.0 * torch.randn(n_atoms, 3, generator=gen), 4.0 * torch.randn(n_beads, 3, generator=gen)
    V = torch.randn(n_beads, F, 3, generator=gen)
    big = [b for b, s in enumerate(sizes) if s >= 2]
    pair = None
    if big:
        own = torch.nonzero(mapping == big[0]).flatten()[:2].tolist()
        V[big[0], inp["chan"][own[1]]] = V[big[0], inp["chan"][own[0]]]
        pair = (own[0], own[1])
    elif n_atoms > 1:
        own = [int(torch.nonzero(mapping == 0)[0]), int(torch.nonzero(mapping == 1)[0])]
        V[1, 0], inp["cg_xyz"][1] = V[0, 0], inp["cg_xyz"][0]
        pair = (own[0], own[1])
    inp["V"] = V
    inp["bonds"] = make_bonds(n_atoms, n_bonds, gen, pair)
    return inp


# ---- what selects a path on the host (restated; tests/test_elbo_cpu.py holds the library's predicates to it)

KL_ROUND = 4 * 1024                  # elbo_fwd: KB = 4 rounds of 1024 threads in flight
CHUNK = 2048                         # CH = BOND_CH = LT_CH
LT_NP_ELEMS = 2 * 1024               # loss_tail_k: LT_NP register slots x 1024 threads


def kl_blocks(n_beads, F):
    nk = n_beads * F
    return 0 if nk < 16384 else min((nk + 1023) // 1024, 128)


def bond_blocks(n_atoms, n_bonds, gamma, workspace=True):
    """Blocks of elbo_bond_k; 0: the bond term runs in elbo_fwd's single block."""
    return (n_atoms + 63) // 64 if workspace and gamma != 0.0 and n_bonds > 0 and n_atoms * n_bonds >= 512 * 1024 else 0


def fwd_groups(n_atoms):
    """G of elbo_fwd's bond scan."""
    return min(4, 1024 // n_atoms) if 2 * n_atoms <= 1024 else 1


def tail_supported(n_beads, F, n_atoms, n_bonds):
    return 1 <= n_beads <= 2048 and 1 <= n_atoms <= 4096 and n_atoms + n_beads <= 3072 and F >= 1 and n_bonds >= 0


# cgv_elbo_fwd, KL path: (n_beads, F, blocks of elbo_kl_k, 4-deep rounds of the single block), 5 atoms and 6 bonds
KL_CASES = [(1, 1, 0, 1), (3, 30, 0, 1), (7, 585, 0, 1), (64, 64, 0, 1), (17, 241, 0, 2), (127, 129, 0, 4),
            (128, 128, 16, 4), (300, 440, 128, 33)]
KL_ATOMS, KL_BONDS = 5, 6

# cgv_elbo_fwd, bond path: (n_atoms, n_bonds, gamma, workspace, G of elbo_fwd or 0, blocks of elbo_bond_k, chunks), 3 x 8
# bead elements.  atoms x bonds >= 512 x 1024 sends the bond term to elbo_bond_k WHEN there is a workspace: the shapes of
# the issue's table that cross it (1025 atoms; 2047 .. 4100 bonds at 300 atoms) run elbo_fwd's single block -- which the
# table is about -- through the no-workspace fallback, and elbo_bond_k with a workspace.
BOND_CASES = (
    [(n, max(1, round(1.2 * n)), GAMMA, True, g, 0, 1) for n, g in ((2, 4), (256, 4), (257, 3), (341, 3), (342, 2), (512, 2), (513, 1))]
    + [(1025, 1230, GAMMA, False, 1, 0, 1), (1025, 1230, GAMMA, True, 0, 17, 1)]
    + [(300, m, GAMMA, True, 3, 0, 1) for m in (1, 15, 16, 17)]
    + [(300, m, GAMMA, False, 3, 0, c) for m, c in ((2047, 1), (2048, 1), (2049, 2), (4100, 3))]
    + [(300, m, GAMMA, True, 0, 5, c) for m, c in ((2047, 1), (2048, 1), (2049, 2), (4100, 3))]
    + [(300, 0, GAMMA, True, 3, 0, 0), (300, 360, 0.0, True, 3, 0, 1)]
    + [(65, 8066, GAMMA, True, 0, 2, 4), (700, 750, GAMMA, True, 0, 11, 1), (513, 1022, GAMMA, True, 1, 0, 1)])
BOND_BEADS, BOND_F = 3, 8


def _even(n_atoms, n_beads):
    return [n_atoms // n_beads + (1 if b < n_atoms % n_beads else 0) for b in range(n_beads)]


# cgv_loss_tail: name -> (bead sizes, F, n_bonds, gamma, offset, unsorted)
TAIL_CASES = {
    "base-offset": ([10, 12, 7, 11, 9, 13, 8, 10], 16, 96, GAMMA, True, True),          # 2 frames x 40 atoms, 4 beads each
    "base-no-offset": ([10, 12, 7, 11, 9, 13, 8, 10], 16, 96, GAMMA, False, True),
    "bead-sizes-1-32-33-64-65": ([1, 32, 33, 64, 65], 80, 234, GAMMA, True, True),      # single pass | two | two | three passes
    "empty-bead": ([5, 0, 7, 3], 8, 60, GAMMA, True, True),
    "bonds-2049": ([30] * 10, 32, 2049, GAMMA, True, True),                             # the second LT_CH chunk: one bond
    "bonds-4100": ([30] * 10, 32, 4100, GAMMA, True, True),                             # ... and a third
    "atoms-2050": (_even(2050, 41), 64, 2460, GAMMA, True, False),                      # atom loops past the register slots
    "atoms-3000": (_even(3000, 72), 64, 3600, GAMMA, True, False),                      # n_atoms + n_beads = 3072: the last supported
    "kl-loop-F-2050": ([5], 2050, 64, GAMMA, True, True),                               # KL loop past the register slots
    "beads-1025": ([1] * 1025, 4, 600, GAMMA, True, True),                              # last block's sum: two trips; beads > bonds
    "gamma-0": ([10, 12, 7, 11, 9, 13, 8, 10], 16, 96, 0.0, True, True),
    "no-bonds": ([10, 12, 7, 11, 9, 13, 8, 10], 16, 0, GAMMA, True, True),
}
TAIL_UNSUPPORTED = (_even(3001, 72), 64, 3600, GAMMA, True, False)                      # n_atoms + n_beads = 3073
