"""GPU parity: the HIP path (through the C ABI) against (a) golden vectors produced by the
reference, (b) the CPU oracle on the same seeded inputs, (c) size-independent properties.
Tolerance: north_star's 1e-4 relative fp32 (norm-relative, written below); integer/index
work (edge lists, CSR plans) is bit-exact."""
import contextlib
import numpy as np
import pytest
import torch

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd.graph import EdgeGeometry, EdgePlan
from oracle import cgvae_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-4        # BASELINE.json: "within 1e-4 relative fp32"


def t(a):
    return torch.from_numpy(np.asarray(a))


def dev(a):
    return t(a).to(DEV)


def rel_err(got, ref):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def assert_close(got, ref, what="", tol=REL):
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: relative error {e:.3e} > {tol:.1e}"


def load_block(block, g):
    sd = {k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}
    block.load_state_dict(sd, strict=True)
    return block.to(DEV)


def check_param_grads(block, g, tol=REL):
    for name, p in block.named_parameters():
        ref = g["g." + name]
        if ref.size == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
        else:
            assert p.grad is not None, name
            assert_close(p.grad, ref, "grad " + name, tol)


# --------------------------------------------------------------------------- K7 / K6 / K1
def test_csr_plan_is_sorted_by_row_then_partner_then_edge_id():
    gen = torch.Generator().manual_seed(0)
    n, E = 37, 900
    nbrs = torch.randint(0, n, (E, 2), generator=gen)
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n)
    for key_col, rowptr, eid, dst, src in ((0, plan.rowptr_d, plan.eid_d, plan.dst_d, plan.src_d),
                                           (1, plan.rowptr_s, plan.eid_s, plan.dst_s, plan.src_s)):
        nb = nbrs.numpy()
        order = np.lexsort((np.arange(E), nb[:, 1 - key_col], nb[:, key_col]))
        assert np.array_equal(eid.cpu().numpy(), order)
        if key_col == 0:                                  # ... which is what the C oracle defines
            import ctypes as C
            from test_oracle_c import _load as load_orc
            orc = load_orc()
            rp, perm = np.zeros(n + 1, dtype=np.int32), np.zeros(E, dtype=np.int32)
            orc.orc_csr_sorted(nb.ctypes.data, nb[:, 1:].ctypes.data, 2, E, n, n, rp.ctypes.data, perm.ctypes.data)
            assert np.array_equal(perm, order) and np.array_equal(rp, rowptr.cpu().numpy())
        assert np.array_equal(dst.cpu().numpy(), nbrs[order, 0].numpy())
        assert np.array_equal(src.cpu().numpy(), nbrs[order, 1].numpy())
        want = np.searchsorted(nbrs[order, key_col].numpy(), np.arange(n + 1), side="left")
        assert np.array_equal(rowptr.cpu().numpy(), want)
    empty = EdgePlan.from_nbrs(torch.zeros(0, 2, dtype=torch.long, device=DEV), 5)
    assert empty.rowptr_d.cpu().tolist() == [0] * 6
    mp = EdgePlan.from_mapping(torch.tensor([2, 0, 0, 1, 2, 2], device=DEV), 4)
    assert mp.rowptr_d.cpu().tolist() == [0, 2, 3, 6, 6]
    assert mp.src_d.cpu().tolist() == [1, 2, 3, 0, 4, 5]
    assert mp.rowptr_s.cpu().tolist() == list(range(7)) and mp.dst_s.cpu().tolist() == [2, 0, 0, 1, 2, 2]


@pytest.mark.parametrize("R,cutoff", [(8, 6.0), (10, 3.0), (10, 25.0)])
def test_edge_geometry_matches_oracle(R, cutoff):
    gen = torch.Generator().manual_seed(1)
    n = 50
    xyz = torch.rand(n, 3, generator=gen) * 5
    xyz[7] = xyz[3]                                       # coincident pair: d = sqrt(3e-8)
    und = O.get_neighbor_list(xyz, 4.5, True)
    nbrs, _ = O.make_directed(und)
    nbrs = torch.cat([nbrs, torch.tensor([[3, 7], [7, 3]])])
    r = xyz[nbrs[:, 1]] - xyz[nbrs[:, 0]]
    dist, unit = O.preprocess_r(r)
    env = O.cosine_envelope(dist, cutoff)
    want = torch.cat([O.painn_rbf(dist, R, cutoff) * env[:, None], env[:, None], unit], dim=1)
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n)
    for geom in (EdgeGeometry(plan, R, cutoff, r_edges=r.to(DEV)),
                 EdgeGeometry(plan, R, cutoff, pos_dst=xyz.to(DEV), pos_src=xyz.to(DEV))):
        got_d = geom.columns(geom.geom_d).cpu()
        got_s = geom.columns(geom.geom_s).cpu()
        U = geom.unit_offset
        assert torch.equal(geom.geom_d[:, U:U + 3], geom.geom_d[:, U + 3:U + 6])      # unit stored twice
        assert_close(got_d, want[plan.eid_d.cpu().long()], "geom_d", 2e-6)
        assert_close(got_s, want[plan.eid_s.cpu().long()], "geom_s", 2e-6)
    assert (want[:, :R].abs().sum(1) == 0).any() or cutoff > 4.5      # beyond-cutoff rows exercised for cutoff 3.0


@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_distance_embed_golden_through_the_fused_kernel(tag):
    """a7 ``DistanceEmbed`` (modules.py:175-197) standalone against the reference's own output: the filter
    w = (rbf Wd^T + bd) * env exists only inside the fused edge kernels, so it is read back through K2 on a star graph
    (receiver i <- one source, edge vector of length dist_i along x): with phi = 1 and v_src = (0, 1, 0),
    ds_i = w[F:2F], dv_i[:, y] = w[0:F], dv_i[:, x] = w[2F:3F] * unit_x.  The golden's special distances (0, cutoff,
    1.5 cutoff) are covered: d = sqrt(r_x^2 + 3e-8) reproduces them within an ulp, where the outputs are continuous
    (limits n pi / cut at 0, zero from the cutoff on)."""
    g = load_golden(f"g1_distance_embed_{tag}")
    R, cutoff = int(g["R"]), float(g["cutoff"])
    dist, want = t(g["dist"]).double(), t(g["out"])
    E, F = dist.shape[0], want.shape[1] // 3
    rx = (dist ** 2 - 3e-8).clamp_min(0).sqrt().float()
    r = torch.stack([rx, torch.zeros(E), torch.zeros(E)], dim=1)
    nbrs = torch.stack([torch.arange(E), torch.full((E,), E)], dim=1)             # receiver i <- source E
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), E + 1)
    geom = EdgeGeometry(plan, R, cutoff, r_edges=r.to(DEV))
    phi = torch.ones(E + 1, 3 * F, device=DEV)
    v = torch.zeros(E + 1, F, 3, device=DEV)
    v[E, :, 1] = 1.0
    ds, dv = cg.ops.equi_message(phi, v, dev(g["p.block.1.weight"]), dev(g["p.block.1.bias"]), plan, geom, True)
    assert_close(ds[:E], want[:, F:2 * F], "filter slice 1")
    assert_close(dv[:E, :, 1], want[:, :F], "filter slice 0")
    d32 = (rx.double() ** 2 + 3e-8).sqrt()
    ux = (rx.double() / d32).float()
    assert_close(dv[:E, :, 0], want[:, 2 * F:] * ux[:, None], "filter slice 2 (times unit_x)")
    assert float(ds[E].abs().max()) == 0.0 and float(dv[E].abs().max()) == 0.0      # a receiver without edges
    beyond = dist >= cutoff * 1.2
    assert bool(beyond.any()) and float(ds[:E][beyond].abs().max()) == 0.0           # exactly zero past the cutoff


def test_scatter_matches_reference_semantics():
    g = load_golden("g5_scatter")
    idx = dev(g["index"])
    assert_close(cg.scatter_add(dev(g["src2"]), idx, dim=0, dim_size=7), g["add2"], "add2", 1e-6)
    assert_close(cg.scatter_add(dev(g["src3"]), idx, dim=0), g["add3"], "add3", 1e-6)
    assert_close(cg.scatter_mean(dev(g["src2"]), idx, dim=0), g["mean2"], "mean2", 1e-6)
    assert_close(cg.scatter_mean(dev(g["src3"]), idx, dim=0, dim_size=7), g["mean3"], "mean3", 1e-6)


@pytest.mark.parametrize("E,C,n", [(5000, 1800, 97), (300, 7, 11), (1, 4, 3), (4096, 600, 1)])
def test_scatter_add_and_grad_vs_fp64(E, C, n):
    gen = torch.Generator().manual_seed(E)
    src = torch.randn(E, C, generator=gen)
    idx = torch.randint(0, n, (E,), generator=gen)
    want = torch.zeros(n, C, dtype=torch.float64).index_add_(0, idx, src.double())
    x = src.to(DEV).requires_grad_(True)
    out = cg.scatter_add(x, idx.to(DEV), dim_size=n)
    assert_close(out, want, "scatter_add", 1e-5)   # fp32 running sum of up to 4096 rows vs fp64
    gout = torch.randn(n, C, generator=gen)
    out.backward(gout.to(DEV))
    assert torch.equal(x.grad.cpu(), gout[idx])
    mean = cg.scatter_mean(src.to(DEV), idx.to(DEV), dim_size=n)
    cnt = torch.bincount(idx, minlength=n).clamp(min=1)[:, None]
    assert_close(mean, want / cnt, "scatter_mean", 1e-5)


# --------------------------------------------------------------------------- K2 / K4 blocks vs golden
@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_equi_message_block_golden(tag):
    g = load_golden(f"g1_equi_message_{tag}")
    F = g["s"].shape[1]
    blk = load_block(cg.EquiMessageBlock(F, "swish", int(g["R"]), float(g["cutoff"]), 0.0), g)
    s = dev(g["s"]).requires_grad_(True)
    v = dev(g["v"]).requires_grad_(True)
    ds, dv = blk(s, v, dev(g["r_ij"]), dev(g["nbrs"]))
    assert_close(ds, g["ds"], "ds")
    assert_close(dv, g["dv"], "dv")
    ((ds * dev(g["gout_s"])).sum() + (dv * dev(g["gout_v"])).sum()).backward()
    assert_close(s.grad, g["gin_s"], "grad s")
    assert_close(v.grad, g["gin_v"], "grad v")
    check_param_grads(blk, g)


@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_equi_message_block_scalar_only_backward(tag):
    """gv = None path (the encoder's case: the vector channel is never consumed)."""
    g = load_golden(f"g1_equi_message_{tag}")
    F = g["s"].shape[1]
    P = {"blk." + k[2:]: t(v).clone().requires_grad_(True) for k, v in g.items() if k.startswith("p.")}
    s0 = t(g["s"]).requires_grad_(True)
    ds0, _ = O.equi_message_block(s0, t(g["v"]), t(g["r_ij"]), t(g["nbrs"]), P, "blk", O.swish, int(g["R"]),
                                  float(g["cutoff"]))
    (ds0 * t(g["gout_s"])).sum().backward()
    for with_dv in (True, False):
        blk = load_block(cg.EquiMessageBlock(F, "swish", int(g["R"]), float(g["cutoff"]), 0.0), g)
        blk.with_dv = with_dv
        s = dev(g["s"]).requires_grad_(True)
        ds, dv = blk(s, dev(g["v"]), dev(g["r_ij"]), dev(g["nbrs"]))
        assert_close(ds, g["ds"], "ds")
        if not with_dv:
            assert float(dv.abs().max()) == 0.0
        (ds * dev(g["gout_s"])).sum().backward()
        assert_close(s.grad, s0.grad, "grad s (scalar only)")
        for name, p in blk.named_parameters():
            ref = P["blk." + name].grad
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            else:
                assert_close(p.grad, ref, "grad " + name)


@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_contractive_block_golden(tag):
    g = load_golden(f"g1_contractive_{tag}")
    F = g["s"].shape[1]
    blk = load_block(cg.ContractiveMessageBlock(F, "swish", int(g["R"]), float(g["cutoff"]), 0.0), g)
    s = dev(g["s"]).requires_grad_(True)
    v = dev(g["v"]).requires_grad_(True)
    dS, dV = blk(s, v, dev(g["r_iI"]), dev(g["mapping"]))
    assert_close(dS, g["dS"], "dS")
    assert_close(dV, g["dV"], "dV")
    ((dS * dev(g["gout_S"])).sum() + (dV * dev(g["gout_V"])).sum()).backward()
    assert_close(s.grad, g["gin_s"], "grad s")
    assert_close(v.grad, g["gin_v"], "grad v")
    check_param_grads(blk, g)


@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_equi_pseudo_block_golden(tag):
    g = load_golden(f"g1_equi_pseudo_{tag}")
    F = g["s"].shape[1]
    blk = load_block(cg.EquiMessagePsuedo(F, "swish", int(g["R"]), float(g["cutoff"]), 0.0), g)
    ins = [dev(g[k]).requires_grad_(True) for k in ("s", "sbar", "v", "vbar")]
    outs = blk(*ins, dev(g["r_ij"]), dev(g["nbrs"]))
    for o, k in zip(outs, ("dh", "dhbar", "dv", "dvbar")):
        assert_close(o, g[k], k)
    sum((o * dev(g["gout_" + k])).sum() for o, k in zip(outs, ("h", "hbar", "v", "vbar"))).backward()
    for x, k in zip(ins, ("s", "sbar", "v", "vbar")):
        assert_close(x.grad, g["gin_" + k], "grad " + k)
    check_param_grads(blk, g)


@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_update_block_golden(tag):
    g = load_golden(f"g1_update_{tag}")
    F = g["s"].shape[1]
    blk = load_block(cg.UpdateBlock(F, "swish", 0.0), g)
    s = dev(g["s"]).requires_grad_(True)
    v = dev(g["v"]).requires_grad_(True)
    ds, dv = blk(s, v)
    assert_close(ds, g["ds"], "ds")
    assert_close(dv, g["dv"], "dv")
    ((ds * dev(g["gout_s"])).sum() + (dv * dev(g["gout_v"])).sum()).backward()
    assert_close(s.grad, g["gin_s"], "grad s")
    assert_close(v.grad, g["gin_v"], "grad v")
    check_param_grads(blk, g)


# --------------------------------------------------------------------------- model level vs golden
def _golden_model(g, det=False):
    m = cg.build_model(int(g["F"]), int(g["R"]), float(g["atom_cutoff"]), float(g["cg_cutoff"]),
                       int(g["enc_nconv"]), int(g["dec_nconv"]), int(g["n_cgs"]), det=det, seed=None)
    m.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("tag", ["ncg3", "ncg6"])
@pytest.mark.parametrize("prepared", [True, False])
def test_model_forward_loss_and_grads_golden(tag, prepared):
    g = load_golden(f"g2_model_{tag}")
    model = _golden_model(g)
    batch = {k[2:]: dev(v) for k, v in g.items() if k.startswith("b.")}
    if prepared:
        batch = cg.prepare_batch(batch)
    out = model(batch, eps=dev(g["eps"]))
    for o, k in zip(out, ("mu", "sigma", "prior_mu", "prior_std", "xyz", "xyz_recon")):
        assert_close(o, g[k], k)
    loss, kl, recon, graph = cg.loss_terms(out, batch, float(g["beta"]), float(g["gamma"]))
    for o, k in zip((loss, kl, recon, graph), ("loss", "kl", "recon", "graph")):
        assert_close(o, g[k], k)
    loss.backward()
    live = set(g["live_params"].tolist())
    for name, p in model.named_parameters():
        if name in live:
            assert p.grad is not None, name
            assert_close(p.grad, g["g." + name], "grad " + name)            # observed <= 2.3e-6 (tools/grad_err_probe.py)
        else:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
    det = _golden_model(g, det=True)
    out_det = det(batch)
    assert_close(out_det[5], g["det_xyz_recon"], "det xyz_recon")


@pytest.mark.parametrize("tag", ["ncg3"])
def test_skip_dead_vector_channel_is_output_neutral(tag):
    g = load_golden(f"g2_model_{tag}")
    model = _golden_model(g, det=True)
    batch = cg.prepare_batch({k[2:]: dev(v) for k, v in g.items() if k.startswith("b.")})
    ref = [o.clone() for o in model(batch)]
    model.encoder.set_skip_dead_vector_channel(True)
    model.prior_net.set_skip_dead_vector_channel(True)
    # the outputs do not depend on the encoder's vector channel at all; the two runs only differ in the order the
    # scalar messages are summed (shared-source walk with the vector channel, per-receiver walk without it)
    for a, b in zip(model(batch), ref):
        assert_close(a, b, "skip-dead-vector-channel output", 2e-6)


# --------------------------------------------------------------------------- K0 radius graph
def test_radius_graph_bit_exact_golden():
    g = load_golden("g3_radius_graph")
    for name in sorted({k.split(".")[0] for k in g}):
        xyz, cut = g[name + ".xyz"], float(g[name + ".cutoff"])
        for und, key in ((True, "und"), (False, "dir")):
            got = cg.get_neighbor_list(xyz, DEV, cut, undirected=und).cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got, g[f"{name}.{key}"]), (name, key)


def test_radius_graph_batched_matches_oracle_per_frame():
    gen = torch.Generator().manual_seed(4)
    sizes = [22, 1, 166, 64, 2]
    frames = [torch.rand(n, 3, generator=gen) * 12.0 for n in sizes]
    fp = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    for cutoff, und in ((8.5, True), (12.0, False), (3.0, True)):
        got = cg.radius_graph(torch.cat(frames).to(DEV), fp.to(DEV), cutoff, und).cpu()
        want = torch.cat([O.get_neighbor_list(x, cutoff, und) + int(o) for x, o in zip(frames, fp[:-1])])
        assert torch.equal(got, want)


# --------------------------------------------------------------------------- full-size parity vs live oracle
def _oracle_params_from(model):
    return {k: v.detach().cpu().clone().requires_grad_(v.dtype == torch.float32) for k, v in model.state_dict().items()}


def test_full_width_block_vs_oracle_F600():
    """EquiMessageBlock at the real width (F=600, R=8, dipeptide-like graph) against the oracle."""
    torch.manual_seed(0)
    F, R, cutoff, n = 600, 8, 9.5, 66
    gen = torch.Generator().manual_seed(2)
    xyz = torch.rand(n, 3, generator=gen) * 6.0
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 8.5, True))
    r = xyz[nbrs[:, 1]] - xyz[nbrs[:, 0]]
    blk = cg.EquiMessageBlock(F, "swish", R, cutoff, 0.0)
    for p in blk.parameters():
        if p.dim() == 1:
            p.data.normal_(0, 0.2)
    P = {"b." + k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    s = torch.randn(n, F, generator=gen)
    v = torch.randn(n, F, 3, generator=gen)
    gs, gv = torch.randn(n, F, generator=gen), torch.randn(n, F, 3, generator=gen)
    s0, v0 = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ds0, dv0 = O.equi_message_block(s0, v0, r, nbrs, P, "b", O.swish, R, cutoff)
    ((ds0 * gs).sum() + (dv0 * gv).sum()).backward()
    blk = blk.to(DEV)
    s1, v1 = s.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    ds1, dv1 = blk(s1, v1, r.to(DEV), nbrs.to(DEV))
    ((ds1 * gs.to(DEV)).sum() + (dv1 * gv.to(DEV)).sum()).backward()
    assert_close(ds1, ds0, "ds")
    assert_close(dv1, dv0, "dv")
    assert_close(s1.grad, s0.grad, "grad s")
    assert_close(v1.grad, v0.grad, "grad v")
    for name, p in blk.named_parameters():
        ref = P["b." + name].grad
        if ref is not None:
            assert_close(p.grad, ref, "grad " + name)


@pytest.mark.parametrize("workload,n_frames,F", [("dipeptide", 4, 600), ("chignolin", 1, 128)])
def test_model_step_vs_live_oracle(workload, n_frames, F):
    """Whole model (run_ala wiring) on synthetic frames: outputs, ELBO terms and gradients
    against the CPU oracle run live on the host cores."""
    w = cg.data.WORKLOADS[workload]
    batch = cg.synthetic_batch(workload, n_frames=n_frames, seed=0, device=DEV)
    model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"],
                           w["n_cgs"], seed=123)
    hp = O.Hyper(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], w["enc_nconv"], w["dec_nconv"], w["n_cgs"])
    P = _oracle_params_from(model)
    cpu_batch = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    # the device radius graph must equal the oracle's, bit for bit
    start = 0
    for k in range(n_frames):
        fr = cpu_batch["nxyz"][start:start + w["n_atoms"], 1:]
        want = O.get_neighbor_list(fr, w["atom_cutoff"], True) + start
        sel = (cpu_batch["nbr_list"][:, 0] >= start) & (cpu_batch["nbr_list"][:, 0] < start + w["n_atoms"])
        assert torch.equal(cpu_batch["nbr_list"][sel], want)
        start += w["n_atoms"]
    eps = torch.randn(cpu_batch["CG_nxyz"].shape[0], F, generator=torch.Generator().manual_seed(9))
    out0 = O.model_forward(cpu_batch, P, hp, eps=eps)
    loss0, kl0, recon0, graph0 = O.loss_terms(out0, cpu_batch, w["beta"], w["gamma"])
    loss0.backward()
    model = model.to(DEV)
    out1 = model(batch, eps=eps.to(DEV))
    loss1, kl1, recon1, graph1 = cg.loss_terms(out1, batch, w["beta"], w["gamma"])
    loss1.backward()
    for a, b, k in zip(out1, out0, ("mu", "sigma", "prior_mu", "prior_std", "xyz", "xyz_recon")):
        assert_close(a, b, k)
    for a, b, k in ((loss1, loss0, "loss"), (kl1, kl0, "kl"), (recon1, recon0, "recon"), (graph1, graph0, "graph")):
        assert_close(a, b, k)
    n_live = 0
    for name, p in model.named_parameters():
        ref = P[name].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
        else:
            n_live += 1
            assert_close(p.grad, ref, "grad " + name)                      # REL: observed <= 1.8e-5, u_mat / v_mat of the decoder (tools/grad_err_probe.py)
    assert n_live > 50


def test_rotation_equivariance_and_translation_invariance():
    """Properties the reference never tested: xyz_recon rotates with the input, mu does not move."""
    w = cg.data.WORKLOADS["dipeptide"]
    batch = cg.synthetic_batch("dipeptide", n_frames=2, seed=3, device=DEV)
    model = cg.build_model(64, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 2, w["n_cgs"], det=True).to(DEV)
    out = model(batch)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(1)))
    if torch.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    Q = Q.to(DEV)
    shift = torch.tensor([1.5, -2.0, 0.7], device=DEV)
    b2 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items() if k != "_graph"}
    b2["nxyz"][:, 1:] = batch["nxyz"][:, 1:] @ Q.T + shift
    b2["CG_nxyz"][:, 1:] = batch["CG_nxyz"][:, 1:] @ Q.T + shift
    out2 = model(cg.prepare_batch(b2))
    assert_close(out2[0], out[0], "mu invariance", 1e-4)
    assert_close(out2[5], out[5] @ Q.T + shift, "xyz_recon equivariance", 1e-4)


# --------------------------------------------------------------------------- trainer: arena + fused clip/Adam + hipGraph
def test_trainer_trajectory_matches_oracle_training():
    """Five full training steps (3 eager, then the captured hipGraph replayed twice) against the oracle's
    reference-style loop (zero_grad, backward, clip_grad_norm_(0.01), torch Adam), step by step:
    loss, gradient norm and clip coefficient at every step; Adam's moments and the parameters after the first step
    (tight: they are linear / quadratic in the clipped gradient) and after the last one."""
    from test_full_size_parity import OracleTraining, _check_moments, _check_norm_and_clip, _check_parameters
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["dipeptide"]
    F, frames, lr = 64, 4, 1e-3
    batch = cg.synthetic_batch("dipeptide", n_frames=frames, seed=5, device=DEV)
    model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 2, w["n_cgs"], det=True, seed=123)
    hp = O.Hyper(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 2, w["n_cgs"], det=True)
    P = _oracle_params_from(model)
    P0 = {k: v.detach().clone() for k, v in P.items()}
    cpu_batch = {k: v.cpu() for k, v in batch.items() if torch.is_tensor(v)}
    oracle = OracleTraining(cpu_batch, P, hp, w, lr)
    model = model.to(DEV)
    tr = Trainer(model, lr=lr, beta=w["beta"], gamma=w["gamma"])
    ref_losses, losses = [], []
    for k in range(5):
        if k == 3:
            tr.capture(batch, warmup=0)        # capturing executes nothing on the device: the replays are steps 4 and 5
        ref = oracle.step(None)
        tr.step(batch)
        ref_losses.append(float(ref["loss"]))
        losses.append(float(tr.last_loss))
        # the loss of step k sees parameters that took k Adam steps; where |clipped g| ~ 1e-8 (Adam's eps) an update
        # is ill-conditioned (test_full_size_parity._check_parameters), so the bound grows with k: 1e-4 (north_star)
        # on the first step, 1e-4 * (1 + k) afterwards
        assert abs(losses[-1] - ref_losses[-1]) <= 1e-4 * (1 + k) * abs(ref_losses[-1]), (k, losses, ref_losses)
        _check_norm_and_clip(tr, ref, f"step {k + 1}")
        if k == 0:
            _check_moments(tr, model, oracle, "step 1")
            _check_parameters(tr, model, oracle, P0, 1, lr, "step 1")
    assert tr.replays == 2 and int(tr.state[0].item()) == 5 and tr.skipped_steps() == 0
    assert ref_losses[-1] < ref_losses[0]                      # it actually trains
    _check_parameters(tr, model, oracle, P0, 5, lr, "step 5")


def test_direct_gradient_writes_equal_autograd_accumulation():
    """Arena mode writes weight gradients in place (primitives._direct_grad); they must equal what
    plain autograd accumulation produces, including for a parameter used twice in one step."""
    from coarsegrainingvae_amd.trainer import ParamArena
    torch.manual_seed(0)
    lin = cg.primitives.Linear(24, 16).to(DEV)
    x1, x2 = torch.randn(5, 24, device=DEV), torch.randn(7, 24, device=DEV)
    (lin(x1).pow(2).sum() + lin(x2).sum()).backward()
    ref_w, ref_b = lin.weight.grad.clone(), lin.bias.grad.clone()
    arena = ParamArena(list(lin.parameters()))
    assert lin.weight._cgv_direct and not arena.accumulated
    arena.g.fill_(float("nan"))                                # direct writes must not depend on a zero-fill
    arena.zero_grad()
    (lin(x1).pow(2).sum() + lin(x2).sum()).backward()
    assert_close(lin.weight.grad, ref_w, "weight grad", 1e-5)
    assert_close(lin.bias.grad, ref_b, "bias grad", 1e-5)


# --------------------------------------------------------------------------- decoder tail
@pytest.mark.parametrize("offset", [True, False])
def test_reconstruct_matches_indexing_ops(offset):
    """cgvae.py:462-481 as tensor ops (advanced-index gathers + scatter_mean) vs the fused launch, values and
    gradients; ragged beads including an empty one."""
    from coarsegrainingvae_amd.graph import EdgePlan
    gen = torch.Generator().manual_seed(5)
    sizes = [7, 1, 0, 23, 70, 4]                      # atoms per bead (bead 2 is empty, bead 4 spans > one wave)
    n_beads, F = len(sizes), 96
    mapping = torch.cat([torch.full((n,), b, dtype=torch.int64) for b, n in enumerate(sizes)])
    perm = torch.randperm(mapping.numel(), generator=gen)
    mapping = mapping[perm].to(DEV)                   # atoms of a bead are not contiguous in general
    n_atoms = mapping.numel()
    model_chan = cg.CGequiVAE.CG2ChannelIdx(None, mapping)
    v = torch.randn(n_beads, F, 3, generator=gen).to(DEV)
    cg_xyz = torch.randn(n_beads, 3, generator=gen).to(DEV)
    gout = torch.randn(n_atoms, 3, generator=gen).to(DEV)
    vd, cd = v.double().requires_grad_(True), cg_xyz.double().requires_grad_(True)
    rel = vd[mapping, model_chan, :]
    if offset:
        cnt = torch.bincount(mapping, minlength=n_beads).clamp(min=1).double().unsqueeze(1)
        mean = torch.zeros(n_beads, 3, dtype=torch.float64, device=DEV).index_add_(0, mapping, rel) / cnt
        rel = rel - mean[mapping]
    ref = rel + cd[mapping]
    ref.backward(gout.double())
    plan = EdgePlan.from_mapping(mapping, n_beads)
    vg, cgx = v.clone().requires_grad_(True), cg_xyz.clone().requires_grad_(True)
    out = cg.ops.reconstruct(vg, cgx, model_chan, plan, offset)
    out.backward(gout)
    assert_close(out, ref, "xyz_recon", 1e-6)
    assert_close(vg.grad, vd.grad, "g_v", 1e-6)
    assert_close(cgx.grad, cd.grad, "g_cg_xyz", 1e-6)


# --------------------------------------------------------------------------- skinny GEMMs (bead-level Dense layers)
@pytest.mark.parametrize("M,N,K", [(12, 600, 600), (12, 5400, 600), (36, 600, 600), (12, 600, 1200), (12, 1800, 600),
                                   (1, 4, 4), (64, 72, 40), (17, 52, 1000), (3, 5400, 24),
                                   # beyond 64 rows: the reduction-split tile kernels (csrc/tile_gemm.hip)
                                   (332, 600, 600), (332, 1800, 600), (96, 600, 1200), (65, 52, 1000), (100, 36, 28),
                                   (1000, 64, 64)])
def test_skinny_linear_fwd_bwd_vs_fp64(M, N, K):
    gen = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen)
    gy = torch.randn(M, N, generator=gen)
    xd, Wd_, bd_ = (t.double().requires_grad_(True) for t in (x, W, b))
    yd = torch.nn.functional.linear(xd, Wd_, bd_)
    yd.backward(gy.double())
    lin = cg.primitives.Linear(K, N).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    xg = x.to(DEV).requires_grad_(True)
    y = lin(xg)
    y.backward(gy.to(DEV))
    assert_close(y, yd, "y", 2e-6)
    assert_close(xg.grad, xd.grad, "gx", 2e-6)
    assert_close(lin.weight.grad, Wd_.grad, "gW", 2e-6)
    assert_close(lin.bias.grad, bd_.grad, "gb", 2e-6)
    # no-bias flavour (u_mat / v_mat) on a 3-D input
    y2 = cg.primitives.linear(xg.detach().reshape(1, M, K), lin.weight.detach())
    assert_close(y2[0], (xd @ Wd_.t()).detach(), "y no bias", 2e-6)


@pytest.mark.parametrize("M,N,K,act", [(12, 1800, 600, 0), (12, 600, 1200, 1), (36, 1200, 600, 0), (64, 5400, 24, 1),
                                        (96, 5400, 600, 0), (80, 1800, 600, 1), (128, 600, 132, 1), (65, 4100, 64, 0)])
def test_skinny_bwd_input_row_split_is_deterministic_and_rearms(M, N, K, act):
    """The row-split bwd_input meets in a workspace: repeated launches must agree bit for bit (fixed summation
    order, no stale partial ever read), and the one-block-per-column-tile flavour (no workspace) must agree
    to rounding."""
    from coarsegrainingvae_amd import _lib
    gen = torch.Generator().manual_seed(N + K)
    gy = torch.randn(M, N, generator=gen).to(DEV)
    z = torch.randn(M, N, generator=gen).to(DEV)
    W = (torch.randn(N, K, generator=gen) / N ** 0.5).to(DEV)
    lib = _lib.load()
    nbytes = lib.cgv_skinny_bwd_input_workspace_bytes(M, N, K)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(4):
        gx = torch.full((M, K), float("nan"), device=DEV)
        ws.fill_(255)                                      # NaN bit patterns: stale partials must never be read
        _lib.call("cgv_skinny_linear_bwd_input", gy.data_ptr(), z.data_ptr() if act else None, W.data_ptr(),
                  gx.data_ptr(), M, N, K, act, ws.data_ptr(), nbytes, _lib.stream_ptr())
        outs.append(gx)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    g = gy.double()
    if act:
        sg = torch.sigmoid(z.double())
        g = g * (sg * (1 + z.double() * (1 - sg)))
    assert_close(outs[0], g @ W.double(), "gx split", 2e-6)
    gx1 = torch.full((M, K), float("nan"), device=DEV)
    _lib.call("cgv_skinny_linear_bwd_input", gy.data_ptr(), z.data_ptr() if act else None, W.data_ptr(), gx1.data_ptr(),
              M, N, K, act, None, 0, _lib.stream_ptr())
    assert_close(gx1, g @ W.double(), "gx single", 2e-6)


def test_skinny_direct_gradient_accumulation():
    from coarsegrainingvae_amd.trainer import ParamArena
    torch.manual_seed(1)
    lin = cg.primitives.Linear(600, 1800).to(DEV)
    x1, x2, x3 = torch.randn(12, 600, device=DEV), torch.randn(36, 600, device=DEV), torch.randn(100, 600, device=DEV)
    (lin(x1).pow(2).sum() + lin(x2).sum() + lin(x3).pow(2).sum()).backward()       # skinny, skinny, tile
    ref_w, ref_b = lin.weight.grad.clone(), lin.bias.grad.clone()
    arena = ParamArena(list(lin.parameters()))
    arena.g.fill_(float("nan"))
    arena.zero_grad()
    (lin(x1).pow(2).sum() + lin(x2).sum() + lin(x3).pow(2).sum()).backward()
    assert_close(lin.weight.grad, ref_w, "weight grad", 1e-5)
    assert_close(lin.bias.grad, ref_b, "bias grad", 1e-5)


@pytest.mark.parametrize("M,F", [(12, 600), (36, 200), (332, 64)])
def test_dense_with_fused_swish_vs_fp64(M, F):
    """Dense(activation=swish): bias + Swish fused into the GEMM epilogue, Swish' into the backward
    operand loads (M <= 64), or the hipBLASLt + tensor-op path (M = 332)."""
    gen = torch.Generator().manual_seed(M + F)
    dense = cg.Dense(F, 2 * F, activation=cg.Swish())
    with torch.no_grad():
        dense.bias.normal_(0, 0.5, generator=gen)
    x = torch.randn(M, F, generator=gen)
    gy = torch.randn(M, 2 * F, generator=gen)
    xd = x.double().requires_grad_(True)
    Wd_, bd_ = dense.weight.detach().double().requires_grad_(True), dense.bias.detach().double().requires_grad_(True)
    yd = torch.nn.functional.silu(torch.nn.functional.linear(xd, Wd_, bd_))
    yd.backward(gy.double())
    dense = dense.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = dense(xg)
    y.backward(gy.to(DEV))
    assert_close(y, yd, "y", 3e-6)
    assert_close(xg.grad, xd.grad, "gx", 3e-6)
    assert_close(dense.weight.grad, Wd_.grad, "gW", 3e-6)
    assert_close(dense.bias.grad, bd_.grad, "gb", 3e-6)


@pytest.mark.parametrize("n,F", [pytest.param(12, 600, id="12-600-0"), pytest.param(96, 600, id="96-600-0"),
                                 pytest.param(64, 128, id="64-128-0")])      # (ids: as before the fused-forward legs left)
def test_fused_update_block_equals_composition(n, F):
    """The single-node UpdateBlock path (arena-managed parameters, merged [u_mat; v_mat] product, grouped
    weight gradients) against the tensor-op composition and the fp64 oracle formulas; 12 beads run on the skinny
    kernels, 64 / 96 beads (3n = 192 / 288 rows) on the tile kernels; the norm / gate are element-wise launches behind
    the products."""
    from coarsegrainingvae_amd.trainer import ParamArena
    from coarsegrainingvae_amd.ops import _UpdateBlockFused
    torch.manual_seed(3)
    blk = cg.UpdateBlock(F, "swish", 0.0).to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.2)
    s = torch.randn(n, F, device=DEV)
    v = torch.randn(n, F, 3, device=DEV)
    gs, gv = torch.randn(n, F, device=DEV), torch.randn(n, F, 3, device=DEV)

    def run(residual):
        for p in blk.parameters():
            if not getattr(p, "_cgv_direct", False):
                p.grad = None                                   # plain autograd accumulation: start from scratch
        s1, v1 = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
        ds, dv = blk(s1, v1, residual=residual)
        ((ds * gs).sum() + (dv * gv).sum()).backward()
        return ds.detach(), dv.detach(), s1.grad, v1.grad, [p.grad.clone() for p in blk.parameters()]

    ref = {r: run(r) for r in (False, True)}                       # composition (no arena yet)
    for p in blk.parameters():
        p.grad = None
    _ = run(False)
    arena = ParamArena(list(blk.parameters()))
    assert _UpdateBlockFused.usable(s, v, blk.u_mat.weight, blk.v_mat.weight, blk.s_dense[0], blk.s_dense[1])
    for residual in (False, True):
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        got = run(residual)
        for a, b, name in zip(got[:4], ref[residual][:4], ("ds", "dv", "g_s", "g_v")):
            assert_close(a, b, f"{name} residual={residual}", 2e-5)
        for a, b, (name, _) in zip(got[4], ref[residual][4], blk.named_parameters()):
            assert_close(a, b, f"grad {name} residual={residual}", 2e-5)


# --------------------------------------------------------------------------- edge cases the fused kernels must survive
def _block_vs_oracle(F, R, n, nbrs, xyz, with_gv=True, seed=0, tol=REL, grads=None):
    gen = torch.Generator().manual_seed(seed)
    cutoff = 6.0
    r = xyz[nbrs[:, 1]] - xyz[nbrs[:, 0]] if nbrs.shape[0] else torch.zeros(0, 3)
    blk = cg.EquiMessageBlock(F, "swish", R, cutoff, 0.0)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.3, generator=gen)
    P = {"b." + k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    s, v = torch.randn(n, F, generator=gen), torch.randn(n, F, 3, generator=gen)
    gs, gv = torch.randn(n, F, generator=gen), torch.randn(n, F, 3, generator=gen)
    s0, v0 = s.clone().requires_grad_(True), v.clone().requires_grad_(True)
    ds0, dv0 = O.equi_message_block(s0, v0, r, nbrs, P, "b", O.swish, R, cutoff)
    ((ds0 * gs).sum() + ((dv0 * gv).sum() if with_gv else 0.0)).backward()
    if F % 4:
        # widths the Dense kernels do not take (they raise: no library fallback): the node MLP of THIS test runs on torch
        # ops with the same parameters -- the subject here is the edge kernel's odd-width (scalar-access) instantiation
        d0, d1 = blk.inv_message.inv_dense[0], blk.inv_message.inv_dense[1]
        l0, l1 = torch.nn.Linear(F, F), torch.nn.Linear(F, 3 * F)
        l0.weight, l0.bias, l1.weight, l1.bias = d0.weight, d0.bias, d1.weight, d1.bias
        blk.inv_message.inv_dense = torch.nn.Sequential(l0, torch.nn.Sequential(torch.nn.SiLU(), l1))     # keys 0.* and 1.1.*
    blk = blk.to(DEV)
    s1, v1 = s.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    ds1, dv1 = blk(s1, v1, r.to(DEV), nbrs.to(DEV))
    ((ds1 * gs.to(DEV)).sum() + ((dv1 * gv.to(DEV)).sum() if with_gv else 0.0)).backward()
    assert_close(ds1, ds0, "ds", tol) if float(ds0.abs().max()) > 0 else None
    assert_close(dv1, dv0, "dv", tol) if float(dv0.abs().max()) > 0 else None
    assert_close(s1.grad, s0.grad, "grad s", tol) if float(s0.grad.abs().max()) > 0 else None
    if with_gv and float(v0.grad.abs().max()) > 0:
        assert_close(v1.grad, v0.grad, "grad v", tol)
    for name, p in blk.named_parameters():
        ref = P["b." + name.replace("inv_dense.1.1.", "inv_dense.1.")].grad
        if ref is not None and float(ref.abs().max()) > 0:
            assert_close(p.grad, ref, "grad " + name, tol)
    if grads is not None:
        grads.append({"s": s1.grad.clone(), **{name: p.grad.clone() for name, p in blk.named_parameters() if p.grad is not None}})
    return ds1, dv1


@pytest.mark.parametrize("F,R", [(7, 8), (1, 4), (129, 10), (130, 6), (600, 12), (66, 16), (34, 20)])
@pytest.mark.parametrize("with_gv", [True, False])
def test_equi_message_odd_widths_and_all_rbf_counts(F, R, with_gv):
    """Odd channel counts take the scalar-access (PAIR = false) instantiation; every compiled n_rbf runs."""
    gen = torch.Generator().manual_seed(F)
    n = 23
    xyz = torch.rand(n, 3, generator=gen) * 4.0
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 3.0, True))
    _block_vs_oracle(F, R, n, nbrs, xyz, with_gv, seed=F + R)


def test_equi_message_degenerate_graphs():
    gen = torch.Generator().manual_seed(11)
    F, R, n = 24, 8, 9
    xyz = torch.rand(n, 3, generator=gen) * 4.0
    # (a) no edges at all: outputs are exactly zero, gradients flow nowhere
    empty = torch.zeros(0, 2, dtype=torch.long)
    ds, dv = _block_vs_oracle(F, R, n, empty, xyz)
    assert float(ds.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0
    # (b) isolated nodes, a self-contained pair, duplicated edges, one high-degree hub (asymmetric list)
    nbrs = torch.tensor([[0, 1], [1, 0], [0, 1], [5, 2], [5, 3], [5, 4], [5, 6], [5, 7], [5, 0], [2, 5]])
    _block_vs_oracle(F, R, n, nbrs, xyz)
    # (c) coincident atoms (distance = sqrt(3e-8)) and an edge beyond the RBF cutoff
    xyz2 = xyz.clone()
    xyz2[1] = xyz2[0]
    xyz2[8] = xyz2[0] + 50.0
    nbrs2 = torch.tensor([[0, 1], [1, 0], [0, 8], [8, 0], [2, 3], [3, 2]])
    _block_vs_oracle(F, R, n, nbrs2, xyz2)


def test_ragged_batch_model_parity():
    """Frames of different sizes in one batch (CG_collate offsets, per-frame plans) against the oracle."""
    F, R = 32, 8
    atom_cutoff, cg_cutoff, n_cgs = 4.0, 9.5, 3
    gen = torch.Generator().manual_seed(2)
    frames = []
    for n_atoms in (9, 22, 5):
        xyz = torch.rand(n_atoms, 3, generator=gen) * 5.0
        z = torch.randint(1, 9, (n_atoms,), generator=gen).float()
        mapping = (torch.arange(n_atoms) * n_cgs) // n_atoms
        cgx = torch.stack([xyz[mapping == b].mean(0) for b in range(n_cgs)])
        f = {"nxyz": torch.cat([z[:, None], xyz], 1), "CG_nxyz": torch.cat([torch.arange(n_cgs).float()[:, None], cgx], 1),
             "num_atoms": torch.LongTensor([n_atoms]), "num_CGs": torch.LongTensor([n_cgs]), "CG_mapping": mapping,
             "bond_edge_list": torch.stack([torch.arange(n_atoms - 1), torch.arange(1, n_atoms)], 1)}
        f["nbr_list"] = O.get_neighbor_list(xyz, atom_cutoff, True)
        f["CG_nbr_list"] = O.get_neighbor_list(cgx, cg_cutoff, True)
        frames.append(f)
    cpu_batch = O.cg_collate(frames)
    assert torch.equal(cg.CG_collate(frames)["nbr_list"], cpu_batch["nbr_list"])
    model = cg.build_model(F, R, atom_cutoff, cg_cutoff, 2, 2, n_cgs, det=True, seed=5)
    hp = O.Hyper(F, R, atom_cutoff, cg_cutoff, 2, 2, n_cgs, det=True)
    P = _oracle_params_from(model)
    out0 = O.model_forward(cpu_batch, P, hp)
    loss0 = O.loss_terms(out0, cpu_batch, 0.05, 25.0)[0]
    loss0.backward()
    model = model.to(DEV)
    batch = cg.prepare_batch({k: v.to(DEV) for k, v in cg.CG_collate(frames).items()})
    out1 = model(batch)
    loss1 = cg.loss_terms(out1, batch, 0.05, 25.0)[0]
    loss1.backward()
    assert_close(out1[5], out0[5], "xyz_recon")
    assert_close(loss1, loss0, "loss")
    for name, p in model.named_parameters():
        ref = P[name].grad
        if ref is not None and float(ref.abs().max()) > 0:
            assert_close(p.grad, ref, "grad " + name)                      # REL: observed <= 1.8e-5, u_mat / v_mat of the decoder (tools/grad_err_probe.py)


def test_batched_radius_graph_dataset_path():
    """CGDataset.generate_neighbor_list (one batched K0 launch per graph kind) == per-frame oracle lists."""
    props = cg.data.synthetic_frames(5, 22, 3, 6.0, seed=4)
    ds = cg.CGDataset(props)
    ds.generate_neighbor_list(4.0, 9.5, device=DEV, undirected=True)
    for k in range(5):
        assert torch.equal(ds.props["nbr_list"][k], O.get_neighbor_list(props["nxyz"][k][:, 1:4], 4.0, True))
        assert torch.equal(ds.props["CG_nbr_list"][k], O.get_neighbor_list(props["CG_nxyz"][k][:, 1:4], 9.5, True))
    ds.generate_neighbor_list(4.0, None, device=DEV)                 # --cg_radius_graph: bead graph from bonds
    assert ds.props["CG_nbr_list"][0].shape[1] == 2


def test_equi_message_high_degree_split_path():
    """Dense graph (degree 79 > 48): the launcher picks the split-segment kernels (4 waves per receiver)."""
    gen = torch.Generator().manual_seed(8)
    n = 80
    xyz = torch.rand(n, 3, generator=gen) * 3.0
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 9.0, True))
    assert nbrs.shape[0] >= 48 * n
    _block_vs_oracle(48, 10, n, nbrs, xyz, True, seed=1)
    _block_vs_oracle(48, 10, n, nbrs, xyz, False, seed=2)


@pytest.mark.parametrize("F,R", [(600, 10), (88, 8), (132, 12), (4, 10), (52, 4), (600, 16)])
def test_scalar_only_backward_on_the_matrix_cores(F, R, options):
    """equi_msg_bwd_mfma_k (no vector gradient upstream, >= 48 edges per node, n_rbf + 1 <= 16): N = A^T x gathered rows
    with 4 edges per fp32 MFMA, against the oracle's autograd AND against the packed-FMA walk of the same launch
    (CGV_OPT_MSG_BWD_MFMA = 0) -- ragged segments (lengths that are no multiple of 4 or of the 4 waves' slices), an
    isolated node, an asymmetric edge set, a channel count that leaves the last 128-channel tile mostly empty, a width of a
    single 16-byte piece.  n_rbf = 16 does not fit the 16 rows of a tile and stays on the FMA walk."""
    gen = torch.Generator().manual_seed(F + R)
    n = 90
    xyz = torch.rand(n, 3, generator=gen) * 3.0
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 9.0, True))
    keep = torch.rand(nbrs.shape[0], generator=gen) < 0.8                   # ragged, asymmetric
    keep &= (nbrs[:, 0] != 5) & (nbrs[:, 1] != 5)                           # node 5: no edges at all
    nbrs = nbrs[keep]
    assert nbrs.shape[0] >= 48 * n
    got = []
    for mode in (1, 0):
        options.set("msg_bwd_mfma", mode)
        torch.manual_seed(11)                                                # (the block draws its weights from the global generator)
        _block_vs_oracle(F, R, n, nbrs, xyz, False, seed=3, grads=got)
    a, b = got
    for key in a:
        assert_close(a[key], b[key].double(), "both kernels: " + key, 2e-5)
    differs = any(not torch.equal(a[key], b[key]) for key in a)
    assert differs == (R + 1 <= 16), "the option must select between two kernels exactly where the matrix-core one applies"


@pytest.mark.parametrize("M", [12, 332])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_mlp_head_fused_activation_vs_fp64(M, act):
    """MLPHead = Sequential(Linear, Tanh | ReLU, Linear) with the activation fused into the first product
    (skinny kernels at M = 12, tile kernels at M = 332) against fp64 autograd; state_dict keys as nn.Sequential."""
    from coarsegrainingvae_amd.primitives import MLPHead
    torch.manual_seed(M)
    F = 600
    head = MLPHead(cg.primitives.Linear(F, F), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU(), cg.primitives.Linear(F, F))
    assert sorted(head.state_dict()) == ["0.bias", "0.weight", "2.bias", "2.weight"]
    x = torch.randn(M, F)
    gy = torch.randn(M, F)
    ref = torch.nn.Sequential(torch.nn.Linear(F, F), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU(), torch.nn.Linear(F, F)).double()
    ref.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    xd = x.double().requires_grad_(True)
    ref(xd).backward(gy.double())
    head = head.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = head(xg)
    y.backward(gy.to(DEV))
    assert_close(y, ref(xd).detach(), "y", 2e-6)
    assert_close(xg.grad, xd.grad, "gx", 5e-6)
    for (n, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
        assert_close(p.grad, q.grad, "grad " + n, 5e-6)


def test_embedding_plan_gradient_matches_nn_embedding():
    """ops.embedding: lookup + plan-based weight gradient (one segment sum) == nn.Embedding incl. padding_idx."""
    torch.manual_seed(2)
    emb = torch.nn.Embedding(100, 24, padding_idx=0).to(DEV)
    idx = torch.randint(0, 9, (57,), device=DEV)
    idx[3] = 0                                               # a padding row in the batch: its gradient stays zero
    gout = torch.randn(57, 24, device=DEV)
    ref = emb(idx)
    ref.backward(gout)
    want = emb.weight.grad.clone()
    emb.weight.grad = None
    out = cg.ops.embedding(emb, idx.float())                 # ids arrive as the float column of nxyz
    out.backward(gout)
    assert torch.equal(out, ref)
    assert_close(emb.weight.grad, want, "embedding weight grad", 1e-6)
    assert float(emb.weight.grad[0].abs().max()) == 0.0


# --------------------------------------------------------------------------- hipGraph replay across batches
def test_captured_step_replays_on_other_batches():
    """Trainer.capture on one batch, then step() on OTHER batches of the same molecules: they are loaded into the
    captured batch's buffers (data.copy_batch_into: coordinates copied, plans re-sorted and geometry recomputed in
    place) and the graph is replayed.  Must equal an eager trainer fed the same sequence; a batch whose edge
    count exceeds the reserved capacity runs eagerly."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["dipeptide"]

    def make(seed, box=None):
        frames = cg.data.synthetic_frames(4, 22, w["n_cgs"], box or w["box"], seed=seed)
        ds = cg.CGDataset(frames)
        ds.generate_neighbor_list(ATOM_CUT, w["cg_cutoff"], device=DEV, undirected=True)
        return cg.CG_collate([ds[i] for i in range(4)])

    ATOM_CUT = 3.5                                            # sparse enough that the edge count differs per batch
    seqs = [make(1), make(2), make(3), make(2)]
    assert len({b["nbr_list"].shape[0] for b in seqs}) > 1
    dense = make(4, box=2.5)                                  # everything within the cutoff: far more edges
    assert dense["nbr_list"].shape[0] > 1.3 * max(b["nbr_list"].shape[0] for b in seqs)

    def run(use_graph):
        model = cg.build_model(64, w["n_rbf"], ATOM_CUT, w["cg_cutoff"], 2, 2, w["n_cgs"], det=True, seed=7).to(DEV)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
        first = cg.data.prepare_batch({k: v.clone() for k, v in seqs[0].items()}, DEV, edge_slack=0.25)
        losses = [float(tr.step(first))]                      # builds the arena
        if use_graph:
            tr.capture(first, warmup=0)
        for b in seqs[1:] + [dense, seqs[1]]:
            losses.append(float(tr.step({k: v.clone() for k, v in b.items()})))
        losses.append(float(tr.step({k: v.clone() for k, v in seqs[2].items()}, train=False)))
        return losses, [p.detach().clone() for p in model.parameters()], tr

    ref_losses, ref_params, _ = run(False)
    losses, params, tr = run(True)
    assert tr.replays == 4                                    # seqs[1], seqs[2], seqs[1 again], seqs[1]; dense + eval: eager
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-5 * abs(b), (losses, ref_losses)
    for p, q in zip(params, ref_params):
        assert_close(p, q, "parameter after replayed steps", 1e-5)


def test_sgd_through_the_fused_step_equals_torch_sgd():
    """Trainer(optimizer="sgd"): clip_grad_norm_(0.01) + torch.optim.SGD(lr) (scripts/run_ala.py:43, utils.py:151-157) as
    cgv_optim_prepare + cgv_sgd_apply over the arena -- eager steps, then the captured step -- against the same trainer with
    the library's clip + SGD (fused_optimizer=False)."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["dipeptide"]
    batch = cg.synthetic_batch("dipeptide", n_frames=4, seed=3, device=DEV)

    def run(fused):
        model = cg.build_model(32, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 2, w["n_cgs"], det=True, seed=11).to(DEV)
        tr = Trainer(model, lr=0.05, beta=w["beta"], gamma=w["gamma"], fused_optimizer=fused, optimizer="sgd")
        losses = [float(tr.step(batch)) for _ in range(3)]
        if fused:
            assert tr.m is None and tr._rank_hi == 0
            tr.capture(batch, warmup=0)
        losses += [float(tr.step(batch)) for _ in range(2)]
        if fused:
            assert tr.replays == 2
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l_ref, p_ref = run(False)
    l_fused, p_fused = run(True)
    for a, b in zip(l_fused, l_ref):
        assert abs(a - b) <= 1e-5 * abs(b), (l_fused, l_ref)
    assert l_ref[-1] < l_ref[0]
    for k in p_ref:
        assert_close(p_fused[k], p_ref[k], k, 1e-5)


def test_captured_fused_decoder_replays_on_other_bead_edge_counts():
    """The channel-group decoder kernels (csrc/decoder_layer.hip) stage the bead graph in LDS.  They stage the plan's
    CAPACITY of records and take the edge structure from rowptr on the device, so a captured step replays on batches
    whose BEAD graph has fewer or MORE edges than the captured batch's (a short cg_cutoff leaves it sparse and
    different per frame).  Must equal an eager trainer fed the same sequence."""
    from coarsegrainingvae_amd import decoder_fused
    from coarsegrainingvae_amd.trainer import Trainer
    n_atoms, n_cgs, F, R, atom_cut, cg_cut = 60, 10, 64, 8, 5.0, 1.5

    def make(seed):
        ds = cg.CGDataset(cg.data.synthetic_frames(1, n_atoms, n_cgs, 6.0, seed=seed))
        ds.generate_neighbor_list(atom_cut, cg_cut, device=DEV, undirected=True)
        return cg.CG_collate([ds[0]])

    pool = [make(s) for s in range(1, 40)]
    counts = [b["CG_nbr_list"].shape[0] for b in pool]
    order = sorted(range(len(pool)), key=lambda k: counts[k])
    first = pool[order[len(order) // 2]]                       # captured on a median batch ...
    seqs = [pool[order[0]], pool[order[-1]], pool[order[len(order) // 3]], pool[order[-2]]]      # ... replayed on sparser and denser ones
    n_first = first["CG_nbr_list"].shape[0]
    assert min(b["CG_nbr_list"].shape[0] for b in seqs) < n_first < max(b["CG_nbr_list"].shape[0] for b in seqs)
    assert min(counts) >= 1

    def run(use_graph):
        model = cg.build_model(F, R, atom_cut, cg_cut, 1, 2, n_cgs, det=True, seed=7).to(DEV)
        tr = Trainer(model, lr=1e-3, beta=0.05, gamma=10.0)
        cap = cg.data.prepare_batch({k: v.clone() for k, v in first.items()}, DEV, edge_slack=1.0)
        losses = [float(tr.step(cap))]                        # builds the arena (per-block decoder path)
        losses.append(float(tr.step(cap)))                    # fused decoder loop from here on
        calls0 = decoder_fused.calls
        if use_graph:
            tr.capture(cap, warmup=0)
        for b in seqs:
            losses.append(float(tr.step({k: v.clone() for k, v in b.items()})))
        assert decoder_fused.calls > calls0                   # the channel-group path did run
        return losses, [p.detach().clone() for p in model.parameters()], tr

    ref_losses, ref_params, _ = run(False)
    losses, params, tr = run(True)
    assert tr.replays == len(seqs)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 1e-5 * abs(b), (losses, ref_losses)
    for p, q in zip(params, ref_params):
        assert_close(p, q, "parameter after replayed steps", 1e-5)


# --------------------------------------------------------------------------- K7b / K2g: receiver groups, shared-source forward
def _group_order_reference(dst_d, src_d, rb):
    """Restatement of the receiver-group order (include/cgvae_hip.h, K7b): positions of the dst-sorted view sorted,
    stably, by (receiver // rb, source); meta = (slot | head << 8 | last step of the group << 9 | step mask << 16, next step's source); a
    duplicated edge opens a new step."""
    E = len(dst_d)
    pos = np.lexsort((np.arange(E), src_d, dst_d // rb))
    dg, sg = dst_d[pos], src_d[pos]
    grp = dg // rb
    meta = np.zeros((E, 2), dtype=np.int64)
    q = 0
    while q < E:
        r = q + 1                                        # a step: one source, strictly increasing receivers
        while r < E and grp[r] == grp[q] and sg[r] == sg[q] and dg[r] > dg[r - 1]:
            r += 1
        mask = 0
        for u in range(q, r):
            mask |= 1 << int(dg[u] - grp[u] * rb)
        more = r < E and grp[r] == grp[q]
        nxt = sg[r] if more else sg[q]
        for u in range(q, r):
            meta[u, 0] = int(dg[u] - grp[u] * rb) | (0x100 if u == q else 0) | (0 if more else 0x200) | (mask << 16)
            meta[u, 1] = nxt
        q = r
    return pos, dg, sg, meta


@pytest.mark.parametrize("rb", [2, 4])
@pytest.mark.parametrize("n,E", [(37, 900), (5, 3), (64, 4000), (3, 9000)])   # last: > 4096 keys per group (spill path)
def test_receiver_group_order_is_bit_exact(rb, n, E):
    gen = torch.Generator().manual_seed(n + E + rb)
    nbrs = torch.randint(0, n, (E, 2), generator=gen)              # duplicates and self loops included
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n, capacity=E + 50).enable_groups(rb)
    pos, dg, sg, meta = _group_order_reference(plan.dst_d[:E].cpu().numpy(), plan.src_d[:E].cpu().numpy(), rb)
    assert np.array_equal(plan.pos_g[:E].cpu().numpy(), pos)
    assert np.array_equal(plan.dst_g[:E].cpu().numpy(), dg) and np.array_equal(plan.src_g[:E].cpu().numpy(), sg)
    assert np.array_equal(plan.meta_g[:2 * E].cpu().numpy().reshape(E, 2), meta)
    # the two-pass radix construction gives the same arrays
    one_launch = [t.clone() for t in (plan.pos_g, plan.dst_g, plan.src_g, plan.meta_g)]
    plan._build_groups(radix=True)
    for a, b in zip(one_launch, (plan.pos_g, plan.dst_g, plan.src_g, plan.meta_g)):
        assert torch.equal(a[:E], b[:E]) if a.numel() != 2 * plan.capacity else torch.equal(a[:2 * E], b[:2 * E])
    plan._build_groups()
    # an in-place rebuild on another edge list refreshes the group order too
    nbrs2 = torch.randint(0, n, (E + 7, 2), generator=gen)
    plan.rebuild_from_nbrs(nbrs2.to(DEV))
    E2 = E + 7
    pos, dg, sg, meta = _group_order_reference(plan.dst_d[:E2].cpu().numpy(), plan.src_d[:E2].cpu().numpy(), rb)
    assert np.array_equal(plan.pos_g[:E2].cpu().numpy(), pos)
    assert np.array_equal(plan.meta_g[:2 * E2].cpu().numpy().reshape(E2, 2), meta)


def _equi_message_fp64(phi, v, Wd, bd, rows, dst, src, R, U, n):
    """m_k = phi[src] * (a . Wd^T + env * bd);  ds = sum m_1;  dv = sum m_2 * unit + m_0 * v[src]   (conv.py:505-563)."""
    F = phi.shape[1] // 3
    a, env, unit = rows[:, :R].double(), rows[:, R].double(), rows[:, U:U + 3].double()
    w = a @ Wd.double().t() + env[:, None] * bd.double()[None, :]
    m = (phi.double()[src] * w).reshape(-1, 3, F)
    ds = torch.zeros(n, F, dtype=torch.float64).index_add_(0, dst, m[:, 1])
    msg = m[:, 2, :, None] * unit[:, None, :] + m[:, 0, :, None] * v.double()[src]
    dv = torch.zeros(n, F, 3, dtype=torch.float64).index_add_(0, dst, msg)
    return ds, dv


@pytest.mark.parametrize("rb", [2, 4])
@pytest.mark.parametrize("F,R,n,box,cut", [(600, 10, 83, 6.0, 5.5), (24, 8, 10, 3.0, 9.0), (130, 6, 41, 5.0, 2.5),
                                            (64, 10, 7, 3.0, 9.0), (256, 12, 166, 14.0, 12.0)])
def test_shared_source_forward_matches_fp64_and_plain_kernel(F, R, n, box, cut, rb):
    """K2g against an fp64 evaluation of the block's math and against the per-receiver kernel: dense and sparse
    graphs, a receiver count that is not a multiple of the group size, isolated receivers, fused residuals."""
    from coarsegrainingvae_amd import ops
    gen = torch.Generator().manual_seed(F + n + rb)
    xyz = torch.rand(n, 3, generator=gen) * box
    xyz[-1] += 100.0                                                          # an isolated node: empty segment
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, cut, True))
    nbrs = torch.cat([nbrs, torch.tensor([[1, 0], [1, 0], [2, 0]])])        # duplicates / asymmetric extras
    plain = EdgePlan.from_nbrs(nbrs.to(DEV), n)
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n).enable_groups(rb)
    xd = xyz.to(DEV)
    g_plain = EdgeGeometry(plain, R, 6.0, pos_dst=xd, pos_src=xd)
    geom = EdgeGeometry(plan, R, 6.0, pos_dst=xd, pos_src=xd)
    assert geom.geom_g is not None and g_plain.geom_g is None
    phi, v = torch.randn(n, 3 * F, generator=gen), torch.randn(n, F, 3, generator=gen)
    Wd, bd = torch.randn(3 * F, R, generator=gen), torch.randn(3 * F, generator=gen)
    s_res, v_res = torch.randn(n, F, generator=gen), torch.randn(n, F, 3, generator=gen)
    E = plan.n_edges
    # the group records carry the plan's meta words (as int bits) next to the geometry
    rec = geom.geom_g[:E].cpu()
    assert torch.equal(rec[:, [R + 1, R + 5]].view(torch.int32), plan.meta_g[:2 * E].cpu().view(E, 2))
    assert torch.equal(rec[:, :R + 1], geom.geom_d[:E].cpu()[plan.pos_g[:E].cpu().long()][:, :R + 1])
    ds64, dv64 = _equi_message_fp64(phi, v, Wd, bd, geom.geom_g[:E].cpu(), plan.dst_g[:E].cpu().long(),
                                    plan.src_g[:E].cpu().long(), R, geom.group_unit_offset, n)
    args = [x.to(DEV) for x in (phi, v, Wd, bd)]
    ds, dv = ops.equi_message(*args, plan, geom, True)
    ds_p, dv_p = ops.equi_message(*args, plain, g_plain, True)
    assert_close(ds, ds64, "ds vs fp64", 2e-6)
    assert_close(dv, dv64, "dv vs fp64", 2e-6)
    assert_close(ds, ds_p, "ds vs per-receiver kernel", 2e-6)
    assert_close(dv, dv_p, "dv vs per-receiver kernel", 2e-6)
    assert float(ds[-1].abs().max()) == 0.0 and float(dv[-1].abs().max()) == 0.0
    ds_r, dv_r = ops.equi_message(*args, plan, geom, True, s_res.to(DEV), v_res.to(DEV))
    assert_close(ds_r, ds64 + s_res.double(), "residual s", 2e-6)
    assert_close(dv_r, dv64 + v_res.double(), "residual v", 2e-6)
    # the group order is used by the forward only; gradients still come from the source-sorted walk
    a = [x.clone().requires_grad_(True) for x in args]
    b = [x.clone().requires_grad_(True) for x in args]
    gs, gv = torch.randn(n, F, generator=gen).to(DEV), torch.randn(n, F, 3, generator=gen).to(DEV)
    for xs, pl, ge in ((a, plan, geom), (b, plain, g_plain)):
        o = ops.equi_message(*xs, pl, ge, True)
        ((o[0] * gs).sum() + (o[1] * gv).sum()).backward()
    for x, y, name in zip(a, b, ("phi", "v", "Wd", "bd")):
        assert_close(x.grad, y.grad, "grad " + name, 1e-6)


@pytest.mark.parametrize("F,R,n,kind", [(600, 10, 83, "dense"), (600, 10, 332, "dense"), (130, 6, 41, "holes"), (24, 8, 10, "tiny"),
                                        (256, 10, 64, "one_edge"), (64, 8, 29, "holes"), (600, 10, 200, "hub")])
def test_grouped_forward_on_awkward_graphs(F, R, n, kind):
    """K2g (cgv_equi_msg_fwd_grouped, called directly: one block per (group of 2 receivers, channel tile), its four waves
    on quarters of the group's edge range).  Against fp64 and, bit for bit, against itself over repeated launches.
    Graphs: dense; receivers without edges ahead of, between and behind the others; seven edges (most waves idle); one
    edge; one hub receiver holding most edges (8000 terms per sum)."""
    _lib = cg._lib
    gen = torch.Generator().manual_seed(F + n + 3)
    xyz = torch.rand(n, 3, generator=gen) * 5.0
    if kind == "dense":
        nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 9.0, True))
    elif kind == "holes":                                   # receivers 0-3, a middle run and the last five have no edges
        dst = torch.randint(4, n - 5, (40 * n,), generator=gen)
        dst = dst[(dst < n // 2) | (dst > n // 2 + 6)]
        nbrs = torch.stack([dst, torch.randint(0, n, (len(dst),), generator=gen)], dim=1)
    elif kind == "tiny":
        nbrs = torch.tensor([[2, 1], [2, 3], [3, 1], [7, 0], [7, 1], [7, 2], [7, 7]])
    elif kind == "one_edge":
        nbrs = torch.tensor([[37, 5]])
    else:                                                   # hub: receiver 100 sees everybody 40 times over (duplicates: new steps)
        hub = torch.stack([torch.full((40 * n,), 100), torch.arange(40 * n) % n], dim=1)
        rest = torch.randint(0, n, (300, 2), generator=gen)
        nbrs = torch.cat([hub, rest])
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n).enable_groups(2)
    xd = xyz.to(DEV)
    geom = EdgeGeometry(plan, R, 6.0, pos_dst=xd, pos_src=xd)
    E = plan.n_edges
    phi, v = torch.randn(n, 3 * F, generator=gen), torch.randn(n, F, 3, generator=gen)
    Wd, bd = torch.randn(3 * F, R, generator=gen), torch.randn(3 * F, generator=gen)
    s_res, v_res = torch.randn(n, F, generator=gen), torch.randn(n, F, 3, generator=gen)
    ds64, dv64 = _equi_message_fp64(phi, v, Wd, bd, geom.geom_g[:E].cpu(), plan.dst_g[:E].cpu().long(),
                                    plan.src_g[:E].cpu().long(), R, geom.group_unit_offset, n)
    args = [x.to(DEV) for x in (phi, v, Wd, bd)]
    assert _lib.load().cgv_equi_msg_grouped_supported(F, R, 2)

    def grouped(s_r=None, v_r=None):
        ds = torch.full((n, F), float("nan"), device=DEV)       # every receiver is written, the edgeless ones too
        dv = torch.full((n, F, 3), float("nan"), device=DEV)
        _lib.call("cgv_equi_msg_fwd_grouped", *map(_lib.ptr, args[:2]), _lib.ptr(geom.geom_g), _lib.ptr(plan.rowptr_d),
                  _lib.ptr(plan.src_g), *map(_lib.ptr, args[2:]), _lib.ptr(ds), _lib.ptr(dv), n, F, R, 2, n, E,
                  _lib.ptr(s_r), _lib.ptr(v_r), _lib.stream_ptr())
        return ds, dv

    ds, dv = grouped()
    tol = 2e-6 if kind != "hub" else 2e-5                      # (8000 terms per sum on the hub)
    assert_close(ds, ds64, "ds vs fp64", tol)
    assert_close(dv, dv64, "dv vs fp64", tol)
    ds_r, dv_r = grouped(s_res.to(DEV), v_res.to(DEV))
    assert_close(ds_r, ds64 + s_res.double(), "residual s", tol)
    assert_close(dv_r, dv64 + v_res.double(), "residual v", tol)
    deg = torch.bincount(plan.dst_g[:E].cpu().long(), minlength=n)
    for i in torch.nonzero(deg == 0).flatten().tolist():       # no edges: exactly the residual (or zero)
        assert float(ds[i].abs().max()) == 0.0 and float(dv[i].abs().max()) == 0.0
        assert torch.equal(ds_r[i].cpu(), s_res[i]) and torch.equal(dv_r[i].cpu(), v_res[i])
    for _ in range(5):                                          # repeated launches: same bits
        ds2, dv2 = grouped()
        assert torch.equal(ds2, ds) and torch.equal(dv2, dv)


def test_batch_graph_uses_receiver_groups_on_dense_atom_graphs(options):
    batch = cg.synthetic_batch("chignolin", n_frames=1, seed=3, device=DEV)
    g = batch["_graph"]
    assert g.atom.group_rb == 2 and g.cg.group_rb == 0 and g.a2b.group_rb == 0
    assert g.geometry("atom", 10, 25.0).geom_g is not None
    options.set("fwd_group", 0)
    g0 = cg.synthetic_batch("chignolin", n_frames=1, seed=3, device=DEV)["_graph"]
    assert g0.atom.group_rb == 0 and g0.geometry("atom", 10, 25.0).geom_g is None


# --------------------------------------------------------------------------- EquiMessageCross / EquivariantDecoder
@pytest.mark.parametrize("tag", ["F8R8", "F24R10"])
def test_equi_message_cross_golden(tag):
    g = load_golden(f"g8_equi_cross_{tag}")
    F, R = g["s"].shape[1], int(g["R"])
    blk = load_block(cg.EquiMessageCross(F, "swish", R, float(g["cutoff"]), 0.0), g)
    s, v = dev(g["s"]).requires_grad_(True), dev(g["v"]).requires_grad_(True)
    dh, dv = blk(s, v, dev(g["r_ij"]), dev(g["nbrs"]))
    assert_close(dh, g["dh"], "dh")
    assert_close(dv, g["dv"], "dv")
    ((dh * dev(g["gout_s"])).sum() + (dv * dev(g["gout_v"])).sum()).backward()
    assert_close(s.grad, g["gin_s"], "grad s")
    assert_close(v.grad, g["gin_v"], "grad v")
    check_param_grads(blk, g)


@pytest.mark.parametrize("name", ["block", "cross"])
def test_edge_weighted_message_blocks_golden(name):
    """``edge_wgt`` (conv.py:527-533, 384-397): per-edge weights folded into the filter inputs of the edge records
    (EdgeGeometry.scaled) -- forward, input gradients and every parameter gradient against the reference's own outputs."""
    g = load_golden(f"g10_edge_wgt_{name}")
    F, R = g["s"].shape[1], int(g["R"])
    cls = cg.EquiMessageBlock if name == "block" else cg.EquiMessageCross
    blk = load_block(cls(F, "swish", R, float(g["cutoff"]), 0.0), g)
    s, v = dev(g["s"]).requires_grad_(True), dev(g["v"]).requires_grad_(True)
    ds, dv = blk(s, v, dev(g["r_ij"]), dev(g["nbrs"]), edge_wgt=dev(g["edge_wgt"]))
    assert_close(ds, g["ds"], "ds")
    assert_close(dv, g["dv"], "dv")
    ((ds * dev(g["gout_s"])).sum() + (dv * dev(g["gout_v"])).sum()).backward()
    assert_close(s.grad, g["gin_s"], "grad s")
    assert_close(v.grad, g["gin_v"], "grad v")
    check_param_grads(blk, g)
    # and the pseudo-vector block takes the argument and ignores it, like the reference (conv.py:187-242)
    if name == "block":
        gp = load_golden("g1_equi_pseudo_F8R8")
        pb = load_block(cg.EquiMessagePsuedo(gp["s"].shape[1], "swish", int(gp["R"]), float(gp["cutoff"]), 0.0), gp)
        args = [dev(gp[k]) for k in ("s", "sbar", "v", "vbar", "r_ij", "nbrs")]
        out = pb(*args, edge_wgt=torch.rand(gp["nbrs"].shape[0], device=DEV))
        assert_close(out[0], gp["dh"], "dh with an (ignored) edge_wgt")


def test_encoder_dir_mp_golden():
    """``EquiEncoder(dir_mp=True)`` (cgvae.py:266-331): the atom list -- here one direction per pair -- is the directed
    edge list as given, the bead list is still symmetrised.  Outputs, and every parameter gradient, against the
    reference's own; a bundle prepared without the flag is refused."""
    g = load_golden("g11_encoder_dir_mp")
    F, R = int(g["F"]), int(g["R"])
    enc = load_block(cg.EquiEncoder(n_conv=2, n_atom_basis=F, n_rbf=R, activation="swish", cutoff=float(g["cutoff"]), dir_mp=True), g)
    args = [dev(g[k]) for k in ("z", "xyz", "cg_xyz", "mapping", "nbr_list", "cg_nbr_list")]
    H, h = enc(*args)
    assert_close(H, g["H"], "H")
    assert_close(h, g["h"], "h")
    ((H * dev(g["gout_H"])).sum() + (h * dev(g["gout_h"])).sum()).backward()
    check_param_grads(enc, g)
    from coarsegrainingvae_amd.graph import BatchGraph
    sym = BatchGraph(args[1], args[2], args[3], args[4], args[5])                     # symmetrised atom list
    assert sym.atom.n_edges == 2 * g["nbr_list"].shape[0]
    with pytest.raises(RuntimeError, match="dir_mp"):
        enc(*args, graph=sym)
    one_way = BatchGraph(args[1], args[2], args[3], args[4], args[5], dir_mp=True)
    assert one_way.atom.n_edges == g["nbr_list"].shape[0] and one_way.cg.n_edges == 2 * g["cg_nbr_list"].shape[0]
    H2, _ = enc(*args, graph=one_way)
    assert_close(H2, g["H"], "H through a prepared dir_mp bundle")


@pytest.mark.parametrize("flavour", ["cross", "plain"])
def test_equivariant_decoder_golden(flavour):
    g = load_golden(f"g8_equivariant_decoder_{flavour}")
    F, R = g["H"].shape[1], int(g["R"])
    dec = load_block(cg.EquivariantDecoder(F, R, float(g["cutoff"]), int(g["n_conv"]), "swish", cross_flag=(flavour == "cross")), g)
    H = dev(g["H"]).requires_grad_(True)
    n = H.shape[0]
    S, V = dec(dev(g["cg_xyz"]), dev(g["nbrs"]), torch.arange(n, device=DEV), H)
    assert_close(S, g["S"], "S")
    assert_close(V, g["V"], "V")
    ((S * dev(g["gout_S"])).sum() + (V * dev(g["gout_V"])).sum()).backward()
    assert_close(H.grad, g["gin_H"], "grad H")
    check_param_grads(dec, g)


def test_cgvae_trains_with_the_equivariant_decoder():
    """``CGequiVAE(equivaraintconv=EquivariantDecoder(...))`` (run_pdb.py:330-345): forward equals the oracle's
    composition of the same blocks, and the trainer steps it (arena, fused optimiser, captured graph)."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["dipeptide"]
    F, R = 64, w["n_rbf"]
    torch.manual_seed(123)
    enc = cg.EquiEncoder(n_conv=2, n_atom_basis=F, n_rbf=R, activation="swish", cutoff=w["cg_cutoff"], dir_mp=False, cg_mp=False)
    dec = cg.EquivariantDecoder(n_atom_basis=F, n_rbf=R, cutoff=w["atom_cutoff"], num_conv=2, activation="swish")
    prior = cg.CGprior(n_conv=2, n_atom_basis=F, n_rbf=R, activation="swish", cutoff=w["cg_cutoff"], dir_mp=False)
    mu = torch.nn.Sequential(torch.nn.Linear(F, F), torch.nn.ReLU(), torch.nn.Linear(F, F))
    sg = torch.nn.Sequential(torch.nn.Linear(F, F), torch.nn.ReLU(), torch.nn.Linear(F, F))
    model = cg.CGequiVAE(enc, dec, mu, sg, w["n_cgs"], F, prior_net=prior, det=True).to(DEV)
    batch = cg.synthetic_batch("dipeptide", n_frames=4, seed=2, device=DEV)
    # decoder parity against the oracle on the model's own latent (no autograd graph may outlive this block: its
    # AccumulateGrad nodes would be pinned to this stream and the trainer captures on another one)
    with torch.no_grad():
        out = model(batch)
        assert len(out) == 6 and out[5].shape == batch["nxyz"][:, 1:].shape
        P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        g = batch["_graph"]
        Hlat = model.encoder(batch["nxyz"][:, 0], batch["nxyz"][:, 1:], batch["CG_nxyz"][:, 1:], batch["CG_mapping"],
                             batch["nbr_list"], batch["CG_nbr_list"], graph=g)[0].cpu()
        S0, V0 = O.equivariant_decoder_forward(batch["CG_nxyz"][:, 1:].cpu(), batch["CG_nbr_list"].cpu(), Hlat, P, 2, R,
                                               w["atom_cutoff"])
        S1, V1 = model.equivaraintconv(batch["CG_nxyz"][:, 1:], batch["CG_nbr_list"], batch["CG_mapping"], Hlat.to(DEV),
                                       graph=g)
        assert_close(S1, S0, "decoder S")
        assert_close(V1, V0, "decoder V")
    del out, S1, V1
    tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
    losses = [float(tr.step(batch)) for _ in range(3)]
    tr.capture(batch, warmup=0)
    losses += [float(tr.step(batch)) for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# --------------------------------------------------------------------------- dataset build on the device
def test_build_dataset_on_device_matches_reference_semantics():
    """datasets.py:459-506 batched: rotations preserve every interatomic distance and are the same for the atoms and
    the beads of a frame, bead coordinates are the scatter_mean of the rotated atoms, the per-frame dicts collate, and
    the batched radius graphs equal the per-frame rule (data.py:65-82)."""
    gen = torch.Generator().manual_seed(4)
    T, n, n_cgs = 7, 22, 3
    traj = torch.rand(T, n, 3, generator=gen) * 6.0
    mapping = (torch.arange(n) * n_cgs) // n
    z = torch.randint(1, 9, (n,), generator=gen)
    bonds = torch.stack([torch.arange(n - 1), torch.arange(1, n)], dim=1)
    ds = cg.build_dataset(mapping, traj.numpy(), 8.5, 9.5, z.numpy(), bonds, order=2, generator=torch.Generator().manual_seed(1), device=DEV)
    assert len(ds) == T and set(ds.props) == {"nxyz", "CG_nxyz", "num_atoms", "num_CGs", "CG_mapping", "bond_edge_list"}
    for t_ in range(T):
        f = ds[t_]
        xyz = f["nxyz"][:, 1:]
        assert torch.equal(f["nxyz"][:, 0], z.float()) and torch.equal(f["CG_nxyz"][:, 0], torch.arange(n_cgs).float())
        assert_close(torch.cdist(xyz, xyz), torch.cdist(traj[t_], traj[t_]), "pair distances under rotation", 1e-5)
        assert_close(xyz.norm(dim=1), traj[t_].norm(dim=1), "rotation about the origin", 1e-5)
        assert_close(f["CG_nxyz"][:, 1:], O.scatter_mean(xyz, mapping, 0), "bead means", 1e-6)
        assert torch.equal(f["bond_edge_list"], cg.get_high_order_edge(bonds, 2, n))
    plain = cg.build_dataset(mapping, traj, 8.5, 9.5, z, bonds, rotate=False, device=DEV)
    assert torch.equal(plain[3]["nxyz"][:, 1:], traj[3])
    given = cg.build_dataset(mapping, traj, 8.5, 9.5, z, bonds, cg_traj=torch.zeros(T, n_cgs, 3), rotate=False, device=DEV)
    assert float(given[0]["CG_nxyz"][:, 1:].abs().max()) == 0.0
    ds.generate_neighbor_list(8.5, 9.5, device=DEV)
    for t_ in (0, T - 1):
        assert torch.equal(ds[t_]["nbr_list"], O.get_neighbor_list(ds[t_]["nxyz"][:, 1:], 8.5, True))
        assert torch.equal(ds[t_]["CG_nbr_list"], O.get_neighbor_list(ds[t_]["CG_nxyz"][:, 1:], 9.5, True))
    batch = cg.prepare_batch(cg.CG_collate([ds[i] for i in range(4)]), DEV)
    assert batch["nxyz"].shape == (4 * n, 4) and batch["CG_nxyz"].shape == (4 * n_cgs, 4)


@pytest.mark.parametrize("M,K,N", [(96, 600, 1800), (332, 600, 600), (100, 64, 132)])
def test_tile_layer_backward_under_the_trainer_queue_vs_fp64(M, K, N):
    """Arena-managed Dense layer beyond 64 rows with the weight-gradient queue active (what the trainer does): no
    prologue launch, act'(z) inside bwd_input's operand loads, weight + bias gradients from the grouped MFMA launch."""
    from coarsegrainingvae_amd.primitives import Swish, wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    gen = torch.Generator().manual_seed(M + N)
    layer = cg.Dense(K, N, bias=True, activation=Swish()).to(DEV)
    with torch.no_grad():
        layer.bias.copy_(torch.randn(N, generator=gen).to(DEV))
    x = torch.randn(M, K, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(M, N, generator=gen).to(DEV)
    layer(x).sum().backward()                                # gradients exist -> the arena can adopt them
    arena = ParamArena(list(layer.parameters()))
    for second in (False, True):                             # first write of a step, then accumulation
        if not second:
            arena.zero_grad()
            x.grad = None
        with wgrad_queue.collect():
            (layer(x) * gout).sum().backward()
            assert len(wgrad_queue.items) == 1               # queued, not launched layer by layer
        wgrad_queue.flush()
    x64, W64, b64 = x.detach().double().cpu(), layer.weight.detach().double().cpu(), layer.bias.detach().double().cpu()
    x64.requires_grad_(True); W64.requires_grad_(True); b64.requires_grad_(True)
    z = x64 @ W64.t() + b64
    ((z * torch.sigmoid(z)) * gout.double().cpu()).sum().backward()
    assert_close(x.grad, 2 * x64.grad, "grad x (two passes)", 2e-6)
    assert_close(layer.weight.grad, 2 * W64.grad, "grad W (write + accumulate)", 2e-6)
    assert_close(layer.bias.grad, 2 * b64.grad, "grad b (write + accumulate)", 2e-6)


def test_shared_source_forward_at_full_size_properties():
    """BASELINE configs[4] size (2000 atoms, 851k directed edges, F = 600, n_rbf = 10): too large for the CPU oracle in
    a test, so size-independent properties -- the shared-source walk equals the per-receiver kernel (itself
    oracle-checked at small sizes), is linear in phi, and summing the outputs over receivers equals the edge-wise
    total computed from the plan (a checksum that does not depend on the segment structure)."""
    from coarsegrainingvae_amd import ops
    w = cg.data.WORKLOADS["protein2000"]
    g = cg.synthetic_batch("protein2000", seed=1, device=DEV)["_graph"]
    plan = g.atom
    assert plan.group_rb == 2 and plan.n_edges > 800000
    F, R = 600, w["n_rbf"]
    geom = g.geometry("atom", R, w["cg_cutoff"])
    gen = torch.Generator().manual_seed(0)
    phi, v = torch.randn(plan.n_src, 3 * F, generator=gen).to(DEV), torch.randn(plan.n_src, F, 3, generator=gen).to(DEV)
    Wd, bd = torch.randn(3 * F, R, generator=gen).to(DEV), torch.randn(3 * F, generator=gen).to(DEV)
    ds, dv = ops.equi_message(phi, v, Wd, bd, plan, geom, True)
    plain = EdgePlan.from_nbrs(g.atom_nbrs, plan.n_dst)
    g_plain = EdgeGeometry(plain, R, w["cg_cutoff"], pos_dst=g.xyz, pos_src=g.xyz)
    ds_p, dv_p = ops.equi_message(phi, v, Wd, bd, plain, g_plain, True)
    assert_close(ds, ds_p, "ds vs per-receiver kernel", 5e-6)
    assert_close(dv, dv_p, "dv vs per-receiver kernel", 5e-6)
    ds2, dv2 = ops.equi_message(-2.0 * phi, v, Wd, bd, plan, geom, True)
    assert_close(ds2, -2.0 * ds, "linearity in phi (ds)", 1e-6)
    assert_close(dv2, -2.0 * dv, "linearity in phi (dv)", 1e-6)
    # checksum: sum_i ds[i, f] = sum_e phi[src_e, F + f] * w_1(e, f), evaluated edge-wise in fp64 on a channel subset
    E = plan.n_edges
    ch = torch.arange(0, F, 97, device=DEV)
    rec = geom.geom_d[:E].double()
    w1 = rec[:, :R] @ Wd[F + ch].double().t() + rec[:, R:R + 1] * bd[F + ch].double()[None, :]
    total = (phi[plan.src_d[:E].long()][:, F + ch].double() * w1).sum(0)
    assert_close(ds[:, ch].double().sum(0), total, "column checksum of ds", 1e-5)


@pytest.mark.parametrize("n,E", [(37, 900), (5, 0), (3, 5000), (400, 300), (166, 21000)])
def test_csr_by_rows_equals_the_radix_construction(n, E, options):
    """K7: the few-launch by-rows construction and the two-radix-pass one give identical arrays (dense rows beyond the
    LDS key budget, empty rows, no edges, mapping plans)."""
    gen = torch.Generator().manual_seed(n * 7 + E)
    nbrs = torch.randint(0, n, (E, 2), generator=gen).to(DEV)
    mapping = torch.randint(0, max(n // 3, 1), (n,), generator=gen).to(DEV)
    fields = ("rowptr_d", "eid_d", "dst_d", "src_d", "rowptr_s", "eid_s", "dst_s", "src_s")
    rows = (EdgePlan.from_nbrs(nbrs, n), EdgePlan.from_mapping(mapping, max(n // 3, 1)))
    options.set("csr_build", 1)
    radix = (EdgePlan.from_nbrs(nbrs, n), EdgePlan.from_mapping(mapping, max(n // 3, 1)))
    for a, b in zip(rows, radix):
        for f in fields:
            x, y = getattr(a, f), getattr(b, f)
            m = a.n_edges if not f.startswith("rowptr") else x.numel()
            assert torch.equal(x[:m], y[:m]), f


@pytest.mark.parametrize("captured", [False, True])
def test_deferred_update_equals_in_step_update(captured):
    """Trainer(defer_update=True): a step ends with the norm / clip / skip decision, its parameter pass opens the next step
    (decoder range on a side stream beside the encoder forward).  After flush() the parameters, moments and losses are
    bit-identical to the in-step update -- through eager steps, captured graphs, and train / validation alternation."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["chignolin"]

    def run(defer):
        model = cg.build_model(64, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 3, w["n_cgs"], det=True, seed=123).to(DEV)
        batch = cg.synthetic_batch("chignolin", n_frames=2, seed=4, device=DEV)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"], defer_update=defer, rank_update=False)
        losses = [float(tr.step(batch)) for _ in range(3)]
        if captured:
            tr.capture(batch, warmup=0, train=True)
        for k in range(6):
            train = k not in (2, 3)                       # two validation steps in the middle (utils.py:159-160)
            if captured and not tr.has_graph(train):
                tr.capture(batch, warmup=0, train=train)
            losses.append(float(tr.step(batch, train=train)))
            if k == 4:
                tr.lr = 5e-4                              # plateau scheduler: the pending update keeps the old rate
        tr.flush()
        torch.cuda.synchronize()
        return losses, {k: v.clone() for k, v in model.state_dict().items()}, tr.m.clone(), tr

    l0, p0, m0, _ = run(False)
    l1, p1, m1, tr = run(True)
    assert tr.defer_update and (not captured or tr.replays >= 4)
    assert l0 == l1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    # the moment arenas have the same content (the arena order is the same in both runs)
    assert torch.equal(m0, m1)


@pytest.fixture
def wgrad_tiling(request):
    from coarsegrainingvae_amd import options
    options.set("wgrad_tiling", request.param)
    yield request.param
    options.reset()


@pytest.mark.parametrize("wgrad_tiling", [0, 1], indirect=True)
def test_wgrad_gram_norm_and_fused_adam_vs_fp64(wgrad_tiling):
    """cgv_wgrad_gram: ||g^T x||_F^2 from the operand rows (+ bias gradient); cgv_grouped_wgrad_adam: the Adam update of
    the weights from tiles of g^T x that are never stored.  Checked against fp64 torch on the shapes the chignolin and
    update block produce (12 / 36 / 40 rows, with and without an activation derivative), under both column tilings of
    the fused update (option wgrad_tiling: balanced or widest tiles).  The decision pass runs here on an empty flat range
    (n = 0); the flat norm, Adam and SGD kernels of csrc/optim.hip are tested in tests/test_optim_gpu.py, whose reference
    takes the betas as the fp32 values the C ABI receives -- the rtol of 2e-5 on v below is mostly 1 - 0.999f against 0.001."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    lib = cg._lib.load()
    g = torch.Generator(device=DEV).manual_seed(5)
    shapes = [(12, 600, 600, 1, True), (12, 1800, 600, 0, True), (36, 1200, 600, 0, False), (40, 200, 328, 2, True),
              (7, 76, 52, 1, False)]
    n_total = sum(N * K for _, N, K, _, _ in shapes)
    arena_g = torch.full((n_total,), float("nan"), device=DEV)           # never read, never written
    arena_p = torch.randn(n_total, device=DEV, generator=g)
    arena_m = 0.1 * torch.randn(n_total, device=DEV, generator=g)
    arena_v = 0.01 * (0.1 + torch.rand(n_total, device=DEV, generator=g))     # away from 0: m / sqrt(v) stays conditioned
    p0, m0, v0 = arena_p.double().clone(), arena_m.double().clone(), arena_v.double().clone()
    items, refs, off = [], [], 0
    for M, N, K, act, bias in shapes:
        gy = torch.randn(M, N, device=DEV, generator=g)
        x = torch.randn(M, K, device=DEV, generator=g)
        z = torch.randn(M, N, device=DEV, generator=g) if act else None
        gb = torch.full((N,), float("nan"), device=DEV) if bias else None
        items.append((gy, x, z, act, arena_g[off:off + N * K].view(N, K), gb, False))
        gd = gy.double()
        if act:
            zd = z.double()
            sg = torch.sigmoid(zd)
            d = {1: sg * (1 + zd * (1 - sg)), 2: 1 - torch.tanh(zd) ** 2}[act]
            gd = gd * d
        refs.append((gd.T @ x.double(), gd.sum(0), off))
        off += N * K
    q = WeightGradQueue()
    table, blocks, lds = q.small_table(items)
    sumsq = torch.zeros(len(items), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.cgv_wgrad_gram_workspace_bytes(len(items))), dtype=torch.uint8, device=DEV)
    cg._lib.call("cgv_wgrad_gram", cg._lib.ptr(table), len(items), max(it[0].shape[0] for it in items), cg._lib.ptr(sumsq),
                 cg._lib.ptr(ws), ws.numel(), cg._lib.stream_ptr())
    for k, (gw, gbias, _) in enumerate(refs):
        assert abs(float(sumsq[k]) - float((gw ** 2).sum())) <= 1e-6 * float((gw ** 2).sum())
        if items[k][5] is not None:
            assert torch.allclose(items[k][5].double(), gbias, rtol=1e-5, atol=1e-5)
    # the decision pass on an empty materialised range + these norms, then the fused update
    state = torch.zeros(lib.cgv_optim_state_floats(), device=DEV)
    partial = torch.zeros(lib.cgv_optim_partial_floats(), device=DEV)
    lr, b1, b2, eps, max_norm = 1e-3, 0.9, 0.999, 1e-8, 0.01
    for step in range(2):
        cg._lib.call("cgv_optim_prepare_extra", arena_g.data_ptr(), 0, cg._lib.ptr(sumsq), len(items), b1, b2, max_norm, 1.0,
                     None, 0.0, cg._lib.ptr(state), cg._lib.ptr(partial), cg._lib.stream_ptr())
        cg._lib.call("cgv_grouped_wgrad_adam", cg._lib.ptr(table), len(items), blocks, lds, cg._lib.ptr(arena_g),
                     cg._lib.ptr(arena_p), cg._lib.ptr(arena_m), cg._lib.ptr(arena_v), lr, b1, b2, eps, cg._lib.ptr(state),
                     cg._lib.stream_ptr())
        norm = sum(float((gw ** 2).sum()) for gw, _, _ in refs) ** 0.5
        assert abs(float(state[1]) - norm) <= 1e-5 * norm
        clip = min(1.0, max_norm / (norm + 1e-6))
        for gw, _, o in refs:
            gflat = (gw * clip).reshape(-1)
            sl = slice(o, o + gflat.numel())
            m0[sl] = b1 * m0[sl] + (1 - b1) * gflat
            v0[sl] = b2 * v0[sl] + (1 - b2) * gflat * gflat
            bc1, bc2 = 1 - b1 ** (step + 1), 1 - b2 ** (step + 1)
            p0[sl] -= (lr / bc1) * m0[sl] / (v0[sl].sqrt() / bc2 ** 0.5 + eps)
    assert torch.isnan(arena_g).all()                                    # the gradient arena was never touched
    assert torch.allclose(arena_m.double(), m0, rtol=2e-5, atol=1e-9)
    assert torch.allclose(arena_v.double(), v0, rtol=2e-5, atol=1e-12)
    err = (arena_p.double() - p0).abs()
    assert float(err.max()) <= 5e-6, (float(err.max()), int(err.argmax()), [r[2] for r in refs])


def test_wgrad_gram_mfma_norm_vs_fp64():
    """cgv_wgrad_gram_mfma: ||g^T x||_F^2 and the bias gradient from up to 128 operand rows (fp64 MFMA tiles of the two
    Gram matrices), against fp64 torch -- row counts on and off the 16-row tile grid, ragged column slices, with and
    without an activation derivative, and records that address rank segments of a gathered buffer."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    lib = cg._lib.load()
    assert lib.cgv_wgrad_gram_mfma_max_rows() == 128
    g = torch.Generator(device=DEV).manual_seed(11)
    shapes = [(48, 600, 600, 1, True), (96, 1800, 600, 0, True), (64, 5400, 600, 0, False), (128, 200, 328, 2, True),
              (41, 76, 52, 1, True), (100, 1204, 36, 0, True), (12, 600, 600, 1, True)]
    items, refs = [], []
    for M, N, K, act, bias in shapes:
        gy = torch.randn(M, N, device=DEV, generator=g)
        x = torch.randn(M, K, device=DEV, generator=g)
        z = torch.randn(M, N, device=DEV, generator=g) if act else None
        gb = torch.full((N,), float("nan"), device=DEV) if bias else None
        items.append((gy, x, z, act, torch.empty(N, K, device=DEV), gb, False))
        gd = gy.double()
        if act:
            zd = z.double()
            sg = torch.sigmoid(zd)
            gd = gd * {1: sg * (1 + zd * (1 - sg)), 2: 1 - torch.tanh(zd) ** 2}[act]
        refs.append((float(((gd.T @ x.double()) ** 2).sum()), gd.sum(0)))
    q = WeightGradQueue()
    table, _blocks, rows = q.strip_table([it for it in items if it[0].shape[0] >= 32])
    small, _b, _l = q.small_table([it for it in items if it[0].shape[0] < 32])
    ws = torch.empty(int(lib.cgv_wgrad_gram_mfma_workspace_bytes(len(items), 128)), dtype=torch.uint8, device=DEV)
    n_big = sum(1 for it in items if it[0].shape[0] >= 32)
    sumsq = torch.zeros(len(items), dtype=torch.float64, device=DEV)
    cg._lib.call("cgv_wgrad_gram_mfma", cg._lib.ptr(table), n_big, rows, cg._lib.ptr(sumsq), cg._lib.ptr(ws), ws.numel(),
                 cg._lib.stream_ptr())
    cg._lib.call("cgv_wgrad_gram_mfma", cg._lib.ptr(small), len(items) - n_big, 12, sumsq.data_ptr() + 8 * n_big, cg._lib.ptr(ws),
                 ws.numel(), cg._lib.stream_ptr())
    for k, (ref, gbias) in enumerate(refs):
        assert abs(float(sumsq[k]) - ref) <= 1e-7 * ref, (shapes[k], float(sumsq[k]), ref)     # (act' is applied in fp32)
        if items[k][5] is not None:
            assert torch.allclose(items[k][5].double(), gbias, rtol=1e-5, atol=2e-5), shapes[k]
    # gathered operands: 8 rank segments of 12 rows each, [g | x | other layers' rows] per segment
    world, M, N, K = 8, 12, 1800, 600
    total = M * (N + K) + 128
    recv = torch.randn(world * total, device=DEV, generator=g)
    gb = torch.full((N,), float("nan"), device=DEV)
    seg = recv.view(world, total)
    gd = seg[:, :M * N].reshape(world * M, N).double()
    xd = seg[:, M * N:M * (N + K)].reshape(world * M, K).double()
    table, _blocks, rows = q.strip_table([(M, N, K, 0, M * N, torch.empty(N, K, device=DEV), gb, False, recv, total)], seg=world)
    assert rows == world * M
    cg._lib.call("cgv_wgrad_gram_mfma", cg._lib.ptr(table), 1, rows, cg._lib.ptr(sumsq), cg._lib.ptr(ws), ws.numel(),
                 cg._lib.stream_ptr())
    ref = float(((gd.T @ xd) ** 2).sum())
    assert abs(float(sumsq[0]) - ref) <= 1e-9 * ref
    assert torch.allclose(gb.double(), gd.sum(0), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("captured", [False, True])
def test_rank_update_training_matches_materialised_gradients(captured):
    """Trainer(rank_update=True) -- bead-level weight gradients never written -- against rank_update=False: same losses,
    norms and parameters up to the rounding of the norm (Gram form vs sum of squared entries)."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["chignolin"]

    def run(rank):
        model = cg.build_model(64, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 3, w["n_cgs"], det=True, seed=123).to(DEV)
        batch = cg.synthetic_batch("chignolin", n_frames=2, seed=4, device=DEV)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"], rank_update=rank)
        losses = [float(tr.step(batch)) for _ in range(3)]
        if captured:
            tr.capture(batch, warmup=0, train=True)
        for k in range(5):
            losses.append(float(tr.step(batch, train=(k != 2))))       # one validation step in between
        norm = float(tr.state[1])
        return losses, {k: v.clone() for k, v in model.state_dict().items()}, norm, tr

    l0, p0, n0, _ = run(False)
    l1, p1, n1, tr = run(True)
    assert tr.rank_steps >= 2 and tr.rank_fallbacks == 0 and tr._rank_hi > 0
    assert abs(n0 - n1) <= 1e-5 * n0
    assert np.allclose(l0, l1, rtol=1e-5)
    for k in p0:
        assert torch.allclose(p0[k], p1[k], rtol=1e-4, atol=1e-6), k


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("workload,F,enc", [("chignolin", 64, 2), ("dipeptide", 32, 3)])
def test_activation_derivative_applied_downstream_trains_alike(workload, F, enc, captured, options):
    """``act_downstream`` 1: the second layer of a Dense(Swish) -> Dense chain on the tile kernels stores its input
    gradient times Swish'(z) of the first (cgv_tile_linear_bwd_input_out / cgv_tile_pair_linear_bwd_input_out: encoder
    pair launches, unpaired message / contractive blocks, the atom-level update blocks), whose backward launches then run
    without an activation -- against 0 (Swish'(z) in the first layer's operand loads): the same products of the same
    operands, so losses, norms and parameters agree to rounding of the weight-gradient sums."""
    from coarsegrainingvae_amd.trainer import Trainer
    from coarsegrainingvae_amd import primitives
    w = cg.data.WORKLOADS[workload]
    calls = {"n": 0}
    real = cg._lib.call

    def counting(name, *a, **k):
        if name in ("cgv_tile_linear_bwd_input_out", "cgv_tile_pair_linear_bwd_input_out"):
            calls["n"] += 1
        return real(name, *a, **k)

    def run(flag):
        options.set("act_downstream", flag)
        model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], enc, 2, w["n_cgs"], seed=123).to(DEV)
        batch = cg.synthetic_batch(workload, seed=4, device=DEV)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
        gen = torch.Generator(device=DEV).manual_seed(1)
        eps = torch.randn(batch["CG_nxyz"].shape[0], F, device=DEV, generator=gen)
        losses = [float(tr.step(batch, eps=eps)) for _ in range(3)]
        if captured:
            tr.capture(batch, eps=eps, warmup=0, train=True)
        losses += [float(tr.step(batch, eps=eps)) for _ in range(3)]
        return losses, {k: v.clone() for k, v in model.state_dict().items()}, float(tr.state[1])

    l0, p0, n0 = run(0)
    cg._lib.call = counting
    try:
        l1, p1, n1 = run(1)
    finally:
        cg._lib.call = real
    assert calls["n"] >= 3 * (enc + 1)                       # the epilogue form did run (every eager step, every chain)
    assert np.allclose(l0, l1, rtol=2e-6), (l0, l1)
    assert abs(n0 - n1) <= 2e-6 * n0
    for k in p0:
        assert torch.allclose(p0[k], p1[k], rtol=1e-5, atol=1e-7), k


def _two_layer_fp64(x, l1, l2s, gos):
    """fp64 gradients of sum_k <l2s[k](swish(l1(x))), gos[k]> w.r.t. x, l1.weight, l1.bias and every l2 weight."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    W1, b1 = l1.weight.detach().double().cpu().requires_grad_(True), l1.bias.detach().double().cpu().requires_grad_(True)
    z = x64 @ W1.t() + b1
    a = z * torch.sigmoid(z)
    W2 = [l.weight.detach().double().cpu().requires_grad_(True) for l in l2s]
    total = sum(((a @ w.t() + l.bias.detach().double().cpu()) * go.double().cpu()).sum() for w, l, go in zip(W2, l2s, gos))
    total.backward()
    return x64.grad, W1.grad, b1.grad, [w.grad for w in W2]


@pytest.mark.parametrize("M,N", [(332, 600), (64, 600), (96, 5400), (12, 600)])
def test_downstream_activation_flag_lives_for_one_backward_of_a_retained_graph(M, N, options):
    """Dense(Swish) -> Dense(sole_consumer=True) (modules.py:103-114; the ``inv_dense`` chains of conv.py:31-61): the second
    layer's backward-input launch may store gx * Swish'(z) of the first and flag that node (``act_done``).  The flag is
    valid for the backward that set it only: backward a retained graph twice, the second time with the consumer's fused
    epilogue taken away (what a different dispatch -- row split refused, split workspace not ready inside a capture --
    amounts to); the first layer must then apply Swish'(z) itself again.  Both backwards against fp64."""
    from coarsegrainingvae_amd.primitives import Dense, Swish
    options.set("act_downstream", 1)
    torch.manual_seed(3)
    K = 600
    l1, l2 = Dense(K, K, activation=Swish()).to(DEV), Dense(K, N).to(DEV)
    x = torch.randn(M, K, device=DEV, requires_grad=True)
    go = torch.randn(M, N, device=DEV)
    out = l2(l1(x), sole_consumer=True)
    consumer = out.grad_fn
    fused_with = consumer.producer
    ref = _two_layer_fp64(x, l1, [l2], [go])
    for attempt in range(3):
        for t in (x, l1.weight, l1.bias, l2.weight):
            t.grad = None
        # second backward: the consumer does not apply the epilogue; third: it does again
        consumer.producer = None if attempt == 1 else fused_with
        out.backward(go, retain_graph=True)
        assert_close(x.grad, ref[0], f"gx, backward {attempt}", 2e-5)
        assert_close(l1.weight.grad, ref[1], f"gW1, backward {attempt}", 2e-5)
        assert_close(l1.bias.grad, ref[2], f"gb1, backward {attempt}", 2e-5)
        assert_close(l2.weight.grad, ref[3][0], f"gW2, backward {attempt}", 2e-5)


@pytest.mark.parametrize("M", [332, 12])
def test_two_fused_consumers_of_one_activated_tensor_unclaim_the_producer(M, options):
    """``sole_consumer=True`` twice on the SAME activated tensor: neither layer may hand the producer dL/dz (autograd would
    add one consumer's dL/dz to the other's dL/da).  ``_claim_producer`` lets the first claim, the second un-claims for
    both; the gradients are the plain ones (fp64)."""
    from coarsegrainingvae_amd.primitives import Dense, Swish
    options.set("act_downstream", 1)
    torch.manual_seed(4)
    K = 600
    l1, l2, l3 = Dense(K, K, activation=Swish()).to(DEV), Dense(K, K).to(DEV), Dense(K, 1800).to(DEV)
    x = torch.randn(M, K, device=DEV, requires_grad=True)
    a = l1(x)
    o2, o3 = l2(a, sole_consumer=True), l3(a, sole_consumer=True)
    assert o2.grad_fn.producer is None and o3.grad_fn.producer is None
    g2, g3 = torch.randn_like(o2), torch.randn_like(o3)
    ref = _two_layer_fp64(x, l1, [l2, l3], [g2, g3])
    torch.autograd.backward([o2, o3], [g2, g3])
    assert_close(x.grad, ref[0], "gx", 2e-5)
    assert_close(l1.weight.grad, ref[1], "gW1", 2e-5)
    assert_close(l2.weight.grad, ref[3][0], "gW2", 2e-5)
    assert_close(l3.weight.grad, ref[3][1], "gW3", 2e-5)


@pytest.mark.parametrize("M,N,K,act_out,with_add", [(332, 1800, 600, 1, False), (704, 600, 1200, 1, True), (97, 604, 52, 2, False)])
def test_backward_input_with_the_downstream_activation_epilogue_vs_fp64(M, N, K, act_out, with_add):
    """cgv_tile_linear_bwd_input_out / cgv_tile_pair_linear_bwd_input_out: gx = (add + (gy * act'(z)) W) * act_out'(z_out),
    ragged tiles, with and without the added gradient, one NULL z_out in the pair form."""
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=g)
    gy, z, W, zo, add = rnd(M, N), rnd(M, N), rnd(N, K) / N ** 0.5, rnd(M, K), rnd(M, K)
    gy2, z2, W2, zo2 = rnd(M, N), rnd(M, N), rnd(N, K) / N ** 0.5, rnd(M, K)

    def act_bwd(t, code):
        t = t.double()
        if code == 1:
            sg = torch.sigmoid(t)
            return sg * (1 + t * (1 - sg))
        return 1 - torch.tanh(t) ** 2

    ref = ((gy.double() * act_bwd(z, 1)) @ W.double() + (add.double() if with_add else 0)) * act_bwd(zo, act_out)
    gx = torch.empty(M, K, device=DEV)
    cg._lib.call("cgv_tile_linear_bwd_input_out", cg._lib.ptr(gy), cg._lib.ptr(z), cg._lib.ptr(W), cg._lib.ptr(add) if with_add else None,
                 cg._lib.ptr(gx), M, N, K, 1, cg._lib.ptr(zo), act_out, cg._lib.stream_ptr())
    assert_close(gx, ref, "single", 5e-6)
    ref2 = gy2.double() @ W2.double()                        # second problem: no activations at all, NULL z_out
    ref1 = (gy.double() @ W.double()) * act_bwd(zo, act_out)
    ga, gb = torch.empty(M, K, device=DEV), torch.empty(M, K, device=DEV)
    cg._lib.call("cgv_tile_pair_linear_bwd_input_out", cg._lib.ptr(gy), None, cg._lib.ptr(W), None, cg._lib.ptr(ga), cg._lib.ptr(gy2), None,
                 cg._lib.ptr(W2), None, cg._lib.ptr(gb), M, N, K, 0, 0, cg._lib.ptr(zo), act_out, None, 0, cg._lib.stream_ptr())
    assert_close(ga, ref1, "pair a", 5e-6)
    assert_close(gb, ref2, "pair b", 5e-6)
    cg._lib.call("cgv_tile_pair_linear_bwd_input_out", cg._lib.ptr(gy), cg._lib.ptr(z), cg._lib.ptr(W), None, cg._lib.ptr(ga), cg._lib.ptr(gy2),
                 cg._lib.ptr(z2), cg._lib.ptr(W2), None, cg._lib.ptr(gb), M, N, K, 1, 1, cg._lib.ptr(zo), act_out, cg._lib.ptr(zo2), 1,
                 cg._lib.stream_ptr())
    assert_close(ga, ((gy.double() * act_bwd(z, 1)) @ W.double()) * act_bwd(zo, act_out), "pair a, both activations", 5e-6)
    assert_close(gb, ((gy2.double() * act_bwd(z2, 1)) @ W2.double()) * act_bwd(zo2, 1), "pair b, both activations", 5e-6)


@pytest.mark.parametrize("M,N,K,with_add", [(96, 5400, 600, False), (64, 4096, 200, True), (17, 4800, 64, True)])
def test_row_split_backward_input_with_the_downstream_activation_vs_fp64(M, N, K, with_add):
    """cgv_skinny_linear_bwd_input_out: the reduction launch of the row-split product (few rows x a very long reduction:
    the decoder's Dense(F -> 9 F) at 96 bead rows) multiplies the sum by Swish'(z_out) of the layer before."""
    from coarsegrainingvae_amd.primitives import skinny_bwd_input_out
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=g)
    gy, z, W, zo, add = rnd(M, N), rnd(M, N), rnd(N, K) / N ** 0.5, rnd(M, K), rnd(M, K)
    sw = lambda t: torch.sigmoid(t.double()) * (1 + t.double() * (1 - torch.sigmoid(t.double())))
    ref = ((gy.double() * sw(z)) @ W.double() + (add.double() if with_add else 0)) * sw(zo)
    gx = torch.empty(M, K, device=DEV)
    assert skinny_bwd_input_out(gy, z, W, add if with_add else None, gx, M, N, K, 1, zo, 1)
    assert_close(gx, ref, "row-split product, Swish' downstream", 5e-6)
    ref0 = (gy.double() @ W.double()) * sw(zo)
    assert skinny_bwd_input_out(gy, None, W, None, gx, M, N, K, 0, zo, 1)
    assert_close(gx, ref0, "no activation of its own", 5e-6)


@pytest.mark.parametrize("M,N,K", [(96, 1800, 600), (96, 5400, 600), (128, 5400, 600), (70, 1036, 204), (33, 4100, 64),
                                   (16, 2048, 64)])
def test_backward_input_reduction_split_over_blocks_is_deterministic_and_exact(M, N, K, options):
    """cgv_tile_bwd_input_split + CGV_OPT_BWD_INPUT_SPLIT: few output tiles x a long reduction run as 2-4 blocks per tile, the
    last block to arrive adding the partial tiles in share order.  Every share count against fp64 and against the unsplit
    launch, repeated launches bit-identical (the tickets reset themselves), the epilogues (added gradient, Swish' of the
    layer before, the pair form with one NULL z_out) applied once by the combining block; a stream without a registered
    workspace runs unsplit."""
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + K)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=g)
    gy, z, W, zo, add = rnd(M, N), rnd(M, N), rnd(N, K) / N ** 0.5, rnd(M, K), rnd(M, K)
    gy2, W2 = rnd(M, N), rnd(N, K) / N ** 0.5
    sw = lambda t: torch.sigmoid(t.double()) * (1 + t.double() * (1 - torch.sigmoid(t.double())))
    ref = ((gy.double() * sw(z)) @ W.double() + add.double()) * sw(zo)
    ref_plain, ref2 = gy.double() @ W.double(), gy2.double() @ W2.double()
    P = cg._lib.ptr

    def single():
        gx = torch.empty(M, K, device=DEV)
        cg._lib.call("cgv_tile_linear_bwd_input_out", P(gy), P(z), P(W), P(add), P(gx), M, N, K, 1, P(zo), 1, cg._lib.stream_ptr())
        return gx

    def pair():
        ga, gb = torch.empty(M, K, device=DEV), torch.empty(M, K, device=DEV)
        cg._lib.call("cgv_tile_pair_linear_bwd_input_out", P(gy), None, P(W), None, P(ga), P(gy2), None, P(W2), P(add), P(gb), M, N, K,
                     0, 0, P(zo), 1, None, 0, cg._lib.stream_ptr())
        return ga, gb

    options.set("bwd_input_split", 1)
    unsplit, (ua, ub) = single(), pair()
    assert_close(unsplit, ref, "unsplit", 5e-6)
    for shares in (-1, 2, 3, 4):
        options.set("bwd_input_split", shares)
        first = single()
        assert_close(first, ref, f"shares {shares}", 5e-6)
        assert_close(first, unsplit.double(), f"shares {shares} against the unsplit launch", 2e-6)
        for _ in range(3):
            assert torch.equal(single(), first), f"shares {shares}: repeated launches differ"
        ga, gb = pair()
        assert_close(ga, ref_plain * sw(zo), f"pair a, shares {shares}", 5e-6)
        assert_close(gb, ref2 + add.double(), f"pair b, shares {shares}", 5e-6)
        assert_close(ga, ua.double(), f"pair a against the unsplit launch, shares {shares}", 2e-6)
        ga2, gb2 = pair()
        assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
    # another stream of the same thread: no workspace registered for it inside ... the host mirror registers one per stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = single()
    side.synchronize()
    assert torch.equal(other, first)
    # the C ABI refuses a workspace that is too small or misaligned, and NULL unregisters
    lib = cg._lib.load()
    small = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    assert lib.cgv_tile_bwd_input_split(small.data_ptr(), small.numel(), cg._lib.stream_ptr()) != 0
    big = torch.zeros(64 * 1024 + 4 * 1024 * 1024 + 16, dtype=torch.uint8, device=DEV)
    assert lib.cgv_tile_bwd_input_split(big.data_ptr() + 4, big.numel() - 16, cg._lib.stream_ptr()) != 0
    assert lib.cgv_tile_bwd_input_split(None, 0, cg._lib.stream_ptr()) == 0
    cg._lib._SPLIT_TLS.cur = None                             # (this thread's registration was replaced just above)
    gx = torch.empty(M, K, device=DEV)
    rc = lib.cgv_tile_linear_bwd_input_out(P(gy), P(z), P(W), P(add), P(gx), M, N, K, 1, P(zo), 1, cg._lib.stream_ptr())
    assert rc == 0
    assert torch.equal(gx, unsplit), "no workspace registered: the unsplit launch"
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1500, 1400, 600, 1), (1411, 1796, 52, 0), (2000, 1800, 600, 2)])
def test_tile_forward_lds_staged_kernel_vs_fp64(shape):
    """cgv_tile_linear_fwd on shapes with >= 448 output tiles of 64 x 64 takes the LDS-staged kernel (tile_fwd_lds_k):
    ragged row / column / reduction tails, bias + activation epilogue, pre-activation output."""
    M, N, K, act = shape
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    y = torch.full((M, N), float("nan"), device=DEV)
    z = torch.full((M, N), float("nan"), device=DEV)
    cg._lib.call("cgv_tile_linear_fwd", cg._lib.ptr(x), cg._lib.ptr(W), cg._lib.ptr(b), cg._lib.ptr(y), cg._lib.ptr(z), M, N, K, act,
                 cg._lib.stream_ptr())
    zr = x.double() @ W.double().T + b.double()
    yr = {0: zr, 1: zr * torch.sigmoid(zr), 2: torch.tanh(zr)}[act]
    assert torch.allclose(y.double(), yr, rtol=1e-5, atol=1e-5)
    if act:
        assert torch.allclose(z.double(), zr, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(332, 1800, 600, 1), (704, 600, 1200, 0), (77, 36, 580, 2), (64, 64, 608, 0), (130, 68, 1188, 1),
                                   (2000, 1800, 600, 0), (333, 1796, 596, 1)])
def test_tile_forward_ring_kernel_vs_fp64(shape, options):
    """The LDS-staged forward with a ring of three slabs of global loads in flight (tile_fwd_ring_k; option
    tile_fwd_lds_min = 3 forces it on every shape it is compiled for: 19 or 38 slabs of 32, i.e. K = 577 .. 608 and
    1185 .. 1216): mid-size and ragged shapes, ragged reduction tails, bias + activation epilogue, pre-activation output."""
    options.set("tile_fwd_lds_min", 3)
    M, N, K, act = shape
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    y = torch.full((M, N), float("nan"), device=DEV)
    z = torch.full((M, N), float("nan"), device=DEV)
    cg._lib.call("cgv_tile_linear_fwd", cg._lib.ptr(x), cg._lib.ptr(W), cg._lib.ptr(b), cg._lib.ptr(y), cg._lib.ptr(z), M, N, K, act,
                 cg._lib.stream_ptr())
    zr = x.double() @ W.double().T + b.double()
    yr = {0: zr, 1: zr * torch.sigmoid(zr), 2: torch.tanh(zr)}[act]
    assert torch.allclose(y.double(), yr, rtol=1e-5, atol=1e-5)
    if act:
        assert torch.allclose(z.double(), zr, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(100, 8, 8), (70, 12, 4), (333, 20, 8), (96, 4, 24)])
def test_tile_gemms_with_reductions_shorter_than_a_step(shape):
    """Tile forward / bwd_input with K (resp. N) below the 16-float step of the kernels: the lanes beyond the reduction
    read a clamped, in-range address and must contribute nothing -- operands sit at the very end of their allocation
    neighbourhood and are surrounded by NaNs, so an out-of-row read shows."""
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(N * K)
    def fenced(rows, cols):
        buf = torch.full((rows * cols + 64,), float("nan"), device=DEV)
        t = buf[32:32 + rows * cols].view(rows, cols)
        t.copy_(torch.randn(rows, cols, device=DEV, generator=g))
        return t
    x, W, gy = fenced(M, K), fenced(N, K), fenced(M, N)
    b = torch.randn(N, device=DEV, generator=g)
    y, z = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    cg._lib.call("cgv_tile_linear_fwd", cg._lib.ptr(x), cg._lib.ptr(W), cg._lib.ptr(b), cg._lib.ptr(y), cg._lib.ptr(z), M, N, K, 0,
                 cg._lib.stream_ptr())
    assert torch.allclose(y.double(), x.double() @ W.double().T + b.double(), rtol=1e-5, atol=1e-5)
    gx = torch.empty(M, K, device=DEV)
    cg._lib.call("cgv_tile_linear_bwd_input", cg._lib.ptr(gy), cg._lib.ptr(W), cg._lib.ptr(gx), M, N, K, cg._lib.stream_ptr())
    assert torch.allclose(gx.double(), gy.double() @ W.double(), rtol=1e-5, atol=1e-5)


def test_rank_update_kernels_on_random_shapes():
    """cgv_wgrad_gram / cgv_grouped_wgrad_adam over 24 random problems in one table (1 - 40 rows, widths in multiples of
    4 from 4 to 700, every activation code, with / without bias): norms against fp64, one Adam step against fp64."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    lib = cg._lib.load()
    rng = np.random.default_rng(7)
    g = torch.Generator(device=DEV).manual_seed(11)
    shapes = []
    for k in range(24):
        M = int(rng.integers(1, 41))
        N, K = 4 * int(rng.integers(1, 176)), 4 * int(rng.integers(1, 176))
        shapes.append((M, N, K, int(rng.integers(0, 4)), bool(rng.integers(0, 2))))
    shapes[0] = (40, 700, 4, 1, True)
    shapes[1] = (1, 4, 700, 0, False)
    n_total = sum(N * K for _, N, K, _, _ in shapes)
    arena_g = torch.zeros(n_total, device=DEV)
    arena_p = torch.randn(n_total, device=DEV, generator=g)
    arena_m = torch.zeros(n_total, device=DEV)
    arena_v = torch.zeros(n_total, device=DEV)
    p0 = arena_p.double().clone()
    items, refs, off = [], [], 0
    for M, N, K, act, bias in shapes:
        gy = torch.randn(M, N, device=DEV, generator=g)
        x = torch.randn(M, K, device=DEV, generator=g)
        z = torch.randn(M, N, device=DEV, generator=g) if act else None
        gb = torch.full((N,), float("nan"), device=DEV) if bias else None
        items.append((gy, x, z, act, arena_g[off:off + N * K].view(N, K), gb, False))
        gd = gy.double()
        if act:
            zd = z.double()
            sg = torch.sigmoid(zd)
            gd = gd * {1: sg * (1 + zd * (1 - sg)), 2: 1 - torch.tanh(zd) ** 2, 3: (zd > 0).double()}[act]
        refs.append((gd.T @ x.double(), gd.sum(0), off))
        off += N * K
    assert all(lib.cgv_rank_update_supported(M, N, K) for M, N, K, _, _ in shapes)
    table, blocks, lds = WeightGradQueue().small_table(items)
    sumsq = torch.zeros(len(items), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(lib.cgv_wgrad_gram_workspace_bytes(len(items))), dtype=torch.uint8, device=DEV)
    cg._lib.call("cgv_wgrad_gram", cg._lib.ptr(table), len(items), max(it[0].shape[0] for it in items), cg._lib.ptr(sumsq),
                 cg._lib.ptr(ws), ws.numel(), cg._lib.stream_ptr())
    for k, (gw, gbias, _) in enumerate(refs):
        want = float((gw ** 2).sum())
        assert abs(float(sumsq[k]) - want) <= 2e-6 * want + 1e-12, (k, shapes[k])
        if items[k][5] is not None:
            assert torch.allclose(items[k][5].double(), gbias, rtol=1e-5, atol=1e-5), (k, shapes[k])
    state = torch.zeros(lib.cgv_optim_state_floats(), device=DEV)
    partial = torch.zeros(lib.cgv_optim_partial_floats(), device=DEV)
    lr, b1, b2, eps, max_norm = 1e-2, 0.9, 0.999, 1e-8, 1e9                  # no clipping: the update is lr * sign-like
    cg._lib.call("cgv_optim_prepare_extra", arena_g.data_ptr(), 0, cg._lib.ptr(sumsq), len(items), b1, b2, max_norm, 1.0,
                 None, 0.0, cg._lib.ptr(state), cg._lib.ptr(partial), cg._lib.stream_ptr())
    cg._lib.call("cgv_grouped_wgrad_adam", cg._lib.ptr(table), len(items), blocks, lds, cg._lib.ptr(arena_g), cg._lib.ptr(arena_p),
                 cg._lib.ptr(arena_m), cg._lib.ptr(arena_v), lr, b1, b2, eps, cg._lib.ptr(state), cg._lib.stream_ptr())
    for k, (gw, _, o) in enumerate(refs):
        gflat = gw.reshape(-1)
        sl = slice(o, o + gflat.numel())
        m1, v1 = (1 - b1) * gflat, (1 - b2) * gflat * gflat
        want = p0[sl] - (lr / (1 - b1)) * m1 / (v1.sqrt() / (1 - b2) ** 0.5 + eps)
        assert torch.allclose(arena_m[sl].double(), m1, rtol=2e-5, atol=3e-6), (k, shapes[k])     # fp32 sums of <= 40 terms
        # first Adam step: |update| = lr wherever |g| >> eps; compare where the gradient is not tiny
        big = gflat.abs() > 1e-3
        assert torch.allclose(arena_p[sl].double()[big], want[big], rtol=1e-5, atol=1e-5), (k, shapes[k])
    assert float(arena_g.abs().max()) == 0.0                               # never written


@pytest.mark.parametrize("rounds,mixed", [(1, 1), (2, 1), (2, 0), (5, 1)])
def test_flat_rank_update_equals_the_tiled_launch_bit_for_bit(rounds, mixed, options):
    """cgv_grouped_wgrad_adam_flat (contiguous ranges of a weight's p / m / v per block, x for all K columns + the g rows of
    the range in LDS) against cgv_grouped_wgrad_adam (64 rows x one k tile per block) on the same records: the operand rows
    are summed in the same order, so p, m and v agree BIT FOR BIT after two updates -- ragged sizes (a weight smaller
    than one block, K of 4, ranges that end mid row), activations, 1 - 16 rows, and a 36-row layer that stays tiled in the
    same table (WeightGradQueue.rank_table: flat records first, each part with its own block prefix) -- as a second launch
    or, ``rank_mixed``, in the same launch with its blocks dealt among the flat ones; a skipped step
    leaves the arenas alone; shapes beyond the layout (17 rows, x beyond the LDS budget) are refused by the plan."""
    import ctypes as C
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    from coarsegrainingvae_amd.trainer import Trainer
    lib = cg._lib.load()
    options.set("rank_mixed", mixed)
    g = torch.Generator(device=DEV).manual_seed(77 + rounds)
    shapes = [(12, 600, 600, 1), (36, 1200, 600, 1), (12, 1800, 600, 0), (12, 600, 1200, 1), (16, 52, 900, 2), (1, 4, 700, 0),
              (7, 700, 4, 1), (3, 333 * 4, 36, 3), (12, 5400, 600, 0), (5, 8, 8, 1)]
    n_total = sum(N * K for _, N, K, _ in shapes)
    arena_g = torch.zeros(n_total, device=DEV)
    p0 = torch.randn(n_total, device=DEV, generator=g)
    items, off = [], 0
    for M, N, K, act in shapes:
        gy, x = torch.randn(M, N, device=DEV, generator=g), torch.randn(M, K, device=DEV, generator=g)
        z = torch.randn(M, N, device=DEV, generator=g) if act else None
        items.append((gy, x, z, act, arena_g[off:off + N * K].view(N, K), None, False))
        off += N * K
    q = WeightGradQueue()
    t_table, t_items, t_flat, t_tiled = q.rank_table(items, -1)
    f_table, f_items, f_flat, f_tiled = q.rank_table(items, rounds * 2048)
    assert t_flat[0] == 0 and t_tiled[0] == len(items) and [id(a) for a in t_items] == [id(a) for a in items]
    assert f_flat[0] == len(items) - 1 and f_flat[3] == rounds * 2048 and f_tiled[0] == 1 and f_items[-1][0].shape[0] == 36
    ws = torch.empty(int(lib.cgv_wgrad_gram_workspace_bytes(len(items))), dtype=torch.uint8, device=DEV)
    sums = []
    for table in (t_table, f_table):                  # the norm launch reads either table (block fields unused)
        sumsq = torch.zeros(len(items), dtype=torch.float64, device=DEV)
        cg._lib.call("cgv_wgrad_gram", cg._lib.ptr(table), len(items), 36, cg._lib.ptr(sumsq), cg._lib.ptr(ws), ws.numel(), cg._lib.stream_ptr())
        sums.append(sumsq)
    order = [[id(a) for a in f_items].index(id(a)) for a in items]
    assert torch.equal(sums[0], sums[1][order])
    state = torch.zeros(lib.cgv_optim_state_floats(), device=DEV)
    partial = torch.zeros(lib.cgv_optim_partial_floats(), device=DEV)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8

    class Arena:                                        # what Trainer.rank_update_launch reads of its trainer
        pass
    holder = Arena()
    holder.arena = Arena()
    holder.arena.g = arena_g
    out = []
    for table, ordered, flat, tiled, sq in ((t_table, t_items, t_flat, t_tiled, sums[0]), (f_table, f_items, f_flat, f_tiled, sums[1])):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        state.zero_()
        rank = (table, len(items), tiled[1], tiled[2], ordered, 36, flat)
        for _step in range(2):
            cg._lib.call("cgv_optim_prepare_extra", arena_g.data_ptr(), 0, cg._lib.ptr(sq), len(items), b1, b2, 0.5, 1.0,
                         None, 0.0, cg._lib.ptr(state), cg._lib.ptr(partial), cg._lib.stream_ptr())       # clipped: ||g|| >> 0.5
            Trainer.rank_update_launch(holder, rank, p, m, v, lr, b1, b2, eps, state)
        out.append((p, m, v))
    for a, b, name in zip(out[0], out[1], "pmv"):
        assert torch.equal(a, b), f"{name}: flat and tiled layouts differ (max {float((a - b).abs().max()):.3e})"
    assert float((out[1][0] != p0).float().mean()) > 0.9 and float(out[1][2].min()) >= 0.0     # (a relu layer with every row off stays)
    assert float(arena_g.abs().max()) == 0.0                               # never written
    # a skipped step (loss above the threshold): nothing moves
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    loss = torch.full((1,), 10.0, device=DEV)
    cg._lib.call("cgv_optim_prepare_extra", arena_g.data_ptr(), 0, cg._lib.ptr(sums[1]), len(items), b1, b2, 0.5, 1.0, cg._lib.ptr(loss), 1.0,
                 cg._lib.ptr(state), cg._lib.ptr(partial), cg._lib.stream_ptr())
    Trainer.rank_update_launch(holder, (f_table, len(items), f_tiled[1], f_tiled[2], f_items, 36, f_flat), p, m, v, lr, b1, b2, eps, state)
    assert torch.equal(p, p0) and float(m.abs().max()) == 0.0
    nb, lds = C.c_int(), C.c_int()
    assert lib.cgv_rank_flat_plan(17, 600, 600, 0, C.byref(nb), C.byref(lds)) != 0          # more than 16 rows
    assert lib.cgv_rank_flat_plan(12, 600, 1800, 0, C.byref(nb), C.byref(lds)) != 0         # x [12, 1800] beyond the LDS budget
    assert lib.cgv_rank_flat_plan(12, 600, 600, 0, C.byref(nb), C.byref(lds)) == 0 and nb.value == (600 * 150 + 4095) // 4096


def test_prefetched_double_buffered_steps_equal_plain_replays():
    """``Trainer.enable_prefetch``: the next batch is loaded into a second buffer set on a side stream while the current
    step's graph runs.  Same batches, same order => the same losses and parameters as loading each batch on the main
    stream right before its step (det=True: no random stream involved), bit for bit."""
    from coarsegrainingvae_amd.trainer import Trainer
    w = cg.data.WORKLOADS["dipeptide"]
    F = 64
    batches = [cg.synthetic_batch("dipeptide", n_frames=4, seed=40 + k, device=DEV) for k in range(4)]
    runs = []
    for prefetch in (False, True):
        first = cg.data.prepare_batch({k: v.clone() for k, v in batches[0].items() if not k.startswith("_")}, edge_slack=0.25)
        model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 2, 2, w["n_cgs"], det=True, seed=123).to(DEV)
        tr = Trainer(model, lr=1e-3, beta=w["beta"], gamma=w["gamma"])
        tr.step(first)
        tr.step(first)
        tr.capture(first, warmup=0)
        if prefetch:
            tr.enable_prefetch()
        losses = []
        for i in range(9):
            nxt = batches[(i + 1) % 4] if prefetch else None
            tr.step(batches[i % 4], prefetch=nxt)
            losses.append(tr.last_loss.clone())
        assert tr.replays == 9
        runs.append((torch.stack(losses).cpu(), tr.arena.p.clone().cpu()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_in_place_batch_update_by_job_tables_is_bit_exact():
    """``BatchGraph.update`` through the job tables (cgv_plan_jobs_build / cgv_geom_jobs_build: all sorted views in 4
    launches, all record arrays in 1) leaves exactly the arrays a freshly prepared batch has: both CSR views of the atom
    and bead plans, the receiver-group order, the embedding groupings, every cached edge-record array."""
    w = cg.data.WORKLOADS["chignolin"]
    model = cg.build_model(32, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 1, 1, w["n_cgs"], det=True, seed=1).to(DEV)
    raw = lambda seed: {k: v for k, v in cg.synthetic_batch("chignolin", n_frames=2, seed=seed, device=DEV).items() if not k.startswith("_")}
    held = cg.data.prepare_batch(raw(1), edge_slack=0.25)
    with torch.no_grad():
        model(held)                                  # creates the geometries / embedding plans the model uses
    for seed in (2, 3):
        fresh = cg.data.prepare_batch(raw(seed))
        with torch.no_grad():
            out_fresh = model(fresh)
        assert cg.data.copy_batch_into(held, fresh)
        a, b = held["_graph"], fresh["_graph"]
        for name in ("atom", "cg"):
            pa, pb = getattr(a, name), getattr(b, name)
            E = pb.n_edges
            assert pa.n_edges == E
            for f in ("rowptr_d", "rowptr_s"):
                assert torch.equal(getattr(pa, f), getattr(pb, f)), (name, f)
            for f in ("eid_d", "dst_d", "src_d", "eid_s", "dst_s", "src_s"):
                assert torch.equal(getattr(pa, f)[:E], getattr(pb, f)[:E]), (name, f)
        E = b.atom.n_edges
        for f in ("dst_g", "src_g", "pos_g"):
            assert torch.equal(getattr(a.atom, f)[:E], getattr(b.atom, f)[:E]), f
        assert torch.equal(a.atom.meta_g[:2 * E], b.atom.meta_g[:2 * E])
        for key, ga in a._geom.items():
            gb = b._geom[key]
            plan = a._positions(key[0])[0]
            n = plan.n_edges
            assert torch.equal(ga.geom_d[:n], gb.geom_d[:n]) and torch.equal(ga.geom_s[:n], gb.geom_s[:n]), key
            if ga.geom_g is not None:
                assert torch.equal(ga.geom_g[:n], gb.geom_g[:n]), key
        for key, (pa, _idx) in a._embed.items():
            pb = b._embed[key][0]
            assert torch.equal(pa.rowptr_d, pb.rowptr_d) and torch.equal(pa.eid_d, pb.eid_d), key
        with torch.no_grad():
            out_held = model(held)
        for x, y in zip(out_held, out_fresh):
            assert torch.equal(x, y)


def test_reparam_sample_draws_standard_normals_in_the_launch():
    """cgv_reparam_sample: z = mu + sigma * eps with eps drawn in the launch (Philox4x32-10 + Box-Muller): moments and
    tails of a standard normal, a fresh draw per launch, the same draw for the same {seed, draw number}, eps stored, and
    the backward of the autograd wrapper."""
    from coarsegrainingvae_amd import ops
    n = 1 << 20
    mu = torch.randn(n, device=DEV)
    sigma = torch.rand(n, device=DEV) + 0.5
    rng = torch.tensor([1234567, 0, 0], dtype=torch.int64, device=DEV)
    eps, z = torch.empty_like(mu), torch.empty_like(mu)
    call = lambda e, zz, r: cg._lib.call("cgv_reparam_sample", cg._lib.ptr(mu), cg._lib.ptr(sigma), cg._lib.ptr(e), cg._lib.ptr(zz),
                                         n, cg._lib.ptr(r), cg._lib.stream_ptr())
    call(eps, z, rng)
    torch.cuda.synchronize()
    assert rng.tolist() == [1234567, 1, 0]                               # draw number advanced, ticket re-armed
    assert torch.allclose(z, mu + eps * sigma, rtol=1e-6, atol=1e-6)     # one fma here, mul + add there
    e = eps.double()
    assert abs(float(e.mean())) < 4e-3 and abs(float(e.var()) - 1.0) < 6e-3
    assert abs(float((e ** 3).mean())) < 2e-2 and abs(float((e ** 4).mean()) - 3.0) < 5e-2
    assert 0.6815 < float((e.abs() < 1).double().mean()) < 0.6840 and 0.0024 < float((e.abs() > 3).double().mean()) < 0.0030
    assert abs(float((e[:-1] * e[1:]).mean())) < 4e-3 and abs(float((e[:-4:4] * e[2::4][:e[:-4:4].numel()]).mean())) < 8e-3
    eps2, z2 = torch.empty_like(mu), torch.empty_like(mu)
    call(eps2, z2, rng)                                                  # next draw
    assert not torch.equal(eps2, eps) and abs(float((eps2.double() * e).mean())) < 4e-3
    rng_again = torch.tensor([1234567, 0, 0], dtype=torch.int64, device=DEV)
    eps3, z3 = torch.empty_like(mu), torch.empty_like(mu)
    call(eps3, z3, rng_again)
    assert torch.equal(eps3, eps) and torch.equal(z3, z)                 # same seed, same draw number: same numbers
    m = torch.randn(12, 600, device=DEV, requires_grad=True)
    s = (torch.rand(12, 600, device=DEV) + 0.5).requires_grad_()
    out = ops.reparam_sample(m, s)
    g = torch.randn_like(out)
    gm, gs = torch.autograd.grad(out, (m, s), g)
    eps_used = (out.detach() - m.detach()) / s.detach()
    assert torch.equal(gm, g) and torch.allclose(gs, g * eps_used, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("M,N,K,same_x,acts", [(12, 600, 600, True, (2, 2)), (12, 600, 600, False, (0, 4)), (7, 64, 132, True, (3, 3)),
                                                (16, 128, 64, False, (1, 0)), (12, 600, 1200, True, (2, 5))])
def test_pair_linear_equals_two_linear_layers(M, N, K, same_x, acts):
    """_PairLinearFn (layer j of a mu / sigma head pair in one launch, forward and backward-input) against two
    _LinearFn calls: outputs, input gradients (summed when both read the same input), weight / bias gradients."""
    from coarsegrainingvae_amd.primitives import _LinearFn, _PairLinearFn
    g = torch.Generator(device=DEV).manual_seed(M * 1000 + N + K)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)
    xa = mk(M, K).requires_grad_()
    xb = xa if same_x else mk(M, K).requires_grad_()
    wa, wb = (0.05 * mk(N, K)).requires_grad_(), (0.05 * mk(N, K)).requires_grad_()
    ba, bb = mk(N).requires_grad_(), mk(N).requires_grad_()
    ga, gb = mk(M, N), mk(M, N)
    ya, yb = _PairLinearFn.apply(xa, xb, wa, ba, wb, bb, acts[0], acts[1])
    ins = (xa, wa, ba, wb, bb) if same_x else (xa, xb, wa, ba, wb, bb)
    got = torch.autograd.grad((ya, yb), ins, (ga, gb))
    ra, rb = _LinearFn.apply(xa, wa, ba, acts[0]), _LinearFn.apply(xb, wb, bb, acts[1])
    want = torch.autograd.grad((ra, rb), ins, (ga, gb))
    assert rel_err(ya, ra) <= 1e-6 and rel_err(yb, rb) <= 1e-6
    for a, b in zip(got, want):
        assert rel_err(a, b) <= 2e-6, (a.shape, rel_err(a, b))


def test_device_drawn_noise_path_equals_supplied_noise_path():
    """The training step with the noise drawn inside the reparametrisation launch (cgv_reparam_sample; KL gradients handed
    to its backward, cgv_reparam_bwd) against the same step with that very noise supplied as ``eps`` (torch.addcmul,
    separate autograd contributions): same loss, same gradients.  The generator is deterministic in {seed, draw number},
    so the noise of the first run is drawn again by a direct call."""
    from coarsegrainingvae_amd import ops
    from coarsegrainingvae_amd.train import loss_terms
    w = cg.data.WORKLOADS["chignolin"]
    F = 64
    batch = cg.synthetic_batch("chignolin", n_frames=2, seed=9, device=DEV)
    model = cg.build_model(F, w["n_rbf"], w["atom_cutoff"], w["cg_cutoff"], 1, 2, w["n_cgs"], seed=5).to(DEV)
    n = batch["CG_nxyz"].shape[0]
    rng = ops._rng_block(torch.device(DEV))
    seed, draw = 424242, 7
    # what the launch will draw for this {seed, draw number}
    probe = torch.tensor([seed, draw, 0], dtype=torch.int64, device=DEV)
    zeros, ones = torch.zeros(n * F, device=DEV), torch.ones(n * F, device=DEV)
    eps, z = torch.empty(n * F, device=DEV), torch.empty(n * F, device=DEV)
    cg._lib.call("cgv_reparam_sample", cg._lib.ptr(zeros), cg._lib.ptr(ones), cg._lib.ptr(eps), cg._lib.ptr(z), n * F,
                 cg._lib.ptr(probe), cg._lib.stream_ptr())
    eps = eps.view(n, F)

    def run(supplied):
        model.zero_grad(set_to_none=True)
        rng.copy_(torch.tensor([seed, draw, 0], dtype=torch.int64))
        out = model(batch, eps=eps if supplied else None)
        loss, *_ = loss_terms(out, batch, w["beta"], w["gamma"])
        loss.backward()
        return float(loss), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    l_dev, g_dev = run(False)
    assert rng.tolist()[1] == draw + 1                                   # the step did draw
    l_sup, g_sup = run(True)
    assert abs(l_dev - l_sup) <= 1e-6 * abs(l_sup)
    assert g_dev.keys() == g_sup.keys() and len(g_dev) > 30
    for k in g_sup:
        assert rel_err(g_dev[k], g_sup[k]) <= 5e-5, k                   # z is one fma there, a rounded product + sum here


@pytest.mark.parametrize("n,F", [(3, 30), (3, 32), (5, 6)])
def test_kl_gradients_survive_the_reparametrisation_backward_at_any_size(n, F):
    """``reparam_sample`` parks d(beta KL)/d{mu, sigma} of the ELBO launch for its own backward, which adds them in one
    launch on aligned quads.  When n * F is not a multiple of 4 (F = 30, 3 beads) that launch cannot run: the parked
    terms must still reach mu and sigma.  Against the same loss with the very same noise supplied (plain autograd)."""
    from coarsegrainingvae_amd import ops
    gen = torch.Generator().manual_seed(n * 100 + F)
    mk = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    mu0, ls0, pmu0, pls0 = mk(n, F), mk(n, F), mk(n, F), mk(n, F)
    n_atoms = 2 * n
    proj, xyz = mk(F, 6), mk(n_atoms, 3)
    bonds = torch.stack([torch.arange(n_atoms - 1), torch.arange(1, n_atoms)], dim=1).to(DEV)
    rng = ops._rng_block(torch.device(DEV))
    seed, draw = 99, 3
    probe = torch.tensor([seed, draw, 0], dtype=torch.int64, device=DEV)
    pad = (n * F + 3) // 4 * 4
    zeros, ones = torch.zeros(pad, device=DEV), torch.ones(pad, device=DEV)
    eps, z = torch.empty(pad, device=DEV), torch.empty(pad, device=DEV)
    cg._lib.call("cgv_reparam_sample", cg._lib.ptr(zeros), cg._lib.ptr(ones), cg._lib.ptr(eps), cg._lib.ptr(z), n * F,
                 cg._lib.ptr(probe), cg._lib.stream_ptr())
    eps = eps[:n * F].view(n, F).clone()

    def run(supplied):
        leaves = [t.clone().requires_grad_(True) for t in (mu0, ls0, pmu0, pls0)]
        mu, pmu = leaves[0] * 1.0, leaves[2] * 1.0
        sigma, pstd = torch.exp(leaves[1] / 2), torch.exp(leaves[3] / 2)
        rng.copy_(torch.tensor([seed, draw, 0], dtype=torch.int64))
        zs = torch.addcmul(mu, eps, sigma) if supplied else ops.reparam_sample(mu, sigma)
        recon = (zs @ proj).reshape(n_atoms, 3)
        loss, _terms = ops.elbo_loss(mu, sigma, pmu, pstd, xyz, recon, bonds, 0.7, 3.0)
        loss.backward()
        return float(loss), [t.grad.clone() for t in leaves]

    l_dev, g_dev = run(False)
    l_sup, g_sup = run(True)
    assert abs(l_dev - l_sup) <= 1e-6 * abs(l_sup)
    for a, b, name in zip(g_dev, g_sup, ("mu", "log var", "prior mu", "prior log var")):
        assert rel_err(a, b) <= 1e-5, (name, rel_err(a, b))


@pytest.mark.parametrize("n,F,R,full,drop", [(40, 100, 10, False, None), (150, 64, 8, True, None), (24, 600, 10, True, "scalars"),
                                             (33, 132, 12, False, "vectors")])
def test_dense_bead_graph_message_kernels_equal_the_general_ones(n, F, R, full, drop, options):
    """K3 on dense bead graphs (>= 16 edges per node: the per-filter kernels pseudo_*_dense_k) against the general
    kernels (option pseudo_fwd = 2; themselves pinned to the golden vectors): ragged segments, a partial channel wave,
    segments longer than the staged index chunk (150 fully connected nodes), and a layer whose scalar or vector outputs
    go unused (upstream gradients absent).  Same operations, another summation order: fp32 rounding apart."""
    from coarsegrainingvae_amd import ops
    gen = torch.Generator().manual_seed(n * 7 + F)
    pos = 3.0 * torch.randn(n, 3, generator=gen)
    if full:
        pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    else:                                                # ragged: every node keeps 17 .. n - 1 random neighbours
        pairs = []
        for i in range(n):
            k = int(torch.randint(17, n, (1,), generator=gen))
            others = [j for j in torch.randperm(n, generator=gen).tolist() if j != i][:k]
            pairs += [(i, j) for j in others]
    nbrs = torch.tensor(pairs, dtype=torch.long)
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n)
    assert plan.n_edges >= 16 * n
    geom = EdgeGeometry(plan, R, 12.0, pos_dst=pos.to(DEV), pos_src=pos.to(DEV))
    rn = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    base = [rn(n, 9 * F), rn(n, F), rn(n, F), rn(n, F, 3), rn(n, F, 3), 0.3 * rn(9 * F, R), 0.3 * rn(9 * F)]
    gouts = [rn(n, F), rn(n, F), rn(n, F, 3), rn(n, F, 3)]
    used = {"scalars": (2, 3), "vectors": (0, 1)}.get(drop, (0, 1, 2, 3))

    def run(variant, residual):
        options.set("pseudo_fwd", variant)
        ins = [t.clone().requires_grad_(True) for t in base]
        outs = ops.pseudo_message(*ins, plan, geom, residual)
        torch.autograd.backward([outs[k] for k in used], [gouts[k] for k in used])
        return [o.detach() for o in outs], [t.grad for t in ins]

    for residual in (False, True):
        o_gen, g_gen = run(2, residual)
        o_dense, g_dense = run(0, residual)
        names = ["dh", "dhbar", "dv", "dvbar", "g_phi", "g_s", "g_sbar", "g_v", "g_vbar", "gWd", "gbd"]
        for name, a, b in zip(names, o_gen + g_gen, o_dense + g_dense):
            assert_close(b, a, f"{name} (residual={residual})", 3e-6)


@pytest.mark.parametrize("rows_per_block", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K", [(130, 52, 100), (64, 600, 600), (7, 20, 36), (300, 1800, 64)])
def test_skinny_forward_row_blocks(M, N, K, rows_per_block, options):
    """cgv_skinny_linear_fwd with its thread blocks owning 16 .. 64 rows each (blockIdx.y; option skinny_rows, 0 = the
    built-in rule), any row count: y = swish(x W^T + b) and the saved pre-activation against fp64."""
    from coarsegrainingvae_amd import _lib
    lib = _lib.load()
    assert lib.cgv_skinny_fwd_supported(M, N, K) and not lib.cgv_skinny_fwd_supported(M, N + 2, K)
    options.set("skinny_rows", rows_per_block)
    gen = torch.Generator().manual_seed(M + N + K)
    x, W, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    y = torch.full((M + 1, N), float("nan"), device=DEV)                  # one guard row behind the output
    z = torch.full((M + 1, N), float("nan"), device=DEV)
    xg, Wg, bg = x.to(DEV), W.to(DEV), b.to(DEV)
    _lib.call("cgv_skinny_linear_fwd", _lib.ptr(xg), _lib.ptr(Wg), _lib.ptr(bg), _lib.ptr(y), _lib.ptr(z), M, N, K, 1, _lib.stream_ptr())
    zd = x.double() @ W.double().t() + b.double()
    assert_close(z[:M], zd, "z", 2e-6)
    assert_close(y[:M], zd * torch.sigmoid(zd), "y", 2e-6)
    assert torch.isnan(y[M]).all() and torch.isnan(z[M]).all()


@pytest.mark.parametrize("n,E", [(40, 20000), (300, 45000), (7, 700), (5000, 60000)])
def test_job_table_replan_equals_fresh_plan_on_long_rows_with_repeats(n, E):
    """cgv_plan_jobs_build on rows long enough for the counting placement (>= 96 edges, partners from a range that fits
    the LDS histogram) -- random directed edges WITH repeated (dst, src) pairs, which the counting path orders by edge id
    -- and on rows / ranges that keep the comparison ranking: every array equals the freshly constructed plan's."""
    import ctypes as C
    from coarsegrainingvae_amd import _lib
    from coarsegrainingvae_amd.graph import PlanJob
    gen = torch.Generator().manual_seed(n + E)
    nbrs = torch.randint(0, n, (E, 2), generator=gen).to(DEV)
    fresh = EdgePlan.from_nbrs(nbrs, n)
    other = torch.randint(0, n, (E // 2, 2), generator=gen).to(DEV)
    held = EdgePlan.from_nbrs(other, n, capacity=E + 8)
    jobs = held.nbrs_jobs(nbrs)
    table = (PlanJob * len(jobs))(*jobs)
    _lib.call("cgv_plan_jobs_build", C.addressof(table), len(jobs), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert held.n_edges == E
    for f in ("rowptr_d", "rowptr_s"):
        assert torch.equal(getattr(held, f), getattr(fresh, f)), f
    for f in ("eid_d", "dst_d", "src_d", "eid_s", "dst_s", "src_s"):
        assert torch.equal(getattr(held, f)[:E], getattr(fresh, f)[:E]), f


# --------------------------------------------------------------------------- round-4 advisor findings
def test_device_noise_differs_between_ranks_and_repeats_within_one():
    """Data parallel: every rank seeds torch with 123 (run_ala.py:36-41); the device generator folds the rank in
    (ops.sample_seed), so the ranks' shards draw different eps (cgvae.py:445-449 on the concatenated batch) while one
    rank's stream is reproducible."""
    from coarsegrainingvae_amd import ops
    mu, sigma = torch.zeros(12, 64, device=DEV), torch.ones(12, 64, device=DEV)
    state0 = ops.get_sample_rng_state(DEV)
    try:
        torch.manual_seed(123)
        draws = {}
        for rank in (0, 1, 7, 0):
            ops.reseed_sample_rng(DEV, rank=rank)
            draws.setdefault(rank, []).append(ops.reparam_sample(mu, sigma).clone())
        assert torch.equal(draws[0][0], draws[0][1])
        for a, b in ((0, 1), (0, 7), (1, 7)):
            x, y = draws[a][0], draws[b][0]
            assert not torch.equal(x, y)
            assert float((x == y).float().mean()) < 0.01                  # not a shifted copy of the same block either
            assert abs(float(torch.corrcoef(torch.stack([x.flatten(), y.flatten()]))[0, 1])) < 0.15
    finally:
        ops.set_sample_rng_state(DEV, state0)


def test_layer_whose_output_leaves_the_loss_gets_a_zero_gradient_not_last_steps():
    """Arena-managed (direct-write) parameters get no zero fill at the start of a step.  When a Dense's output does not
    reach the loss (only its forked input alias does: primitives._LinearFn.backward with gy None) the arena slice must
    not keep the previous step's gradient -- torch would have materialised a zero (modules.py:103-114 under autograd)."""
    from coarsegrainingvae_amd.primitives import Dense, Swish
    from coarsegrainingvae_amd.trainer import ParamArena
    torch.manual_seed(0)
    lin = Dense(64, 64, bias=True, activation=Swish()).to(DEV)
    x = torch.randn(12, 64, device=DEV, requires_grad=True)
    y, alias = lin.forward_fork(x)
    (y.sum() + alias.sum()).backward()                                    # first backward: ordinary gradients exist
    arena = ParamArena([lin.weight, lin.bias])
    # step 1: both outputs used -> real gradient, written in place
    arena.zero_grad()
    y, alias = lin.forward_fork(x)
    (y * y).sum().add(alias.sum()).backward()
    assert arena.zero_unwritten() == 0
    g1 = lin.weight.grad.clone()
    assert float(g1.abs().max()) > 0
    # step 2: only the alias reaches the loss
    arena.zero_grad()
    y, alias = lin.forward_fork(x)
    alias.sum().backward()
    arena.zero_unwritten()
    assert float(lin.weight.grad.abs().max()) == 0.0 and float(lin.bias.grad.abs().max()) == 0.0
    # step 3: a layer no backward node reaches at all (module unused in this step): zero_unwritten fills it
    arena.zero_grad()
    lin.weight.grad.copy_(g1)
    assert arena.zero_unwritten() == 2
    assert float(lin.weight.grad.abs().max()) == 0.0


def test_quad_heads_equal_the_separate_heads():
    """Layer j of the prior's and the encoder's (mu, sigma) heads in one launch (cgv_multi_linear_fwd / _bwd_input) against
    the four heads applied one by one (cgvae.py:398-401, 500-503): outputs, input gradients and weight gradients."""
    from coarsegrainingvae_amd.primitives import (ACT_STD_ENC, ACT_STD_PRIOR, Linear, MLPHead, quad_heads)
    from torch import nn
    torch.manual_seed(3)
    F, n = 64, 12
    mk = lambda: MLPHead(Linear(F, F), nn.Tanh(), Linear(F, F)).to(DEV)
    heads = [mk() for _ in range(4)]
    xp = (0.3 * torch.randn(n, F, device=DEV)).requires_grad_()
    xe = (0.3 * torch.randn(n, F, device=DEV)).requires_grad_()
    up = [torch.randn(n, F, device=DEV) for _ in range(4)]
    out = quad_heads((heads[0], heads[1], xp, ACT_STD_PRIOR), (heads[2], heads[3], xe, ACT_STD_ENC))
    assert out is not None
    sum((o * u).sum() for o, u in zip(out, up)).backward()
    got = [o.detach().clone() for o in out] + [xp.grad.clone(), xe.grad.clone()]
    got_w = [p.grad.clone() for h in heads for p in h.parameters()]
    xp.grad = xe.grad = None
    for h in heads:
        h.zero_grad(set_to_none=True)
    # the same with torch ops in fp64
    ref_heads = [nn.Sequential(nn.Linear(F, F), nn.Tanh(), nn.Linear(F, F)).double().to(DEV) for _ in range(4)]
    for r, h in zip(ref_heads, heads):
        r.load_state_dict({k: v.double() for k, v in h.state_dict().items()})
    xpd, xed = xp.detach().double().requires_grad_(), xe.detach().double().requires_grad_()
    ref = [ref_heads[0](xpd), 1e-9 + torch.exp(ref_heads[1](xpd) / 2), ref_heads[2](xed), 1e-12 + torch.exp(ref_heads[3](xed) / 2)]
    sum((o * u.double()).sum() for o, u in zip(ref, up)).backward()
    want = [o.detach() for o in ref] + [xpd.grad, xed.grad]
    want_w = [p.grad for r in ref_heads for p in r.parameters()]
    for k, (a, b) in enumerate(zip(got, want)):
        assert_close(a, b, f"quad heads output / input gradient {k}", 1e-5)
    for k, (a, b) in enumerate(zip(got_w, want_w)):
        assert_close(a, b, f"quad heads parameter gradient {k}", 1e-5)


@pytest.mark.parametrize("n_frames,n_atoms,n_cgs,F,gamma,offset", [(2, 166, 6, 64, 50.0, True), (8, 22, 3, 32, 25.0, True),
                                                                     (1, 2000, 64, 64, 50.0, True), (1, 150, 2, 128, 0.0, True),
                                                                     (2, 40, 4, 16, 5.0, False)])
def test_fused_loss_tail_equals_reconstruct_plus_elbo(n_frames, n_atoms, n_cgs, F, gamma, offset):
    """cgv_loss_tail (decoder tail + ELBO + both backward tails, one launch) against the three launches it replaces
    (cgv_reconstruct_fwd, cgv_elbo_fwd, cgv_reconstruct_bwd: cgvae.py:462-481, scripts/utils.py:81-86, 117-141) and, through
    them, against the oracle's formulas: coordinates, the four scalars and every gradient."""
    from coarsegrainingvae_amd import ops
    gen = torch.Generator().manual_seed(n_atoms + F)
    N, nb = n_frames * n_atoms, n_frames * n_cgs
    per = [sorted(torch.randint(0, n_cgs, (n_atoms,), generator=gen).tolist()) for _ in range(n_frames)]
    for m in per:                                                     # every bead of a frame owns at least one atom
        for k in range(n_cgs):
            m[k] = k
        m.sort()
    mapping = torch.tensor([k + f * n_cgs for f, m in enumerate(per) for k in m])
    mapping = mapping[torch.randperm(N, generator=gen)] if n_atoms < 100 else mapping       # unsorted mappings too
    plan = EdgePlan.from_mapping(mapping.to(DEV), nb)
    if max(np.bincount(mapping.numpy(), minlength=nb)) > F:
        pytest.skip("a bead holds more atoms than channels")
    model = cg.CGequiVAE.__new__(cg.CGequiVAE)
    chan = cg.CGequiVAE.CG2ChannelIdx(model, mapping.to(DEV))
    bonds = torch.tensor([[a + f * n_atoms, a + 1 + f * n_atoms] for f in range(n_frames) for a in range(n_atoms - 1)] +
                         [[0, 0], [3, 1]]).to(DEV)
    mk = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=gen)).to(DEV)
    cg_xyz, xyz = mk(nb, 3, s=4.0), mk(N, 3, s=4.0)
    beta = 0.05
    results = []
    for lazy in (False, True):
        V = mk(nb, F, 3).requires_grad_()
        mu, pmu = mk(nb, F).requires_grad_(), mk(nb, F).requires_grad_()
        sigma, pstd = (0.5 + torch.rand(nb, F, generator=gen)).to(DEV).requires_grad_(), (0.5 + torch.rand(nb, F, generator=gen)).to(DEV).requires_grad_()
        gen.manual_seed(n_atoms + F + 1)                              # the same numbers in both passes
        if lazy is False:
            keep = [t.detach().clone() for t in (V, mu, pmu, sigma, pstd)]
        else:
            with torch.no_grad():
                for t, k in zip((V, mu, pmu, sigma, pstd), keep):
                    t.copy_(k)
        xr = ops.reconstruct(V, cg_xyz, chan, plan, offset, lazy=lazy)
        assert (getattr(xr, "_cgv_tail", None) is not None) == lazy
        loss, terms = ops.elbo_loss(mu, sigma, pmu, pstd, xyz, xr, bonds, beta, gamma)
        if lazy:
            assert xr._cgv_tail.filled
        (3.0 * loss).backward()                                       # (not the unit seed: the scale path too)
        results.append([xr.detach().clone(), terms.clone(), V.grad.clone(), mu.grad.clone(), sigma.grad.clone(), pmu.grad.clone(), pstd.grad.clone()])
    names = ["xyz_recon", "terms", "g_V", "g_mu", "g_sigma", "g_prior_mu", "g_prior_std"]
    for name, a, b in zip(names, results[1], results[0]):
        assert_close(a, b, f"fused loss tail: {name}", 2e-6)
    assert float(results[1][2].abs().max()) > 0


def test_lazy_reconstruct_is_materialised_when_no_loss_launch_fills_it():
    """A lazily reconstructed tensor that reaches the tensor-op loss (no prior net) or ``materialise_reconstruct`` is
    filled by the ordinary tail launch (cgvae.py:462-481)."""
    from coarsegrainingvae_amd import ops
    torch.manual_seed(0)
    mapping = torch.tensor([0, 0, 1, 1, 1, 2, 2, 0]).to(DEV)
    plan = EdgePlan.from_mapping(mapping, 3)
    model = cg.CGequiVAE.__new__(cg.CGequiVAE)
    chan = cg.CGequiVAE.CG2ChannelIdx(model, mapping)
    V = torch.randn(3, 8, 3, device=DEV, requires_grad=True)
    cgx = torch.randn(3, 3, device=DEV)
    ref = ops.reconstruct(V, cgx, chan, plan, True)
    lazy = ops.reconstruct(V, cgx, chan, plan, True, lazy=True)
    assert not lazy._cgv_tail.filled
    ops.materialise_reconstruct(lazy)
    assert torch.equal(lazy, ref)
    lazy.sum().backward()                                             # the ordinary backward launch (no slot gradient)
    g = V.grad.clone()
    V.grad = None
    ref.sum().backward()
    assert torch.equal(g, V.grad)


@pytest.mark.parametrize("shape", [(332, 1800, 600, 1), (704, 1800, 600, 1), (704, 600, 600, 1), (332, 600, 600, 0), (333, 1796, 596, 2),
                                   (96, 5400, 600, 0), (288, 1200, 600, 1), (50, 36, 20, 1), (17, 100, 8, 0), (1000, 340, 1200, 1)])
def test_tile_forward_one_register_tile_per_cu_vs_fp64(shape, options):
    """tile_fwd_bal_k (option tile_fwd_bal: one (16 MT) x (16 NT) register tile per CU, reduction split over 8 waves with a
    two-round LDS sum, XCD-aware tile order): Dense forward modules.py:103-114 on the atom-level and ragged shapes, bias +
    activation epilogue, pre-activation output, rows / columns / reduction tails that do not fill a tile."""
    options.set("tile_fwd_bal", 2)
    M, N, K, act = shape
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    y = torch.full((M, N), float("nan"), device=DEV)
    z = torch.full((M, N), float("nan"), device=DEV)
    cg._lib.call("cgv_tile_linear_fwd", cg._lib.ptr(x), cg._lib.ptr(W), cg._lib.ptr(b), cg._lib.ptr(y), cg._lib.ptr(z), M, N, K, act,
                 cg._lib.stream_ptr())
    zr = x.double() @ W.double().T + b.double()
    yr = {0: zr, 1: zr * torch.sigmoid(zr), 2: torch.tanh(zr)}[act]
    assert torch.allclose(y.double(), yr, rtol=1e-5, atol=1e-5)
    if act:
        assert torch.allclose(z.double(), zr, rtol=1e-5, atol=1e-5)


def test_dense_has_no_library_or_cpu_fallback():
    """no product of the path runs on a library GEMM or on a CPU branch -- CPU tensors raise (modules.py:103-114
    is replaced, not shadowed).  Widths that are not multiples of 4 no longer raise: see the next test."""
    cpu = cg.Dense(32, 32, activation=cg.Swish())
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        cpu(torch.randn(4, 32))
    from coarsegrainingvae_amd.primitives import Linear, gemm_mode_or_none
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        Linear(32, 32)(torch.randn(4, 32))
    # the dispatch predicate never raises (it used to, and took the pair / fusion selection down with it)
    w = torch.randn(30, 30, device=DEV)
    assert gemm_mode_or_none(torch.randn(12, 30, device=DEV), w, None)[0] is None
    assert gemm_mode_or_none(torch.randn(0, 32, device=DEV), torch.randn(32, 32, device=DEV), None) == (None, "Dense / Linear on an input without rows (0 x 32)")
    assert gemm_mode_or_none(torch.randn(12, 32), torch.randn(32, 32), None)[0] is None


@pytest.mark.parametrize("M,K,N,act", [(12, 30, 30, "swish"), (332, 600, 30, None), (96, 30, 90, "swish"), (704, 30, 62, None), (5, 7, 3, None)])
def test_dense_pads_widths_that_are_not_multiples_of_four(M, K, N, act):
    """The reference takes any -n_basis (run_ala.py:419-461); the kernels take widths that are multiples of 4.  Dense /
    Linear zero-pad the others (primitives.linear_fn) and slice the result: output, input gradient, weight and bias
    gradients against fp64 (modules.py:103-114)."""
    torch.manual_seed(M + K + N)
    layer = cg.Dense(K, N, activation=cg.Swish() if act else None).to(DEV)
    layer.bias.data.normal_()
    x = torch.randn(M, K, device=DEV, requires_grad=True)
    gy = torch.randn(M, N, device=DEV)
    y = layer(x)
    assert y.shape == (M, N)
    y.backward(gy)
    x64 = x.detach().double().requires_grad_(True)
    W64, b64 = layer.weight.detach().double().requires_grad_(True), layer.bias.detach().double().requires_grad_(True)
    z64 = x64 @ W64.t() + b64
    y64 = z64 * torch.sigmoid(z64) if act else z64
    y64.backward(gy.double())
    assert_close(y, y64, "y")
    assert_close(x.grad, x64.grad, "grad x")
    assert_close(layer.weight.grad, W64.grad, "grad W")
    assert_close(layer.bias.grad, b64.grad, "grad b")


def test_trainer_step_at_n_basis_30_vs_oracle():
    """`-n_basis 30` (a width the reference accepts and the kernels do not take directly): two Trainer steps of the
    dipeptide model -- forward, ELBO, every live gradient of the first step, norm, clip, and the outputs behind the first
    Adam update -- against the oracle's reference-style step (cgvae.py:486-513, scripts/utils.py:117-157)."""
    from coarsegrainingvae_amd.trainer import Trainer
    from test_full_size_parity import OracleTraining, _check_outputs, _check_norm_and_clip, _oracle_forward_on, _setup, _snapshot
    F = 30
    w, batch, cpu_batch, model, hp, P = _setup("dipeptide", 4, F, enc=2, dec=2)
    oracle = OracleTraining(cpu_batch, P, hp, w, 1e-4)
    tr = Trainer(model, lr=1e-4, beta=w["beta"], gamma=w["gamma"])
    gen = torch.Generator().manual_seed(3)
    for step in (1, 2):
        eps = torch.randn(cpu_batch["CG_nxyz"].shape[0], F, generator=gen)
        ref = oracle.step(eps)
        snap = _snapshot(model)
        tr.step(batch, eps=eps.to(DEV))
        _check_outputs(tr, ref, f"n_basis 30, step {step}", updates=step - 1, own=_oracle_forward_on(snap, cpu_batch, hp, eps))
        _check_norm_and_clip(tr, ref, f"n_basis 30, step {step}")
        if step == 1:
            n_live = 0
            for name, p in model.named_parameters():
                g0 = ref["grads"].get(name)
                if g0 is not None and float(g0.abs().max()) > 0.0:
                    n_live += 1
                    assert_close(p.grad, g0, "grad " + name)
            assert n_live > 50
    assert tr.skipped_steps() == 0


@pytest.mark.parametrize("n_beads,F,R,layers,with_dv", [(12, 600, 10, 2, True), (3, 64, 8, 3, True), (16, 48, 10, 1, True), (12, 128, 8, 2, False)])
def test_fused_prior_loop_equals_per_block_path(n_beads, F, R, layers, with_dv, options):
    """prior_fused (the prior's EquiMessageBlock loop, cgvae.py:381-396 / conv.py:505-563, as one autograd node on the
    channel-group kernels) against the per-block path it replaces: the scalar state, the input gradient and every
    parameter gradient -- incl. the explicit zeros of the two dead filter slices."""
    from coarsegrainingvae_amd import prior_fused
    from coarsegrainingvae_amd.model import CGprior
    from coarsegrainingvae_amd.trainer import ParamArena
    gen = torch.Generator().manual_seed(n_beads + F)
    xyz = torch.rand(n_beads, 3, generator=gen) * 6.0
    nbrs, _ = O.make_directed(O.get_neighbor_list(xyz, 25.0, True))
    if nbrs.shape[0] == 0:
        pytest.skip("no edges")
    torch.manual_seed(5)
    prior = CGprior(n_conv=layers, n_atom_basis=F, n_rbf=R, activation="swish", cutoff=9.5).to(DEV)
    prior.set_skip_dead_vector_channel(not with_dv)
    plan = EdgePlan.from_nbrs(nbrs.to(DEV), n_beads)
    geom = EdgeGeometry(plan, R, 9.5, pos_dst=xyz.to(DEV), pos_src=xyz.to(DEV))
    cg_z = torch.arange(n_beads).float().to(DEV) % 6
    up = torch.randn(n_beads, F, generator=gen).to(DEV)
    params = [p for blk in prior.message_blocks for p in blk.inv_message.parameters() if "dist_filter" not in ""]
    live = [p for p in prior_fused.layer_params(prior)] + [prior.atom_embed.weight]

    def run(fused):
        options.set("fused_prior", int(fused))
        calls0 = prior_fused.calls
        h = prior.features(cg_z, nbrs.to(DEV), plan, geom)
        assert (prior_fused.calls > calls0) == fused
        (h * up).sum().backward()
        return h.detach().clone(), [p.grad.clone() for p in live]
    # first backward builds plain gradients; then an arena makes the parameters direct-write (the fused path's condition)
    run(False)
    arena = ParamArena(live)
    arena.g.fill_(float("nan"))
    arena.zero_grad()
    h0, g0 = run(False)
    arena.g.fill_(float("nan"))
    arena.zero_grad()
    h1, g1 = run(True)
    assert_close(h1, h0, "prior state", 2e-6)
    for k, (a, b) in enumerate(zip(g1, g0)):
        assert bool(torch.isfinite(a).all()), f"parameter gradient {k} has unwritten entries"
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, f"parameter gradient {k} must be exactly zero"
        else:
            assert_close(a, b, f"prior parameter gradient {k}", 2e-5)


@pytest.mark.parametrize("queued", [False, True])
@pytest.mark.parametrize("workload,F,frames", [("chignolin", 64, 1), ("dipeptide", 32, 5)])
def test_bead_mean_inside_the_contractive_block_equals_separate_launches(workload, F, frames, queued, options):
    """Encoder layer 0 (cgvae.py:297-305): H, V = scatter_mean(h), scatter_mean(v) from ONE launch, whose gradient reaches h
    through the store epilogue of the contractive block's first Dense (csrc/tile_gemm.hip BcastAdd) -- against the path it
    replaces (two reductions, a broadcast launch, an accumulation add).  ``queued``: under the trainer's arena + weight
    gradient queue (the fused epilogue) or plain autograd (the slot's ordinary broadcast)."""
    from coarsegrainingvae_amd import ops
    from coarsegrainingvae_amd.primitives import wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    w = cg.data.WORKLOADS[workload]
    torch.manual_seed(17)
    enc = cg.EquiEncoder(n_conv=2, n_atom_basis=F, n_rbf=w["n_rbf"], activation="swish", cutoff=w["cg_cutoff"], dir_mp=False,
                         cg_mp=False).to(DEV)
    batch = cg.synthetic_batch(workload, n_frames=frames, seed=4, device=DEV)
    g = batch["_graph"]
    gen = torch.Generator().manual_seed(1)
    uH = torch.randn(g.a2b.n_dst, F, generator=gen).to(DEV)
    uh = torch.randn(batch["nxyz"].shape[0], F, generator=gen).to(DEV)
    params = [p for p in enc.parameters()]
    calls = []
    real = ops._lib.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    def run(fused):
        options.set("fused_bead_mean", int(fused))
        del calls[:]
        ops._lib.call = spy
        try:
            ctx = wgrad_queue.collect() if queued else contextlib.nullcontext()
            with ctx:
                H, h = enc(batch["nxyz"][:, 0], batch["nxyz"][:, 1:], batch["CG_nxyz"][:, 1:], batch["CG_mapping"],
                           batch["nbr_list"], batch["CG_nbr_list"], graph=g)
                ((H * uH).sum() + (h * uh).sum()).backward()
            if queued:
                wgrad_queue.flush()
        finally:
            ops._lib.call = real
        return H.detach().clone(), h.detach().clone(), [None if p.grad is None else p.grad.clone() for p in params], list(calls)
    run(False)
    arena = None
    if queued:
        live = [p for p in params if p.grad is not None]
        arena = ParamArena(live)
    outs = []
    for fused in (False, True):
        if arena is not None:
            arena.g.fill_(float("nan"))
            arena.zero_grad()
        else:
            for p in params:
                p.grad = None
        outs.append(run(fused))
    (H0, h0, g0, c0), (H1, h1, g1, c1) = outs
    assert "cgv_segment_reduce2" in c1 and "cgv_segment_reduce2" not in c0
    assert c1.count("cgv_segment_broadcast") == (0 if queued else 1) and c0.count("cgv_segment_broadcast") == 1
    if queued:                  # the parked gradient rode a backward-input epilogue (pair launches: the two-source product)
        assert "cgv_tile_linear_bwd_input_act_add_bcast" in c1 or "cgv_tile_linear_bwd_input_sum2" in c1
    assert torch.equal(H1, H0) and torch.equal(h1, h0)            # same per-segment order: bit-identical forward
    n_live = 0
    for k, (a, b) in enumerate(zip(g1, g0)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), f"parameter gradient {k} has unwritten entries"
        assert_close(a, b, f"encoder parameter gradient {k}", 2e-6)
        n_live += float(b.abs().max()) > 0
    assert n_live >= 10


@pytest.mark.parametrize("M,N,K,act", [(332, 600, 600, 1), (704, 1800, 600, 1), (129, 132, 260, 0), (2000, 64, 600, 1), (161, 600, 36, 0)])
def test_split_bf16_weight_gradients_have_fp32_accuracy(M, N, K, act, options):
    """Weight gradients of layers with more than 128 operand rows (autograd of nn.Linear / Dense, modules.py; conv.py:505-563)
    on the bf16 matrix path with SPLIT operands (csrc/wgrad_gathered.hip wgrad_split128_k: three bf16 terms per fp32 value,
    six products, fp32 accumulation) against fp64 -- and against the fp32 MFMA tiles: the error has to be of the same class
    (north_star's tolerance is 1e-4; fp32 kernels sit at 1e-7).  Operands span 12 orders of magnitude (gradients are tiny,
    activations are not): bf16 keeps the fp32 exponent range, nothing is scaled.  Write and accumulate."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    gen = torch.Generator().manual_seed(M + N + K)
    scale_rows = torch.logspace(-9, 0, M).unsqueeze(1)                      # per-row gradient magnitudes 1e-9 .. 1
    gy = (torch.randn(M, N, generator=gen) * scale_rows).to(DEV)
    x = (torch.randn(M, K, generator=gen) * torch.logspace(-3, 2, K).unsqueeze(0)).to(DEV)
    z = torch.randn(M, N, generator=gen).to(DEV) if act else None
    g64 = gy.double().cpu()
    if act:
        s = torch.sigmoid(z.double().cpu())
        g64 = g64 * (s * (1 + z.double().cpu() * (1 - s)))
    ref_W, ref_b = g64.t() @ x.double().cpu(), g64.sum(0)
    q = WeightGradQueue()
    errs = {}
    for split in (0, 1):
        options.set("wgrad_split", split)
        gW, gb = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        q.launch([(gy, x, z, act, gW, gb, False)])
        q.launch([(gy, x, z, act, gW, gb, True)])                            # accumulate: twice the gradient
        # column-wise norm-relative error: every column of gW has its own magnitude (x's columns span 5 orders)
        eW = ((gW.double().cpu() - 2 * ref_W).abs().amax(0) / (2 * ref_W).abs().amax(0)).max()
        eb = (gb.double().cpu() - 2 * ref_b).abs().max() / (2 * ref_b).abs().max()
        errs[split] = (float(eW), float(eb))
    assert errs[1][0] < 2e-6 and errs[1][1] < 2e-6, errs
    assert errs[1][0] < 4 * errs[0][0] + 1e-7, f"split path is not in the fp32 error class: {errs}"


@pytest.mark.parametrize("workload,F,frames,layers", [("chignolin", 64, 2, 2), ("dipeptide", 32, 12, 4), ("chignolin", 600, 2, 3)])
def test_encoder_node_mlps_as_pair_launches_equal_the_layer_by_layer_path(workload, F, frames, layers, options):
    """Contractive block i and message block i + 1 read the same atom state (cgvae.py:286-305): their node MLPs run as pair
    launches of the tile kernels (primitives._TilePairFn: one forward launch per MLP layer, one backward-input launch for the
    two second layers, the first layers' input gradients chained through the epilogues together with the parked bead-mean
    gradient of layer 0).  Against the layer-by-layer path under the trainer's arena + queue: outputs bit for bit (the same
    kernels compute them), every parameter gradient to 2e-6."""
    from coarsegrainingvae_amd import ops
    from coarsegrainingvae_amd.primitives import wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    w = cg.data.WORKLOADS[workload]
    torch.manual_seed(29)
    enc = cg.EquiEncoder(n_conv=layers, n_atom_basis=F, n_rbf=w["n_rbf"], activation="swish", cutoff=w["cg_cutoff"], dir_mp=False,
                         cg_mp=False).to(DEV)
    batch = cg.synthetic_batch(workload, n_frames=frames, seed=5, device=DEV)
    g = batch["_graph"]
    gen = torch.Generator().manual_seed(2)
    uH = torch.randn(g.a2b.n_dst, F, generator=gen).to(DEV)
    uh = torch.randn(batch["nxyz"].shape[0], F, generator=gen).to(DEV)
    params = [p for p in enc.parameters()]
    calls = []
    real = ops._lib.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    def run(pairs):
        options.set("encoder_pairs", int(pairs))
        del calls[:]
        ops._lib.call = spy
        try:
            with wgrad_queue.collect():
                H, h = enc(batch["nxyz"][:, 0], batch["nxyz"][:, 1:], batch["CG_nxyz"][:, 1:], batch["CG_mapping"],
                           batch["nbr_list"], batch["CG_nbr_list"], graph=g)
                ((H * uH).sum() + (h * uh).sum()).backward()
            wgrad_queue.flush()
        finally:
            ops._lib.call = real
        return H.detach().clone(), h.detach().clone(), [None if p.grad is None else p.grad.clone() for p in params], list(calls)
    run(False)
    arena = ParamArena([p for p in params if p.grad is not None])
    outs = []
    for pairs in (False, True):
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        outs.append(run(pairs))
    (H0, h0, g0, c0), (H1, h1, g1, c1) = outs
    n_pairs = layers - 1
    assert c1.count("cgv_tile_pair_linear_fwd") == 2 * n_pairs and "cgv_tile_pair_linear_fwd" not in c0
    # (with act_downstream the second layers' launch is the _out form: Swish' of the first layers in its store epilogue)
    assert c1.count("cgv_tile_pair_linear_bwd_input") + c1.count("cgv_tile_pair_linear_bwd_input_out") == n_pairs
    assert c1.count("cgv_tile_pair_linear_bwd_input_out") == n_pairs
    assert len(c1) == len(c0) - 4 * n_pairs, (len(c0), len(c1))                  # two forward launches and two backward launches per pair
    assert "cgv_segment_broadcast" not in c1                                      # the bead-mean gradient still rides an epilogue
    assert torch.equal(H1, H0) and torch.equal(h1, h0)
    for k, (a, b) in enumerate(zip(g1, g0)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), f"parameter gradient {k} has unwritten entries"
        assert_close(a, b, f"encoder parameter gradient {k}", 2e-6)


@pytest.mark.parametrize("M,act", [(96, "tanh"), (288, "relu"), (65, "tanh")])
def test_head_layers_as_tile_pair_launches_vs_fp64(M, act, options):
    """The (mu, sigma) heads (cgvae.py:366-371 applied at 398-401 / 500-503) on more bead rows than the skinny pair kernels
    take: layer j of both heads as ONE launch of the tile kernels (different activation codes per problem: the sigma head
    ends in c + exp(z / 2)), backward-input of the second layers as one launch, the shared input's gradients chained
    through the first layers' epilogues.  Against fp64 autograd and against the one-by-one path."""
    from coarsegrainingvae_amd.primitives import ACT_STD_ENC, MLPHead, Linear, dual_heads, wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    from coarsegrainingvae_amd import ops
    F = 600
    torch.manual_seed(M)
    mk = lambda: MLPHead(Linear(F, F), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU(), Linear(F, F)).to(DEV)
    mu, sg = mk(), mk()
    x0 = torch.randn(M, F, device=DEV)
    ua, ub = torch.randn(M, F, device=DEV), torch.randn(M, F, device=DEV) * 0.1
    params = list(mu.parameters()) + list(sg.parameters())
    calls = []
    real = ops._lib.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    def run(pairs):
        options.set("head_pairs", int(pairs))
        del calls[:]
        x = x0.clone().requires_grad_(True)
        ops._lib.call = spy
        try:
            with wgrad_queue.collect():
                ya, yb = dual_heads(mu, sg, x, out_act_b=ACT_STD_ENC)
                ((ya * ua).sum() + (yb * ub).sum()).backward()
            wgrad_queue.flush()
        finally:
            ops._lib.call = real
        return ya.detach().clone(), yb.detach().clone(), x.grad.clone(), [p.grad.clone() for p in params], list(calls)
    run(False)
    arena = ParamArena(params)
    res = []
    for pairs in (False, True):
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        res.append(run(pairs))
    (ya0, yb0, gx0, gp0, c0), (ya1, yb1, gx1, gp1, c1) = res
    assert c1.count("cgv_tile_pair_linear_fwd") == 2 and c1.count("cgv_tile_pair_linear_bwd_input") == 1 and len(c1) == len(c0) - 4
    assert torch.equal(ya1, ya0) and torch.equal(yb1, yb0)
    # fp64 reference
    d = lambda t: t.detach().double().cpu()
    xd = d(x0).requires_grad_(True)
    P = [d(p).requires_grad_(True) for p in params]
    f = torch.tanh if act == "tanh" else torch.relu
    ya64 = f(xd @ P[0].t() + P[1]) @ P[2].t() + P[3]
    yb64 = 1e-12 + torch.exp((f(xd @ P[4].t() + P[5]) @ P[6].t() + P[7]) / 2)
    ((ya64 * d(ua)).sum() + (yb64 * d(ub)).sum()).backward()
    assert_close(ya1, ya64.detach(), "mu head", 2e-6)
    assert_close(yb1, yb64.detach(), "sigma head", 2e-6)
    assert_close(gx1, xd.grad, "grad x", 5e-6)
    assert_close(gx1, gx0, "grad x vs one-by-one", 2e-6)
    for k, (a, b) in enumerate(zip(gp1, P)):
        assert_close(a, b.grad, f"parameter gradient {k}", 5e-6)


def test_paired_embedding_lookups_and_their_weight_gradients():
    """ops.embedding2: the encoder's atom-type and the prior's bead-type lookups (cgvae.py:268 / 381) from one launch, their
    weight gradients from one launch -- bit for bit what two ops.embedding calls give (incl. the exact zero row of padding_idx)."""
    from coarsegrainingvae_amd import ops
    torch.manual_seed(4)
    F = 64
    ea, eb = torch.nn.Embedding(100, F, padding_idx=0).to(DEV), torch.nn.Embedding(100, F, padding_idx=0).to(DEV)
    ia = torch.cat([torch.zeros(5), torch.randint(1, 9, (300,)).float()])[torch.randperm(305)].to(DEV)
    ib = torch.randint(0, 7, (24,)).float().to(DEV)
    nx_a, nx_b = torch.zeros(305, 4, device=DEV), torch.zeros(24, 4, device=DEV)     # ids as a strided column, as in a batch
    nx_a[:, 0], nx_b[:, 0] = ia, ib
    ua, ub = torch.randn(305, F, device=DEV), torch.randn(24, F, device=DEV)
    pa, pb = ops.embedding_plan(nx_a[:, 0], 100, 0), ops.embedding_plan(nx_b[:, 0], 100, 0)
    oa, ob = ops.embedding2(ea, nx_a[:, 0], pa, eb, nx_b[:, 0], pb)
    ((oa * ua).sum() + (ob * ub).sum()).backward()
    ga, gb = ea.weight.grad.clone(), eb.weight.grad.clone()
    ea.weight.grad = eb.weight.grad = None
    ra, rb = ops.embedding(ea, nx_a[:, 0], pa), ops.embedding(eb, nx_b[:, 0], pb)
    ((ra * ua).sum() + (rb * ub).sum()).backward()
    assert torch.equal(oa, ra) and torch.equal(ob, rb)
    assert torch.equal(ga, ea.weight.grad) and torch.equal(gb, eb.weight.grad)
    assert float(ga[0].abs().max()) == 0.0 and float(ga.abs().max()) > 0


@pytest.mark.parametrize("M,N,K", [(70, 52, 36), (129, 132, 260), (332, 1800, 600), (33, 1200, 64)])
def test_tile_pair_entry_points_on_ragged_shapes_vs_fp64(M, N, K):
    """The C-ABI pair launches of the tile kernels called directly (cgv_tile_pair_linear_fwd, cgv_tile_pair_linear_bwd_input,
    cgv_tile_linear_bwd_input_sum2): row / column counts that are no multiples of the 16 / 32 / 64-wide tiles, a different
    activation code per problem, NULL and non-NULL `add`, with and without a per-segment gradient -- against fp64."""
    L = cg._lib
    assert L.load().cgv_tile_pair_supported(M, N, K)           # every tile-supported shape (staged kernels: two launches inside the call)
    gen = torch.Generator().manual_seed(M * 7 + N)
    mk = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    xa, xb, Wa, Wb, ba, bb = mk(M, K), mk(M, K), mk(N, K) * 0.1, mk(N, K) * 0.1, mk(N), mk(N)
    ya, yb, za, zb = (torch.full((M, N), float("nan"), device=DEV) for _ in range(4))
    st = L.stream_ptr()
    L.call("cgv_tile_pair_linear_fwd", L.ptr(xa), L.ptr(Wa), L.ptr(ba), L.ptr(ya), L.ptr(za), L.ptr(xb), L.ptr(Wb), L.ptr(bb), L.ptr(yb),
           L.ptr(zb), M, N, K, 1, 2, st)                                     # swish / tanh
    d = lambda t: t.double().cpu()
    za64, zb64 = d(xa) @ d(Wa).t() + d(ba), d(xb) @ d(Wb).t() + d(bb)
    assert_close(za, za64, "z_a", 2e-6)
    assert_close(ya, za64 * torch.sigmoid(za64), "y_a", 5e-6)
    assert_close(yb, torch.tanh(zb64), "y_b", 5e-6)               # (the fp32 tanh itself is good to a few ulp)
    # backward-input of both (different outputs), one with an `add`
    ga, gb, add_b = mk(M, N), mk(M, N), mk(M, K)
    gxa, gxb = torch.full((M, K), float("nan"), device=DEV), torch.full((M, K), float("nan"), device=DEV)
    L.call("cgv_tile_pair_linear_bwd_input", L.ptr(ga), L.ptr(za), L.ptr(Wa), None, L.ptr(gxa), L.ptr(gb), L.ptr(zb), L.ptr(Wb), L.ptr(add_b),
           L.ptr(gxb), M, N, K, 1, 2, st)
    s = torch.sigmoid(za64)
    da = d(ga) * (s * (1 + za64 * (1 - s)))
    db = d(gb) * (1 - torch.tanh(zb64) ** 2)
    assert_close(gxa, da @ d(Wa), "gx_a", 5e-6)
    assert_close(gxb, db @ d(Wb) + d(add_b), "gx_b", 5e-6)
    # both sources into ONE output, + add, + a gradient held per segment of the rows (mean)
    n_seg = 5
    mapping = (torch.arange(M) % n_seg).to(DEV)
    plan = EdgePlan.from_mapping(mapping, n_seg)
    seg = mk(n_seg, K)
    for with_seg in (False, True):
        gx = torch.full((M, K), float("nan"), device=DEV)
        L.call("cgv_tile_linear_bwd_input_sum2", L.ptr(ga), L.ptr(za), L.ptr(Wa), L.ptr(gb), L.ptr(zb), L.ptr(Wb), L.ptr(add_b),
               L.ptr(seg) if with_seg else None, L.ptr(mapping) if with_seg else None, L.ptr(plan.rowptr_d) if with_seg else None, 1,
               L.ptr(gx), M, N, K, 1, 2, st)
        ref = da @ d(Wa) + db @ d(Wb) + d(add_b)
        if with_seg:
            counts = torch.bincount(mapping.cpu(), minlength=n_seg).clamp_min(1).double()
            ref = ref + (d(seg) / counts.unsqueeze(1))[mapping.cpu()]
        assert_close(gx, ref, f"sum2 (segment gradient: {with_seg})", 5e-6)


@pytest.mark.parametrize("M,N,K", [(2000, 600, 1800), (704, 1800, 600), (129, 132, 260), (333, 604, 36), (1537, 68, 1204)])
@pytest.mark.parametrize("streamk", [2, 3, 37])
def test_stream_k_gemm_every_entry_point_vs_fp64(M, N, K, streamk, options):
    """csrc/streamk_gemm.hip forced onto every tile entry point (``streamk`` = 2: one block per CU, 3: two, 37: a grid of 37
    blocks -- ranges that cut tiles anywhere, some tiles shared by many blocks): forward with bias / Swish / z output, single
    and pair; backward-input plain, + add, + per-segment gradient, times the downstream activation derivative, pair, and
    the two-source product -- ragged row / column / reduction counts (no multiples of the 128 x 128 x 32 units; modules.py:
    103-114 and its autograd) against fp64, and bit-identical over repeated launches (parts are summed in range order,
    whoever arrives last)."""
    L = cg._lib
    options.set("streamk", streamk)
    gen = torch.Generator().manual_seed(M * 3 + N + K)
    mk = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    d = lambda t: t.double().cpu()
    st = L.stream_ptr()
    xa, xb, Wa, Wb, ba, bb = mk(M, K), mk(M, K), mk(N, K) * 0.1, mk(N, K) * 0.1, mk(N), mk(N)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    # forward, single (Swish, z kept) and without bias / activation
    y, z = nan(M, N), nan(M, N)
    L.call("cgv_tile_linear_fwd", L.ptr(xa), L.ptr(Wa), L.ptr(ba), L.ptr(y), L.ptr(z), M, N, K, 1, st)
    za64 = d(xa) @ d(Wa).t() + d(ba)
    assert_close(z, za64, "z", 2e-6)
    assert_close(y, za64 * torch.sigmoid(za64), "y", 5e-6)
    y_again = nan(M, N)
    L.call("cgv_tile_linear_fwd", L.ptr(xa), L.ptr(Wa), L.ptr(ba), L.ptr(y_again), L.ptr(z), M, N, K, 1, st)
    assert torch.equal(y, y_again)                           # deterministic
    y0 = nan(M, N)
    L.call("cgv_tile_linear_fwd", L.ptr(xa), L.ptr(Wa), None, L.ptr(y0), None, M, N, K, 0, st)
    assert_close(y0, d(xa) @ d(Wa).t(), "y, no bias / activation", 2e-6)
    # forward pair: swish / tanh
    ya, yb, za, zb = nan(M, N), nan(M, N), nan(M, N), nan(M, N)
    L.call("cgv_tile_pair_linear_fwd", L.ptr(xa), L.ptr(Wa), L.ptr(ba), L.ptr(ya), L.ptr(za), L.ptr(xb), L.ptr(Wb), L.ptr(bb), L.ptr(yb),
           L.ptr(zb), M, N, K, 1, 2, st)
    zb64 = d(xb) @ d(Wb).t() + d(bb)
    assert_close(ya, za64 * torch.sigmoid(za64), "pair y_a", 5e-6)
    assert_close(zb, zb64, "pair z_b", 2e-6)
    # (|z| reaches ~20 at K = 1800: z's own 2e-6 of its maximum is 4e-5 absolute where tanh' is ~1)
    assert_close(yb, torch.tanh(zb64), "pair y_b", 5e-5)
    # backward-input: plain, + add, * act'(z_out), + per-segment gradient
    ga, gb, add, zo = mk(M, N), mk(M, N), mk(M, K), mk(M, K)
    gx = nan(M, K)
    L.call("cgv_tile_linear_bwd_input", L.ptr(ga), L.ptr(Wa), L.ptr(gx), M, N, K, st)
    assert_close(gx, d(ga) @ d(Wa), "gx", 5e-6)
    gx2 = nan(M, K)
    L.call("cgv_tile_linear_bwd_input", L.ptr(ga), L.ptr(Wa), L.ptr(gx2), M, N, K, st)
    assert torch.equal(gx, gx2)
    L.call("cgv_tile_linear_bwd_input_out", L.ptr(ga), None, L.ptr(Wa), L.ptr(add), L.ptr(gx), M, N, K, 0, L.ptr(zo), 1, st)
    s = torch.sigmoid(d(zo))
    assert_close(gx, (d(ga) @ d(Wa) + d(add)) * (s * (1 + d(zo) * (1 - s))), "gx + add, times Swish'(z_out)", 5e-6)
    n_seg = 7
    mapping = (torch.arange(M) % n_seg).to(DEV)
    plan = EdgePlan.from_mapping(mapping, n_seg)
    seg = mk(n_seg, K)
    counts = torch.bincount(mapping.cpu(), minlength=n_seg).clamp_min(1).double()
    L.call("cgv_tile_linear_bwd_input_act_add_bcast", L.ptr(ga), None, L.ptr(Wa), L.ptr(add), L.ptr(seg), L.ptr(mapping), L.ptr(plan.rowptr_d), 1,
           L.ptr(gx), M, N, K, 0, st)
    assert_close(gx, d(ga) @ d(Wa) + d(add) + (d(seg) / counts.unsqueeze(1))[mapping.cpu()], "gx + add + segment mean", 5e-6)
    # pair, and both sources into one output
    gxa, gxb = nan(M, K), nan(M, K)
    L.call("cgv_tile_pair_linear_bwd_input", L.ptr(ga), None, L.ptr(Wa), None, L.ptr(gxa), L.ptr(gb), None, L.ptr(Wb), L.ptr(add),
           L.ptr(gxb), M, N, K, 0, 0, st)
    assert_close(gxa, d(ga) @ d(Wa), "pair gx_a", 5e-6)
    assert_close(gxb, d(gb) @ d(Wb) + d(add), "pair gx_b", 5e-6)
    for with_seg in (False, True):
        L.call("cgv_tile_linear_bwd_input_sum2", L.ptr(ga), None, L.ptr(Wa), L.ptr(gb), None, L.ptr(Wb), L.ptr(add),
               L.ptr(seg) if with_seg else None, L.ptr(mapping) if with_seg else None, L.ptr(plan.rowptr_d) if with_seg else None, 1,
               L.ptr(gx), M, N, K, 0, 0, st)
        ref = d(ga) @ d(Wa) + d(gb) @ d(Wb) + d(add)
        if with_seg:
            ref = ref + (d(seg) / counts.unsqueeze(1))[mapping.cpu()]
        assert_close(gx, ref, f"two sources (segment gradient: {with_seg})", 5e-6)
    # the tickets are back at zero (the split reduction of tile_bwd_input_k shares them)
    ws = L._SPLIT_WS[(torch.cuda.current_device(), int(torch.cuda.current_stream().cuda_stream))]
    torch.cuda.synchronize()
    assert int(ws[: 64 * 1024].view(torch.int32).abs().max()) == 0


def test_stream_k_default_dispatch_takes_the_many_row_long_reduction_products(options):
    """The default rule (CGV_OPT_STREAMK = 0): a single 2000 x 1800 -> 600 backward-input product runs on the stream-K
    kernel, the 704-row products and every pair launch on the register tiles -- the same numbers either way (fp64)."""
    L = cg._lib
    gen = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    for M, N, K in ((2000, 1800, 600), (704, 1800, 600)):
        g, W = mk(M, N), mk(N, K) * 0.1
        out = {}
        for opt in (0, 1, 2):
            options.set("streamk", opt)
            gx = torch.empty(M, K, device=DEV)
            L.call("cgv_tile_linear_bwd_input", L.ptr(g), L.ptr(W), L.ptr(gx), M, N, K, L.stream_ptr())
            assert_close(gx, g.double().cpu() @ W.double().cpu(), f"{M} rows, streamk {opt}", 5e-6)
            out[opt] = gx
        same_as_sk = torch.equal(out[0], out[2])
        assert same_as_sk == (M >= 1536), (M, same_as_sk)    # (the two kernels sum in different orders: bit-equality names the kernel)


@pytest.mark.parametrize("M,N,K,act", [(96, 600, 600, 1), (64, 5400, 600, 1), (33, 132, 260, 0), (96, 68, 1204, 2), (48, 600, 36, 0), (80, 1800, 600, 1)])
def test_strip_layout_with_split_operands_has_fp32_accuracy(M, N, K, act, options):
    """Weight gradients of layers with 33 .. 96 operand rows (the bead-level Dense layers of a large bead batch: 96 beads of the
    dipeptide batch, 64 of the 2000-atom graph; autograd of modules.py:103-114) on the bf16 matrix path with split operands in
    the STRIP layout (csrc/wgrad_gathered.hip strip_xplanes_k + strip_split_k: x split once per problem, g once per strip)
    against fp64 and against the fp32 MFMA strips: same error class.  Operands span 12 orders of magnitude; ragged row /
    column counts; write and accumulate; several problems of different shapes in one table."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    gen = torch.Generator().manual_seed(M + N + K)
    scale_rows = torch.logspace(-9, 0, M).unsqueeze(1)
    gy = (torch.randn(M, N, generator=gen) * scale_rows).to(DEV)
    x = (torch.randn(M, K, generator=gen) * torch.logspace(-3, 2, K).unsqueeze(0)).to(DEV)
    z = torch.randn(M, N, generator=gen).to(DEV) if act else None
    g64 = gy.double().cpu()
    if act == 1:
        s = torch.sigmoid(z.double().cpu())
        g64 = g64 * (s * (1 + z.double().cpu() * (1 - s)))
    elif act == 2:
        g64 = g64 * (1 - torch.tanh(z.double().cpu()) ** 2)
    ref_W, ref_b = g64.t() @ x.double().cpu(), g64.sum(0)
    # a second, smaller problem in the same table (other shape, no bias)
    gy2, x2 = torch.randn(40, 64, generator=gen).to(DEV), torch.randn(40, 132, generator=gen).to(DEV)
    ref2 = gy2.double().cpu().t() @ x2.double().cpu()
    q = WeightGradQueue()
    errs = {}
    for split in (0, 2):                                     # (2: the split strips at every row count they take)
        options.set("strip_split", split)
        gW, gb = torch.full((N, K), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
        gW2 = torch.full((64, 132), float("nan"), device=DEV)
        q.launch([(gy, x, z, act, gW, gb, False), (gy2, x2, None, 0, gW2, None, False)])
        q.launch([(gy, x, z, act, gW, gb, True), (gy2, x2, None, 0, gW2, None, True)])   # accumulate: twice the gradient
        eW = ((gW.double().cpu() - 2 * ref_W).abs().amax(0) / (2 * ref_W).abs().amax(0)).max()
        eb = (gb.double().cpu() - 2 * ref_b).abs().max() / (2 * ref_b).abs().max()
        e2 = (gW2.double().cpu() - 2 * ref2).abs().max() / (2 * ref2).abs().max()
        errs[split] = (float(eW), float(eb), float(e2))
    assert max(errs[2]) < 2e-6, errs
    assert errs[2][0] < 4 * errs[0][0] + 1e-7 and errs[2][2] < 4 * errs[0][2] + 1e-7, f"split strips are not in the fp32 error class: {errs}"
    # deterministic
    options.set("strip_split", 2)
    a, b = torch.empty(N, K, device=DEV), torch.empty(N, K, device=DEV)
    q.launch([(gy, x, z, act, a, None, False)])
    q.launch([(gy, x, z, act, b, None, False)])
    assert torch.equal(a, b)
