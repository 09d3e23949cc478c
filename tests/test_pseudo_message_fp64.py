"""The pseudo-vector message kernels (K3, csrc/pseudo_msg.hip: pseudo_fwd_k in its six forms, pseudo_fwd_dense_k,
pseudo_bwd_recv_k, pseudo_bwd_src_k plain / staged / <8>, the two *_dense_k backward passes, pseudo_bwd_reduce and the
deferred reduction) against a float64 reference of the same block, one tensor at a time, on every dispatch path.

``cg.EquiMessagePsuedo`` runs on the device with ``plan=`` / ``geom=``; the reference is tests/pseudo_message_cases.py
(``oracle.cgvae_oracle.equi_message_pseudo`` in fp64 on the block's own parameters).  The run table, the graphs and which
kernels each run reaches are stated there and checked without a GPU in tests/test_pseudo_message_cpu.py.

Per tensor (4 outputs, 4 input gradients, 6 parameter gradients; the four filter tensors a second time per filter row
block [kF, (k+1)F) on its own scale), with err = max |x - ref| / max |ref|:
  hard gate    err_kernel <= 1e-4                                     (REL of tests/test_hip_parity.py)
  sharper gate err_kernel <= K * err_fp32_oracle + 16 * 2**-24
where err_fp32_oracle is the error of the same oracle function run in float32 on the CPU against its float64 run.
Where the reference is exactly zero (absent upstream arm, isolated node, edge beyond the cutoff) the kernel's value must
be exactly zero, and every compared value must be finite.

Measured on an MI355X (pytest -s prints every figure and a WORST line per run before it asserts), worst over all compared
tensors of a run: err_kernel, and err_kernel / err_fp32_oracle among the tensors with err_kernel above the floor ("-": none is)
  width:1-4                      1.4e-06 (grad dist_embed.bias q3)     3.52 (grad inv_dense.0.bias)
  width:7-6 7-10 65-8 66-16      4.5e-07 6.9e-07 4.7e-07 6.8e-07       -
  width:129-10 130-6 64-12       4.1e-07 3.6e-07 4.8e-07               -
  width:34-20                    1.1e-06 (grad dist_embed.weight q5)   0.90 (grad dist_embed.weight q5)
  chunk:12-64 64-8 65-8 97-8     3.1e-07 8.2e-07 4.4e-07 5.8e-07       -
  chunk:257-8 300-8 5-320        6.1e-07 4.2e-07 5.4e-07               -
  segments-general, fwd 0..6     1.1e-06 (grad sbar)                   3.73 (grad sbar)               the same under every variant
  segments-dense:24-10, fwd 0    4.9e-06 (grad inv_dense.1.weight q0)  12.15 (grad dist_embed.bias q2)  also deferred, and every arm
  segments-dense:24-10, 2 4 5    2.0e-06 (dhbar)                       12.49 (grad dist_embed.bias q6)
  segments-dense:24-20, fwd 0    1.8e-06 (grad dist_embed.weight q4)   69.98 / deferred 73.84 (grad dist_embed.bias q0), see below
  segments-dense:24-20, 2 4 5    3.1e-06 (grad sbar)                   18.78 (grad dist_embed.bias q8)
  segments-dense:65-10, 0 / 2 4 5  2.1e-06 / 2.2e-06                   8.93 / 9.46 (grad dist_embed.bias q3 / q5)
  segments-dense:65-20, 0 / 2 4 5  1.9e-06 / 2.0e-06                   8.82 / 6.94 (grad dist_embed.bias q7 / q6)
  width:65-8 arms x residual     below the floor                       -
  geometry:coincident-far        3.3e-07                               -          geometry:empty: every figure exactly 0
  chunk:97-8 deferred            5.5e-07 (grad inv_dense.1.bias q3)    -
Over all 2888 figures both errors have the same spread: err_kernel median 3.5e-7, maximum 4.9e-6; err_fp32_oracle median
3.9e-7, maximum 2.4e-6.  No tensor of the kernels is out of family.  The ratios above 4 are all filter gradients (and what
is computed from them) on the dense graph: the kernels add the 423 edge terms one after the other in each lane, node by node and
then over the chunks (rounding error ~ sqrt(N) 2**-24 = 1.2e-6), the oracle's autograd sums the same terms with torch's blocked pairwise reduction
(~ log N 2**-24) -- a legitimate difference of summation order.  ONE figure is out of family, on the oracle's side: block q0
of grad dist_embed.bias at segments-dense:24-20 has err_fp32_oracle = 1.7e-8, a quarter of 2**-24 and a fifth to a
thirteenth of the other eight blocks of the same tensor (8.9e-8 .. 2.3e-7) -- the fp32 sum happened to round to the
nearest float -- while err_kernel of that block (1.19e-6 / 1.25e-6) sits among those of its neighbours (3.4e-7 .. 1.6e-6).
Its ratio (70 / 74) measures the oracle's luck, so it is left out of K; the tensor still has to pass, and does, because
the floor carries it: 64 * 1.7e-8 + 9.5e-7 = 2.0e-6.  Worst ratio without it 18.78 -> K = 64, the smallest power of two
that is at least twice it.

Kernels reached (pseudo_message_cases.kernel_paths; all 13 in one session): widths, chunks <= 97, geometry ->
pseudo_fwd_k<8>, pseudo_bwd_recv_k<8>, pseudo_bwd_src_k<2>, pseudo_bwd_reduce; chunk:257 / 300 -> pseudo_fwd_k<2>,
pseudo_bwd_recv_k<2>; segments-general fwd 1 -> <2>, 2 / 3 / 4 / 6 -> the staged forms <2> <4> <8> <1>, 5 -> <8>;
segments-dense fwd 0 -> pseudo_fwd_dense_k, pseudo_bwd_recv_dense_k, pseudo_bwd_src_dense_k; 2 -> pseudo_bwd_src_k<2, staged>;
4 -> pseudo_bwd_src_k<8>; 5 -> pseudo_bwd_src_k<2>; deferred -> cgv_pseudo_msg_bwd_deferred + cgv_filter_reduce_jobs.
"""
import ctypes

import pytest
import torch

import coarsegrainingvae_amd as cg
import pseudo_message_cases as C
from coarsegrainingvae_amd.graph import EdgeGeometry, EdgePlan
from test_hip_parity import REL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 64                # from the measured worst ratio 18.78, see the module docstring
FLOOR = 16 * 2.0 ** -24
REACHED = set()       # kernel paths (pseudo_message_cases.PATHS) of the runs of this session, printed with every WORST line


def _block(c):
    """The block with the case's parameters (pseudo_message_cases.block_params), on the device."""
    _, P = C.case_inputs(c)
    blk = cg.EquiMessagePsuedo(c.F, "swish", c.R, c.graph.cutoff, 0.0)
    missing, unexpected = blk.load_state_dict(P, strict=False)
    assert not unexpected and all(k.startswith("inv_message.dist_filter.") for k in missing), (missing, unexpected)
    return blk.to(DEV)


class _Spy:
    """Call log of the C ABI (names in launch order) while the block runs."""

    def __enter__(self):
        from coarsegrainingvae_amd import _lib
        self.lib, self.real, self.names = _lib, _lib.call, []

        def spy(name, *a, **k):
            self.names.append(name)
            return self.real(name, *a, **k)
        _lib.call = spy
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


def _check(run, options):
    from coarsegrainingvae_amd.primitives import wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    c = C.case(run.case)
    g, F, n = c.graph, c.F, c.graph.n
    E = g.nbrs.shape[0]
    options.set("pseudo_fwd", run.variant)
    assert options.get("pseudo_fwd") == run.variant and options.get("pseudo_chunks") == 0
    inp, _ = C.case_inputs(c)
    blk = _block(c)
    params = [dict(blk.named_parameters())[k] for k in C.PARAMS]
    nbrs_d, xyz_d = g.nbrs.to(DEV), g.xyz.to(DEV)
    plan = EdgePlan.from_nbrs(nbrs_d, n)
    assert plan.n_edges == E and (E >= 16 * n) == run.case.startswith("segments-dense")
    deg = torch.bincount(plan.dst_d[:E].long(), minlength=n).cpu().tolist() if E else [0] * n
    assert deg == C.in_degrees(g)
    if run.case.startswith("segments-dense"):
        assert plan.n_edges >= 16 * n and deg[:10] == [0, 1, 3, 4, 5, 7, 8, 9, 129, 257]
    geom = EdgeGeometry(plan, c.R, g.cutoff, pos_dst=xyz_d, pos_src=xyz_d)
    u = [inp[f"u{k}"].to(DEV) for k in range(4)]

    def once():
        ins = [inp[k].to(DEV).requires_grad_(True) for k in C.INS]
        outs = blk(*ins, None, nbrs_d, plan=plan, geom=geom, residual=run.residual)
        sum((outs[k] * u[k]).sum() for k in C.ARMS[run.arm]).backward()
        return ins, outs

    if run.deferred:
        # as the trainer runs it: arena-managed parameters (direct gradient writes), the weight-gradient queue collecting
        once()                                                            # gradients exist -> the arena can adopt them
        arena = ParamArena(params)
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        with _Spy() as log:
            with wgrad_queue.collect():
                ins, outs = once()
                assert len(wgrad_queue.filters) == 1                      # queued, not reduced inside the backward
            wgrad_queue.flush()
        assert "cgv_pseudo_msg_bwd_deferred" in log.names and "cgv_pseudo_msg_bwd" not in log.names
        assert log.names.count("cgv_filter_reduce_jobs") == 1
    else:
        with _Spy() as log:
            ins, outs = once()
        assert log.names.count("cgv_pseudo_msg_bwd") == 1 and "cgv_pseudo_msg_bwd_deferred" not in log.names
    assert log.names.count("cgv_pseudo_msg_fwd_rows") == 1
    paths = C.run_paths(run)
    REACHED.update(paths)

    if run.residual:                                                      # the same V as rows [3 i + xyz][f], bit for bit
        rows = getattr(outs[2], "_cgv_rows", None)
        assert rows is not None and torch.equal(rows, outs[2].detach().permute(0, 2, 1).reshape(3 * n, F))
    got = dict(out={k: o.detach() for k, o in zip(C.OUTS, outs)},
               gin={k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in zip(C.INS, ins)},
               gpar={k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in zip(C.PARAMS, params)})
    r64 = C.reference(run.case, run.arm, run.residual)
    r32 = C.reference(run.case, run.arm, run.residual, torch.float32)
    what_run = C.run_id(run)
    failures, worst_err, worst_ratio = [], (0.0, ""), (0.0, "")
    for (what, r), (_, a), (_, b) in zip(C.compared(r64, F), C.compared(got, F), C.compared(r32, F)):
        a = a.cpu().double()
        if not bool(torch.isfinite(a).all()):
            failures.append(f"{what}: unwritten or non-finite entries")
            continue
        if bool(((r == 0) & (a != 0)).any()):
            failures.append(f"{what}: non-zero where the reference is exactly zero")
        if r.numel() == 0 or float(r.abs().max()) == 0.0:
            continue
        e1, e0 = rel_err(a, r), rel_err(b, r)
        ratio = e1 / max(e0, 1e-30)
        worst_err = max(worst_err, (e1, what))
        if e1 > FLOOR:
            worst_ratio = max(worst_ratio, (ratio, what))
        print(f"{what_run} {what}: kernel {e1:.3e} fp32 oracle {e0:.3e} ratio {ratio:.2f}")
        if e1 > REL:
            failures.append(f"{what}: relative error {e1:.3e} > {REL:.1e}")
        if e1 > K * e0 + FLOOR:
            failures.append(f"{what}: relative error {e1:.3e} against {e0:.3e} of the fp32 oracle (K = {K})")
    print(f"{what_run} WORST err_kernel {worst_err[0]:.3e} ({worst_err[1]}) ratio above the floor {worst_ratio[0]:.2f} "
          f"({worst_ratio[1]}) paths {sorted(paths)} reached so far {len(REACHED)}/{len(C.PATHS)}")
    assert not failures, what_run + "\n" + "\n".join(failures)
    return got, inp


def _ids(runs):
    return [C.run_id(r) for r in runs]


@pytest.mark.parametrize("run", C.RUNS_WIDTHS, ids=_ids(C.RUNS_WIDTHS))
def test_widths_and_radial_bases_on_the_general_path(run, options):
    """Odd widths, one live lane in the last channel block (65, 129), F R not a multiple of four (filter rows not staged in
    pass A), all seven compiled n_rbf: pseudo_fwd_k<8>, pseudo_bwd_recv_k<8>, pseudo_bwd_src_k<2>, pseudo_bwd_reduce."""
    _check(run, options)


@pytest.mark.parametrize("run", C.RUNS_CHUNKS, ids=_ids(C.RUNS_CHUNKS))
def test_source_chunks_and_the_launch_size_switch(run, options):
    """n <= 64: a node per chunk; 65, 97: 24 chunks with empty tail chunks; 257, 300: 64 chunks of 5 nodes and the
    > 256-block side of the PSEUDO_EB_WIDE / PSEUDO_EB_NARROW switch; (5, 320): a 5-block-wide channel grid."""
    _check(run, options)


@pytest.mark.parametrize("run", C.RUNS_GENERAL, ids=_ids(C.RUNS_GENERAL))
def test_segment_lengths_on_the_general_path_under_every_forward_variant(run, options):
    """Segments of 0, 1, 2, 3, 7, 8, 9, 16, 17, 130 and 257 edges (duplicates in the last), an isolated node, nodes with
    outgoing edges only; pseudo_fwd = 0..6 (2, 3, 4, 6 stage 128-edge chunks: one and two chunk boundaries)."""
    got, _ = _check(run, options)
    g = C.case(run.case).graph
    for k in C.OUTS:
        assert float(got["out"][k][g.named["isolated"]].abs().max()) == 0.0
        assert float(got["out"][k][g.named["only_out"]].abs().max()) == 0.0


@pytest.mark.parametrize("run", C.RUNS_DENSE, ids=_ids(C.RUNS_DENSE))
def test_segment_lengths_on_the_dense_path(run, options):
    """E >= 16 n with segments of 0, 1, 3, 4, 5, 7, 8, 9, 129 and 257 edges and a 130-edge source segment: the per-filter
    kernels (pseudo_fwd = 0), the staged pass B (2), pseudo_bwd_src_k<8> (4) and the plain walk (5)."""
    _check(run, options)


@pytest.mark.parametrize("run", C.RUNS_ARMS, ids=_ids(C.RUNS_ARMS))
def test_upstream_arms_and_residual(run, options):
    """Each output alone in the loss, scalars only, vectors only, all four; deltas and updated states.  General path: the
    absent gradients are NULL; dense path: ops._PseudoMessage hands zeros to the per-filter kernels."""
    _check(run, options)


@pytest.mark.parametrize("run", C.RUNS_GEOMETRY, ids=_ids(C.RUNS_GEOMETRY))
def test_geometry_edges(run, options):
    """Coincident beads, an edge beyond the cutoff, no edge at all."""
    got, inp = _check(run, options)
    if run.case == "geometry:empty":
        for k, x in zip(C.OUTS, C.INS):
            want = inp[x].to(DEV) if run.residual else torch.zeros_like(got["out"][k])
            assert torch.equal(got["out"][k], want), k
        for k in C.PARAMS:
            assert float(got["gpar"][k].abs().max()) == 0.0, k
    else:
        far = C.case(run.case).graph.named["far"]
        if not run.residual:
            assert float(got["out"]["dh"][far].abs().max()) == 0.0


@pytest.mark.parametrize("run", C.RUNS_DEFERRED, ids=_ids(C.RUNS_DEFERRED))
def test_deferred_filter_gradient_reduction_under_the_trainer_queue(run, options):
    """cgv_pseudo_msg_bwd_deferred + ONE cgv_filter_reduce_jobs launch (K = 9) produce gWd / gbd in the gradient arena."""
    _check(run, options)


# --------------------------------------------------------------------------- bounds, by direct call
GUARD = 64            # floats in front of and behind every output buffer


class _Guarded:
    """A tensor of ``shape`` inside a larger NaN-filled allocation."""

    def __init__(self, *shape):
        numel = 1
        for d in shape:
            numel *= d
        self.whole = torch.full((GUARD + numel + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.whole[GUARD:GUARD + numel].view(*shape)
        self.numel = numel

    def untouched(self):
        return bool(torch.isnan(self.whole).all())

    def check(self, what):
        assert bool(torch.isnan(self.whole[:GUARD]).all()), f"{what}: written in front of the buffer"
        assert bool(torch.isnan(self.whole[GUARD + self.numel:]).all()), f"{what}: written behind the buffer"
        assert bool(torch.isfinite(self.t).all()), f"{what}: entries left unwritten"


@pytest.mark.parametrize("graph", ["dense", "sparse"])
@pytest.mark.parametrize("residual", [0, 1])
def test_entry_points_stay_inside_their_buffers(graph, residual, options):
    """cgv_pseudo_msg_fwd_rows and cgv_pseudo_msg_bwd at n = 5, F = 65 (one live lane in the second channel block), R = 10
    (F R not a multiple of four): guard floats untouched, every float inside written, a short workspace refused."""
    from coarsegrainingvae_amd import _lib
    n, F, R = 5, 65, 10
    if graph == "dense":                                                  # 20 ordered pairs four times over: E = 80 = 16 n
        pairs = [(i, j) for i in range(n) for j in range(n) if i != j] * 4
    else:
        pairs = C.sparse_graph(n).nbrs.tolist()
    nbrs = torch.tensor(pairs, dtype=torch.long).to(DEV)
    E = nbrs.shape[0]
    assert (E >= 16 * n) == (graph == "dense")
    gen = torch.Generator().manual_seed(n + F + E)
    rn = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    pos = 2.0 * rn(n, 3)
    plan = EdgePlan.from_nbrs(nbrs, n)
    geom = EdgeGeometry(plan, R, 9.5, pos_dst=pos, pos_src=pos)
    phi, s, sbar, v, vbar = rn(n, 9 * F), rn(n, F), rn(n, F), rn(n, F, 3), rn(n, F, 3)
    Wd, bd = 0.3 * rn(9 * F, R), 0.3 * rn(9 * F)
    p, st = _lib.ptr, _lib.stream_ptr()
    # forward
    dh, dhbar, dv, dvbar, rows = _Guarded(n, F), _Guarded(n, F), _Guarded(n, F, 3), _Guarded(n, F, 3), _Guarded(3 * n, F)
    _lib.call("cgv_pseudo_msg_fwd_rows", p(phi), p(s), p(sbar), p(v), p(vbar), p(geom.geom_d), p(plan.rowptr_d), p(plan.src_d),
              p(Wd), p(bd), p(dh.t), p(dhbar.t), p(dv.t), p(dvbar.t), p(rows.t), n, F, R, residual, E, st)
    torch.cuda.synchronize()
    for name, buf in zip(("dh", "dhbar", "dv", "dvbar", "dv_rows"), (dh, dhbar, dv, dvbar, rows)):
        buf.check(name)
    assert torch.equal(rows.t, dv.t.permute(0, 2, 1).reshape(3 * n, F))
    # backward
    gh, ghb, gv, gvb = rn(n, F), rn(n, F), rn(n, F, 3), rn(n, F, 3)
    ws_bytes = int(_lib.load().cgv_pseudo_msg_bwd_workspace_bytes(n, F, R))
    assert ws_bytes == 4 * C.pseudo_chunks(n) * 9 * (R + 1) * F + 256
    ws = _Guarded(ws_bytes // 4)

    def backward(bytes_given):
        outs = [_Guarded(n, 9 * F), _Guarded(n, F), _Guarded(n, F), _Guarded(n, F, 3), _Guarded(n, F, 3), _Guarded(9 * F, R),
                _Guarded(9 * F)]
        call = lambda: _lib.call(
            "cgv_pseudo_msg_bwd", p(phi), p(s), p(sbar), p(v), p(vbar), p(geom.geom_d), p(plan.rowptr_d), p(plan.src_d),
            p(geom.geom_s), p(plan.rowptr_s), p(plan.dst_s), p(Wd), p(bd), p(gh), p(ghb), p(gv), p(gvb),
            *[p(o.t) for o in outs], n, F, R, residual, E, p(ws.t), ctypes.c_size_t(bytes_given), st)
        return outs, call
    outs, call = backward(ws_bytes - 1)
    with pytest.raises(RuntimeError, match="workspace too small"):
        call()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and ws.untouched()
    outs, call = backward(ws_bytes)
    call()
    torch.cuda.synchronize()
    for name, buf in zip(("g_phi", "g_s", "g_sbar", "g_v", "g_vbar", "gWd", "gbd"), outs):
        buf.check(name)
    assert bool(torch.isnan(ws.whole[:GUARD]).all()) and bool(torch.isnan(ws.whole[GUARD + ws.numel:]).all())
    used = C.pseudo_chunks(n) * 9 * (R + 1) * F                           # the partial sums: every chunk writes its own
    assert bool(torch.isfinite(ws.t[:used]).all()) and bool(torch.isnan(ws.t[used:]).all())
