"""The encoder message kernels (K2 / K4, csrc/equi_msg.hip and csrc/equi_msg_grp.hip: equi_msg_fwd_k in its eight forms,
equi_msg_fwd_grp_k<2 | 4>, equi_msg_bwd_k in its eight forms, equi_msg_bwd_mfma_k, equi_msg_bwd_reduce and
equi_msg_bwd_reduce_jobs_k) against a float64 reference of the same block, one tensor at a time, on every dispatch path.

``cg.EquiMessageBlock`` / ``cg.ContractiveMessageBlock`` run on the device with ``plan=`` / ``geom=``; the reference is
tests/equi_message_cases.py (``oracle.cgvae_oracle.equi_message_block`` / ``contractive_message_block`` in fp64 on the block's
own parameters).  The run table, the graphs and which template instance each run reaches are stated there and checked
without a GPU in tests/test_equi_message_cpu.py.

Per tensor (2 outputs, the input gradients, 6 parameter gradients; the four filter tensors ``inv_dense.1.*`` and
``dist_embed.*`` a second time per slice [kF, (k+1)F) on its own scale -- the slices carry m_0 v_j, m_1 and m_2 unit), with
err = max |x - ref| / max |ref|:
  hard gate    err_kernel <= 1e-4                                     (REL of tests/test_hip_parity.py)
  sharper gate err_kernel <= K * err_fp32_oracle + 16 * 2**-24
where err_fp32_oracle is the error of the same oracle function run in float32 on the CPU against its float64 run.
Where the reference is exactly zero (absent upstream arm, filter slices 0 and 2 under a scalar-only loss, a source without
an outgoing edge, an edge beyond the cutoff) the kernel's value must be exactly zero, and every compared value must be
finite.  The arena runs pre-fill the directly written gradients with NaN.

Measured on an MI355X (pytest -s prints every figure and a WORST line per run before it asserts), worst over all compared
tensors of a run: err_kernel, and err_kernel / err_fp32_oracle among the tensors with err_kernel above the floor ("-": none is)
  box, widths 1-4 7-6 4-8 130-10              9.3e-07 (grad inv_dense.1.bias slice 2) 3.6e-07 5.9e-07 3.3e-07     -
  box, widths 129-12 132-16 34-20 600-10      3.4e-07 6.3e-07 5.4e-07 4.6e-07                                      -
  box, arms x residual, F 8 / 7               <= 3.9e-07 / <= 6.6e-07 (grad inv_dense.1.bias slice 0)              -
  segments-walk 8-10 7-10 130-6 132-12        6.6e-07 7.6e-07 (grad dist_embed.weight slice 1) 5.7e-07 4.8e-07     -
  segments-walk, arms x residual              <= 7.6e-07 (grad dist_embed.weight slice 1, F 7, arm ds)             -
  segments-split 8-10 7-10 130-6              9.3e-07 (grad dist_embed.weight slice 0) 8.0e-07 6.5e-07             -
  segments-split 132-12                       1.5e-06 (grad dist_embed.weight slice 2)                             2.42 (the same slice)
  segments-split, arms x residual             <= 9.3e-07; arm ds on the matrix cores 5.9e-07, n_rbf 16 / 20 7.3e-07 / 5.9e-07   -
  skipped vector channel (6 runs)             <= 9.2e-07 (segments-split, grad dist_embed.weight)                  -
  geometry:coincident-far                     3.5e-07 (grad dist_embed.bias slice 1)                               -     geometry:empty: every figure exactly 0
  chunks:split-130  130-10 all / 8-8 ds, ds FMA walk, dv   3.2e-07 / 4.3e-07 3.6e-07 6.2e-07                       -
  chunks:split-701  8-10 all, ds, ds FMA walk, dv          4.4e-07 2.6e-07 2.6e-07 4.4e-07                         -
  chunks:walk-1541  130-6 all / 8-8 all, ds, dv            3.1e-07 / 6.4e-07 3.8e-07 6.4e-07                       -
  bipartite 8-10 (all, residual, ds, dv) 7-10 130-20       <= 5.5e-07, 5.0e-07, 9.4e-07 (grad dist_embed.weight slice 0)   -
  deferred (5 runs)                           <= 9.3e-07 (segments-split 8-10, grad dist_embed.weight slice 0, as in-launch)   -
  option pairs                                <= 9.3e-07 on either side, but
  segments-split 8-10, msg_bwd_split = 0      1.4e-06 (grad dist_embed.weight slice 2)                             2.41 (grad v)
  cgv_filter_reduce_jobs, 33 slices           <= 3.2e-07 (K 3, R 4, F 7, 352 chunks, gbd slice 0)                  -   (largest ratio below the floor 3.11)
Over all 1701 figures both errors have the same spread: err_kernel median 2.4e-7, maximum 1.5e-6; err_fp32_oracle median
2.9e-7, maximum 6.6e-6.  Five figures lie above the floor 16 * 2**-24 = 9.5e-7, all on the 16-node hub graph, where one
filter-gradient entry is a sum over 820 edge terms that the kernels add one after the other per lane and node while the
oracle's autograd sums them pairwise (a difference of summation order); their ratios are 2.42, 2.42, 2.41, 1.43 and 1.08.
No ratio was left out.  Worst ratio 2.42 -> K = 8, the smallest power of two that is at least twice it.  Below the floor
the largest ratios (up to 9.9, grad dist_embed.bias slices on the same graph, err_fp32_oracle 7.6e-8) measure how well the
oracle's fp32 sum happened to round, not the kernels.

Template instances reached (equi_message_cases.kernel_paths; all 21 in one session): box -> equi_msg_fwd_k<dv, 4 waves, pair | scalar>,
equi_msg_bwd_k<gv | no gv, walk, pair | scalar>; segments-walk and chunks:walk-1541 -> equi_msg_fwd_k<dv, 1 wave>, the walk
backward, arm ds with even F the pipelined scalar-only walk; segments-split and chunks:split-* -> equi_msg_fwd_grp_k<2> (even F;
fwd_group = 4 -> <4>, fwd_group = 0 or odd F -> equi_msg_fwd_k<dv, 4 waves>), equi_msg_bwd_k<split>, arm ds with F % 4 == 0 and
n_rbf <= 12 -> equi_msg_bwd_mfma_k; with_dv = False -> equi_msg_fwd_k<no dv> in its four forms; bipartite -> the 4-wave forward,
the walk backward; in-launch -> equi_msg_bwd_reduce, deferred -> cgv_equi_msg_bwd_deferred + equi_msg_bwd_reduce_jobs_k.
"""
import ctypes

import pytest
import torch

import coarsegrainingvae_amd as cg
import equi_message_cases as C
from coarsegrainingvae_amd.graph import EdgeGeometry, EdgePlan, receiver_group_size
from test_hip_parity import REL, rel_err
from test_pseudo_message_fp64 import _Spy

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 8                 # from the measured worst ratio 2.42, see the module docstring
FLOOR = 16 * 2.0 ** -24
REACHED = set()       # template instances (equi_message_cases.PATHS) of the runs of this session, printed with every WORST line


def _block(r, P):
    """The block with the run's parameters (equi_message_cases.block_params), on the device."""
    g = C.graph(r.case)
    cls = cg.EquiMessageBlock if g.mapping is None else cg.ContractiveMessageBlock
    blk = cls(r.F, "swish", r.R, g.cutoff, 0.0)
    missing, unexpected = blk.load_state_dict(P, strict=False)
    assert not unexpected and all(k.startswith(("inv_message.dist_filter.", "h_att.", "v_att.")) for k in missing), (missing, unexpected)
    blk.with_dv = r.with_dv
    return blk.to(DEV)


class _Launch:
    """One run on the device: options set, block, plan and geometry built, the plan facts that select the kernels checked."""

    def __init__(self, r, options):
        g = self.g = C.graph(r.case)
        self.r = r
        for field, name in C.OPTION_NAMES.items():
            if getattr(r, field) != -1:
                options.set(name, getattr(r, field))
            assert options.get(name) == getattr(r, field)
        self.inp, P = C.run_inputs(r)
        self.blk = _block(r, P)
        self.names = C.param_names(g)
        self.params = [dict(self.blk.named_parameters())[k] for k in self.names]
        E = g.nbrs.shape[0]
        self.index_d = (g.nbrs if g.mapping is None else g.mapping).to(DEV)
        pos_s, pos_d = g.pos_src.to(DEV), g.pos_dst.to(DEV)
        if g.mapping is None:
            plan = EdgePlan.from_nbrs(self.index_d, g.n_src)
            rb = receiver_group_size(plan)                                # as graph.BatchGraph plans the atom graph
            assert rb == C.group_size(g.n_dst, E, r.fwd_group)
            if rb:
                plan.enable_groups(rb)
        else:
            plan = EdgePlan.from_mapping(self.index_d, g.n_dst)
        self.plan = plan
        assert (plan.n_edges, plan.n_src, plan.n_dst) == (E, g.n_src, g.n_dst)
        deg_in = torch.bincount(plan.dst_d[:E].long(), minlength=g.n_dst).cpu().tolist() if E else [0] * g.n_dst
        deg_out = torch.bincount(plan.src_s[:E].long(), minlength=g.n_src).cpu().tolist() if E else [0] * g.n_src
        assert deg_in == C.in_degrees(g) and deg_out == C.out_degrees(g)
        assert (torch.diff(plan.rowptr_s.long()).cpu().tolist() if E else [0] * g.n_src) == deg_out
        # E against the thresholds of the launchers, as the case states them
        kind = r.case.partition(":")[0] if not r.case.startswith("chunks:") else r.case
        want_split = {"box": False, "segments-walk": False, "segments-split": True, "geometry": False, "bipartite": False,
                      "chunks:split-130": True, "chunks:split-701": True, "chunks:walk-1541": False}[kind]
        assert (E >= 48 * g.n_src) == want_split
        if kind in ("segments-split", "chunks:split-130", "chunks:split-701"):
            assert E >= 16 * g.n_dst and E < 200 * g.n_src
        if kind in ("segments-walk", "chunks:walk-1541"):
            assert E < 16 * g.n_dst and g.n_dst > 64
        self.geom = EdgeGeometry(plan, r.R, g.cutoff, pos_dst=pos_d, pos_src=pos_s)
        self.u = [self.inp[f"u{k}"].to(DEV) for k in range(2)]
        self.in_names = C.in_names(g, r.residual)
        self.managed = False                                              # set once a ParamArena owns the gradients

    def once(self):
        """Forward + backward from fresh leaves; parameter gradients not managed by an arena start from None."""
        r, g = self.r, self.g
        if not self.managed:
            for p in self.params:
                p.grad = None
        ins = {k: self.inp[k].to(DEV).requires_grad_(True) for k in self.in_names}
        if g.mapping is None:
            outs = self.blk(ins["s"], ins["v"], None, self.index_d, plan=self.plan, geom=self.geom, residual=r.residual)
        else:
            outs = self.blk(ins["s"], ins["v"], None, self.index_d, plan=self.plan, geom=self.geom,
                            residual=(ins["H"], ins["V"]) if r.residual else None)
        sum((outs[k] * self.u[k]).sum() for k in C.ARMS[r.arm]).backward()
        return ins, outs

    def result(self, ins, outs):
        zeros = lambda t, g: g.detach().clone() if g is not None else torch.zeros_like(t)
        return dict(out={k: o.detach() for k, o in zip(C.OUTS, outs)}, gin={k: zeros(t, t.grad) for k, t in ins.items()},
                    gpar={k: zeros(p, p.grad) for k, p in zip(self.names, self.params)})


def _run_on_device(r, options):
    """(result, launch): the run as the table states it, with its entry points spied."""
    from coarsegrainingvae_amd.primitives import wgrad_queue
    from coarsegrainingvae_amd.trainer import ParamArena
    L = _Launch(r, options)
    if r.deferred:
        # as the trainer runs it: arena-managed parameters (direct gradient writes), the weight-gradient queue collecting
        L.once()                                                          # gradients exist -> the arena can adopt them
        arena = ParamArena(L.params)
        L.managed = True
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        with _Spy() as log:
            with wgrad_queue.collect():
                ins, outs = L.once()
                assert len(wgrad_queue.filters) == 1                      # queued, not reduced inside the backward
                ws, n_chunks, k_live = wgrad_queue.filters[0][:3]
                sh = C.bwd_shape(L.g.n_src, L.g.nbrs.shape[0], r.bwd_split)
                assert (n_chunks, k_live) == (sh.n_chunks, C.k_live(r))
            wgrad_queue.flush()
        assert log.names.count("cgv_equi_msg_bwd_deferred") == 1 and "cgv_equi_msg_bwd" not in log.names
        assert log.names.count("cgv_filter_reduce_jobs") == 1
    else:
        with _Spy() as log:
            ins, outs = L.once()
        assert log.names.count("cgv_equi_msg_bwd") == 1 and "cgv_equi_msg_bwd_deferred" not in log.names
        assert "cgv_filter_reduce_jobs" not in log.names
    paths = C.kernel_paths(r)
    grouped = any(p.startswith("fwd_grp") for p in paths)
    assert log.names.count("cgv_equi_msg_fwd_grouped") == int(grouped) and log.names.count("cgv_equi_msg_fwd") == 1 - int(grouped)
    if grouped:
        assert f"fwd_grp{L.plan.group_rb}" in paths and L.geom.geom_g is not None
    return L.result(ins, outs), L


def _gates(r, got, L):
    """Every compared tensor of the run against the reference; prints each figure and the WORST line, then asserts."""
    r64, r32 = C.reference(r), C.reference(r, torch.float32)
    what_run = C.run_id(r)
    paths = C.kernel_paths(r)
    REACHED.update(paths)
    failures, worst_err, worst_ratio = [], (0.0, ""), (0.0, "")
    for (what, ref), (_, a), (_, b) in zip(C.compared(r64, r.F, r.with_dv), C.compared(got, r.F, r.with_dv), C.compared(r32, r.F, r.with_dv)):
        a = a.cpu().double()
        if not bool(torch.isfinite(a).all()):
            failures.append(f"{what}: unwritten or non-finite entries")
            continue
        if bool(((ref == 0) & (a != 0)).any()):
            failures.append(f"{what}: non-zero where the reference is exactly zero")
        if ref.numel() == 0 or float(ref.abs().max()) == 0.0:
            continue
        e1, e0 = rel_err(a, ref), rel_err(b, ref)
        ratio = e1 / max(e0, 1e-30)
        worst_err = max(worst_err, (e1, what))
        if e1 > FLOOR:
            worst_ratio = max(worst_ratio, (ratio, what))
        print(f"{what_run} {what}: kernel {e1:.3e} fp32 oracle {e0:.3e} ratio {ratio:.2f}")
        if e1 > REL:
            failures.append(f"{what}: relative error {e1:.3e} > {REL:.1e}")
        if e1 > K * e0 + FLOOR:
            failures.append(f"{what}: relative error {e1:.3e} against {e0:.3e} of the fp32 oracle (K = {K})")
    if not r.with_dv:                                                     # vector channel skipped: exactly the residual, or zero
        dv = got["out"]["dv"]
        want = L.inp["v" if L.g.mapping is None else "V"].to(DEV) if r.residual else torch.zeros_like(dv)
        if not torch.equal(dv, want):
            failures.append("dv: the skipped vector channel changed its output")
    print(f"{what_run} WORST err_kernel {worst_err[0]:.3e} ({worst_err[1]}) ratio above the floor {worst_ratio[0]:.2f} "
          f"({worst_ratio[1]}) paths {sorted(paths)} reached so far {len(REACHED)}/{len(C.PATHS)}")
    assert not failures, what_run + "\n" + "\n".join(failures)


def _check(r, options):
    got, L = _run_on_device(r, options)
    _gates(r, got, L)
    return got, L


def _ids(runs):
    return [C.run_id(r) for r in runs]


def _flat(got):
    return [(part + " " + k, t) for part in ("out", "gin", "gpar") for k, t in got[part].items()]


@pytest.mark.parametrize("r", C.RUNS_WIDTHS, ids=_ids(C.RUNS_WIDTHS))
def test_widths_and_radial_bases(r, options):
    """Odd widths (scalar-access instantiation), one channel, one 16-byte piece, one and two live channels in the second
    128-channel tile, the model's 600, all seven compiled n_rbf: forward split over four waves, backward walk."""
    _check(r, options)


@pytest.mark.parametrize("r", C.RUNS_SEGMENTS, ids=_ids(C.RUNS_SEGMENTS))
def test_segment_lengths_on_the_walk_and_split_paths(r, options):
    """Outgoing degrees 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129 (and hubs of 200 and 260 on the split graph), a node
    without any edge, nodes with incoming edges only, repeated edges; even and odd widths."""
    got, L = _check(r, options)
    iso = L.g.named["isolated"]
    for k in C.OUTS:
        assert float(got["out"][k][iso].abs().max()) == 0.0
    for k in ("s", "v"):
        assert float(got["gin"][k][iso].abs().max()) == 0.0 and float(got["gin"][k][L.g.named["only_in"]].abs().max()) == 0.0


@pytest.mark.parametrize("r", C.RUNS_ARMS, ids=_ids(C.RUNS_ARMS))
def test_upstream_arms_and_residual(r, options):
    """ds alone in the loss (scalar-only kernels: the pipelined walk, the matrix-core kernel, and n_rbf = 16 / 20 which stay
    off it), dv alone (gs == nullptr with gv present), both; deltas and updated states."""
    got, _ = _check(r, options)
    F = r.F
    for k in list(got["gpar"])[-C.N_FILTERED:]:
        for q in set(range(3)) - C.ALIVE[r.arm]:
            assert float(got["gpar"][k][q * F:(q + 1) * F].abs().max()) == 0.0, (k, q)
    if r.arm == "ds":
        assert float(got["gin"]["v"].abs().max()) == 0.0


@pytest.mark.parametrize("r", C.RUNS_NO_DV, ids=_ids(C.RUNS_NO_DV))
def test_skipped_vector_channel(r, options):
    """``with_dv`` = False (the encoder's dead vector channel): equi_msg_fwd_k<WITH_DV = false> in its four forms."""
    _check(r, options)


@pytest.mark.parametrize("r", C.RUNS_GEOMETRY, ids=_ids(C.RUNS_GEOMETRY))
def test_geometry_edges(r, options):
    """Coincident nodes, an edge beyond the cutoff, no edge at all."""
    got, L = _check(r, options)
    if r.case == "geometry:empty":
        for k, x in zip(C.OUTS, ("s", "v")):
            want = L.inp[x].to(DEV) if r.residual else torch.zeros_like(got["out"][k])
            assert torch.equal(got["out"][k], want), k
        for k in got["gpar"]:
            assert float(got["gpar"][k].abs().max()) == 0.0, k
    elif not r.residual:
        far = L.g.named["far"]
        for k in C.OUTS:
            assert float(got["out"][k][far].abs().max()) == 0.0
        for k in ("s", "v"):
            assert float(got["gin"][k][far].abs().max()) == 0.0


@pytest.mark.parametrize("r", C.RUNS_CHUNKS, ids=_ids(C.RUNS_CHUNKS))
def test_more_nodes_per_chunk_and_further_reduction_trips(r, options):
    """130 nodes (split: 136 partial sums, second trip of the reduction loop partly valid), 701 (split: two nodes per chunk,
    a one-node last chunk, a padding chunk, third trip), 1541 (walk: five nodes per chunk, waves striding by four)."""
    _check(r, options)


@pytest.mark.parametrize("r", C.RUNS_BIPARTITE, ids=_ids(C.RUNS_BIPARTITE))
def test_atoms_to_beads(r, options):
    """ContractiveMessageBlock: n_dst != n_src, an empty bead, a bead of one atom, receiver-shaped residual."""
    got, L = _check(r, options)
    if not r.residual:
        for k in C.OUTS:
            assert float(got["out"][k][L.g.named["empty_bead"]].abs().max()) == 0.0


@pytest.mark.parametrize("r", C.RUNS_DEFERRED, ids=_ids(C.RUNS_DEFERRED))
def test_deferred_filter_gradient_reduction_under_the_trainer_queue(r, options):
    """cgv_equi_msg_bwd_deferred + ONE cgv_filter_reduce_jobs launch (K = 3, and K = 1 behind the matrix-core kernel)
    produce gWd / gbd in the NaN-filled gradient arena."""
    _check(r, options)


@pytest.mark.parametrize("pair", C.OPTION_PAIRS, ids=[C.run_id(a) + " / " + C.run_id(b).rpartition("|")[2] for a, b in C.OPTION_PAIRS])
def test_option_pairs_change_the_summation_order_only(pair, options):
    """Each side passes the gates; outputs / gradients differ bitwise exactly where kernel_paths names two different forward /
    backward kernels."""
    a, b = pair
    got_a, _ = _check(a, options)
    options.reset()
    got_b, _ = _check(b, options)
    pa, pb = C.kernel_paths(a), C.kernel_paths(b)
    fwd_differs = {p for p in pa if p.startswith("fwd")} != {p for p in pb if p.startswith("fwd")}
    bwd_differs = {p for p in pa if p.startswith("bwd")} != {p for p in pb if p.startswith("bwd")}
    out_bits = any(not torch.equal(got_a["out"][k], got_b["out"][k]) for k in C.OUTS)
    grad_bits = any(not torch.equal(got_a[part][k], got_b[part][k]) for part in ("gin", "gpar") for k in got_a[part])
    assert out_bits == fwd_differs, "the option must select between two forward kernels exactly where kernel_paths says so"
    assert grad_bits == bwd_differs, "the option must select between two backward kernels exactly where kernel_paths says so"


@pytest.mark.parametrize("r", C.DETERMINISM_RUNS, ids=_ids(C.DETERMINISM_RUNS))
def test_three_launches_give_the_same_bits(r, options):
    L = _Launch(r, options)
    first = _flat(L.result(*L.once()))
    for _ in range(2):
        again = _flat(L.result(*L.once()))
        for (what, x), (_, y) in zip(first, again):
            assert torch.equal(x, y), what


# --------------------------------------------------------------------------- the joint reduction, by direct call
JOBS = [(1, 4, 7, 8), (3, 20, 130, 136), (9, 4, 130, 352), (3, 4, 7, 352), (1, 20, 130, 136)]         # (K, R, F, n_chunks)


class _Job(ctypes.Structure):             # cgv::FilterReduceJob, as primitives.flush_filters builds it
    _fields_ = [("part", ctypes.c_void_p), ("gWd", ctypes.c_void_p), ("gbd", ctypes.c_void_p), ("n_chunks", ctypes.c_int),
                ("K", ctypes.c_int), ("R", ctypes.c_int), ("F", ctypes.c_int)]


def _reduce(jobs, parts):
    """One cgv_filter_reduce_jobs launch over ``jobs``; NaN-filled outputs of NINE slices each."""
    from coarsegrainingvae_amd import _lib
    assert ctypes.sizeof(_Job) == _lib.load().cgv_filter_reduce_job_bytes()
    outs = [(torch.full((9 * F, R), float("nan"), device=DEV), torch.full((9 * F,), float("nan"), device=DEV)) for _, R, F, _ in jobs]
    table = (_Job * len(jobs))(*[_Job(p.data_ptr(), gW.data_ptr(), gb.data_ptr(), nc, k, R, F)
                                 for (k, R, F, nc), p, (gW, gb) in zip(jobs, parts, outs)])
    _lib.call("cgv_filter_reduce_jobs", ctypes.addressof(table), len(jobs), _lib.stream_ptr())
    torch.cuda.synchronize()
    return outs


def test_joint_reduction_of_a_mixed_job_table():
    """cgv_filter_reduce_jobs on 5 jobs of synthetic partial sums, K = 1, 3 and 9 in ONE table (nine z blocks per job), R = 4
    and 20, F = 7 and 130, 8, 136 and 352 chunks (one, two and three trips): against the fp64 sum over the chunks at the
    sharper gate, bit for bit against one table per job, exact zeros in slices 0 and 2 for K = 1, nothing written beyond
    the job's own slices, rows or columns."""
    from coarsegrainingvae_amd import _lib
    assert len(JOBS) <= _lib.load().cgv_filter_reduce_jobs_max()
    gen = torch.Generator().manual_seed(77)
    parts = [torch.randn(nc, k, R + 1, F, generator=gen) for k, R, F, nc in JOBS]            # part[chunk][k][n][f]
    parts_d = [p.to(DEV) for p in parts]
    joint = _reduce(JOBS, parts_d)
    alone = [_reduce([job], [p])[0] for job, p in zip(JOBS, parts_d)]
    failures = []
    for j, ((k, R, F, nc), p, (gW, gb), (gW1, gb1)) in enumerate(zip(JOBS, parts, joint, alone)):
        live = range(9) if k == 9 else ((1,) if k == 1 else range(3))
        written = 9 if k == 9 else 3
        s64, s32 = p.double().sum(0), p.sum(0)                                               # [k, R + 1, F]
        for what, x, x1, col in (("gWd", gW, gW1, slice(0, R)), ("gbd", gb, gb1, R)):
            x, x1 = x.cpu(), x1.cpu()
            assert torch.equal(torch.isnan(x), torch.isnan(x1)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(x1)), \
                f"job {j} {what}: differs from the same job in a table of its own"
            assert bool(torch.isnan(x[written * F:]).all()), f"job {j} {what}: rows beyond slice {written - 1} written"
            assert bool(torch.isfinite(x[:written * F]).all()), f"job {j} {what}: rows left unwritten"
            for kk in range(written):
                blk = x[kk * F:(kk + 1) * F].double()
                if kk not in live:
                    assert float(blk.abs().max()) == 0.0, f"job {j} {what}: slice {kk} of a K = 1 job is not exactly zero"
                    continue
                i = kk if k != 1 else 0
                ref, y32 = s64[i, col].t() if what == "gWd" else s64[i, col], s32[i, col].t() if what == "gWd" else s32[i, col]
                e1, e0 = rel_err(blk, ref), rel_err(y32, ref)
                print(f"job {j} (K {k} R {R} F {F} chunks {nc}) {what} slice {kk}: kernel {e1:.3e} fp32 sum {e0:.3e} ratio {e1 / max(e0, 1e-30):.2f}")
                if e1 > K * e0 + FLOOR or e1 > REL:
                    failures.append(f"job {j} {what} slice {kk}: {e1:.3e} against {e0:.3e}")
    assert not failures, "\n".join(failures)
