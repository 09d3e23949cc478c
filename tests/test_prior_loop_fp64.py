"""prior_fused (the prior net's message-block loop on the channel-group kernels of csrc/decoder_layer.hip: ``prior_msg_fwd_k``,
``prior_msg_bwd_k<R, QS>``, ``dec_dense_fwd_k`` / ``dec_dense_bwd_k`` at N = K = F, ``cgv_decoder_slices_to_dense``) against a
float64 reference of the same loop, one tensor at a time, on every kernel path.

The reference, the case table and which template instance each case reaches are tests/prior_loop_cases.py
(``oracle.cgvae_oracle.equi_message_block`` looped as CGprior.forward loops it, in fp64 on the module's own parameters);
tests/test_prior_loop_cpu.py checks without a GPU that the cases are what they claim.

LOOP level (``test_fused_prior_loop_vs_fp64``): ``CGprior.features(..., h0=h)`` from a dense random h, the loss
``(h_out * up).sum()``, with ``fused_prior`` 0 and 1 from the same state on the same NaN-filled arena.  Per tensor (h_out,
grad h_in, the six parameter gradients of every layer; W2, b2, Wd, bd a second time per filter slice on its own scale), with
err = max |x - ref| / max |ref|:
  hard gate    err_fused <= 1e-4                                      (BASELINE.json's criterion)
  sharper gate err_fused <= K * err_per_block + 16 * 2**-24
every entry finite, exactly zero wherever the reference is exactly zero (the q0 / q2 slices), and bit for bit: a receiver
without incoming edge keeps its state, a source without outgoing edge (or with edges beyond the cutoff only) gets the
upstream weight alone, and slack in the plan's capacity changes no bit.

KERNEL level (``test_prior_msg_fwd_kernel_vs_fp64`` and the tests after it): ``cgv_prior_msg_fwd`` by direct call on dense
random a1, s and v -- the only place where the vector channel ``v_out`` and the ``phi`` rows of slices 0 and 2 are read:
the loop returns h alone.
  hard gate    err_kernel <= 1e-4
  sharper gate err_kernel <= K_FWD * err_fp32_oracle + 16 * 2**-24
where err_fp32_oracle is the error of the same oracle function run in float32 on the CPU against its float64 run.

Measured on an MI355X (pytest -s prints every figure and a WORST line per case before it asserts), worst over all tensors
of a case (per-slice blocks included): err_fused, err_fused / err_per_block
  chignolin-12-600        3.5e-07 (layer 1 grad Wd q1)   1.47 (layer 1 grad b2 q1)     the same under thin / col0 / col3
  lane3-12-432-thin       3.2e-07 (layer 0 grad Wd q1)   1.23 (layer 0 grad W1)
  lane6-12-440-thin       3.0e-07 (layer 0 grad Wd q1)   2.02 (layer 1 grad b2 q1)
  odd8-8-436              6.0e-07 (layer 1 grad Wd q1)   1.19 (layer 0 grad bd q1)
  widest-8-864-thin       3.1e-07 (layer 0 grad Wd q1)   1.47 (layer 0 grad b1)
  narrowest-5-16-R4       2.6e-07 (layer 0 grad Wd q1)   1.41 (layer 1 grad bd q1)
  rbf6-6-32               3.1e-07 (layer 1 grad Wd q1)   1.77 (layer 0 grad b2 q1)
  rbf12-8-64              3.8e-07 (layer 1 grad Wd q1)   1.52 (layer 1 grad W2 q1)
  rbf16-7-48              7.2e-07 (layer 1 grad Wd q1)   1.35 (layer 0 grad W2 q1)
  rbf20-7-200             6.6e-07 (layer 0 grad Wd q1)   1.57 (layer 1 grad b2 q1)     the same under slack
  capacity-16-64          2.7e-07 (layer 0 grad Wd q1)   1.35 (layer 1 grad W2 q1)
  pair-2-32               4.0e-07 (layer 0 grad Wd q1)   1.67 (layer 1 grad bd q1)
  sparse-10-64            2.6e-07 (layer 0 grad Wd q1)   1.69 (layer 1 grad b1)        one layer: 2.4e-07, 1.13 (h_out)
  silent-source-9-64      5.2e-07 (layer 0 grad Wd q1)   1.23 (layer 1 grad bd q1)
  deep-12-128             3.0e-07 (layer 0 grad W2 q1)   1.82 (layer 1 grad b2 q1)
  single-12-128           3.3e-07 (layer 0 grad Wd q1)   1.34 (layer 0 grad bd q1)     the same under slack
Worst ratio 2.02 -> K = 8, the smallest power of two that is at least twice it.  No error of the fused loop exceeds the
floor 16 * 2**-24 = 9.5e-7 (the ratio "above the floor" of every WORST line is 0), so the ratios compare two errors of a few
1e-7 each.  The thin / col0 / col3 variants of 12 x 600 give the figures of the default run: both worst tensors belong to
the top layer, which no slice sum reaches.
The forward kernel: err_kernel, err_kernel / err_fp32_oracle
  chignolin-12-600        2.2e-07 (phi q0)               0.86 (v_out)       second launch of the chain 2.4e-07 (phi q0)
  capacity-16-64          1.4e-07 (v_out)                1.08 (v_out)
  sparse-10-64            1.4e-07 (phi q0)               0.74 (v_out)       second launch of the chain 1.5e-07 (v_out), 0.77
  rbf20-7-200             1.5e-07 (phi q2)               1.38 (s_out)       the same under slack
  narrowest-5-16-R4       1.9e-07 (phi q2)               1.49 (phi q2)
  the loop's own launches, layer by layer: 12 x 600 3.1e-07 (layer 1 v), 1.07 (layer 1 h); sparse 1.9e-07 (layer 1 phi), 0.64
Worst ratio 1.49 -> K_FWD = 4.

What the gates catch (checked once on a scratch copy of the kernels): ``prior_msg_fwd_k`` without wave 0's partial in the
v_out sum fails every forward-kernel test and no loop-level one; ``prior_msg_bwd_k<R, 6>`` dropping the dense base when
slices are present fails the four cases of the 6-slice lane class (thin, lane6, odd8, widest) with errors of order 1 and no
other; tests/test_hip_parity.py::test_fused_prior_loop_equals_per_block_path passes under both.
"""
import pytest
import torch

import prior_loop_cases as C
from coarsegrainingvae_amd.graph import EdgeGeometry, EdgePlan
from test_hip_parity import REL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 8                 # from the measured worst ratio 2.02, see the module docstring
K_FWD = 4             # from the measured worst ratio 1.49
FLOOR = 16 * 2.0 ** -24
_GOT = {}             # case -> {fused: result} of this session (the bit-for-bit tests compare two cases)


def _plan_and_geometry(name):
    """The case's plan and edge records on the device; with slack, capacity > E and NaN records past the last edge."""
    from coarsegrainingvae_amd import decoder_fused
    st = C.setup(name)
    c = st.case
    E = st.nbrs.shape[0]
    nbrs_d = st.nbrs.to(DEV)
    plan = EdgePlan.from_nbrs(nbrs_d, c.n, capacity=C.capacity(c, E))
    xyz_d = st.xyz.to(DEV)
    geom = EdgeGeometry(plan, c.R, C.CUTOFF, pos_dst=xyz_d, pos_src=xyz_d)
    assert (plan.n_edges, plan.n_dst, plan.n_src) == (E, c.n, c.n)
    deg_in = torch.bincount(plan.dst_d[:E].long(), minlength=c.n).cpu().tolist()
    deg_out = torch.bincount(plan.src_s[:E].long(), minlength=c.n).cpu().tolist()
    assert deg_in == C.in_degrees(st.nbrs, c.n) and deg_out == C.out_degrees(st.nbrs, c.n)
    if c.slack > 0:
        assert plan.capacity > E and decoder_fused.staged_edges(plan) > E
        geom.geom_d[E:].fill_(float("nan"))                               # whatever lies past the last edge must not matter
        geom.geom_s[E:].fill_(float("nan"))
    else:
        assert decoder_fused.staged_edges(plan) == E
    return st, nbrs_d, plan, geom


def _prior(st):
    """CGprior carrying the case's parameters (prior_loop_cases.params) in its message blocks, on the device."""
    from coarsegrainingvae_amd import prior_fused
    from coarsegrainingvae_amd.model import CGprior
    c = st.case
    torch.manual_seed(5)
    prior = CGprior(n_conv=c.layers, n_atom_basis=c.F, n_rbf=c.R, activation="swish", cutoff=C.CUTOFF)
    missing, unexpected = prior.load_state_dict({k[len(C.PREFIX) + 1:]: v for k, v in st.P.items()}, strict=False)
    assert not unexpected, unexpected
    prior = prior.to(DEV)
    live = prior_fused.layer_params(prior)
    keys = [k for l in range(c.layers) for k in C.layer_keys(l)]
    assert len(live) == len(keys) and all(torch.equal(p.detach().cpu(), st.P[k]) for p, k in zip(live, keys))
    return prior, live


def _run_loop(name, options):
    """{fused: {"h_out", "gh", "grads"}} of a case: per-block path and fused loop from the same state on the same arena."""
    if name in _GOT:
        return _GOT[name]
    from coarsegrainingvae_amd import prior_fused
    from coarsegrainingvae_amd.trainer import ParamArena
    st, nbrs_d, plan, geom = _plan_and_geometry(name)
    c = st.case
    for opt, value in c.options.items():
        options.set(opt, value)
    prior, live = _prior(st)
    up = st.inp["up"].to(DEV)
    keys = [k for l in range(c.layers) for k in C.layer_keys(l)]

    def run(fused, managed):
        options.set("fused_prior", int(fused))
        h = st.inp["h"].to(DEV).requires_grad_(True)
        calls0 = prior_fused.calls
        if fused:
            assert prior_fused.usable(prior, h, plan, geom), "the case is not on the fused path"
        h_out = prior.features(None, nbrs_d, plan, geom, h0=h)
        assert prior_fused.calls == calls0 + int(fused)                   # moved exactly when it should
        (h_out * up).sum().backward()
        assert not managed or all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(live, arena.grad_views))
        return dict(h_out=h_out.detach().clone(), gh=h.grad.clone(), grads={k: p.grad.clone() for k, p in zip(keys, live)})
    # a first plain backward builds the gradients; then an arena makes the parameters direct-write (the fused path's condition)
    arena = None
    h_probe = st.inp["h"].to(DEV).requires_grad_(True)
    assert not prior_fused.usable(prior, h_probe, plan, geom)             # plain autograd gradients: never fused
    run(False, False)
    arena = ParamArena(live)
    got = {}
    for fused in (False, True):
        arena.g.fill_(float("nan"))
        arena.zero_grad()
        got[fused] = run(fused, True)
    torch.cuda.synchronize()
    _GOT[name] = got
    return got


def _gates(label, items, other, k_gate):
    """``items``: (what, reference, kernel value, yardstick value).  Prints every figure and the WORST line, returns the
    failures."""
    failures, worst_err, worst_ratio, worst_above = [], (0.0, ""), (0.0, ""), (0.0, "")
    for what, ref, a, b in items:
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        if not bool(torch.isfinite(a).all()):
            failures.append(f"{what}: unwritten or non-finite entries")
            continue
        if bool(((ref == 0) & (a != 0)).any()):
            failures.append(f"{what}: non-zero where the reference is exactly zero")
        if float(ref.abs().max()) == 0.0:
            continue
        e1, e0 = rel_err(a, ref), rel_err(b, ref)
        ratio = e1 / e0 if e0 > 0.0 else (float("inf") if e1 > 0.0 else 0.0)
        worst_err = max(worst_err, (e1, what))
        if ratio != float("inf"):
            worst_ratio = max(worst_ratio, (ratio, what))
        if e1 > FLOOR:
            worst_above = max(worst_above, (ratio, what))
        print(f"{label} {what}: kernel {e1:.3e} {other} {e0:.3e} ratio {ratio:.2f}")
        if e1 > REL:
            failures.append(f"{what}: relative error {e1:.3e} > {REL:.1e}")
        if e1 > k_gate * e0 + FLOOR:
            failures.append(f"{what}: relative error {e1:.3e} against {e0:.3e} of the {other} (K = {k_gate})")
    print(f"{label} WORST err_kernel {worst_err[0]:.3e} ({worst_err[1]}) ratio {worst_ratio[0]:.2f} ({worst_ratio[1]}) "
          f"ratio above the floor {worst_above[0]:.2f} ({worst_above[1]})")
    return failures


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_prior_loop_vs_fp64(name, options):
    st = C.setup(name)
    c = st.case
    got = _run_loop(name, options)
    ref = C.loop_reference(name)
    items = [(what, r, a, b) for (what, r), (_, a), (_, b) in zip(C.compared(ref, c), C.compared(got[True], c), C.compared(got[False], c))]
    failures = _gates(name, items, "per-block", K)
    # bit for bit: nothing arrives -> the state is kept; nothing is sent -> the upstream weight alone comes back
    deg, out = C.in_degrees(st.nbrs, c.n), C.out_degrees(st.nbrs, c.n)
    far = [C.FAR] if c.graph == "silent" else []
    h_in, up = st.inp["h"].to(DEV), st.inp["up"].to(DEV)
    for i in [i for i, d in enumerate(deg) if d == 0] + far:
        if not torch.equal(got[True]["h_out"][i], h_in[i]):
            failures.append(f"h_out[{i}]: a receiver without incoming message changed its state")
    for j in [j for j, d in enumerate(out) if d == 0] + far:
        if not torch.equal(got[True]["gh"][j], up[j]):
            failures.append(f"grad h_in[{j}]: a source without outgoing message got more than the upstream weight")
    assert not failures, name + "\n" + "\n".join(failures)


@pytest.mark.parametrize("a,b", [("single-12-128", "single-12-128-slack"), ("rbf20-7-200", "slack-7-200")])
def test_slack_in_the_plans_capacity_changes_no_bit(a, b, options):
    """capacity > E: the kernels stage ``staged_edges(plan)`` records (NaN past the last edge) and walk rows clamped by
    ``min(rowptr[i + 1], E)``: every tensor of the fused loop has the same bits as without slack."""
    assert C.ref_key(a) == C.ref_key(b) and C.CASES[a].options == C.CASES[b].options
    got_a = _run_loop(a, options)[True]
    options.reset()
    got_b = _run_loop(b, options)[True]
    for (what, x), (_, y) in zip(C.compared(got_a, C.CASES[a]), C.compared(got_b, C.CASES[b])):
        assert torch.equal(x, y), what


# ------------------------------------------------------------------------------------------- the forward kernel alone
def _msg_fwd(st, plan, geom, layer, a1, s, v, with_dv):
    """One ``cgv_prior_msg_fwd`` launch with layer ``layer``'s parameters into NaN-filled outputs: (phi, s_out, v_out)."""
    from coarsegrainingvae_amd import _lib
    from coarsegrainingvae_amd.decoder_fused import staged_edges
    c = st.case
    _, _, W2, b2, Wd, bd = (st.P[k].to(DEV).contiguous() for k in C.layer_keys(layer))
    full = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    phi, s_out, v_out = full(c.n, 3 * c.F), full(c.n, c.F), full(c.n, c.F, 3)
    _lib.call("cgv_prior_msg_fwd", _lib.ptr(a1), _lib.ptr(W2), _lib.ptr(b2), _lib.ptr(s), _lib.ptr(v), _lib.ptr(geom.geom_d),
              _lib.ptr(plan.rowptr_d), _lib.ptr(plan.src_d), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(phi), _lib.ptr(s_out),
              _lib.ptr(v_out), c.n, c.F, c.R, staged_edges(plan), int(with_dv), _lib.stream_ptr())
    torch.cuda.synchronize()
    return phi, s_out, v_out


def _kernel_chain(name, n_launches):
    st, _, plan, geom = _plan_and_geometry(name)
    s, v = st.inp["s"].to(DEV), st.inp["v"].to(DEV)
    out = []
    for l, a1 in zip(range(n_launches), (st.inp["a1"].to(DEV), st.inp["a1b"].to(DEV))):
        phi, s, v = _msg_fwd(st, plan, geom, l, a1, s, v, True)          # the next launch reads these very buffers
        out.append(dict(phi=phi, s_out=s, v_out=v))
    return st, plan, geom, out


def _kernel_gates(name, got, n_launches):
    r64, r32 = C.kernel_reference(name, torch.float64, n_launches), C.kernel_reference(name, torch.float32, n_launches)
    items = [(what, r, a, b) for (what, r), (_, a), (_, b) in
             zip(C.compared_kernel(r64), C.compared_kernel(got), C.compared_kernel(r32))]
    return _gates(name + " fwd", items, "fp32 oracle", K_FWD)


@pytest.mark.parametrize("name", C.KERNEL_CASES)
def test_prior_msg_fwd_kernel_vs_fp64(name):
    """phi (all three slices), s_out and v_out of one launch; then ``with_dv`` = 0: v_out is v bit for bit, s_out and phi
    keep their bits."""
    st, plan, geom, got = _kernel_chain(name, 1)
    failures = _kernel_gates(name, got, 1)
    deg = C.in_degrees(st.nbrs, st.case.n)
    for i in [i for i, d in enumerate(deg) if d == 0]:
        if not (torch.equal(got[0]["s_out"][i], st.inp["s"][i].to(DEV)) and torch.equal(got[0]["v_out"][i], st.inp["v"][i].to(DEV))):
            failures.append(f"node {i}: a receiver without incoming edge changed its state")
    v = st.inp["v"].to(DEV)
    phi0, s0, v0 = _msg_fwd(st, plan, geom, 0, st.inp["a1"].to(DEV), st.inp["s"].to(DEV), v, False)
    if not torch.equal(v0, v):
        failures.append("with_dv = 0: v_out is not v bit for bit")
    if not (torch.equal(s0, got[0]["s_out"]) and torch.equal(phi0, got[0]["phi"])):
        failures.append("with_dv = 0: s_out or phi changed")
    assert not failures, name + "\n" + "\n".join(failures)


@pytest.mark.parametrize("name", C.CHAIN_CASES)
def test_prior_msg_fwd_kernel_reads_its_own_vector_state(name):
    """Two launches, the second on the first one's own s_out / v_out (and layer 1's parameters): the layout ``v_out`` is
    written in is the one ``v`` is read in, and the v_j term multiplies what the layer below produced."""
    _, _, _, got = _kernel_chain(name, 2)
    failures = _kernel_gates(name, got, 2)
    assert not failures, name + "\n" + "\n".join(failures)


@pytest.mark.parametrize("name", C.CHAIN_CASES)
def test_forward_launches_of_the_loop_vs_fp64_layer_by_layer(name):
    """The loop's own forward launch sequence (``_PriorLoopFn.forward``: ``cgv_decoder_dense_fwd`` with swish, then
    ``cgv_prior_msg_fwd``, from v = 0) replayed by direct calls, so that every layer's (h_l, v_l, phi_l) can be read: the loop
    itself returns the last h alone.  Layer 0 runs the v_j term on zeros, layer 1 on what layer 0 wrote."""
    from coarsegrainingvae_amd import _lib
    from coarsegrainingvae_amd.primitives import ACT_SWISH
    st, _, plan, geom = _plan_and_geometry(name)
    c = st.case
    h, v = st.inp["h"].to(DEV), torch.zeros(c.n, c.F, 3, device=DEV)
    got = []
    for l in range(c.layers):
        W1, b1 = (st.P[k].to(DEV).contiguous() for k in C.layer_keys(l)[:2])
        a1, z1 = torch.full((c.n, c.F), float("nan"), device=DEV), torch.full((c.n, c.F), float("nan"), device=DEV)
        _lib.call("cgv_decoder_dense_fwd", _lib.ptr(h), _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(a1), _lib.ptr(z1), c.n, c.F, c.F,
                  ACT_SWISH, _lib.stream_ptr())
        phi, h, v = _msg_fwd(st, plan, geom, l, a1, h, v, True)
        got.append((h, v, phi))
    r64, r32 = C.loop_reference(name), C.loop_reference(name, torch.float32)
    items = []
    for l in range(c.layers):
        for what, k in (("h", 0), ("v", 1), ("phi", 2)):
            items.append((f"layer {l} {what}", r64["layers"][l][k], got[l][k], r32["layers"][l][k]))
    failures = _gates(name + " layers", items, "fp32 oracle", K_FWD)
    assert not failures, name + "\n" + "\n".join(failures)
