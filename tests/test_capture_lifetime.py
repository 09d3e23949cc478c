"""Lifetime of what a captured step recorded.  A hipGraph holds raw device addresses: every buffer a capture handed to a
kernel must stay allocated for as long as the graph may be replayed.  ``Trainer.step`` runs a batch that does not fit the
captured buffers eagerly (data.copy_batch_into), and such a step may REPLACE a workspace (more rows: a larger plan).  If
the old tensor went back to the caching allocator, the next replay would write into memory that belongs to somebody else
-- silently.  Each scenario grows a workspace after a capture, then checks, BEFORE any further replay, that no storage the
capture recorded from outside the graph's private pool has been freed; only then does it replay and compare the numbers
with an all-eager trainer fed the same batches and noise.

(No ``torch.cuda.empty_cache()`` here: it would turn a stale address into a page fault.)"""
import pytest
import torch
from torch.multiprocessing.reductions import StorageWeakRef

import coarsegrainingvae_amd as cg
from coarsegrainingvae_amd import _lib
from coarsegrainingvae_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
W = cg.data.WORKLOADS["dipeptide"]


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


class CaptureWatch:
    """Every storage handed to the library (``_lib.ptr``) while a stream capture is in progress: a weak reference and its
    address.  ``classify(graph)`` right after the capture sorts them by the allocator's own view: a storage inside a
    segment of the graph's private pool was born in the capture and may expire with it; every other one was allocated
    outside and must outlive the graph."""

    def __init__(self):
        self.seen = {}                   # storage address -> (StorageWeakRef, bytes)
        self.outside = {}

    def __enter__(self):
        self._ptr = _lib.ptr

        def ptr(t):
            if t is not None and torch.cuda.is_current_stream_capturing():
                st = t.untyped_storage()
                self.seen.setdefault(st.data_ptr(), (StorageWeakRef(st), st.nbytes()))
            return self._ptr(t)
        _lib.ptr = ptr
        return self

    def __exit__(self, *exc):
        _lib.ptr = self._ptr

    def classify(self, graph):
        pool = tuple(graph.pool())
        segments = torch.cuda.memory_snapshot()
        assert segments and all("segment_pool_id" in s for s in segments), "allocator snapshot without pool ids"
        own = [(s["address"], s["address"] + s["total_size"]) for s in segments if tuple(s["segment_pool_id"]) == pool]
        self.outside = {a: v for a, v in self.seen.items() if not any(lo <= a < hi for lo, hi in own)}
        assert self.outside, "the capture handed the library no tensor"
        return self

    def assert_alive(self, what):
        dead = [(hex(a), n) for a, (ref, n) in self.outside.items() if ref.expired()]
        assert not dead, f"{what}: {len(dead)} storage(s) recorded by a live captured graph were freed: {dead[:8]}"


def _make(frames, seed):
    ds = cg.CGDataset(cg.data.synthetic_frames(frames, W["n_atoms"], W["n_cgs"], W["box"], seed=seed))
    ds.generate_neighbor_list(W["atom_cutoff"], W["cg_cutoff"], device=DEV, undirected=True)
    return cg.CG_collate([ds[i] for i in range(frames)])


def _eps(batch, F, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(batch["CG_nxyz"].shape[0], F, generator=gen).to(DEV)


def _copy(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


WORKSPACES = ("_rank_ws", "_mfma_partial", "_rank_ws2")


def _sizes(tr):
    return {n: (None if getattr(tr, n) is None else (getattr(tr, n).data_ptr(), getattr(tr, n).untyped_storage().nbytes()))
            for n in WORKSPACES}


@pytest.mark.parametrize("gram_rows,recapture", [(0, False), (128, False), (0, True), (128, True)])
def test_mfma_rank_update_workspaces_outlive_the_captured_step(gram_rows, recapture, options):
    """Scenario 1 (and 3 with ``recapture``): the two-pass MFMA rank update (rank_rows_mfma 128; ``gram_rows`` 128 takes the
    norm from the Gram launch and its workspace _rank_ws2, 0 from the tile pass and _mfma_partial).  Captured on 8-frame
    batches (24 bead rows on the FMA rank update, the three stacked heads' 72 rows on the MFMA one); an eager 14-frame step
    (42 / 126 rows: every bead layer on the MFMA path) needs more room and replaces the workspaces.  With ``recapture`` the
    learning rate changes first, and the step re-captures before the growth."""
    F, lr = 64, 1e-3
    options.set("rank_rows_mfma", 128)
    options.set("rank_gram_rows", gram_rows)
    first, others, big = _make(8, 1), [_make(8, s) for s in (2, 3, 4)], _make(14, 5)
    e0, eb = _eps(first, F, 10), _eps(big, F, 11)
    e_others = [_eps(b, F, 12 + k) for k, b in enumerate(others)]

    def run(captured):
        model = cg.build_model(F, W["n_rbf"], W["atom_cutoff"], W["cg_cutoff"], 2, 2, W["n_cgs"], seed=7).to(DEV)
        tr = Trainer(model, lr=lr, beta=W["beta"], gamma=W["gamma"])
        cap = cg.data.prepare_batch(_copy(first), DEV, edge_slack=0.25)
        losses = [float(tr.step(cap, eps=e0))]                       # builds the arena
        watch = CaptureWatch()
        if captured:
            with watch:
                tr.capture(cap, warmup=1, eps=e0)                    # one real step on the side stream: the workspaces exist
            watch.classify(tr._graph)
        else:
            tr.step(_copy(first), eps=e0)                            # the capture's warm-up step
        if recapture:
            losses.append(float(tr.step(_copy(others[0]), eps=e_others[0])))
            tr.lr = lr / 2
            if captured:
                watch = CaptureWatch()
                replays = tr.replays
                with watch:
                    losses.append(float(tr.step(_copy(others[1]), eps=e_others[1])))   # re-capture, then its replay
                assert tr.replays == replays + 1 and tr._graphs[True]["lr"] == lr / 2
                watch.classify(tr._graph)
            else:
                losses.append(float(tr.step(_copy(others[1]), eps=e_others[1])))
        before = _sizes(tr)
        replays = tr.replays
        losses.append(float(tr.step(_copy(big), eps=eb)))              # does not fit: eager
        assert tr.replays == replays
        after = _sizes(tr)
        grown = [n for n in WORKSPACES if before[n] is not None and after[n][1] > before[n][1]]
        assert tr.rank_steps_mfma >= 2 and tr.rank_fallbacks == 0
        sentinels = []
        if captured:
            # the growth really happened, to a buffer the graph recorded
            recorded = [n for n in grown if before[n][0] in watch.outside]
            assert recorded, (before, after, gram_rows)
            for n in grown:                                            # where a freed buffer's memory would go next
                s = torch.arange(before[n][1], dtype=torch.int32, device=DEV).to(torch.uint8)
                sentinels.append((s, s.clone()))
            watch.assert_alive("after the eager step that grew " + ", ".join(grown))
        else:
            assert grown
        for b, e in [(others[2], e_others[2]), (others[0], e_others[0])]:
            losses.append(float(tr.step(_copy(b), eps=e)))
        if captured:
            assert tr.replays == replays + 2
        torch.cuda.synchronize()
        for s, ref in sentinels:
            assert torch.equal(s, ref), "a tensor allocated after the growth step was overwritten by a replay"
        return losses, tr, model

    l_ref, tr_ref, m_ref = run(False)
    l_cap, tr_cap, m_cap = run(True)
    assert len(l_ref) == len(l_cap)
    for a, b in zip(l_cap, l_ref):
        assert abs(a - b) <= 1e-5 * abs(b), (l_cap, l_ref)
    for (name, p), q in zip(m_cap.named_parameters(), m_ref.parameters()):
        assert rel_err(p, q) <= 1e-5, name
    for what in ("m", "v"):
        assert rel_err(getattr(tr_cap, what), getattr(tr_ref, what)) <= 1e-5, what


def test_strip_workspace_outlives_the_graph_that_recorded_it(options, monkeypatch):
    """Scenario 2, at the queue level (no model reaches the 32 MB floor): one strip launch on the split-operand path
    (strip_split 2) captured into a hipGraph, then an eager strip launch whose x planes need more than the workspace holds.
    The replaced workspace must stay allocated while the graph lives; the replay then still forms gy^T x (+ bias) with fp32
    accuracy (the bound of test_strip_layout_with_split_operands_has_fp32_accuracy)."""
    from coarsegrainingvae_amd.primitives import WeightGradQueue
    monkeypatch.setattr(WeightGradQueue, "_strip_ws", {})
    options.set("strip_split", 2)
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5)

    def problems(n, M, N, K, bias):
        out = []
        for _ in range(n):
            gy, x = torch.randn(M, N, generator=gen).to(DEV), torch.randn(M, K, generator=gen).to(DEV)
            gW = torch.full((N, K), float("nan"), device=DEV)
            gb = torch.full((N,), float("nan"), device=DEV) if bias else None
            out.append((gy, x, None, 0, gW, gb, False))
        return out

    def check(items, what):
        for gy, x, _z, _a, gW, gb, _acc in items:
            ref = gy.double().cpu().t() @ x.double().cpu()
            e = float(((gW.double().cpu() - ref).abs().amax(0) / ref.abs().amax(0)).max())
            assert e < 2e-6, f"{what}: weight gradient error {e:.2e}"
            if gb is not None:
                rb = gy.double().cpu().sum(0)
                assert float((gb.double().cpu() - rb).abs().max() / rb.abs().max()) < 2e-6, what

    small = problems(2, 64, 64, 256, True)
    big = problems(8, 96, 64, 8192, False)
    q = WeightGradQueue()
    q.launch(small)                                          # eager: the workspace exists before the capture (32 MB floor)
    torch.cuda.synchronize()
    (ws,) = WeightGradQueue._strip_ws.values()
    old_ptr, old_bytes = ws.data_ptr(), ws.numel()
    del ws                                                   # the test holds no reference of its own
    need = 8 * int(lib.cgv_wgrad_strip_split_plane_bytes(96, 8192))
    assert need > old_bytes, (need, old_bytes)

    g = torch.cuda.CUDAGraph()
    q.prepare_capture(torch.device(DEV, torch.cuda.current_device()), flushes=2)
    with CaptureWatch() as watch:
        with torch.cuda.graph(g):
            q.launch(small)
    tables = q.finish_capture()
    watch.classify(g)
    assert old_ptr in watch.outside

    q.launch(big)                                            # eager, larger plan: the workspace is replaced
    (ws,) = WeightGradQueue._strip_ws.values()
    assert ws.numel() >= need and ws.data_ptr() != old_ptr
    del ws
    sentinel = torch.arange(old_bytes, dtype=torch.int32, device=DEV).to(torch.uint8)
    expect = sentinel.clone()
    watch.assert_alive("after the eager strip launch that replaced the workspace")

    torch.cuda.synchronize()
    check(big, "eager launch on the grown workspace")
    for _gy, _x, _z, _a, gW, gb, _acc in small:
        gW.fill_(float("nan"))
        if gb is not None:
            gb.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    check(small, "replay of the captured launch")
    assert torch.equal(sentinel, expect), "a tensor allocated after the growth was overwritten by the replay"
    del g, tables


def test_recaptures_after_learning_rate_changes_do_not_pin_workspaces():
    """Every capture warms up on a side stream, and the split backward-input reduction keeps a 64 MB workspace per stream for
    the life of the process (_lib.prepare_split_workspace): re-captures (a training run re-captures whenever the learning
    rate changes) must reuse the trainer's warm-up stream, not pin another workspace each time."""
    F = 32
    model = cg.build_model(F, W["n_rbf"], W["atom_cutoff"], W["cg_cutoff"], 2, 2, W["n_cgs"], seed=7).to(DEV)
    tr = Trainer(model, lr=1e-3, beta=W["beta"], gamma=W["gamma"])
    batch = cg.synthetic_batch("dipeptide", n_frames=4, seed=1, device=DEV)
    tr.step(batch)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    tr.step(batch)
    torch.cuda.synchronize()
    step_bytes = torch.cuda.max_memory_allocated() - m0      # one eager step's worth
    tr.capture(batch, warmup=1)
    torch.cuda.synchronize()
    n_ws, base = len(_lib._SPLIT_WS), torch.cuda.memory_allocated()
    for k in range(6):
        tr.lr = tr.lr * 0.7
        if k % 2:
            tr.step(batch)                                   # re-captures (warmup 0) and replays
        else:
            tr.capture(batch, warmup=1)
    torch.cuda.synchronize()
    assert len(_lib._SPLIT_WS) == n_ws, (n_ws, len(_lib._SPLIT_WS))
    grew = torch.cuda.memory_allocated() - base
    assert grew <= step_bytes + _lib._SPLIT_BYTES, f"{grew / 2**20:.1f} MiB more after 6 re-captures (one step: {step_bytes / 2**20:.1f} MiB)"
