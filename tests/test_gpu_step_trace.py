"""The in-situ step timeline (include/dccn.h ``dccn_step_trace_*``) held to account (``-m gpu``).

bench.py's ``step.boundaries`` and the timeline tools judge every performance change through the stamps the instrumented launches
of the receiver step leave in a device ring.  Held here, on small engines whose plans the library's own queries name:

* slots      the non-empty slots of a traced step are exactly the launches the plan issues (dccn_rx_dense_tail_fused,
             dccn_rx_bwd_fused_supported under the knobs in force), for the training and for the evaluation step;
* stamps     every marked block has an exit not before its entry on both counters, the marked blocks of a slot are the
             block indices 0 .. grid - 1 of its launch and nothing else, and the grid is the one the route queries give;
* order      within a step a launch starts no earlier than the one before it ended, zero margin, and steps follow each other;
* ring       a ring of 3 after five steps holds steps 2, 3, 4; guard bands around it and every word of an un-issued slot or
             of a block index past a grid stay as they were;
* arithmetic a traced engine computes bit for bit what an untraced one does (which transfers the fp64 parity of
             test_gpu_engine.py / test_gpu_tile_variants.py to the marked code paths);
* switch     refused enables change nothing, disable stops the writes and the count, refused steps, the receive step, the
             equaliser step and stand-alone operators never write;
* graphs     a step captured while a trace is enabled carries no stamps: its replays write nothing, before or after disable.

No test here releases a ring while a graph that was captured under it exists.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gemm_route_query import knobs, route, snapshot
from test_gpu_engine import make_case

pytestmark = pytest.mark.gpu
WORKSPACE = -2                          # DCCN_ERR_WORKSPACE (include/dccn.h)
SENTINEL = 0x5a5a5a5a5a5a5a5a
GUARD = 4096                            # words of each guard band


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def geo(lib):
    L, B, W = C.c_int(0), C.c_int(0), C.c_int(0)
    lib.dccn_step_trace_geometry(C.byref(L), C.byref(B), C.byref(W))
    assert (L.value, B.value, W.value) == (8, 4096, 4)
    return L.value, B.value, W.value


@pytest.fixture(autouse=True)
def trace_is_off_and_knobs_are_back(lib):
    before = snapshot(lib)
    yield
    assert lib.dccn_step_trace_enable(None, 0, 0) == 0
    torch.cuda.synchronize()
    assert snapshot(lib) == before


class Ring:
    """A zeroed ring of `steps` entries in the interior of a larger tensor, sentinel-filled guard bands on both sides."""

    def __init__(self, lib, geo, steps):
        self.lib, self.geo, self.steps = lib, geo, steps
        self.n = steps * geo[0] * geo[1] * geo[2]
        assert lib.dccn_step_trace_bytes(steps) == 8 * self.n
        self.whole = torch.full((GUARD + self.n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        self.ring = self.whole[GUARD:GUARD + self.n]
        self.ring.zero_()
        torch.cuda.synchronize()

    def enable(self):
        return self.lib.dccn_step_trace_enable(C.c_void_p(self.ring.data_ptr()), 8 * self.n, self.steps)

    def disable(self):
        assert self.lib.dccn_step_trace_enable(None, 0, 0) == 0

    def read(self):
        """(synchronises) the ring as uint64 [steps, launches, blocks, words]; the guards are checked on every read"""
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + self.n:] == SENTINEL).all(), "a stamp landed outside the ring"
        return w[GUARD:GUARD + self.n].view(np.uint64).reshape((self.steps,) + self.geo).copy()


def steps_counted(lib):
    return int(lib.dccn_step_trace_steps())


# ---- the cases: shapes of test_gpu_engine.CASES, knobs on a pinned table ------------------------------------------------
# (name, frames, nbits, kin, F, D, knobs)
CASES = [
    ("ragged", 13, 2, 20, 12, 50, {}),
    ("bpsk_36", 36, 1, 80, 64, 320, {}),                         # few-row tiles (fewrow.h marks)
    ("qam8_nocp_100", 100, 3, 64, 64, 320, {}),
    ("qam16_73", 73, 4, 80, 64, 320, {}),                        # the quad-lane tail as its own launch
    ("qpsk_100", 100, 2, 80, 64, 320, {}),
    ("qpsk_100_tail_own", 100, 2, 80, 64, 320, {0: 0}),          # knob 0 = 0: tail as its own launch
    ("qam8_tail_own", 100, 3, 64, 64, 320, {13: 0}),
    ("bpsk_36_unfused_bwd", 36, 1, 80, 64, 320, {11: 0}),        # few-row backward grid, C-Conv weight gradient alone
    ("qpsk_100_cw_kmajor", 100, 2, 80, 64, 320, {11: 0, 3: 7, 1: 7}),
    ("qpsk_100_cw_generic", 100, 2, 80, 64, 320, {11: 0, 3: 0}),
    ("qpsk_100_cw_gemm16", 100, 2, 80, 64, 320, {11: 0, 3: 1}),
    ("qpsk_100_bw_generic", 100, 2, 80, 64, 320, {11: 0, 1: 0}),
    ("qpsk_100_bw_gemm16", 100, 2, 80, 64, 320, {11: 0, 1: 1}),
    ("qpsk_300_all_own", 300, 2, 80, 64, 320, {0: 0, 11: 0}),    # several blocks on every launch, every launch its own
]
IDS = [c[0] for c in CASES]
_inputs = {}


def inputs(case):
    """dims, the parameters and three batches of a case, built once"""
    name, batch, nbits, kin, F, D, _ = case
    key = (batch, nbits, kin, F, D)
    if key not in _inputs:
        dims, _, x0, b0, p = make_case(batch, nbits, kin=kin, F=F, D=D, seed=0)
        more = [make_case(batch, nbits, kin=kin, F=F, D=D, seed=s)[2:4] for s in (1, 2)]
        _inputs[key] = (dims, p, [(x0, b0)] + more)
    return _inputs[key]


def engine(case, train=True):
    """(inside `knobs`) an engine of the case whose tuning table is its own"""
    from dl_ofdm_amd.engine import RxEngine
    dims, p, batches = inputs(case)
    eng = RxEngine(dims, case[1], params=p, train=train).pin_tuning()
    eng.set_batch(*batches[0])
    return eng


def plan_of(lib, eng, train):
    return dict(tail_fused=bool(lib.dccn_rx_dense_tail_fused(C.byref(eng.shape), 1 if train else 0)),
                bwd_fused=bool(lib.dccn_rx_bwd_fused_supported(C.byref(eng.shape))) if train else None)


def expected_slots(plan, train):
    s = {1, 2}
    if not plan["tail_fused"]:
        s.add(3)
    if train:
        s |= {4, 6}
        if not plan["bwd_fused"]:
            s.add(5)
    return s


def test_the_case_table_takes_both_answers_of_both_plan_queries(lib):
    tail, bwd = set(), set()
    for case in CASES:
        with knobs(lib, case[6]):
            for train in (True, False):
                eng = engine(case, train)
                pl = plan_of(lib, eng, train)
                tail.add((train, pl["tail_fused"]))
                if train:
                    bwd.add(pl["bwd_fused"])
    assert tail == {(True, True), (True, False), (False, True), (False, False)} and bwd == {True, False}


# ---- the grid of each slot's launch, from the route queries ------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def routed(lib, op, *dims):
    st, r = route(lib, op, *dims)
    assert st == 0, (op, dims)
    return r


def tiles(rows, cols, tile):
    return cdiv(rows, tile[0]) * cdiv(cols, tile[1])


def expected_grids(lib, case, plan, train):
    """slot -> blocks of the launch(es) that mark it (blockIdx.x extent), where a query of the library names the launch;
    the fused backward launch (slot 4 with bwd_fused) and the optimizer launch (slot 6) have no query: their stamps are held
    to the prefix property alone."""
    _, batch, nbits, kin, F, D, _ = case
    S = 7
    rows, dK, dN, cells = batch * S, S * 2 * F, 2 * D, batch * D
    g = {1: tiles(rows, 2 * F, routed(lib, "cconv_fwd", rows, kin, F)["tile"])}
    if plan["tail_fused"]:
        blocks = C.c_int(0)
        assert lib.dccn_dense_tail_grid(batch, dK, dN, nbits, None, None, None, C.byref(blocks)) == 0
        g[2] = blocks.value
    else:
        g[2] = tiles(batch, dN, routed(lib, "dense_fwd", batch, dK, dN)["tile"])
        # the tail's own launch: a thread per cell in blocks of 256, one block per CU at the most; 16-QAM training: four
        # lanes per cell, two blocks per CU at the most (csrc/tail.h)
        quad = train and nbits == 4
        g[3] = min(cdiv(4 * cells if quad else cells, 256), 512 if quad else 256)
    if train and not plan["bwd_fused"]:
        r = routed(lib, "dense_bwd", batch, dK, dN)
        if r["family"] == "two_launch":
            w, x = routed(lib, "dense_bwd_w", batch, dK, dN), routed(lib, "dense_bwd_x", batch, dK, dN)
            g[4] = max(tiles(dK, dN, w["tile"]), tiles(batch, dK, x["tile"]))
        else:
            g[4] = tiles(batch, dK, r["tile"]) + tiles(dK, dN, r["wtile"]) * r["splits"]
        r = routed(lib, "cconv_bwd_w", rows, kin, F)
        # the weight-gradient tiles of every k range, then the blocks of the tail's slab reduction: four waves each, a wave
        # per tail parameter and three more (csrc/tail.h tail_finalize_blocks)
        g[5] = tiles(2 * kin, 2 * F, r["tile"]) * r["splits"] + (lib.dccn_tail_param_count(nbits) + 6) // 4
    return g


def check_entry(e, slots, grids, nblocks, what):
    """one ring entry [launches, blocks, words] of one step: the slot set, the stamps, the order"""
    written = {s for s in range(e.shape[0]) if e[s].any()}
    assert written == slots, "%s: slots written %s, the plan issues %s" % (what, sorted(written), sorted(slots))
    spans = []
    for s in sorted(slots):
        w0, c0, w1, c1 = (e[s, :, k] for k in range(4))
        m = w0 != 0
        n = int(m.sum())
        assert n > 0 and m[:n].all(), "%s slot %d: the marked blocks are not the indices 0 .. %d" % (what, s, n - 1)
        assert not e[s, n:].any(), "%s slot %d: a word of a block index past the grid was written" % (what, s)
        assert (w1[:n] != 0).all() and (c0[:n] != 0).all() and (c1[:n] != 0).all(), "%s slot %d: a block without exit" % (what, s)
        assert (w1[:n] >= w0[:n]).all() and (c1[:n] >= c0[:n]).all(), "%s slot %d: exit before entry" % (what, s)
        if s in grids:
            assert n == min(grids[s], nblocks), "%s slot %d: %d blocks marked, grid %d" % (what, s, n, grids[s])
        spans.append((s, int(w0[:n].min()), int(w1[:n].max()), n))
    print("%s: %s" % (what, " ".join("slot%d[ticks %d..%d, %d blocks]" % sp for sp in spans)))
    for (sa, _, end_a, _), (sb, start_b, _, _) in zip(spans, spans[1:]):
        assert start_b >= end_a, "%s: slot %d starts %d ticks before slot %d ends" % (what, sb, end_a - start_b, sa)
    return spans


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_slots_stamps_and_order_of_a_traced_step(lib, geo, case, train):
    with knobs(lib, case[6]):
        eng = engine(case, train)
        plan = plan_of(lib, eng, train)
        grids = expected_grids(lib, case, plan, train)
        step = eng.train_step if train else eng.eval_step
        step()                                             # (first call of a kernel: attribute settings, code load)
        ring = Ring(lib, geo, 2)
        assert ring.enable() == 0
        step()
        step()
        t = ring.read()
        ring.disable()
        assert steps_counted(lib) == 2
        print("%s plan %s grids %s" % (case[0], plan, grids))
        spans = [check_entry(t[i], expected_slots(plan, train), grids, geo[1], "%s step %d" % (case[0], i)) for i in (0, 1)]
        assert spans[1][0][1] >= spans[0][-1][2], "step 1 starts before step 0 ended"
        assert [sp[3] for sp in spans[0]] == [sp[3] for sp in spans[1]]
        if plan["tail_fused"]:
            assert spans[0][1][0] == 2 and spans[0][1][3] == min(grids[2], geo[1])


# ---- ring and footprint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[4], CASES[13]], ids=[IDS[4], IDS[13]])
def test_a_ring_of_three_after_five_steps(lib, geo, case):
    from dl_ofdm_amd.steptrace import decode_ring
    with knobs(lib, case[6]):
        eng = engine(case)
        plan = plan_of(lib, eng, True)
        slots, grids = expected_slots(plan, True), expected_grids(lib, case, plan, True)
        eng.train_step()
        ring = Ring(lib, geo, 3)
        assert ring.enable() == 0
        eng.train_step()
        eng.train_step()
        early = ring.read()                                 # entries 0, 1 = steps 0, 1; entry 2 untouched
        assert steps_counted(lib) == 2 and not early[2].any()
        for _ in range(3):
            eng.train_step()
        late = ring.read()
        ring.disable()
    assert steps_counted(lib) == 5
    start = lambda e: int(e[1, :, 0][e[1, :, 0] != 0].min())          # noqa: E731  (slot 1 runs in every step)
    # entry 2 holds step 2 (after step 1), entry 0 step 3 (no longer step 0), entry 1 step 4 (no longer step 1)
    assert start(early[0]) < start(early[1]) < start(late[2]) < start(late[0]) < start(late[1])
    recs = decode_ring(late.reshape(-1), 5, 3, geo)
    assert [r[1]["start"] for r in recs] == [start(late[2]), start(late[0]), start(late[1])]
    for i in range(3):
        check_entry(late[i], slots, grids, geo[1], "%s entry %d" % (case[0], i))


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def state_of(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).clone() for k in ("params", "adam_m", "adam_v", "grads", "metrics_buf", "adam_state", "prob", "dz")}


def three_steps(case, traced_ring=None):
    eng = engine(case)
    if traced_ring is not None:
        assert traced_ring.enable() == 0
    for x, bits in inputs(case)[2]:
        eng.train_step(x, bits)
    st = state_of(eng)
    if traced_ring is not None:
        traced_ring.disable()
    return st


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_traced_engine_computes_the_bits_of_an_untraced_one(lib, geo, case):
    with knobs(lib, case[6]):
        a, b = three_steps(case), three_steps(case)
        for k in a:
            assert torch.equal(a[k], b[k]), "two untraced engines differ in %s: the premise does not hold" % k
        ring = Ring(lib, geo, 2)
        t = three_steps(case, ring)
        assert steps_counted(lib) == 3 and ring.read().any()
        for k in a:
            assert torch.equal(a[k], t[k]), "tracing changed %s" % k


# ---- switch semantics -----------------------------------------------------------------------------------------------------
def test_a_refused_enable_changes_nothing(lib, geo):
    case = CASES[4]
    eng = engine(case)
    eng.train_step()
    other = Ring(lib, geo, 3)
    ptr = C.c_void_p(other.ring.data_ptr())
    # nothing in force: nothing comes into force
    for nbytes, steps in ((8 * other.n - 8, 3), (8 * other.n, 0), (8 * other.n, -1), (0, 3)):
        assert lib.dccn_step_trace_enable(ptr, nbytes, steps) == WORKSPACE
    before = steps_counted(lib)
    eng.train_step()
    assert not other.read().any() and steps_counted(lib) == before
    # a trace in force stays in force, its counter included
    mine = Ring(lib, geo, 2)
    assert mine.enable() == 0
    eng.train_step()
    for nbytes, steps in ((8 * other.n - 8, 3), (8 * other.n, 0), (8 * other.n, -1)):
        assert lib.dccn_step_trace_enable(ptr, nbytes, steps) == WORKSPACE
    assert steps_counted(lib) == 1
    eng.train_step()
    t = mine.read()
    mine.disable()
    assert steps_counted(lib) == 2 and t[0].any() and t[1].any() and not other.read().any()


def test_after_disable_steps_write_nothing_and_count_nothing(lib, geo):
    eng = engine(CASES[4])
    ring = Ring(lib, geo, 2)
    assert ring.enable() == 0
    eng.train_step()
    t0 = ring.read()
    ring.disable()
    eng.train_step()
    eng.eval_step()
    assert steps_counted(lib) == 1 and np.array_equal(ring.read(), t0) and not t0[1].any()
    # enabling again restarts the count; the caller's zeroing is the caller's business
    assert ring.enable() == 0 and steps_counted(lib) == 0
    ring.disable()


@pytest.mark.parametrize("bad,nbits", [("x_prenormalised=2", 2), ("16qam_without_z", 4), ("no_dfft_unfused_backward", 2),
                                        ("second_x_norm_without_the_ride", 2)])
def test_a_refused_step_takes_no_entry(lib, geo, bad, nbits):
    import test_gpu_step_refusals as R
    eng = R.engine(nbits)
    keep = []
    bufs = R.bad_set(bad, eng, keep)
    ring = Ring(lib, geo, 2)
    assert ring.enable() == 0
    assert R.step(eng, bufs) == R.INVALID_ARG
    assert lib.dccn_rx_eval_step(C.byref(eng.shape), None, eng._stream()) == R.INVALID_ARG
    t = ring.read()
    assert steps_counted(lib) == 0 and not t.any()
    eng.train_step()                                       # the next accepted step takes entry 0
    t = ring.read()
    ring.disable()
    assert steps_counted(lib) == 1 and t[0].any() and not t[1].any()


def test_only_the_receiver_steps_are_traced(lib, geo):
    """dccn_rx_receive_step, an equaliser step and a stand-alone operator under an enabled trace"""
    from dl_ofdm_amd.receive import RxReceiver
    from test_gpu_equalizer import _trainer
    case = CASES[4]
    dims, p, batches = inputs(case)
    rx = RxReceiver(dims, case[1], params=p)
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer()
    rng = np.random.RandomState(8)
    xe = (rng.standard_normal((5, 7, 80, 2)) * 2).astype(np.float32)
    be = rng.randint(0, 2, (5, tx.frame_size, 2)).astype(np.int32)
    M, K, N = 37, 128, 64
    x, w, b = (torch.randn(*s, device="cuda") for s in ((M, K), (K, N), (N,)))
    y = torch.empty(M, N, device="cuda")
    ring = Ring(lib, geo, 2)
    assert ring.enable() == 0
    rx.receive(batches[0][0])
    tr.train_step(xe, be, graph=False)
    assert lib.dccn_dense_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, N, None) == 0
    t = ring.read()
    ring.disable()
    assert steps_counted(lib) == 0 and not t.any()
    assert torch.allclose(y, x @ w + b, rtol=1e-4, atol=1e-4)         # (the operator did run)


# ---- graphs --------------------------------------------------------------------------------------------------------------
def graph_run(case, fork, ring=None):
    """capture + three replays [+ disable] + two replays on a fresh engine; the graph is destroyed before this returns"""
    eng = engine(case)
    counted = None
    try:
        if ring is not None:
            assert ring.enable() == 0
        for _ in range(4):
            eng.train_step(graph=True, fork=fork)
        if ring is not None:
            torch.cuda.synchronize()
            counted = steps_counted(eng.lib)
            ring.disable()
        for _ in range(2):
            eng.train_step(graph=True, fork=fork)
        st = state_of(eng)
    finally:
        torch.cuda.synchronize()
        eng.close_graph()
        torch.cuda.synchronize()
    return st, counted


@pytest.mark.parametrize("fork", [False, True], ids=["one_stream", "forked"])
@pytest.mark.parametrize("case", [CASES[4], CASES[13]], ids=[IDS[4], IDS[13]])
def test_a_step_captured_under_a_trace_carries_no_stamps(lib, geo, case, fork):
    with knobs(lib, case[6]):
        ref, _ = graph_run(case, fork)
        ring = Ring(lib, geo, 2)                           # (outlives the graph: graph_run destroys it and synchronises)
        got, counted = graph_run(case, fork, ring)
        t = ring.read()
    assert counted == 0 and steps_counted(lib) == 0, "the capture took a ring entry"
    assert not t.any(), "replays of a step captured under a trace wrote %d words of the ring" % int((t != 0).sum())
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


def eq_graph_run(ring=None):
    from test_gpu_equalizer import _trainer
    _, tx, _, _, _, _, tr = _trainer()
    rng = np.random.RandomState(8)
    x = (rng.standard_normal((5, 7, 80, 2)) * 2).astype(np.float32)
    bits = rng.randint(0, 2, (5, tx.frame_size, 2)).astype(np.int32)
    try:
        if ring is not None:
            assert ring.enable() == 0
        for _ in range(4):
            tr.train_step(x, bits, graph=True)
        if ring is not None:
            torch.cuda.synchronize()
            ring.disable()
        for _ in range(2):
            tr.train_step(x, bits, graph=True)
        torch.cuda.synchronize()
        st = {k: getattr(tr, k).clone() for k in ("params", "adam_m", "adam_v")}
    finally:
        torch.cuda.synchronize()
        for pl in tr._plans.values():
            pl.close()
        torch.cuda.synchronize()
    return st


def test_a_captured_equaliser_step_carries_no_stamps(lib, geo):
    ref = eq_graph_run()
    ring = Ring(lib, geo, 2)                               # (outlives the graph: eq_graph_run closes the plan's graphs)
    got = eq_graph_run(ring)
    t = ring.read()
    assert steps_counted(lib) == 0 and not t.any()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
