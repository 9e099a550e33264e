"""The receiver step decides its whole plan before its first launch (csrc/dccn_abi.hip rx_step_plan): a refused call -- eager
or inside a capture -- has launched nothing, and the step accepts exactly the buffer sets the plan queries promise (``-m gpu``).
Shapes: the N = 64 geometry at 36 frames (one short row tile), the smallest batch of the suite."""
import ctypes as C

import pytest
import torch

from test_gpu_engine import make_case

pytestmark = pytest.mark.gpu
BATCH = 36
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)


def engine(nbits, **kw):
    from dl_ofdm_amd.engine import RxEngine
    dims, _, x, bits, p = make_case(BATCH, nbits)
    eng = RxEngine(dims, BATCH, params=p, train=True, **kw)
    eng.set_batch(x, bits)
    return eng


def variant(eng, **fields):
    """eng.buffers with some fields replaced (a new dccn_rx_buffers; the engine's own stays as it is)"""
    from dl_ofdm_amd import _lib
    vals = {f: getattr(eng.buffers, f) for f, _ in _lib.RxBuffers._fields_}
    vals.update(fields)
    return _lib.RxBuffers(*[vals[f] for f, _ in _lib.RxBuffers._fields_])


def step(eng, bufs):
    return eng.lib.dccn_rx_train_step(C.byref(eng.shape), C.byref(bufs), eng.hp, eng._stream())


def pinned_table(eng, key, value):
    n = int(eng.lib.dccn_tuning_count())
    table = (C.c_int * n)()
    assert eng.lib.dccn_tuning_snapshot(table, n) == n
    table[key] = value
    return table


def bad_set(case, eng, keep):
    """the four buffer sets of the issue; `keep` holds what the set points to"""
    if case == "x_prenormalised=2":
        return variant(eng, x_prenormalised=2)
    if case == "16qam_without_z":
        assert eng.lib.dccn_rx_dense_tail_fused(C.byref(eng.shape), 1) == 0
        return variant(eng, z=0)
    if case == "no_dfft_unfused_backward":
        keep.append(pinned_table(eng, 11, 0))
        return variant(eng, dfft=0, tuning=C.addressof(keep[-1]))
    assert case == "second_x_norm_without_the_ride"
    assert eng.lib.dccn_rx_norm_rides_backward(C.byref(eng.shape)) == 0
    keep.append(torch.empty_like(eng.x_norm))
    return variant(eng, x_next=eng.x.data_ptr(), x_norm_next=keep[-1].data_ptr())


@pytest.mark.parametrize("case,nbits", [("x_prenormalised=2", 2), ("16qam_without_z", 4), ("no_dfft_unfused_backward", 2),
                                        ("second_x_norm_without_the_ride", 2)])
def test_a_refused_step_launches_nothing(case, nbits):
    """Every output of the forward holds a sentinel and every piece of training state a copy: after the refused call all of
    them are bit for bit what they were.  (Before the plan was made first, the last three cases returned the same status
    after R0 / the forward / the backward had run.)"""
    eng = engine(nbits)
    eng.train_step()
    outputs = [eng.x_norm, eng.fft_out, eng.dz, eng.prob]
    for t in outputs:
        t.fill_(7.25)
    eng.metrics_buf.fill_(0x3c)
    watched = outputs + [eng.metrics_buf, eng.params, eng.adam_m, eng.adam_v, eng.adam_state, eng.grads]
    before = [t.clone() for t in watched]
    torch.cuda.synchronize()
    keep = []
    rc = step(eng, bad_set(case, eng, keep))
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    for a, b in zip(before, watched):
        assert torch.equal(a, b)


def test_a_refused_capture_leaves_the_engine_usable():
    eng, fresh = engine(2), engine(2)
    keep = []
    bad = bad_set("no_dfft_unfused_backward", eng, keep)
    g = C.c_void_p(0)
    torch.cuda.synchronize()
    rc = eng.lib.dccn_rx_graph_create(C.byref(eng.shape), C.byref(bad), 1, eng.hp, eng._stream(), C.byref(g))
    assert rc == INVALID_ARG and not g.value
    for e in (eng, fresh):
        for _ in range(3):
            e.train_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.params, fresh.params)


@pytest.mark.parametrize("nbits", [2, 4])
@pytest.mark.parametrize("knob", [None, (0, 0), (11, 0), (13, 3)])
def test_the_plan_queries_and_the_step_agree(knob, nbits):
    """z / dfft may be left out exactly where dccn_rx_dense_tail_fused / dccn_rx_bwd_fused_supported say so, and a step
    without the buffer computes the bits of the step that was given it."""
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    default = lib.dccn_get_tuning(knob[0]) if knob else None
    try:
        if knob:
            assert lib.dccn_set_tuning(*knob) == 0
        full = engine(nbits, want_z=True, want_dfft=True)
        assert full.buffers.z and full.buffers.dfft          # the step the others are held to has both buffers
        full.train_step()
        torch.cuda.synchronize()
        answers = {"z": lib.dccn_rx_dense_tail_fused(C.byref(full.shape), 1),
                   "dfft": lib.dccn_rx_bwd_fused_supported(C.byref(full.shape))}
        for field, answer in answers.items():
            eng = engine(nbits)
            rc = step(eng, variant(eng, **{field: 0}))
            torch.cuda.synchronize()
            assert answer in (0, 1) and rc == (0 if answer else INVALID_ARG), (field, answer, rc)
            if rc == 0:
                assert torch.equal(eng.params, full.params), field
    finally:
        if knob:
            lib.dccn_set_tuning(knob[0], default)
