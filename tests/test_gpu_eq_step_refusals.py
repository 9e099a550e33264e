"""The equaliser step decides its whole plan before its first launch (csrc/eq_step.h eq_step_plan), and the receive steps ask
the decision stage's alignment before theirs: a refused call -- eager or inside a capture -- has launched nothing, and
dccn_eq_group_supported answers 1 exactly where a grouped step is accepted (``-m gpu``).
Shapes: the smallest the suite trains (N = 64, S = 7, QPSK, cp on) at 8 frames; the basic receiver at 36 frames."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_chain_groups import _flags, _rx
from test_gpu_engine import make_case
from test_gpu_equalizer import _trainer

pytestmark = pytest.mark.gpu
B = 8
INVALID_ARG, UNSUPPORTED = -1, -6       # DCCN_ERR_INVALID_ARG, DCCN_ERR_UNSUPPORTED (include/dccn.h)
FLOAT_SENTINEL, BYTE_SENTINEL = 7.25, 0x3c


def variant(bufs, **fields):
    """`bufs` with some fields replaced (a new struct of the same type; the plan's own stays as it is)"""
    vals = {f: getattr(bufs, f) for f, _ in bufs._fields_}
    vals.update(fields)
    return type(bufs)(*[vals[f] for f, _ in bufs._fields_])


def chain(steps=0):
    """a trainer, its plan for B frames with a batch in place, and the batch"""
    _, tx, _, _, _, _, tr = _trainer()
    rng = np.random.RandomState(7)
    x = (rng.standard_normal((B, 7, 80, 2)) * 2).astype(np.float32)
    bits = rng.randint(0, 2, (B, tx.frame_size, 2)).astype(np.int32)
    for _ in range(steps):
        tr.train_step(x, bits, graph=False)
    pl = tr.resident(B)
    pl.set_batch(x, bits)
    return tr, pl, x, bits


def fill(t):
    t.fill_(BYTE_SENTINEL if t.dtype == torch.uint8 else FLOAT_SENTINEL)
    return t


def monitor(tr, pl, keep, **wrong):
    """a dccn_eq_monitor that fits the plan's buffers, but for `wrong`"""
    from dl_ofdm_amd import _lib
    nws = int(tr.lib.dccn_eq_monitor_workspace_size(B + 1, 7, 64))
    chan = torch.zeros(B + 1, 7, 64, 2, device="cuda")
    acc, ws = torch.zeros(5, device="cuda"), torch.zeros(nws, dtype=torch.uint8, device="cuda")
    keep += [chan, acc, ws]
    m = _lib.EqMonitor(chest=pl.chest.data_ptr(), chan=chan.data_ptr(), chan_per_symbol=1, B=B, S=7, K=64,
                       metrics=pl.metrics_buf.data_ptr(), tx_power=pl.tx_power.data_ptr(), acc5=acc.data_ptr(),
                       workspace=ws.data_ptr(), workspace_bytes=nws)
    for f, v in wrong.items():
        setattr(m, f, v)
    keep.append(m)
    return variant(pl.buffers, monitor=C.addressof(m))


def bad_eq_call(case, tr, pl, keep):
    """the refused call of `case`, not yet issued, and further tensors it must not touch"""
    from dl_ofdm_amd import _lib
    lib, st = tr.lib, pl._stream()
    if case == "next_batch_of_another_size":
        y, noise = (torch.zeros(B + 1, 7, 80, 2, device="cuda") for _ in range(2))
        part = torch.zeros((B + 2) // 2, dtype=torch.float64, device="cuda")
        gs = _lib.GenStatic(y=y.data_ptr(), noise=noise.data_ptr(), power_partial=part.data_ptr(), frames=B + 1, S=7, K=64, CP=16,
                            D=int(tr.ofdmobj.frame_size), nbits=2)
        keep += [y, noise, part, gs]
        bufs = variant(pl.buffers, x_next_virtual=C.addressof(gs), gen_next_rides=0)
        return (lambda: lib.dccn_eq_train_step(C.byref(pl.shape), C.byref(bufs), tr.hp, st)), []
    if case == "monitor_of_another_batch":
        bufs = monitor(tr, pl, keep, B=B + 1)
        return (lambda: lib.dccn_eq_train_step(C.byref(pl.shape), C.byref(bufs), tr.hp, st)), keep[:3]
    if case == "monitor_with_a_foreign_tx_power":
        other = torch.zeros(1, device="cuda")
        bufs = monitor(tr, pl, keep, tx_power=other.data_ptr())
        keep.append(other)
        return (lambda: lib.dccn_eq_train_step(C.byref(pl.shape), C.byref(bufs), tr.hp, st)), keep[:3]
    assert case == "receive_llr_off_by_4_bytes"
    from dl_ofdm_amd.receive import row_bytes
    D = int(tr.ofdmobj.frame_size)
    packed = fill(torch.empty(B, row_bytes(D, 2), dtype=torch.uint8, device="cuda"))
    llr = fill(torch.empty(B * D * 2 + 4, device="cuda"))
    prob = fill(torch.empty(B, D, 2, 2, device="cuda"))
    assert llr.data_ptr() % 16 == 0
    ro = _lib.ReceiveOut(packed.data_ptr(), llr.data_ptr() + 4, prob.data_ptr())
    return (lambda: lib.dccn_eq_receive_step(C.byref(pl.shape), C.byref(pl.buffers), C.byref(ro), st)), [packed, llr, prob]


@pytest.mark.parametrize("case", ["next_batch_of_another_size", "monitor_of_another_batch", "monitor_with_a_foreign_tx_power",
                                  "receive_llr_off_by_4_bytes", "rx_receive_llr_off_by_4_bytes"])
def test_a_refused_step_launches_nothing(case):
    """Every output and the whole workspace hold a sentinel and every piece of training state a copy: after the refused call
    all of them are bit for bit what they were.  (Before the plan was made first, every one of these calls returned the same
    status after the forward -- the first three after the backward as well -- had run.)"""
    keep = []
    if case == "rx_receive_llr_off_by_4_bytes":
        from dl_ofdm_amd.receive import RxReceiver
        dims, _, x, _, p = make_case(36, 2)
        rx = RxReceiver(dims, 36, params=p, want_llr=True, want_prob=True)
        rx.receive(x)
        llr = torch.empty(rx.llr.numel() + 4, device="cuda")
        assert llr.data_ptr() % 16 == 0
        watched = [fill(t) for t in (rx.x_norm, rx.fft_out, rx.packed, llr, rx.prob)]
        before = [t.clone() for t in watched]
        torch.cuda.synchronize()
        bufs = variant(rx.buffers, llr=llr.data_ptr() + 4)
        rc = rx.lib.dccn_rx_receive_step(C.byref(rx.shape), C.byref(bufs), rx._stream())
    else:
        tr, pl, _, _ = chain(steps=1)
        watched = [fill(t) for t in (pl.out_eq, pl.chest, tr.grads, pl.metrics_buf, pl.ws)]
        watched += [tr.params, tr.adam_m, tr.adam_v, tr.adam_state]
        call, more = bad_eq_call(case, tr, pl, keep)
        watched += more
        before = [t.clone() for t in watched]
        torch.cuda.synchronize()
        rc = call()
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    for a, b in zip(before, watched):
        assert torch.equal(a, b)


def test_a_refused_capture_leaves_the_trainer_usable():
    tr, pl, x, bits = chain()
    fresh, _, _, _ = chain()
    keep = []
    bad = monitor(tr, pl, keep, B=B + 1)
    g = C.c_void_p(0)
    torch.cuda.synchronize()
    rc = tr.lib.dccn_eq_graph_create(C.byref(pl.shape), C.byref(bad), 1, tr.hp, pl._stream(), C.byref(g))
    assert rc == INVALID_ARG and not g.value
    for t in (tr, fresh):
        for _ in range(3):
            t.train_step(x, bits)
    torch.cuda.synchronize()
    assert torch.equal(tr.params, fresh.params)


@pytest.mark.parametrize("batch", [None, 1170])
def test_group_query_and_grouped_step_agree(tmp_path, batch):
    """two chains (QPSK, 16-QAM) at their own 73 frames, and with the shapes altered to a batch the folded few-row plan does not
    take: the query says 1 and the grouped step runs, or it says 0 and the step returns DCCN_ERR_UNSUPPORTED having launched
    nothing"""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.equalizer_group import EqualizerChainGroup, _ptr_array
    fl = [_flags(nb, tmp_path) for nb in (2, 4)]
    grp = EqualizerChainGroup(fl, [_rx(F, 1) for F in fl])
    lib, act = grp.lib, grp.chains
    for c in act:
        c.begin_epoch()
    grp.step(act, 0)
    t = grp._table(act)
    grp._generate(act, t, 2, 0, False)              # what grp.step(act, 1) does in front of its step
    shapes = [_lib.EqShape.from_buffer_copy(c.loop.pls[1].shape) for c in act]
    for s in shapes:
        s.batch = batch or s.batch
    answer = int(lib.dccn_eq_group_supported(C.byref(shapes[0])))
    watched = [u for c in act for u in (c.tr.params, c.tr.adam_m, c.tr.adam_v, c.tr.adam_state, c.tr.grads, c.loop.pls[1].out_eq,
                                        c.loop.pls[1].chest, c.loop.pls[1].metrics_buf, c.loop.pls[1].ws)]
    before = [u.clone() for u in watched]
    torch.cuda.synchronize()
    rc = lib.dccn_eq_train_step_grouped(2, _ptr_array(shapes), t["bufs"][(1, 1)], grp.hp, grp._stream())
    torch.cuda.synchronize()
    assert answer in (0, 1) and rc == (0 if answer else UNSUPPORTED), (answer, rc)
    assert answer == (0 if batch else 1)
    if not answer:
        for a, b in zip(before, watched):
            assert torch.equal(a, b)
