"""Which C entries the Python front end issues, and what it refuses before issuing any (``-m gpu``).

The other capture / sync / receive tests hold the NUMBERS of sync.py, receive.py, classical_receive.py and equalizer_group.py bit for
bit to the direct ABI calls.  This file holds the DISPATCH: a recording proxy stands in place of the loaded library, forwards every
call and notes the entry's name.  Part A compares the names with a table taken from include/dccn.h and the class docstrings; part
B makes every refused call, and finds no launch entry recorded and a sentinel-filled destination untouched.

"Launch entries" are all ``dccn_*`` calls but the queries: ``*_supported``, ``*_workspace_size``, ``dccn_chain_group_max``,
``dccn_strerror`` and ``dccn_last_hip_error``.

Shapes: the smallest the entries take that still reach every branch -- ``S=7, K=64, CP=16, W=3``, 5 frames, acquisition over 4,
two links, ``cfo_span=7``; a capture of seeded noise, ``lo + 7 T + 2 W`` samples with ``lo = W`` (room for ``(J + 2) T`` from
``lo``, and for five frames cut from any start in ``[lo, lo + T)``).  The content does not matter here: the entries judge sizes."""
import pytest
import torch

import capture_acquire_ref as A
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, K, CP, W = 7, 64, 16, 3
N, J, LINKS, SPAN = 5, 4, 2, 7
T = S * (K + CP)
LO = W
NS = LO + 7 * T + 2 * W
SENT = 0xA5
QUERY_ENDINGS = ("_supported", "_workspace_size")
QUERIES = ("dccn_chain_group_max", "dccn_strerror", "dccn_last_hip_error")


class Recorder:
    """the loaded library with every ``dccn_*`` call noted by name"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dccn_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def clear(self):
        del self.names[:]

    def launches(self):
        return [n for n in self.names if not n.endswith(QUERY_ENDINGS) and n not in QUERIES]

    def queries(self):
        return [n for n in self.names if n.endswith(QUERY_ENDINGS)]


@pytest.fixture(scope="module")
def rec():
    from dl_ofdm_amd import _lib
    r = Recorder(_lib.load())
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_lib", r)              # what _lib.load() hands out from here on
        yield r


@pytest.fixture(scope="module")
def caps():
    """(float32 [NS, 2], int16 [NS, 2]) on the device"""
    noise = torch.randn(NS, 2, generator=torch.Generator().manual_seed(5)).clamp_(-3.9, 3.9)
    return noise.to(DEV), (noise * 2 ** 13).to(torch.int16).to(DEV)


@pytest.fixture(scope="module")
def frames():
    return torch.randn(N, S, K + CP, 2, generator=torch.Generator().manual_seed(6)).to(DEV)


def first_dev(dtype=torch.int64):
    return torch.tensor([LO + 5], dtype=dtype, device=DEV)


def pair():
    return (torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV))


def issued(rec, call):
    rec.clear()
    res = call()
    torch.cuda.synchronize()
    return rec.launches(), res


def refused(rec, exc, match, call, *dests):
    """``call`` raises ``exc`` (``match``), no launch entry was called, and no byte of ``dests`` has changed"""
    for d in dests:
        d.view(torch.uint8).fill_(SENT)
    rec.clear()
    with pytest.raises(exc, match=match):
        call()
    torch.cuda.synchronize()
    assert rec.launches() == [], (match, rec.launches())
    for d in dests:
        assert bool((d.view(torch.uint8) == SENT).all()), match


def sentinel(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=DEV)


# ---- A. entry selection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfo,entry", [(False, "dccn_frame_sync"), (True, "dccn_frame_sync_cfo")])
def test_frame_sync_entries(rec, frames, cfo, entry):
    from dl_ofdm_amd.sync import FrameSync
    fs = FrameSync(S, K, CP, W, N, DEV, cfo=cfo)
    assert issued(rec, lambda: fs.run(frames))[0] == [entry]
    assert issued(rec, lambda: fs.offsets(frames))[0] == [entry]


# (constructor arguments, int16 capture, device start, acquired pair) -> entry
PER_FRAME = [
    (dict(), False, False, False, "dccn_capture_sync"),
    (dict(cfo=True), False, False, False, "dccn_capture_sync"),
    (dict(cfo=True), False, True, False, "dccn_capture_sync_at"),
    (dict(cfo=True, cfo_span=SPAN), False, True, True, "dccn_capture_sync_wide"),
    (dict(cfo=True), True, False, False, "dccn_capture_sync_sc16"),
    (dict(cfo=True), True, True, False, "dccn_capture_sync_sc16"),
]
POOLED = [
    (dict(), False, False, False, "dccn_capture_sync_pooled"),
    (dict(), False, True, False, "dccn_capture_sync_pooled"),
    (dict(cfo_span=SPAN), False, False, True, "dccn_capture_sync_pooled_wide"),
    (dict(cfo_span=SPAN), False, True, True, "dccn_capture_sync_pooled_wide"),
    (dict(), True, False, False, "dccn_capture_sync_pooled_sc16"),
    (dict(), True, True, False, "dccn_capture_sync_pooled_sc16"),
]


def start_of(on_dev, acquired):
    kw = dict(first=first_dev(), lo=LO) if on_dev else dict(first=LO)
    if acquired:
        kw["acquired"] = pair()
    return kw


@pytest.mark.parametrize("ctor,sc16,on_dev,acquired,entry", PER_FRAME)
def test_capture_sync_per_frame_entries(rec, caps, ctor, sc16, on_dev, acquired, entry):
    from dl_ofdm_amd.sync import CaptureSync
    cs = CaptureSync(S, K, CP, W, N, DEV, **ctor)
    assert not cs.pooled and cs.ws is None
    kw = start_of(on_dev, acquired)
    assert issued(rec, lambda: cs.run(caps[sc16], **kw))[0] == [entry]
    assert issued(rec, lambda: cs.offsets(caps[sc16], **kw))[0] == [entry]


@pytest.mark.parametrize("ctor,sc16,on_dev,acquired,entry", POOLED)
def test_capture_sync_pooled_entries(rec, caps, ctor, sc16, on_dev, acquired, entry):
    from dl_ofdm_amd.sync import CaptureSync
    cs = CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_scope="capture", **ctor)
    assert cs.pooled and tuple(cs.cfo.shape) == (1,)
    assert issued(rec, lambda: cs.run(caps[sc16], **start_of(on_dev, acquired)))[0] == [entry]


@pytest.mark.parametrize("ctor,sc16,entry", [(dict(), False, "dccn_capture_acquire"),
                                             (dict(cfo_span=SPAN), False, "dccn_capture_acquire_wide"),
                                             (dict(), True, "dccn_capture_acquire_sc16")])
def test_capture_acquire_entries(rec, caps, ctor, sc16, entry):
    from dl_ofdm_amd.sync import CaptureAcquire
    acq = CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), J, DEV, **ctor)
    launches, first = issued(rec, lambda: acq.run(caps[sc16], LO))
    assert launches == [entry] and first is acq.first and LO <= int(first[0]) < LO + T


def test_group_entries(rec, caps, frames):
    from dl_ofdm_amd.sync import CaptureAcquireGroup, CaptureSyncGroup, FrameSyncGroup
    cap = caps[0]
    fs = FrameSyncGroup(S, K, CP, W, N, LINKS, DEV, cfo=True)
    assert issued(rec, lambda: fs.run([frames, frames]))[0] == ["dccn_frame_sync_grouped"]
    assert issued(rec, lambda: fs.offsets([frames, frames]))[0] == ["dccn_frame_sync_grouped"]
    mixed = [LO, first_dev()]                                    # a start known on the host and one on the device, in one call
    cs = CaptureSyncGroup(S, K, CP, W, N, LINKS, DEV, cfo=True)
    assert issued(rec, lambda: cs.run([cap, cap], mixed, los=LO))[0] == ["dccn_capture_sync_grouped"]
    assert issued(rec, lambda: cs.offsets([cap, cap], mixed, los=[None, LO]))[0] == ["dccn_capture_sync_grouped"]
    cp = CaptureSyncGroup(S, K, CP, W, N, LINKS, DEV, cfo=True, cfo_scope="capture")
    assert issued(rec, lambda: cp.run([cap, cap], mixed, los=LO))[0] == ["dccn_capture_sync_pooled_grouped"]
    assert all(tuple(c.shape) == (1,) for c in cp.cfo) and len(cp.ws) == LINKS
    acq = CaptureAcquireGroup(S, K, CP, A.pilot_sc_of(CP), J, LINKS, DEV)
    launches, firsts = issued(rec, lambda: acq.run([cap, cap], LO))
    assert launches == ["dccn_capture_acquire_grouped"] and firsts is acq.first and len(firsts) == LINKS


# ---- the engines ----------------------------------------------------------------------------------------------------------------------
class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer():
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    Fl = _Flags()
    Fl.opt, Fl.init_learning = 0, 1e-3
    tx = ofdm_tx(Fl)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size, pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=2)
    tr = EqualizerTrainer(Fl, tx, O.init_params(rcfg, seed=24), seed=3)
    tr.load_params(E.init_params(ecfg, seed=23, bias_scale=0.05))
    return tr


class Engine:
    """one solo engine behind the calls the three of them share: ``tail`` is its detector's entry, ``dests`` what a call writes"""

    def __init__(self, kind):
        from dl_ofdm_amd.classical_receive import ClassicalRxReceiver
        from dl_ofdm_amd.engine import RxDims
        from dl_ofdm_amd.receive import RxReceiver
        from dl_ofdm_amd.receiver import Flags
        self.kind = kind
        if kind == "rx":
            self.eng = RxReceiver(RxDims(S=S, kin=K + CP, F=64, D=320, nbits=2), N, CP=CP, pilot_sc=A.pilot_sc_of(CP))
            self.tail, self.dests = "dccn_rx_receive_step", (self.eng.x, self.eng.packed)
        elif kind == "classical":
            self.eng = ClassicalRxReceiver(Flags(nbits=2, channel="EPA"), N)
            self.tail, self.dests = "dccn_classical_receive", (self.eng.x, self.eng.packed)
        else:
            self.eng = _trainer()
            pl = self.eng.resident(N)            # (the plan of this batch size, built ahead: its first use folds the receiver)
            pl.receive()
            self.tail, self.dests = "dccn_eq_receive_step", (pl.x, pl.receive()[0])
        torch.cuda.synchronize()

    def receive(self, x, **kw):
        return self.eng.receive(x, **kw)

    def receive_capture(self, cap, **kw):
        if self.kind == "chain" and "frames" not in kw:
            kw["frames"] = N
        return self.eng.receive_capture(cap, **kw)


@pytest.fixture(scope="module", params=["rx", "classical", "chain"])
def engine(request, rec):
    return Engine(request.param)                 # (built behind the recorder, once for the module)


def result_ptrs(res):
    return [None if t is None else t.data_ptr()
            for t in (res.packed, res.llr, res.prob, res.offset, res.cfo, res.first, res.acquired_cfo, res.acquired_cfo_int)]


ACQUIRED = dict(acquire=J, lo=LO, cfo=True, cfo_scope="capture")
ENGINE_CALLS = [
    ("frames", False, dict(sync=W, cfo=True), ["dccn_frame_sync_cfo"]),
    ("capture", False, ACQUIRED, ["dccn_capture_acquire", "dccn_capture_sync_pooled"]),
    ("capture", False, dict(ACQUIRED, cfo_span=SPAN), ["dccn_capture_acquire_wide", "dccn_capture_sync_pooled_wide"]),
    ("capture", True, ACQUIRED, ["dccn_capture_acquire_sc16", "dccn_capture_sync_pooled_sc16"]),
    # the per-frame cut behind acquisition, and a start the host knows
    ("capture", False, dict(acquire=J, lo=LO, cfo=True), ["dccn_capture_acquire", "dccn_capture_sync_at"]),
    ("capture", False, dict(first=LO), ["dccn_capture_sync"]),
]


@pytest.mark.parametrize("what,sc16,kw,front", ENGINE_CALLS)
def test_engine_entries_and_residency(rec, caps, frames, engine, what, sc16, kw, front):
    if what == "frames":
        call = lambda: engine.receive(frames, **kw)                 # noqa: E731
    else:
        call = lambda: engine.receive_capture(caps[sc16], sync=W, **kw)     # noqa: E731
    launches, res = issued(rec, call)
    assert launches == front + [engine.tail]
    ptrs = result_ptrs(res)
    assert ptrs[0] is not None and ptrs[3] is not None
    if "acquire" in kw:
        assert res.first is not None and res.acquired_cfo is not None and (res.acquired_cfo_int is not None) == ("cfo_span" in kw)
    # the second identical call: the stages are resident -- nothing is sized, queried or built, and the same tensors come back
    launches, res = issued(rec, call)
    assert launches == front + [engine.tail] and rec.queries() == []
    assert result_ptrs(res) == ptrs


# ---- B. refusals: the exception, no launch entry, the destination untouched ------------------------------------------------------------
def test_constructor_refusals(rec):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureAcquireGroup, CaptureSync, CaptureSyncGroup, FrameSync, FrameSyncGroup
    gmax = int(rec.dccn_chain_group_max())
    sc = A.pilot_sc_of(CP)
    solo = (FrameSync, CaptureSync)
    group = (FrameSyncGroup, CaptureSyncGroup)
    sync = [(c, ()) for c in solo] + [(c, (LINKS,)) for c in group]         # (class, what follows `frames`)
    for cls, n in ((CaptureSync, ()), (CaptureSyncGroup, (LINKS,))):
        refused(rec, ValueError, "cfo_scope", lambda: cls(S, K, CP, W, N, *n, DEV, cfo=True, cfo_scope="x"))
        refused(rec, ValueError, "cfo_scope", lambda: cls(S, K, CP, W, N, *n, DEV, cfo_scope="capture"))
    refused(rec, DccnError, "cfo_span", lambda: CaptureSync(S, K, CP, W, N, DEV, cfo_span=SPAN))
    refused(rec, DccnError, "cfo_span", lambda: CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_span=K // 2))
    refused(rec, DccnError, "cfo_span", lambda: CaptureAcquire(S, K, CP, sc, J, DEV, cfo_span=K // 2))
    for cls, n in sync:
        refused(rec, DccnError, "out_kin", lambda: cls(S, K, CP, W, N, *n, DEV, out_kin=K + 1))
        refused(rec, DccnError, None, lambda: cls(S, K, CP, W, 0, *n, DEV))
        refused(rec, DccnError, "supported", lambda: cls(S, K, CP, CP + 1, N, *n, DEV))
    for bad in (0, gmax + 1):
        for cls in group:
            refused(rec, ValueError, None, lambda: cls(S, K, CP, W, N, bad, DEV))
        refused(rec, ValueError, None, lambda: CaptureAcquireGroup(S, K, CP, sc, J, bad, DEV))


def test_frame_sync_run_refusals(rec, frames):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.sync import FrameSync, FrameSyncGroup
    fs, fg = FrameSync(S, K, CP, W, N, DEV), FrameSyncGroup(S, K, CP, W, N, LINKS, DEV)
    out = sentinel(N, S, K + CP, 2)
    outs = [sentinel(N, S, K + CP, 2) for _ in range(LINKS)]
    for bad in (frames.cpu(), frames.double(), frames[:, :, :-1].contiguous()):
        refused(rec, DccnError, None, lambda: fs.run(bad, out=out), out, fs.offset)
        refused(rec, DccnError, None, lambda: fs.offsets(bad), fs.offset)
        refused(rec, DccnError, None, lambda: fg.run([frames, bad], outs=outs), *outs, *fg.offset)
    short = sentinel(N, S, K, 2)
    refused(rec, DccnError, "out", lambda: fs.run(frames, out=short), short, fs.offset)
    refused(rec, DccnError, "out", lambda: fg.run([frames, frames], outs=[outs[0], short]), outs[0], short, *fg.offset)
    refused(rec, ValueError, "one entry per link", lambda: fg.run([frames], outs=outs), *outs)
    refused(rec, ValueError, "one entry per link", lambda: fg.run([frames, frames], outs=outs[:1]), *outs)


def test_capture_sync_run_refusals(rec, caps):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.sync import CaptureSync, CaptureSyncGroup
    cap, cap16 = caps
    out = sentinel(N, S, K + CP, 2)
    short = sentinel(N, S, K, 2)
    outs = [sentinel(N, S, K + CP, 2) for _ in range(LINKS)]
    bad_caps = (cap.cpu(), cap.double(), torch.zeros(NS, 3, device=DEV))
    for scope in ("frame", "capture"):
        cs = CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_scope=scope)
        cg = CaptureSyncGroup(S, K, CP, W, N, LINKS, DEV, cfo=True, cfo_scope=scope)
        for bad in bad_caps:
            refused(rec, DccnError, None, lambda: cs.run(bad, LO, out=out), out, cs.offset)
            refused(rec, DccnError, None, lambda: cg.run([cap, bad], [LO, LO], outs=outs), *outs, *cg.offset)
        refused(rec, DccnError, "out", lambda: cs.run(cap, LO, out=short), short, cs.offset)
        refused(rec, DccnError, "out", lambda: cg.run([cap, cap], [LO, LO], outs=[outs[0], short]), outs[0], short, *cg.offset)
        # a start on the device: its origin, its dtype -- the solo per-frame call, the solo pooled call and the link table
        refused(rec, DccnError, "lo", lambda: cs.run(cap, first_dev(), out=out), out, cs.offset)
        refused(rec, DccnError, "int64", lambda: cs.run(cap, first_dev(torch.int32), out=out, lo=LO), out, cs.offset)
        refused(rec, DccnError, "lo", lambda: cg.run([cap, cap], [LO, first_dev()], outs=outs), *outs, *cg.offset)
        refused(rec, DccnError, "int64", lambda: cg.run([cap, cap], [LO, first_dev(torch.int32)], outs=outs, los=LO), *outs, *cg.offset)
        refused(rec, DccnError, "acquired", lambda: cs.run(cap, first_dev(), out=out, lo=LO, acquired=pair()), out, cs.offset)
        wide = CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_scope=scope, cfo_span=SPAN)
        refused(rec, DccnError, "acquired", lambda: wide.run(cap, first_dev(), out=out, lo=LO), out, wide.offset)
        refused(rec, DccnError, "acquired", lambda: wide.run(cap, first_dev(), out=out, lo=LO, acquired=pair()[::-1]), out, wide.offset)
        refused(rec, DccnError, r"(?s)(?=.*int16)(?=.*cfo_span)",
                lambda: wide.run(cap16, first_dev(), out=out, lo=LO, acquired=pair()), out, wide.offset)
        # per-link lists, and the group classes' float32-only captures
        refused(rec, ValueError, "one entry per link", lambda: cg.run([cap] * 3, [LO, LO], outs=outs), *outs, *cg.offset)
        refused(rec, ValueError, "one entry per link", lambda: cg.run([cap, cap], [LO], outs=outs), *outs, *cg.offset)
        refused(rec, ValueError, "one entry per link", lambda: cg.run([cap, cap], [LO, LO], [T], outs=outs), *outs, *cg.offset)
        refused(rec, ValueError, "one entry per link", lambda: cg.run([cap, cap], [LO, LO], outs=outs, los=[LO] * 3), *outs, *cg.offset)
        refused(rec, DccnError, "float32", lambda: cg.run([cap, cap16], [LO, LO], outs=outs), *outs, *cg.offset)
        refused(rec, DccnError, "scale", lambda: cs.run(cap, LO, out=out, scale=2.0 ** -15), out, cs.offset)
        refused(rec, DccnError, "scale", lambda: cs.run(cap16, LO, out=out, scale=-1.0), out, cs.offset)
    # the per-frame wide cut reads the start where acquisition left it
    wide = CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_span=SPAN)
    refused(rec, DccnError, None, lambda: wide.run(cap, LO, out=out, acquired=pair()), out, wide.offset)
    # a pooled stage writes the frames: no offsets-only call
    cs = CaptureSync(S, K, CP, W, N, DEV, cfo=True, cfo_scope="capture")
    cg = CaptureSyncGroup(S, K, CP, W, N, LINKS, DEV, cfo=True, cfo_scope="capture")
    refused(rec, DccnError, "offsets-only", lambda: cs.offsets(cap, LO), cs.offset)
    refused(rec, DccnError, "offsets-only", lambda: cg.offsets([cap, cap], [LO, LO]), *cg.offset)


def test_capture_acquire_run_refusals(rec, caps):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureAcquireGroup
    cap, cap16 = caps
    sc = A.pilot_sc_of(CP)
    acq, wide, ag = CaptureAcquire(S, K, CP, sc, J, DEV), CaptureAcquire(S, K, CP, sc, J, DEV, cfo_span=SPAN), \
        CaptureAcquireGroup(S, K, CP, sc, J, LINKS, DEV)
    for bad in (cap.cpu(), cap.double(), torch.zeros(NS, 3, device=DEV)):
        refused(rec, DccnError, None, lambda: acq.run(bad, LO), acq.first, acq.cfo)
        refused(rec, DccnError, None, lambda: ag.run([cap, bad], LO), *ag.first, *ag.cfo)
    refused(rec, DccnError, "scale", lambda: acq.run(cap, LO, scale=2.0 ** -15), acq.first)
    refused(rec, DccnError, "scale", lambda: acq.run(cap16, LO, scale=0.0), acq.first)
    refused(rec, DccnError, r"(?s)(?=.*int16)(?=.*cfo_span)", lambda: wide.run(cap16, LO), wide.first, wide.cfo_int)
    refused(rec, DccnError, "float32", lambda: ag.run([cap, cap16], LO), *ag.first)
    refused(rec, ValueError, "one entry per link", lambda: ag.run([cap], LO), *ag.first)
    refused(rec, ValueError, "one entry per link", lambda: ag.run([cap, cap], [LO] * 3), *ag.first)


def test_engine_refusals(rec, caps, frames, engine):
    from dl_ofdm_amd._lib import DccnError
    cap, cap16 = caps
    d = engine.dests
    refused(rec, DccnError, "sync", lambda: engine.receive(frames, cfo=True), *d)
    refused(rec, DccnError, "sync", lambda: engine.receive_capture(cap, first=LO, sync=0), *d)
    refused(rec, DccnError, "not both", lambda: engine.receive_capture(cap, first=LO, acquire=J, sync=W), *d)
    refused(rec, DccnError, "acquire", lambda: engine.receive_capture(cap, sync=W), *d)
    refused(rec, DccnError, "cfo_span", lambda: engine.receive_capture(cap, first=LO, sync=W, cfo=True, cfo_span=SPAN), *d)
    refused(rec, DccnError, "cfo_span", lambda: engine.receive_capture(cap, acquire=J, lo=LO, sync=W, cfo_span=SPAN), *d)
    refused(rec, DccnError, None, lambda: engine.receive_capture(cap, acquire=J, lo=LO, sync=W, cfo=True, cfo_span=-1), *d)
    refused(rec, ValueError, "cfo_scope", lambda: engine.receive_capture(cap, first=LO, sync=W, cfo_scope="capture"), *d)
    # (acquisition runs ahead of the cut: what the cut would object to is judged before it)
    refused(rec, DccnError, "scale", lambda: engine.receive_capture(cap16, acquire=J, lo=LO, sync=W, scale=-1.0), *d)
    refused(rec, DccnError, "scale", lambda: engine.receive_capture(cap, acquire=J, lo=LO, sync=W, scale=2.0 ** -15), *d)
    refused(rec, DccnError, r"(?s)(?=.*int16)(?=.*cfo_span)",
            lambda: engine.receive_capture(cap16, acquire=J, lo=LO, sync=W, cfo=True, cfo_span=SPAN), *d)
    if engine.kind == "chain":
        refused(rec, DccnError, "frames", lambda: engine.receive_capture(cap, first=first_dev(), lo=LO, sync=W, frames=None), *d)


def test_receiver_without_the_frame_description_refuses(rec, caps):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    dims = RxDims(S=S, kin=K + CP, F=64, D=320, nbits=2)
    bare = RxReceiver(dims, N, CP=CP)
    refused(rec, DccnError, "pilot_sc", lambda: bare.receive_capture(caps[0], acquire=J, lo=LO, sync=W), bare.x, bare.packed)
    bare = RxReceiver(dims, N)
    refused(rec, DccnError, "CP", lambda: bare.receive_capture(caps[0], first=LO, sync=W), bare.x, bare.packed)


def test_classical_group_refusals(rec, caps):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    from dl_ofdm_amd.receiver import Flags
    cap, cap16 = caps
    F = Flags(nbits=2, channel="EPA")
    grp = ClassicalReceiveGroup([F, F], N)
    d = [l.x for l in grp.links] + [l.packed for l in grp.links]
    launches, res = issued(rec, lambda: grp.receive_capture([cap, cap], acquire=J, los=LO, sync=W, cfo=True))
    assert launches == ["dccn_capture_acquire_grouped", "dccn_capture_sync_grouped", "dccn_classical_receive_grouped"]
    ptrs = [result_ptrs(r) for r in res]
    launches, res = issued(rec, lambda: grp.receive_capture([cap, cap], acquire=J, los=LO, sync=W, cfo=True))
    assert len(launches) == 3 and rec.queries() == [] and [result_ptrs(r) for r in res] == ptrs
    refused(rec, DccnError, "cfo_span", lambda: grp.receive_capture([cap, cap], acquire=J, los=LO, sync=W, cfo=True, cfo_span=SPAN), *d)
    refused(rec, DccnError, "int16", lambda: grp.receive_capture([cap, cap16], acquire=J, los=LO, sync=W), *d)
    refused(rec, DccnError, "int16", lambda: grp.receive_capture([cap, cap16], firsts=[LO, LO], sync=W), *d)
    refused(rec, ValueError, None, lambda: grp.receive_capture([cap, cap], firsts=[LO], sync=W), *d)
    refused(rec, ValueError, None, lambda: grp.receive_capture([cap], firsts=[LO, LO], sync=W), *d)
    refused(rec, ValueError, None, lambda: grp.receive_capture([cap], acquire=J, los=LO, sync=W), *d)
    refused(rec, DccnError, "not both", lambda: grp.receive_capture([cap, cap], firsts=[LO, LO], acquire=J, sync=W), *d)
    refused(rec, DccnError, "acquire", lambda: grp.receive_capture([cap, cap], sync=W), *d)
    refused(rec, DccnError, "sync", lambda: grp.receive_capture([cap, cap], firsts=[LO, LO], sync=0), *d)
    refused(rec, ValueError, "1\\.\\.", lambda: ClassicalReceiveGroup([], N))
