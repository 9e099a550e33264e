"""One carrier offset per capture on the GPU (``-m gpu``): ``dccn_capture_sync_pooled`` / ``dccn_capture_sync_pooled_grouped`` held

1. bit for bit to ``dccn_capture_sync`` where the two must agree (offset and metric always; the estimate and the frames at one
   frame), to themselves (two runs; a start read from device memory; the grouped call against the solo calls);
2. to the fp64 restatement of the definition (tests/capture_pool_ref.py) evaluated on the GPU's OWN offsets, so that no frame is
   left out: the estimate within ``pool_bound`` (derived there), the frames within frame_cfo_ref.DEROT_TOL max|c|;
3. to their refusals (nothing is launched, for any link);
4. and ``receive_capture(..., cfo_scope="capture")`` of the receiver, the chain and the chain group held to the same receive step
   on the pooled entry's frames, to the call with the true start, and to the solo chains.

Captures: capture_sync_ref's, impaired with ONE offset over the whole capture (radio.apply_cfo_stream)."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A
import capture_pool_ref as P
import capture_sync_ref as CR
import frame_cfo_ref as F
import frame_sync_ref as R
from dl_ofdm_amd.radio import apply_cfo_stream
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = R.S, R.K
GUARD = 64
SENT_X, SENT_OFF, SENT_C, SENT_M, SENT_W = 777.0, -99, 333.0, 555.0, 0x5A
DEV = "cuda"
INVALID, WORKSPACE = -1, -2
FRAME_COUNTS = (1, 3, 5, 73, 259)           # one wave of a block; a ragged block; two blocks; the workload's batch; > 4 * 64
SHAPES = ((16, 3), (4, 4))                  # (CP, W)
CHANNELS = (("ETU", 5.0), ("EPA", 5.0), ("EVA", 30.0), ("AWGN", 30.0))
# (spare: stride = T + spare, shift: first = T + shift, crop: out_kin == K, eps): first even and odd, both strides, both out_kin
LAYOUTS = ((0, 0, False, P.EPS[0]), (0, 1, True, P.EPS[1]), (1, 0, True, P.EPS[0]), (1, 1, False, P.EPS[1]))


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """guarded, sentinel-filled outputs and workspace of one link; ``n_cfo``: 1 (pooled) or n (the per-frame entry)"""

    def __init__(self, lib, n, out_kin, w, n_cfo=1):
        self.n, self.W, self.out_kin, self.n_cfo = n, w, out_kin, n_cfo
        self.n_out, self.n_met = n * S * out_kin * 2, n * (2 * w + 1)
        self.n_ws = int(lib.dccn_capture_sync_pooled_workspace_size(n))
        self.out_buf = torch.full((self.n_out + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.off_buf = torch.full((n + GUARD,), SENT_OFF, dtype=torch.int32, device=DEV)
        self.cfo_buf = torch.full((n_cfo + GUARD,), SENT_C, dtype=torch.float32, device=DEV)
        self.met_buf = torch.full((self.n_met + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        self.ws_buf = torch.full((self.n_ws + GUARD,), SENT_W, dtype=torch.uint8, device=DEV)
        self.status = None

    out = property(lambda self: self.out_buf[:self.n_out].view(self.n, S, self.out_kin, 2))
    offset = property(lambda self: self.off_buf[:self.n])
    cfo = property(lambda self: self.cfo_buf[:self.n_cfo])
    metric = property(lambda self: self.met_buf[:self.n_met].view(self.n, 2 * self.W + 1))

    def guards_intact(self):
        return (bool((self.out_buf[self.n_out:] == SENT_X).all()) and bool((self.off_buf[self.n:] == SENT_OFF).all())
                and bool((self.cfo_buf[self.n_cfo:] == SENT_C).all()) and bool((self.met_buf[self.n_met:] == SENT_M).all())
                and bool((self.ws_buf[self.n_ws:] == SENT_W).all()))

    def untouched(self):
        return (bool((self.out_buf == SENT_X).all()) and bool((self.off_buf == SENT_OFF).all())
                and bool((self.cfo_buf == SENT_C).all()) and bool((self.met_buf == SENT_M).all())
                and bool((self.ws_buf == SENT_W).all()))

    def link(self, cap, first, stride, first_dev=None, lo=0):
        from dl_ofdm_amd import _lib
        return _lib.PooledLink(cap.data_ptr(), int(cap.shape[0]), 0 if first_dev is not None else first,
                               None if first_dev is None else first_dev.data_ptr(), lo, stride, self.out_buf.data_ptr(),
                               self.off_buf.data_ptr(), self.cfo_buf.data_ptr(), self.met_buf.data_ptr(), self.ws_buf.data_ptr(),
                               self.n_ws)


def pooled_run(lib, cap, first, stride, n, cp, w, crop=False, first_dev=None, lo=0):
    """one dccn_capture_sync_pooled call"""
    o = Out(lib, n, K if crop else K + cp, w)
    o.status = lib.dccn_capture_sync_pooled(cap.data_ptr(), int(cap.shape[0]), 0 if first_dev is not None else first,
                                            None if first_dev is None else first_dev.data_ptr(), lo, stride, n, S, K, cp, w,
                                            o.out_kin, o.out_buf.data_ptr(), o.off_buf.data_ptr(), o.cfo_buf.data_ptr(),
                                            o.met_buf.data_ptr(), o.ws_buf.data_ptr(), o.n_ws, stream())
    torch.cuda.synchronize()
    return o


def per_frame_run(lib, cap, first, stride, n, cp, w, crop=False):
    """dccn_capture_sync's CFO instantiation on the same kind of outputs"""
    o = Out(lib, n, K if crop else K + cp, w, n_cfo=n)
    o.status = lib.dccn_capture_sync(cap.data_ptr(), int(cap.shape[0]), first, stride, n, S, K, cp, w, o.out_kin,
                                     o.out_buf.data_ptr(), o.off_buf.data_ptr(), o.cfo_buf.data_ptr(), o.met_buf.data_ptr(), stream())
    torch.cuda.synchronize()
    return o


def grouped_run(lib, links, outs, n, cp, w, out_kin):
    from dl_ofdm_amd import _lib
    table = (_lib.PooledLink * len(links))(*links)
    st = lib.dccn_capture_sync_pooled_grouped(len(links), table, n, S, K, cp, w, out_kin, stream())
    torch.cuda.synchronize()
    for o in outs:
        o.status = st
    return st


def capture_of(channel, snr, CP, spare, eps, frames):
    """(cap float32 [n, 2], stride): the 75-frame case capture, or all 300 frames of the case where more are asked for"""
    if frames <= CR.FRAMES:
        return P.case_capture(channel, snr, CP, spare, eps)
    return P.long_capture(channel, snr, CP, eps, spare)


_dev_caps = {}


def dev_capture(channel, snr, CP, spare, eps, frames):
    key = (channel, snr, CP, spare, eps, frames > CR.FRAMES)
    if key not in _dev_caps:
        capn, stride = capture_of(channel, snr, CP, spare, eps, frames)
        _dev_caps[key] = (capn, dev(capn), stride)
    return _dev_caps[key]


# ---- 1 + 2. bit for bit where the entries must agree; against fp64 on the GPU's own offsets -------------------------------------
worst = {"estimate": 0.0, "derotation": 0.0}


@pytest.mark.parametrize("channel,snr", CHANNELS)
@pytest.mark.parametrize("CP,W", SHAPES)
@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_pooled_estimate_and_frames(lib, n, CP, W, channel, snr):
    T = S * (K + CP)
    assert lib.dccn_capture_sync_supported(S, K, CP, W) == 1
    for spare, shift, crop, eps0 in LAYOUTS:
        capn, cap, stride = dev_capture(channel, snr, CP, spare, eps0, n)
        first = CR.case_first(CP, shift)
        assert stride == T + spare and (first % 2) == shift
        a = pooled_run(lib, cap, first, stride, n, CP, W, crop)
        assert a.status == 0 and a.guards_intact()
        # offset and metric: dccn_capture_sync's, bit for bit; at one frame the estimate and the frames as well
        b = per_frame_run(lib, cap, first, stride, n, CP, W, crop)
        assert b.status == 0
        assert torch.equal(a.offset, b.offset) and same_bits(a.metric, b.metric)
        if n == 1:
            assert same_bits(a.cfo, b.cfo) and same_bits(a.out, b.out)
        # a start read from device memory holding `first`; a second run
        lo = first - 5
        at = pooled_run(lib, cap, 0, stride, n, CP, W, crop, first_dev=dev(np.array([first], np.int64)), lo=lo)
        again = pooled_run(lib, cap, first, stride, n, CP, W, crop)
        for c in (at, again):
            assert c.status == 0 and c.guards_intact()
            assert torch.equal(c.offset, a.offset) and same_bits(c.metric, a.metric) and same_bits(c.cfo, a.cfo)
            assert same_bits(c.out, a.out)
        # fp64 on the GPU's own offsets: the estimate, then the frames with the GPU's own estimate
        off = a.offset.cpu().numpy().astype(np.int64)
        assert np.abs(off).max() <= W
        _, lam, phi, gam = CR.reference(capn, first, stride, n, S, K, CP, W)
        gf, total, eps64 = P.pooled(gam, off, W)
        eps32 = float(a.cfo[0])
        err, bound = float(F.circle(eps32 - eps64)), float(P.pool_bound(phi, gf, total))
        want = P.derotated(capn, first, stride, off, eps32, S, K, CP)
        want = want[:, :, CP:] if crop else want
        derr = float(np.abs(a.out.cpu().numpy().astype(np.float64) - want).max())
        peak = float(np.sqrt((np.asarray(capn, np.float64) ** 2).sum(axis=1)).max())
        worst["estimate"] = max(worst["estimate"], err / bound)
        worst["derotation"] = max(worst["derotation"], derr / (F.DEROT_TOL * peak))
        print("%s %g dB CP %d W %d frames %d layout (%d, %d, %s, %+.3f): eps32 %+.6f, |eps32 - eps64| %.2e = %.3f of the bound %.2e; "
              "|out - out64| %.2e = %.3f of the bound; |eps32 - eps| %.2e; worst so far %.3f / %.3f"
              % (channel, snr, CP, W, n, spare, shift, crop, eps0, eps32, err, err / bound, bound, derr,
                 derr / (F.DEROT_TOL * peak), float(F.circle(eps32 - eps0)), worst["estimate"], worst["derotation"]))
        assert err <= bound
        assert derr <= F.DEROT_TOL * peak


def test_zero_capture(lib):
    CP, W, n = 16, 3, 5
    T = S * (K + CP)
    cap = torch.zeros(n * T + 2 * W, 2, dtype=torch.float32, device=DEV)
    a = pooled_run(lib, cap, W, T, n, CP, W)
    assert a.status == 0 and a.guards_intact()
    assert same_bits(a.cfo, torch.zeros(1, dtype=torch.float32, device=DEV))          # +0, not -0
    assert same_bits(a.out, torch.zeros_like(a.out)) and bool((a.offset == -W).all())


# ---- the grouped call ---------------------------------------------------------------------------------------------------------
def _group_links(lib, n_links, n, CP, W, crop):
    """link i's (cap, first, stride, first_dev, lo): its own case capture, starts on the host and on the device mixed; links 0
    and 1 share a capture"""
    T = S * (K + CP)
    out = []
    for i in range(n_links):
        channel, snr = CHANNELS[(max(i, 1) - 1) % len(CHANNELS)]
        spare, shift, eps0 = (max(i, 1) - 1) % 2, i % 2, P.EPS[(max(i, 1) - 1) % 2]
        _, cap, stride = dev_capture(channel, snr, CP, spare, eps0, n)
        first = CR.case_first(CP, shift) + (T + spare if i == 1 else 0)           # link 1: the shared capture, one frame on
        on_dev = i % 3 == 2
        out.append((cap, first, stride, dev(np.array([first], np.int64)) if on_dev else None, first - 7 if on_dev else 0))
    return out


@pytest.mark.parametrize("n_links", [1, 2, 8])
@pytest.mark.parametrize("n,CP,W,crop", [(5, 16, 3, False), (73, 4, 4, True), (73, 16, 3, False)])
def test_grouped_call_equals_the_solo_calls(lib, n_links, n, CP, W, crop):
    n = min(n, 72) if n_links > 1 else n                                        # (link 1 starts one frame on)
    links = _group_links(lib, n_links, n, CP, W, crop)
    assert n_links < 2 or links[0][0] is links[1][0]
    out_kin = K if crop else K + CP
    outs = [Out(lib, n, out_kin, W) for _ in links]
    st = grouped_run(lib, [o.link(cap, first, stride, fd, lo) for o, (cap, first, stride, fd, lo) in zip(outs, links)], outs, n,
                     CP, W, out_kin)
    assert st == 0
    for i, (o, (cap, first, stride, fd, lo)) in enumerate(zip(outs, links)):
        s = pooled_run(lib, cap, first, stride, n, CP, W, crop, first_dev=fd, lo=lo)
        assert s.status == 0 and o.guards_intact(), i
        assert torch.equal(o.offset, s.offset) and same_bits(o.metric, s.metric) and same_bits(o.cfo, s.cfo), i
        assert same_bits(o.out, s.out), i
        assert not bool((o.out == SENT_X).any()) and float(o.cfo[0]) != SENT_C


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_grouped_calls_write_nothing(lib):
    n, CP, W = 5, 16, 3
    out_kin = K + CP
    links = _group_links(lib, 3, n, CP, W, False)

    def fresh():
        outs = [Out(lib, n, out_kin, W) for _ in links]
        return outs, [o.link(cap, first, stride, fd, lo) for o, (cap, first, stride, fd, lo) in zip(outs, links)]

    caps_before = [l[0].clone() for l in links]
    outs, table = fresh()
    table[1].workspace_bytes -= 1                                               # one link with a short workspace
    assert grouped_run(lib, table, outs, n, CP, W, out_kin) == WORKSPACE and all(o.untouched() for o in outs)
    outs, table = fresh()
    table[2].x_out = links[0][0].data_ptr() + 16 * 1024                         # one link's frames inside another's capture
    assert grouped_run(lib, table, outs, n, CP, W, out_kin) == INVALID and all(o.untouched() for o in outs)
    outs, table = fresh()
    table[0].cfo = None
    assert grouped_run(lib, table, outs, n, CP, W, out_kin) == INVALID and all(o.untouched() for o in outs)
    outs, table = fresh()
    table[2].n_samples = links[2][1] + n * links[2][2] + W - 1                  # the capture too short for the last window
    assert grouped_run(lib, table, outs, n, CP, W, out_kin) == INVALID and all(o.untouched() for o in outs)
    assert all(same_bits(l[0], c) for l, c in zip(links, caps_before))
    # the solo entry: a short workspace, a missing x_out
    cap, first, stride = links[0][:3]
    o = Out(lib, n, out_kin, W)
    st = lib.dccn_capture_sync_pooled(cap.data_ptr(), int(cap.shape[0]), first, None, 0, stride, n, S, K, CP, W, out_kin,
                                      o.out_buf.data_ptr(), o.off_buf.data_ptr(), o.cfo_buf.data_ptr(), o.met_buf.data_ptr(),
                                      o.ws_buf.data_ptr(), o.n_ws - 1, stream())
    torch.cuda.synchronize()
    assert st == WORKSPACE and o.untouched()
    st = lib.dccn_capture_sync_pooled(cap.data_ptr(), int(cap.shape[0]), first, None, 0, stride, n, S, K, CP, W, out_kin,
                                      None, o.off_buf.data_ptr(), o.cfo_buf.data_ptr(), o.met_buf.data_ptr(),
                                      o.ws_buf.data_ptr(), o.n_ws, stream())
    torch.cuda.synchronize()
    assert st == INVALID and o.untouched()


def test_capture_sync_classes(lib):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import CaptureSync, CaptureSyncGroup
    n, CP, W = 73, 16, 3
    _, cap, stride = dev_capture("ETU", 5.0, CP, 0, P.EPS[0], n)
    first = CR.case_first(CP, 0)
    cs = CaptureSync(S, K, CP, W, n, DEV, cfo=True, cfo_scope="capture")
    out, off = cs.run(cap, first)
    torch.cuda.synchronize()
    a = pooled_run(lib, cap, first, stride, n, CP, W)
    assert tuple(cs.cfo.shape) == (1,) and same_bits(cs.cfo, a.cfo) and torch.equal(off, a.offset) and same_bits(out, a.out)
    assert same_bits(cs.metric, a.metric)
    with pytest.raises(_lib.DccnError):
        cs.offsets(cap, first)                                                  # the pooled entry writes the frames
    g = CaptureSyncGroup(S, K, CP, W, n, 2, DEV, cfo=True, cfo_scope="capture")
    outs, offs = g.run([cap, cap], [first, torch.tensor([first], dtype=torch.int64, device=DEV)], los=[0, first - 3])
    torch.cuda.synchronize()
    for i in range(2):
        assert tuple(g.cfo[i].shape) == (1,) and same_bits(g.cfo[i], a.cfo) and torch.equal(offs[i], a.offset)
        assert same_bits(outs[i], a.out)
    # the default scope is the per-frame entry
    d = CaptureSync(S, K, CP, W, n, DEV, cfo=True)
    out_d, off_d = d.run(cap, first)
    torch.cuda.synchronize()
    b = per_frame_run(lib, cap, first, stride, n, CP, W)
    assert tuple(d.cfo.shape) == (n,) and same_bits(d.cfo, b.cfo) and same_bits(out_d, b.out) and not d.pooled


# ---- 4. the receive calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cp", [True, False])
def test_receiver_capture_pooled(cp):
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import CaptureSync
    CP, W, nbits, batch = 16, 3, 2, 73
    T = S * (K + CP)
    kin = K + CP if cp else K
    dims = RxDims(S=S, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=kin, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True, CP=CP, K=None if cp else K)
    _, cap, stride = dev_capture("ETU", 30.0, CP, 0, P.EPS[0], batch)
    with pytest.raises(ValueError):
        rcv.receive_capture(cap, T, sync=W, cfo=False, cfo_scope="capture")
    with pytest.raises(ValueError):
        rcv.receive_capture(cap, T, sync=W, cfo=True, cfo_scope="symbol")
    res = rcv.receive_capture(cap, T, sync=W, cfo=True, cfo_scope="capture")
    torch.cuda.synchronize()
    assert tuple(res.cfo.shape) == (1,) and tuple(res.offset.shape) == (batch,) and bool((res.offset != 0).any())
    got = [t.clone() for t in (res.packed, res.llr, res.prob, rcv.x, res.cfo, res.offset)]
    cs = CaptureSync(S, K, CP, W, batch, DEV, out_kin=kin, cfo=True, cfo_scope="capture")
    want_x, off = cs.run(cap, T)
    torch.cuda.synchronize()
    want_x = want_x.clone()
    assert same_bits(cs.cfo, got[4]) and torch.equal(off, got[5]) and same_bits(got[3], want_x)
    assert abs(float(got[4][0]) - P.EPS[0]) < 2e-3
    ref = rcv.receive(want_x)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
    # the start on the device; and the default scope still the per-frame call
    at = rcv.receive_capture(cap, torch.tensor([T], dtype=torch.int64, device=DEV), sync=W, cfo=True, lo=T - 4, cfo_scope="capture")
    torch.cuda.synchronize()
    assert torch.equal(at.packed, got[0]) and same_bits(at.llr, got[1]) and same_bits(at.cfo, got[4])
    frame = rcv.receive_capture(cap, T, sync=W, cfo=True)
    torch.cuda.synchronize()
    assert tuple(frame.cfo.shape) == (batch,)


class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _chain_params(i, nbits):
    from dl_ofdm_amd.ofdm import ofdm_tx
    Fl = _Flags()
    Fl.nbits, Fl.opt, Fl.init_learning, Fl.cp, Fl.longcp = nbits, 0, 1e-3, True, True
    tx = ofdm_tx(Fl)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size, pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=nbits)
    return Fl, tx, E.init_params(ecfg, seed=21 + 10 * i + nbits, bias_scale=0.05), O.init_params(rcfg, seed=22 + 10 * i + nbits)


_trainers = {}


def _trainer(i, nbits):
    if (i, nbits) not in _trainers:
        from dl_ofdm_amd.equalizer import EqualizerTrainer
        Fl, tx, pe, pr = _chain_params(i, nbits)
        tr = EqualizerTrainer(Fl, tx, pr, seed=3)
        tr.load_params(pe)
        _trainers[(i, nbits)] = tr
    return _trainers[(i, nbits)]


def test_chain_capture_pooled():
    from dl_ofdm_amd.receive import chain_receive
    from dl_ofdm_amd.sync import CaptureSync
    CP, W, B = 16, 3, 73
    T = S * (K + CP)
    tr = _trainer(0, 2)
    _, cap, stride = dev_capture("ETU", 30.0, CP, 0, P.EPS[1], B)
    with pytest.raises(ValueError):
        tr.receive_capture(cap, T, sync=W, cfo_scope="capture")
    res = tr.receive_capture(cap, T, sync=W, cfo=True, want_llr=True, want_prob=True, cfo_scope="capture")    # frames=None: 73
    torch.cuda.synchronize()
    assert tuple(res.offset.shape) == (B,) and tuple(res.cfo.shape) == (1,)
    got = [t.clone() for t in (res.packed, res.llr, res.prob, tr.resident(B).x, res.cfo, res.offset)]
    cs = CaptureSync(S, K, CP, W, B, DEV, cfo=True, cfo_scope="capture")
    want_x, off = cs.run(cap, T)
    torch.cuda.synchronize()
    want_x = want_x.clone()
    assert same_bits(cs.cfo, got[4]) and torch.equal(off, got[5]) and same_bits(got[3], want_x)
    ref = chain_receive(tr, want_x, want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)


def test_acquired_start_gives_the_true_starts_bits():
    """receive_capture(first=None, acquire=4, cfo_scope="capture") of the receiver and of the chain: the acquisition launches in
    front, the pooled cut reads the start on the device"""
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    CP, W, nbits, batch, lo = 16, 3, 2, 12, 5
    T = S * (K + CP)
    cap_np, start = A.build_capture("AWGN", None, CP, 2, 16, 211, 0.0, seed=77)
    cap = dev(apply_cfo_stream(cap_np, 0.11, K))
    true = A.true_first(start, lo, T)
    dims = RxDims(S=S, kin=K + CP, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=K + CP, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, CP=CP, pilot_sc=A.pilot_sc_of(CP))
    tr = _trainer(0, 2)
    calls = ((lambda **kw: rcv.receive_capture(cap, sync=W, cfo=True, cfo_scope="capture", **kw), lambda: rcv.x),
             (lambda **kw: tr.receive_capture(cap, sync=W, cfo=True, want_llr=True, frames=batch, cfo_scope="capture", **kw),
              lambda: tr.resident(batch).x))
    for call, x_of in calls:
        res = call(acquire=4, lo=lo)
        torch.cuda.synchronize()
        assert int(res.first[0]) == true and tuple(res.acquired_cfo.shape) == (1,) and tuple(res.cfo.shape) == (1,)
        got = [t.clone() for t in (res.packed, res.llr, res.offset, res.cfo, x_of())]
        ref = call(first=true)
        torch.cuda.synchronize()
        assert ref.first is None and ref.acquired_cfo is None
        assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and torch.equal(got[2], ref.offset)
        assert same_bits(got[3], ref.cfo) and same_bits(got[4], x_of())
        assert abs(float(got[3][0]) - 0.11) < 1e-3


def test_chain_group_capture_pooled():
    """ChainReceiveGroup.receive_capture(cfo_scope="capture") at 73 frames and mixed modulations: every chain bit for bit the solo
    chain's call (two chains share a capture; known starts on the host and on the device)"""
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    from dl_ofdm_amd.receive import group_receive_capture
    CP, W, B = 16, 3, 73
    T = S * (K + CP)
    mods = (1, 2, 3, 4)
    cs = [_chain_params(i, nb) for i, nb in enumerate(mods)]
    grp = ChainReceiveGroup([c[0] for c in cs], [c[3] for c in cs], B, want_llr=True, want_prob=True)
    for ch, c in zip(grp.chains, cs):
        ch.tr.load_params(c[2])
    caps = [dev_capture(ch, snr, CP, 0, eps0, B)[1] for (ch, snr), eps0 in
            ((CHANNELS[0], P.EPS[0]), (CHANNELS[0], P.EPS[0]), (CHANNELS[1], P.EPS[1]), (CHANNELS[2], P.EPS[0]))]
    firsts = [T, T + 1, torch.tensor([T - 1], dtype=torch.int64, device=DEV), T]
    los = [0, 0, T - 3, 0]
    with pytest.raises(ValueError):
        grp.receive_capture(caps, firsts=firsts, los=los, sync=W, cfo_scope="capture")
    for ch in grp.chains:
        ch.pl.x.fill_(SENT_X)
    res = group_receive_capture(grp, caps, firsts=firsts, los=los, sync=W, cfo=True, cfo_scope="capture")
    torch.cuda.synchronize()
    got = [dict(packed=r.packed.clone(), llr=r.llr.clone(), prob=r.prob.clone(), cfo=r.cfo.clone(), offset=r.offset.clone(),
                out_eq=ch.pl.out_eq.clone(), x=ch.pl.x.clone()) for ch, r in zip(grp.chains, res)]
    for i, nb in enumerate(mods):
        tr = _trainer(i, nb)
        ref = tr.receive_capture(caps[i], firsts[i], sync=W, cfo=True, want_llr=True, want_prob=True, frames=B, lo=los[i],
                                 cfo_scope="capture")
        torch.cuda.synchronize()
        pl = tr.resident(B)
        want = dict(packed=ref.packed, llr=ref.llr, prob=ref.prob, cfo=ref.cfo, offset=ref.offset, out_eq=pl.out_eq, x=pl.x)
        assert tuple(ref.cfo.shape) == (1,)
        for name, v in want.items():
            assert same_bits(got[i][name], v), (i, nb, name)
        assert not bool((got[i]["x"] == SENT_X).any())
