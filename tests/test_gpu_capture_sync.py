"""Frames cut from a contiguous capture on the GPU (``-m gpu``): ``dccn_capture_sync`` held

1. bit for bit to the circular kernels (``dccn_frame_sync`` / ``dccn_frame_sync_cfo``) on padded captures, where the linear
   window of a frame holds exactly what the circular estimator reads (tests/capture_sync_ref.py ``padded_capture``);
2. to the fp64 restatement of its definition on contiguous captures, with the bounds of tests/frame_sync_ref.py and
   tests/frame_cfo_ref.py (the sums have the same S CP terms, so the derivations there apply unchanged);
3. at the capture's edges (a tight capture inside a NaN-filled buffer);
4. to its refusals (nothing is launched);
5. and ``receive_capture`` of the receiver and of the chain held to the plain receive calls on the frames cut with torch."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_sync_ref as CR
import frame_cfo_ref as F
import frame_sync_ref as R
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = R.S, R.K
GUARD = 64
SENT_X, SENT_OFF, SENT_C, SENT_M = 777.0, -99, 333.0, 555.0
DEV = "cuda"
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Out:
    """guarded, sentinel-filled outputs of one call"""

    def __init__(self, n, s, out_kin, w):
        self.n, self.S, self.W, self.out_kin = n, s, w, out_kin
        self.n_out, self.n_met = n * s * out_kin * 2, n * (2 * w + 1)
        self.out_buf = torch.full((self.n_out + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.off_buf = torch.full((n + GUARD,), SENT_OFF, dtype=torch.int32, device=DEV)
        self.cfo_buf = torch.full((n + GUARD,), SENT_C, dtype=torch.float32, device=DEV)
        self.met_buf = torch.full((self.n_met + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        self.status = None

    out = property(lambda self: self.out_buf[:self.n_out].view(self.n, self.S, self.out_kin, 2))
    offset = property(lambda self: self.off_buf[:self.n])
    cfo = property(lambda self: self.cfo_buf[:self.n])
    metric = property(lambda self: self.met_buf[:self.n_met].view(self.n, 2 * self.W + 1))

    def guards_intact(self):
        return (bool((self.out_buf[self.n_out:] == SENT_X).all()) and bool((self.off_buf[self.n:] == SENT_OFF).all())
                and bool((self.cfo_buf[self.n:] == SENT_C).all()) and bool((self.met_buf[self.n_met:] == SENT_M).all()))

    def untouched(self):
        return (bool((self.out_buf == SENT_X).all()) and bool((self.off_buf == SENT_OFF).all())
                and bool((self.cfo_buf == SENT_C).all()) and bool((self.met_buf == SENT_M).all()))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def capture_run(lib, cap, first, stride, n, cp, w, out_kin=None, cfo=False, s=S, k=K, n_samples=None, cap_ptr=None, x_out=None):
    """one dccn_capture_sync call"""
    o = Out(n, s, k + cp if out_kin is None else out_kin, w)
    o.status = lib.dccn_capture_sync(cap.data_ptr() if cap_ptr is None else cap_ptr,
                                     int(cap.shape[0]) if n_samples is None else n_samples, first, stride, n, s, k, cp, w,
                                     o.out_kin, o.out_buf.data_ptr() if x_out is None else x_out, o.off_buf.data_ptr(),
                                     o.cfo_buf.data_ptr() if cfo else None, o.met_buf.data_ptr(), stream())
    torch.cuda.synchronize()
    return o


def circular_run(lib, x, cp, w, out_kin=None, cfo=False, s=S, k=K):
    """one dccn_frame_sync / dccn_frame_sync_cfo call on the same kind of outputs"""
    n = x.shape[0]
    o = Out(n, s, k + cp if out_kin is None else out_kin, w)
    head = (x.data_ptr(), n, s, k, cp, w, o.out_kin, o.out_buf.data_ptr(), o.off_buf.data_ptr())
    if cfo:
        o.status = lib.dccn_frame_sync_cfo(*head, o.cfo_buf.data_ptr(), o.met_buf.data_ptr(), stream())
    else:
        o.status = lib.dccn_frame_sync(*head, o.met_buf.data_ptr(), stream())
    torch.cuda.synchronize()
    return o


# ---- 1. bit-equal to the circular kernels on padded captures ---------------------------------------------------------------
def _padded_inputs(s, k, cp):
    xs = [("exact prefix, eps 0.23, late by 1", F.exact_prefix_frames(9, s, k, cp, seed=40 + cp, eps=0.23, roll=1)),
          ("exact prefix, eps -0.31 per frame", F.exact_prefix_frames(9, s, k, cp, seed=41 + cp, eps=np.linspace(-0.31, 0.4, 9)))]
    if (s, k) == (S, K):
        xs.append(("ETU 5 dB", R.case_frames("ETU", 5.0, cp)[:9]))
        xs.append(("ETU 5 dB with offsets", F.case_frames("ETU", 5.0, cp)[:9]))
    return xs


@pytest.mark.parametrize("s,k,cp,w", [(7, 64, 16, 3), (7, 64, 16, 16), (7, 64, 4, 3), (3, 12, 4, 2)])
def test_padded_capture_gives_the_circular_kernels_bits(lib, s, k, cp, w):
    assert lib.dccn_capture_sync_supported(s, k, cp, w) == 1
    moved = False
    for name, xs in _padded_inputs(s, k, cp):
        assert xs.dtype == np.float32
        for n in (1, 5, 9):
            x = dev(xs[:n])
            capn, first, stride = CR.padded_capture(xs[:n], w)
            # the slots start on even samples (stride = T + 2 W); one sample in front of them all puts every window on an odd one
            caps = [(dev(capn), first), (dev(np.concatenate([np.full((1, 2), 9.0, np.float32), capn])), first + 1)]
            for cfo in (False, True):
                for out_kin in (k + cp, k):
                    b = circular_run(lib, x, cp, w, out_kin=out_kin, cfo=cfo, s=s, k=k)
                    assert b.status == 0
                    for cap, at in caps:
                        assert (at - w) % 2 == (0 if cap is caps[0][0] else 1)
                        a = capture_run(lib, cap, at, stride, n, cp, w, out_kin=out_kin, cfo=cfo, s=s, k=k)
                        assert a.status == 0 and a.guards_intact()
                        assert torch.equal(a.offset, b.offset), name
                        assert same_bits(a.metric, b.metric), name
                        assert same_bits(a.out, b.out), name
                        if cfo:
                            assert same_bits(a.cfo, b.cfo), name
                        else:
                            assert bool((a.cfo_buf == SENT_C).all())
                        moved = moved or bool((a.offset != 0).any())
    assert moved


# ---- 2. against fp64 on contiguous captures --------------------------------------------------------------------------------
def frame_peak(x):
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2).reshape(x.shape[0], -1).max(axis=1)


@pytest.mark.parametrize("CP,W,channel,snr", CR.CASES)
def test_contiguous_capture_against_fp64(lib, CP, W, channel, snr):
    n, T = CR.FRAMES, S * (K + CP)
    for spare, shift in CR.LAYOUTS:
        first = CR.case_first(CP, shift)
        # the plain launch: estimate against fp64, the output the capture's own bits
        capn, stride = CR.case_capture(channel, snr, CP, spare)
        off64, lam64, phi64, gam64, ok = CR.case_reference(channel, snr, CP, W, spare, shift)
        cap = dev(capn)
        r = capture_run(lib, cap, first, stride, n, CP, W)
        assert r.status == 0 and r.guards_intact()
        off = r.offset.cpu().numpy().astype(np.int64)
        lam = r.metric.cpu().numpy().astype(np.float64)
        wrong = int((off[ok] != off64[ok]).sum())
        m_ratio = float((np.abs(lam - lam64).max(axis=1) / (R.METRIC_TOL * phi64.max(axis=1))).max())
        assert (~ok).sum() <= R.CAP * n
        assert (off >= -W).all() and (off <= W).all()
        want = dev(CR.cut(capn, first, stride, off, S, K, CP))
        crop = capture_run(lib, cap, first, stride, n, CP, W, out_kin=K)
        assert crop.status == 0 and crop.guards_intact() and torch.equal(crop.offset, r.offset) and same_bits(crop.metric, r.metric)
        # the CFO launch on the impaired capture: estimate and derotation against fp64
        capn_c, _ = CR.case_capture(channel, snr, CP, spare, cfo=True)
        offc64, lamc64, phic64, gamc64, okc = CR.case_reference(channel, snr, CP, W, spare, shift, cfo=True)
        cap_c = dev(capn_c)
        c = capture_run(lib, cap_c, first, stride, n, CP, W, cfo=True)
        plain_c = capture_run(lib, cap_c, first, stride, n, CP, W)
        assert c.status == 0 and c.guards_intact() and plain_c.status == 0
        offc = c.offset.cpu().numpy().astype(np.int64)
        est = c.cfo.cpu().numpy().astype(np.float64)
        g = CR.gamma_at(gamc64, offc64, W)
        c_ratio = float((F.circle(est - F.cfo_of(g)) / F.cfo_bound(phic64, g))[okc].max())
        wrong_c = int((offc[okc] != offc64[okc]).sum())
        mc_ratio = float((np.abs(c.metric.cpu().numpy().astype(np.float64) - lamc64).max(axis=1)
                          / (R.METRIC_TOL * phic64.max(axis=1))).max())
        want64 = CR.derotated(capn_c, first, stride, offc, est, S, K, CP)
        peak = frame_peak(CR.cut(capn_c, first, stride, offc, S, K, CP))
        d = c.out.cpu().numpy().astype(np.float64) - want64
        d_ratio = float((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).reshape(n, -1).max(axis=1) / (F.DEROT_TOL * peak)).max())
        cc = capture_run(lib, cap_c, first, stride, n, CP, W, out_kin=K, cfo=True)
        print("%s %g dB CP %d W %d stride T+%d first T+%d: undecidable %d / %d (cfo capture), offsets differ on the rest %d / %d, "
              "max |dLambda| / bound %.3g / %.3g, max |cfo - cfo64| / bound %.3g, max |out - out64| / bound %.3g"
              % (channel, snr, CP, W, spare, shift, int((~ok).sum()), int((~okc).sum()), wrong, wrong_c, m_ratio, mc_ratio,
                 c_ratio, d_ratio))
        assert wrong == 0 and wrong_c == 0
        assert m_ratio <= 1.0 and mc_ratio <= 1.0
        assert same_bits(r.out, want)                                                     # the capture's own bits
        assert same_bits(crop.out, want[:, :, CP:].contiguous())
        assert (~okc).sum() <= R.CAP * n
        assert torch.equal(c.offset, plain_c.offset) and same_bits(c.metric, plain_c.metric)     # (the timing side is the same)
        assert np.isfinite(est).all() and (np.abs(est) <= 0.5).all()
        assert c_ratio <= 1.0
        assert d_ratio <= 1.0
        assert cc.status == 0 and cc.guards_intact() and same_bits(cc.cfo, c.cfo) and torch.equal(cc.offset, c.offset)
        assert same_bits(cc.out, c.out[:, :, CP:].contiguous())


# ---- 3. edges: a tight capture inside a NaN-filled buffer --------------------------------------------------------------------
@pytest.mark.parametrize("CP,W,spare,n,lead", [(16, 3, 1, 6, 2), (16, 16, 0, 5, 6), (4, 3, 1, 9, 2), (4, 4, 1, 6, 10)])
def test_tight_capture_in_a_nan_buffer(lib, CP, W, spare, n, lead):
    """first = W and n_samples = first + (n - 1) stride + T + W exactly, the capture ``lead`` samples into a NaN buffer (an even
    count: the capture's base stays on a 16-byte boundary).  With stride = T + 1 every other window starts on an odd sample, and
    with n even the last window ends one sample short of a pair that straddles the capture's end."""
    T = S * (K + CP)
    stride = T + spare
    rs = np.random.RandomState(17 * CP + W)
    xs = F.case_frames("ETU", 5.0, CP)[:n]
    body, _ = CR.contiguous_capture(xs, spare)
    n_samples = W + (n - 1) * stride + T + W
    tight = np.concatenate([rs.standard_normal((W, 2)).astype(np.float32), body[:(n - 1) * stride + T],
                            rs.standard_normal((W, 2)).astype(np.float32)])
    assert tight.shape[0] == n_samples
    buf = torch.full((lead + n_samples + 7, 2), float("nan"), dtype=torch.float32, device=DEV)
    cap = buf[lead:lead + n_samples]
    cap.copy_(dev(tight))
    assert cap.data_ptr() % 16 == 0 and cap.is_contiguous()
    pad = rs.standard_normal((T + 5, 2)).astype(np.float32)
    roomy = dev(np.concatenate([pad, tight, pad]))
    for cfo in (False, True):
        for out_kin in (K + CP, K):
            a = capture_run(lib, cap, W, stride, n, CP, W, out_kin=out_kin, cfo=cfo)
            b = capture_run(lib, roomy, W + T + 5, stride, n, CP, W, out_kin=out_kin, cfo=cfo)
            assert a.status == 0 and b.status == 0 and a.guards_intact()
            assert bool(torch.isfinite(a.out).all()) and bool(torch.isfinite(a.metric).all())
            assert torch.equal(a.offset, b.offset) and same_bits(a.metric, b.metric) and same_bits(a.out, b.out)
            if cfo:
                assert bool(torch.isfinite(a.cfo).all()) and same_bits(a.cfo, b.cfo)
    # one sample less and the call is refused
    short = capture_run(lib, cap, W, stride, n, CP, W, n_samples=n_samples - 1)
    assert short.status == INVALID and short.untouched()
    assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n_samples:]).all())


# ---- 4. refusals launch nothing ------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing(lib):
    CP, W, n = 16, 3, 9
    T = S * (K + CP)
    capn, stride = CR.contiguous_capture(R.case_frames("EVA", 30.0, CP)[:n + 2])
    cap = dev(capn)
    ns = int(cap.shape[0])
    ok = capture_run(lib, cap, T, stride, n, CP, W)
    assert ok.status == 0

    def refused(**kw):
        a = dict(first=T, stride=stride, n=n, cp=CP, w=W)
        a.update(kw)
        r = capture_run(lib, cap, a.pop("first"), a.pop("stride"), a.pop("n"), a.pop("cp"), a.pop("w"), **a)
        assert r.status == INVALID, kw
        assert r.untouched(), kw

    refused(stride=T - 1)
    refused(first=W - 1, cfo=True)
    refused(first=T, n_samples=T + (n - 1) * stride + T + W - 1)             # the last window past n_samples
    refused(first=ns - (n - 1) * stride - T - W + 1)
    refused(w=CP + 1)
    refused(out_kin=K + 1)
    refused(out_kin=K - 1, cfo=True)
    refused(cap_ptr=cap.data_ptr() + 8, n_samples=ns - 1)                    # a misaligned capture
    refused(n=0)
    refused(first=T, stride=1 << 62)                                         # (no overflow on the way to the refusal)
    refused(first=1 << 62)
    # cap overlapping x_out: the output placed inside the capture
    refused(x_out=cap.data_ptr() + 16 * T)
    refused(x_out=cap.data_ptr() + 8 * ns - 16, cfo=True)
    # a shape dccn_frame_sync takes and the capture stage does not (four windows of T + 2 W + 2 samples pass 64 KB)
    assert lib.dccn_frame_sync_supported(24, 64, 16, 1) == 1 and lib.dccn_capture_sync_supported(24, 64, 16, 1) == 0
    big = torch.zeros(3 * 24 * 80, 2, dtype=torch.float32, device=DEV)
    r = capture_run(lib, big, 24 * 80, 24 * 80, 1, 16, 1, s=24, k=64)
    assert r.status == INVALID and r.untouched()
    assert lib.dccn_capture_sync_supported(7, 64, 40, 13) == 0 and lib.dccn_capture_sync_supported(7, 64, 16, 17) == 0
    assert lib.dccn_capture_sync_supported(7, 63, 16, 3) == 0                # an odd frame length


def test_capture_sync_class_refusals():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import CaptureSync
    CP, W, n = 16, 3, 9
    T = S * (K + CP)
    capn, stride = CR.contiguous_capture(R.case_frames("EVA", 30.0, CP)[:n + 2])
    cs = CaptureSync(S, K, CP, W, n, DEV)
    with pytest.raises(_lib.DccnError):
        cs.run(capn, T)                                                      # a host array: no CPU fallback
    with pytest.raises(_lib.DccnError):
        cs.run(dev(capn).double(), T)
    with pytest.raises(_lib.DccnError):
        cs.run(dev(capn).view(-1, 4), T)
    with pytest.raises(_lib.DccnError):
        cs.run(dev(capn), 2)                                                 # first < W
    with pytest.raises(_lib.DccnError):
        cs.run(dev(capn), T, out=torch.empty(n, S, K, 2, device=DEV))
    with pytest.raises(_lib.DccnError):
        CaptureSync(S, K, CP, CP + 1, n, DEV)
    with pytest.raises(_lib.DccnError):
        CaptureSync(S, K, CP, W, n, "cpu")
    # stride=None is T; offsets() writes no frame
    cap = dev(capn)
    out, off = cs.run(cap, T)
    torch.cuda.synchronize()
    off1, out1, met1 = off.clone(), out.clone(), cs.metric.clone()
    assert torch.equal(cs.offsets(cap, T, stride), off1) and same_bits(cs.metric, met1) and same_bits(cs.out, out1)
    assert out.shape == (n, S, K + CP, 2) and off.dtype == torch.int32 and cs.cfo is None


# ---- 5. the receive calls ------------------------------------------------------------------------------------------------------
def gather_frames(cap: torch.Tensor, first, stride, off: torch.Tensor, T):
    """x_cut[f] = cap[b_f + off_f : b_f + off_f + T], with torch"""
    n = off.shape[0]
    b = first + stride * torch.arange(n, device=cap.device, dtype=torch.int64) + off.to(torch.int64)
    idx = b[:, None] + torch.arange(T, device=cap.device, dtype=torch.int64)[None, :]
    return cap[idx]                                                          # [n, T, 2]


@pytest.mark.parametrize("cp", [True, False])
@pytest.mark.parametrize("batch", [12, 73])
def test_receiver_capture_equals_receive_of_the_cut_frames(cp, batch):
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import CaptureSync
    CP, W, nbits = 16, 3, 2
    T = S * (K + CP)
    kin = K + CP if cp else K
    dims = RxDims(S=S, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=kin, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True, CP=CP, K=None if cp else K)
    for impaired in (False, True):
        capn, stride = CR.case_capture("ETU", 30.0, CP, 0, cfo=impaired)
        cap = dev(capn)
        cap0 = cap.clone()
        res = rcv.receive_capture(cap, T, sync=W, cfo=impaired)
        torch.cuda.synchronize()
        assert res.offset.dtype == torch.int32 and tuple(res.offset.shape) == (batch,) and (res.cfo is not None) == impaired
        off = res.offset.clone()
        got = [t.clone() for t in (res.packed, res.llr, res.prob, rcv.x)]
        est = res.cfo.clone() if impaired else None
        again = rcv.receive_capture(cap, T, stride, sync=W, cfo=impaired)       # (stride=None is T)
        torch.cuda.synchronize()
        assert torch.equal(again.offset, off) and torch.equal(again.packed, got[0]) and same_bits(again.llr, got[1])
        assert same_bits(again.prob, got[2]) and same_bits(rcv.x, got[3]) and same_bits(cap, cap0)
        assert bool((off != 0).any())
        if impaired:
            cs = CaptureSync(S, K, CP, W, batch, DEV, out_kin=kin, cfo=True)
            want_x, off_cs = cs.run(cap, T)
            torch.cuda.synchronize()
            assert torch.equal(off_cs, off) and same_bits(cs.cfo, est)
            want_x = want_x.clone()
        else:
            want_x = gather_frames(cap, T, stride, off, T).view(batch, S, K + CP, 2)
            want_x = want_x if cp else want_x[:, :, CP:].contiguous()
        ref = rcv.receive(want_x)
        torch.cuda.synchronize()
        assert ref.offset is None and ref.cfo is None
        assert same_bits(got[3], want_x)
        assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)


def test_receiver_capture_refusals():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    p = O.init_params(O.RxConfig(S=S, kin=80, F=64, D=320, nbits=2), seed=3)
    capn, _ = CR.case_capture("ETU", 30.0, 16, 0)
    cap = dev(capn)
    rcv = RxReceiver(RxDims(S=S, kin=80, F=64, D=320, nbits=2), 8, p)          # no CP given
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, 560, sync=3)
    rcv = RxReceiver(RxDims(S=S, kin=80, F=64, D=320, nbits=2), 8, p, CP=16)
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, 560, sync=0)
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(capn, 560, sync=3)                                # a host array
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, 560, sync=17)
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, 1, sync=3)


class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer(nbits, seed=21):
    """the chain of tests/test_gpu_receive.py, re-stated"""
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    Fl = _Flags()
    Fl.nbits, Fl.opt, Fl.init_learning, Fl.cp = nbits, 0, 1e-3, True
    tx = ofdm_tx(Fl)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size,
                      pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=nbits)
    tr = EqualizerTrainer(Fl, tx, O.init_params(rcfg, seed=seed + 1), seed=3)
    tr.load_params(E.init_params(ecfg, seed=seed, bias_scale=0.05))
    return tx, tr


@pytest.mark.parametrize("B", [12, 73])
def test_chain_capture_equals_chain_receive_of_the_cut_frames(B):
    from dl_ofdm_amd.receive import chain_receive
    from dl_ofdm_amd.sync import CaptureSync
    CP, W = 16, 3
    T = S * (K + CP)
    tx, tr = _trainer(2)
    for impaired in (False, True):
        capn, stride = CR.case_capture("ETU", 30.0, CP, 0, cfo=impaired)
        cap = dev(capn)
        # 73 = every frame whose window lies inside the 75-frame capture from first = T on; 12 is asked for
        res = tr.receive_capture(cap, T, sync=W, cfo=impaired, want_llr=True, want_prob=True, frames=None if B == 73 else B)
        torch.cuda.synchronize()
        assert tuple(res.offset.shape) == (B,) and (res.cfo is not None) == impaired
        off = res.offset.clone()
        got = [t.clone() for t in (res.packed, res.llr, res.prob, tr.resident(B).x)]
        again = tr.receive_capture(cap, T, stride, sync=W, cfo=impaired, want_llr=True, want_prob=True, frames=B)
        torch.cuda.synchronize()
        assert torch.equal(again.offset, off) and torch.equal(again.packed, got[0]) and same_bits(again.llr, got[1])
        assert same_bits(again.prob, got[2])
        if impaired:
            cs = CaptureSync(S, K, CP, W, B, DEV, cfo=True)
            want_x, off_cs = cs.run(cap, T)
            torch.cuda.synchronize()
            assert torch.equal(off_cs, off) and same_bits(cs.cfo, res.cfo)
            want_x = want_x.clone()
        else:
            want_x = gather_frames(cap, T, stride, off, T).view(B, S, K + CP, 2)
        ref = chain_receive(tr, want_x, want_llr=True, want_prob=True)
        torch.cuda.synchronize()
        assert same_bits(got[3], want_x) and bool((off != 0).any())
        assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
