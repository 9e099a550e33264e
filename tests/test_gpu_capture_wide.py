"""Carrier offsets beyond half a subcarrier spacing on the GPU (``-m gpu``):

1. ``dccn_capture_acquire_wide`` held to ``dccn_capture_acquire`` bit for bit where the two must agree (everything at M = 0;
   ``sym_metric``, ``cfo_out`` and column m = 0 of ``phase_metric`` at any M), to the fp64 restatement of its definition
   (tests/capture_wide_ref.py, stage B evaluated at the GPU's own r^ and eps^) within the bounds derived there, (q^, m^) and
   ``first`` exact on every decidable case, and two runs to the same bits; a synthetic K = 16 frame whose shifted bins wrap;
2. ``dccn_capture_sync_wide`` / ``dccn_capture_sync_pooled_wide`` at 1, 3, 5 and 73 frames: with the pair (0, 0) bit for bit
   ``dccn_capture_sync_at`` (cfo) / ``dccn_capture_sync_pooled``; totals and frames held to fp64 on the GPU's own offsets; wild
   device values leave finite output inside a NaN-padded buffer;
3. ``receive_capture(first=None, acquire=16, cfo=True, cfo_span=7)`` of the receiver and of the chain bit for bit the stage
   objects called one after another; groups and the missing ``acquire`` raise."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A
import capture_pool_ref as P
import capture_wide_ref as Wd
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = Wd.S, Wd.K
DEV = "cuda"
GUARD = 64
SENT = 777.0
INVALID = -1
_tally = {"cases": 0, "skipped": 0}


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Acq:
    """guarded, sentinel-filled outputs of one dccn_capture_acquire_wide call (M = None: dccn_capture_acquire)"""

    def __init__(self, lib, cap, lo, J, CP, sc, M, S_=S, K_=K):
        N = K_ + CP
        self.N, self.cols, self.S = N, 1 if M is None else 2 * M + 1, S_
        self.first_buf = torch.full((1 + GUARD,), -99, dtype=torch.int64, device=DEV)
        self.cfo_buf = torch.full((1 + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.int_buf = torch.full((1 + GUARD,), -99, dtype=torch.int32, device=DEV)
        self.sym_buf = torch.full((N + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.ph_buf = torch.full((S_ * self.cols + GUARD,), SENT, dtype=torch.float32, device=DEV)
        n_pilot = int(sc.numel())
        if M is None:
            nws = lib.dccn_capture_acquire_workspace_size(S_, K_, CP, n_pilot, J)
        else:
            nws = lib.dccn_capture_acquire_wide_workspace_size(S_, K_, CP, n_pilot, J, M)
        self.nws = nws
        self.ws = torch.zeros(nws + GUARD, dtype=torch.uint8, device=DEV)
        head = (cap.data_ptr(), int(cap.shape[0]), lo, J, S_, K_, CP, sc.data_ptr(), n_pilot)
        tail = (self.sym_buf.data_ptr(), self.ph_buf.data_ptr(), self.ws.data_ptr(), nws, stream())
        if M is None:
            self.status = lib.dccn_capture_acquire(*head, self.first_buf.data_ptr(), self.cfo_buf.data_ptr(), *tail)
        else:
            self.status = lib.dccn_capture_acquire_wide(*head, M, self.first_buf.data_ptr(), self.cfo_buf.data_ptr(),
                                                        self.int_buf.data_ptr(), *tail)
        torch.cuda.synchronize()

    first = property(lambda self: int(self.first_buf[0]))
    cfo = property(lambda self: float(self.cfo_buf[0]))
    m = property(lambda self: int(self.int_buf[0]))
    sym = property(lambda self: self.sym_buf[:self.N])
    phase = property(lambda self: self.ph_buf[:self.S * self.cols].view(self.S, self.cols))

    def guards_intact(self):
        return (bool((self.first_buf[1:] == -99).all()) and bool((self.cfo_buf[1:] == SENT).all())
                and bool((self.int_buf[1:] == -99).all()) and bool((self.sym_buf[self.N:] == SENT).all())
                and bool((self.ph_buf[self.S * self.cols:] == SENT).all()) and bool((self.ws[self.nws:] == 0).all()))


# ---- 1. acquisition ----------------------------------------------------------------------------------------------------------------
def check_wide(lib, cap_np, cap, sc_np, sc, lo, J, CP, M, ref, narrow, S_=S, K_=K):
    """one wide call held to the narrow call's bits and to the reference; -> (decidable, ratios)"""
    N = K_ + CP
    a = Acq(lib, cap, lo, J, CP, sc, M, S_, K_)
    assert a.status == 0 and a.guards_intact()
    b = Acq(lib, cap, lo, J, CP, sc, M, S_, K_)
    assert b.first == a.first and b.m == a.m and same_bits(a.cfo_buf, b.cfo_buf) and same_bits(a.sym_buf, b.sym_buf)
    assert same_bits(a.ph_buf, b.ph_buf)                                     # two runs, the same bits
    # the anchors: stage A and column m = 0 are the narrow call's bits; at M = 0 so is everything
    assert same_bits(a.cfo_buf, narrow.cfo_buf) and same_bits(a.sym_buf, narrow.sym_buf)
    assert same_bits(a.phase[:, M].contiguous(), narrow.phase[:, 0].contiguous())
    if M == 0:
        assert a.first == narrow.first and a.m == 0 and same_bits(a.ph_buf, narrow.ph_buf)
    lam = a.sym.cpu().numpy().astype(np.float64)
    m_ratio = float(np.abs(lam - ref["lam"]).max() / (A.lambda_tol(J, S_, CP) * ref["phi"].max()))
    assert lo <= a.first < lo + S_ * N and -M <= a.m <= M
    rhat, qhat = (a.first - lo) % N, (a.first - lo) // N
    assert rhat == int(np.argmax(lam))
    est = np.float64(np.float32(a.cfo))
    assert abs(est) <= 0.5
    # stage B at the GPU's own r^ and eps^
    D, bound = Wd.stage_b_wide(cap_np, lo, rhat, float(est), J, S_, K_, CP, sc_np, M)
    ph = a.phase.cpu().numpy().astype(np.float64)
    d_ratio = float((np.abs(ph - D) / bound).max())
    print("CP %d J %d lo %d M %d: |dLambda| / bound %.3g, |dD| / bound %.3g, first %d m^ %d" % (CP, J, lo, M, m_ratio, d_ratio,
                                                                                                a.first, a.m))
    assert (qhat, a.m + M) == Wd.decide(ph)                                  # the kernel's first maximum of its own metric
    assert m_ratio <= 1.0 and d_ratio <= 1.0, (m_ratio, d_ratio)
    ok = ref["a_ok"] and Wd.b_decidable(D, bound)
    if ref["a_ok"]:
        assert rhat == ref["r"]
    if ok:
        q64, mi64 = Wd.decide(D)
        assert (qhat, a.m) == (q64, mi64 - M) and a.first == lo + ref["r"] + q64 * N
    return ok, (m_ratio, d_ratio)


@pytest.mark.parametrize("J", Wd.JS)
@pytest.mark.parametrize("CP", [16, 4])
def test_acquire_wide_against_narrow_and_fp64(lib, CP, J):
    sc_np = A.pilot_sc_of(CP)
    sc = dev(sc_np)
    worst = np.zeros(2)
    for case in [c for c in Wd.gpu_cases() if c[0] == CP and c[1] == J]:
        _, _, lo, ch, snr, eps, M = case
        assert lib.dccn_capture_acquire_wide_supported(S, K, CP, 16, J, M) == 1
        cap_np, _, _ = Wd.case_capture(CP, ch, snr, eps)
        cap = dev(cap_np)
        narrow = Acq(lib, cap, lo, J, CP, sc, None)
        assert narrow.status == 0
        ok, ratios = check_wide(lib, cap_np, cap, sc_np, sc, lo, J, CP, M, Wd.case_stage_a(*case[:6]), narrow)
        worst = np.maximum(worst, ratios)
        _tally["cases"] += 1
        _tally["skipped"] += not ok
    print("CP %d J %d: worst |dLambda| / bound %.3g, |dD| / bound %.3g" % (CP, J, worst[0], worst[1]))


def test_undecidable_share():
    """(after the cases above: what they skipped as undecidable stays under the cap)"""
    print("%d of %d cases undecidable" % (_tally["skipped"], _tally["cases"]))
    assert _tally["cases"] == len(Wd.gpu_cases())
    assert _tally["skipped"] <= Wd.CAP * _tally["cases"]


def test_synthetic_frame_whose_bins_wrap(lib):
    S_, K_, CP, M = (Wd.SYN[k] for k in ("S", "K", "CP", "M"))
    T = S_ * (K_ + CP)
    sc_np = Wd.synthetic_pilot_sc()
    sc = dev(sc_np)
    assert lib.dccn_capture_acquire_wide_supported(S_, K_, CP, 6, 8, M) == 1
    for seed, eps, cut, lo in ((1, 6.3, 17, 3), (2, -7.45, 40, 10)):
        cap_np, start = Wd.synthetic_capture(14, cut, eps, seed)
        cap = dev(cap_np)
        ref = Wd.reference(cap_np, lo, 8, S_, K_, CP, sc_np, M)
        narrow = Acq(lib, cap, lo, 8, CP, sc, None, S_, K_)
        ok, _ = check_wide(lib, cap_np, cap, sc_np, sc, lo, 8, CP, M, ref, narrow, S_, K_)
        assert ok
        a = Acq(lib, cap, lo, 8, CP, sc, M, S_, K_)
        assert a.first == A.true_first(start, lo, T) and a.m == int(np.rint(eps - a.cfo))


def test_wild_pilot_cells_and_refusals(lib):
    CP, J, lo, M = 16, 2, 37, 7
    cap_np, _, _ = Wd.case_capture(CP, "AWGN", 30.0, 2.49)
    cap = dev(cap_np)
    sc_np = A.pilot_sc_of(CP)
    a = Acq(lib, cap, lo, J, CP, dev(sc_np), M)
    wild = np.concatenate([[-5], sc_np, [S * K + 7, 1 << 30]]).astype(np.int32)
    b = Acq(lib, cap, lo, J, CP, dev(wild), M)
    assert a.status == 0 and b.status == 0 and b.guards_intact()
    assert a.first == b.first and a.m == b.m and same_bits(a.ph_buf, b.ph_buf) and same_bits(a.sym_buf, b.sym_buf)
    r = Acq(lib, cap, int(cap.shape[0]) - (J + 2) * S * (K + CP) + 1, J, CP, dev(sc_np), M)
    assert r.status == INVALID and bool((r.first_buf == -99).all()) and bool((r.int_buf == -99).all())
    assert bool((r.ph_buf == SENT).all()) and bool((r.ws == 0).all())


# ---- 2. the cuts --------------------------------------------------------------------------------------------------------------------
class Cut:
    """NaN-padded outputs of one cut"""

    def __init__(self, n, out_kin, W, pooled):
        self.n, self.rows = n, S * out_kin * 2
        self.out_buf = torch.full((n * self.rows + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.out = self.out_buf[:n * self.rows].view(n, S, out_kin, 2)
        self.offset = torch.full((n,), -99, dtype=torch.int32, device=DEV)
        self.ncfo = 1 if pooled else n
        self.cfo_buf = torch.full((self.ncfo + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.cfo = self.cfo_buf[:self.ncfo]
        self.metric = torch.full((n, 2 * W + 1), SENT, dtype=torch.float32, device=DEV)

    def same(self, o):
        return (same_bits(self.out, o.out) and torch.equal(self.offset, o.offset) and same_bits(self.cfo, o.cfo)
                and same_bits(self.metric, o.metric))

    def padding_intact(self):
        return bool(torch.isnan(self.out_buf[self.n * self.rows:]).all()) and bool(torch.isnan(self.cfo_buf[self.ncfo:]).all())


def run_cut(lib, cap, first_dev, lo, n, CP, W, out_kin, pooled, pair):
    """pair None: dccn_capture_sync_at (cfo) / dccn_capture_sync_pooled; else the wide entries with (cfo_int, cfo_frac)"""
    T = S * (K + CP)
    c = Cut(n, out_kin, W, pooled)
    ns = int(cap.shape[0])
    shape = (T, n, S, K, CP, W, out_kin, c.out.data_ptr(), c.offset.data_ptr(), c.cfo.data_ptr(), c.metric.data_ptr())
    extra = () if pair is None else (pair[0].data_ptr(), pair[1].data_ptr())
    if pooled:
        size = lib.dccn_capture_sync_pooled_workspace_size if pair is None else lib.dccn_capture_sync_pooled_wide_workspace_size
        ws = torch.zeros(int(size(n)), dtype=torch.uint8, device=DEV)
        fn = lib.dccn_capture_sync_pooled if pair is None else lib.dccn_capture_sync_pooled_wide
        st = fn(cap.data_ptr(), ns, 0, first_dev.data_ptr(), lo, *shape, *extra, ws.data_ptr(), int(ws.numel()), stream())
    else:
        fn = lib.dccn_capture_sync_at if pair is None else lib.dccn_capture_sync_wide
        st = fn(cap.data_ptr(), ns, first_dev.data_ptr(), lo, *shape, *extra, stream())
    torch.cuda.synchronize()
    assert st == 0
    return c


def _pair(m, frac):
    return (torch.tensor([m], dtype=torch.int32, device=DEV), torch.tensor([frac], dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("CP,W", [(16, 3), (4, 4)])
def test_cut_with_a_zero_pair_is_the_existing_cut(lib, CP, W, pooled):
    T = S * (K + CP)
    cap_np, stride = P.case_capture("ETU", 5.0, CP, 0, 0.137)
    cap = dev(cap_np)
    for n in (1, 3, 5, 73):
        for lo in (T - 6, T - 5):                                            # (lo <= T - W + 1: 73 frames fit from every start)
            first_dev = torch.tensor([T + lo % 2], dtype=torch.int64, device=DEV)             # both window parities
            for out_kin in (K + CP, K):
                a = run_cut(lib, cap, first_dev, lo, n, CP, W, out_kin, pooled, _pair(0, 0.0))
                b = run_cut(lib, cap, first_dev, lo, n, CP, W, out_kin, pooled, None)
                assert a.same(b), (n, lo, out_kin)
                assert a.padding_intact() and bool(torch.isfinite(a.out).all()) and bool((a.offset != -99).all())


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("CP,W", [(16, 3), (4, 4)])
def test_cut_totals_and_frames_against_fp64(lib, CP, W, pooled):
    T = S * (K + CP)
    worst = 0.0
    for eps, m_acq, frac_acq in ((2.49, 2, 0.49), (-3.51, -4, 0.49), (7.45, 7, 0.45), (-31.45, -31, -0.45), (0.2, 0, 0.2)):
        cap_np, stride = P.case_capture("ETU", 5.0, CP, 0, eps)
        cap = dev(cap_np)
        for n, lo in ((1, T - 5), (3, T - 6), (5, T - 5), (73, T - 6)):
            first = T + (n > 3)                                              # both window parities
            first_dev = torch.tensor([first], dtype=torch.int64, device=DEV)
            pair = _pair(m_acq, frac_acq)
            a = run_cut(lib, cap, first_dev, lo, n, CP, W, K + CP, pooled, pair)
            b = run_cut(lib, cap, first_dev, lo, n, CP, W, K + CP, pooled, _pair(0, 0.0))     # the narrow call's bits
            assert a.padding_intact() and torch.equal(a.offset, b.offset) and same_bits(a.metric, b.metric)
            a2 = run_cut(lib, cap, first_dev, lo, n, CP, W, K + CP, pooled, pair)
            assert a.same(a2)                                                # two runs, the same bits
            off = a.offset.cpu().numpy().astype(np.int64)
            # the fraction the prefix gave: the narrow call's estimate, where |.| <= 1/2 the unwrap left it alone
            frac = b.cfo.cpu().numpy().astype(np.float64)
            assert (np.abs(frac) <= 0.5).all()
            I, ok = Wd.unwrap(m_acq, np.float32(frac_acq), frac, K)
            tot = a.cfo.cpu().numpy().astype(np.float64)
            assert (np.abs(tot - (I + frac))[ok] <= Wd.total_bound(I)[ok]).all(), (eps, n)
            assert ok.mean() >= 0.9
            # the frames, against fp64 on the GPU's own offsets, fraction and integer (I read off the GPU's total)
            I_gpu = np.rint(tot - frac).astype(np.int64)
            assert (I_gpu[ok] == I[ok]).all() and (np.abs(I_gpu) <= K // 2).all()
            total = (I_gpu + frac) if not pooled else np.full(n, I_gpu[0] + frac[0])
            want = Wd.derotated(cap_np, first, T, off, total, S, K, CP)
            got = a.out.cpu().numpy().astype(np.float64)
            amp = np.abs(want[..., 0] + 1j * want[..., 1]).reshape(n, -1).max(axis=1)
            err = np.abs(got - want).reshape(n, -1).max(axis=1) / amp
            worst = max(worst, float(err.max() / Wd.DEROT_TOL))
            assert (err <= Wd.DEROT_TOL).all(), (eps, n, float(err.max()))
            # every total lies within half a spacing of the acquired offset, which is the one the capture carries
            assert (np.abs(tot - (m_acq + frac_acq))[ok] <= 0.5 + 1e-5).all() and abs(m_acq + frac_acq - eps) < 1e-6
    print("CP %d W %d pooled %s: worst |out - out64| / (DEROT_TOL max|y|) %.3g" % (CP, W, pooled, worst))


@pytest.mark.parametrize("pooled", [False, True])
def test_wild_device_values_stay_inside(lib, pooled):
    CP, W, n = 16, 3, 5
    T = S * (K + CP)
    cap_np, _ = P.case_capture("ETU", 5.0, CP, 0, 0.137)
    cap = dev(cap_np)
    lo = T - 5
    ref = run_cut(lib, cap, torch.tensor([lo], dtype=torch.int64, device=DEV), lo, n, CP, W, K + CP, pooled, _pair(0, 0.0))
    for m, frac, first in ((10 ** 9, 0.0, lo), (-10 ** 9, 0.3, lo), (0, float("nan"), lo), (3, float("inf"), lo),
                           (2, 0.1, -(1 << 40)), (2, 0.1, 1 << 40)):
        first_dev = torch.tensor([first], dtype=torch.int64, device=DEV)
        a = run_cut(lib, cap, first_dev, lo, n, CP, W, K + CP, pooled, _pair(m, frac))
        assert a.padding_intact() and bool(torch.isfinite(a.out).all()) and bool(torch.isfinite(a.cfo).all()), (m, frac, first)
        assert bool((a.cfo.abs() <= K // 2 + 0.5).all()) and bool((a.offset.abs() <= W).all())
        if first == lo:
            assert torch.equal(a.offset, ref.offset) and same_bits(a.metric, ref.metric)


# ---- 3. the receive calls ------------------------------------------------------------------------------------------------------------
def _offset_capture(CP, eps):
    """12 QPSK frames to receive and room to acquire 16: the capture begins 211 samples into frame 0, AWGN 30 dB"""
    return A.build_capture("AWGN", 30.0, CP, 2, 32, 211, eps, seed=78)


@pytest.mark.parametrize("cfo_scope", ["frame", "capture"])
def test_receiver_span_is_the_stages_one_after_another(cfo_scope):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureSync
    CP, W, nbits, batch, lo, M, J = 16, 3, 2, 12, 5, 7, 16
    T = S * (K + CP)
    dims = RxDims(S=S, kin=K + CP, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=K + CP, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, CP=CP, pilot_sc=A.pilot_sc_of(CP))
    cap_np, start = _offset_capture(CP, -5.37)
    cap = dev(cap_np)
    res = rcv.receive_capture(cap, sync=W, cfo=True, acquire=J, lo=lo, cfo_scope=cfo_scope, cfo_span=M)
    torch.cuda.synchronize()
    assert int(res.first[0]) == A.true_first(start, lo, T) and int(res.acquired_cfo_int[0]) == -5
    assert res.acquired_cfo_int.dtype == torch.int32 and abs(float(res.acquired_cfo[0]) + 0.37) < 0.02
    assert tuple(res.cfo.shape) == ((1,) if cfo_scope == "capture" else (batch,)) and bool(((res.cfo + 5.37).abs() < 0.05).all())
    got = [t.clone() for t in (res.packed, res.llr, res.offset, res.cfo, rcv.x)]
    # the stage objects, one after another
    acq = CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), J, DEV, cfo_span=M)
    cs = CaptureSync(S, K, CP, W, batch, DEV, want_metric=False, cfo=True, cfo_scope=cfo_scope, cfo_span=M)
    first = acq.run(cap, lo)
    out, off = cs.run(cap, first, lo=lo, acquired=(acq.cfo_int, acq.cfo))
    torch.cuda.synchronize()
    assert torch.equal(first, res.first) and torch.equal(acq.cfo_int, res.acquired_cfo_int) and same_bits(acq.cfo, res.acquired_cfo)
    assert same_bits(out, got[4]) and torch.equal(off, got[2]) and same_bits(cs.cfo, got[3])
    ref = rcv.receive(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(ref.packed, got[0]) and same_bits(ref.llr, got[1])
    # cfo_span = 0 is the narrow path, and it does not survive this offset: the span is what finds the integer
    narrow = rcv.receive_capture(cap, sync=W, cfo=True, acquire=J, lo=lo, cfo_scope=cfo_scope)
    torch.cuda.synchronize()
    assert narrow.acquired_cfo_int is None and bool((narrow.cfo.abs() <= 0.5).all())
    for kw in (dict(acquire=0), dict(acquire=J, cfo=False), dict(acquire=0, first=A.true_first(start, lo, T))):
        args = dict(sync=W, cfo=True, lo=lo, cfo_span=M)
        args.update(kw)
        with pytest.raises(_lib.DccnError):
            rcv.receive_capture(cap, **args)
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, sync=W, cfo=True, acquire=J, lo=lo, cfo_span=K // 2)
    with pytest.raises(_lib.DccnError):
        cs.run(cap, first, lo=lo)                                            # the pair is missing
    with pytest.raises(_lib.DccnError):
        CaptureSync(S, K, CP, W, batch, DEV, cfo=False, cfo_span=M)


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


def test_chain_span_is_the_stages_one_after_another():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureSync
    CP, W, B, lo, M, J = 16, 3, 12, 5, 7, 16
    T = S * (K + CP)
    tx, tr = _trainer(2)
    cap_np, start = _offset_capture(CP, 6.62)
    cap = dev(cap_np)
    for cfo_scope in ("frame", "capture"):
        res = tr.receive_capture(cap, sync=W, cfo=True, want_llr=True, frames=B, acquire=J, lo=lo, cfo_scope=cfo_scope, cfo_span=M)
        torch.cuda.synchronize()
        assert int(res.first[0]) == A.true_first(start, lo, T) and int(res.acquired_cfo_int[0]) == 7
        assert bool(((res.cfo - 6.62).abs() < 0.05).all())
        got = [t.clone() for t in (res.packed, res.llr, res.offset, res.cfo)]
        acq = CaptureAcquire(S, K, CP, tx.pilotSc, J, DEV, cfo_span=M)
        cs = CaptureSync(S, K, CP, W, B, DEV, want_metric=False, cfo=True, cfo_scope=cfo_scope, cfo_span=M)
        first = acq.run(cap, lo)
        out, off = cs.run(cap, first, lo=lo, acquired=(acq.cfo_int, acq.cfo))
        ref = tr.receive(out.clone(), want_llr=True)
        torch.cuda.synchronize()
        assert torch.equal(off, got[2]) and same_bits(cs.cfo, got[3])
        assert torch.equal(ref.packed, got[0]) and same_bits(ref.llr, got[1])
    with pytest.raises(_lib.DccnError):
        tr.receive_capture(cap, sync=W, cfo=True, frames=B, lo=lo, cfo_span=M)                 # acquire is missing
    with pytest.raises(_lib.DccnError):
        tr.receive_capture(cap, A.true_first(start, lo, T), sync=W, cfo=True, frames=B, cfo_span=M)


def test_groups_refuse_a_span():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    _, tr = _trainer(2)
    cap = dev(_offset_capture(16, 0.2)[0])
    with pytest.raises(_lib.DccnError, match="cfo_span"):
        ChainReceiveGroup.receive_capture(object.__new__(ChainReceiveGroup), [cap], sync=3, cfo=True, acquire=16, los=5, cfo_span=7)
