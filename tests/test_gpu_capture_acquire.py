"""Coarse acquisition inside a capture on the GPU (``-m gpu``):

1. ``dccn_capture_acquire`` held to the fp64 restatement of its definition (tests/capture_acquire_ref.py) with the bounds derived
   there -- stage B's reference evaluated at the GPU's own r^ and eps^ -- and two runs held to the same bits;
2. J = 1 with BPSK data, where D(q) can tie: q^ is one of the tied maxima;
3. ``dccn_capture_sync_at`` held bit for bit to ``dccn_capture_sync``, a wild ``first_dev`` to the clamped value;
4. ``receive_capture(first=None, acquire=4)`` of the receiver and of the chain held bit for bit to ``receive_capture(first=true
   start)`` on a clean capture."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A
import frame_cfo_ref as F
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = A.S, A.K
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
    """guarded, sentinel-filled outputs of one dccn_capture_acquire call"""

    def __init__(self, lib, cap, lo, J, CP, sc, n_samples=None):
        N = K + CP
        self.first_buf = torch.full((1 + GUARD,), -99, dtype=torch.int64, device=DEV)
        self.cfo_buf = torch.full((1 + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.sym_buf = torch.full((N + GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.ph_buf = torch.full((S + GUARD,), SENT, dtype=torch.float32, device=DEV)
        nws = lib.dccn_capture_acquire_workspace_size(S, K, CP, int(sc.numel()), J)
        self.ws = torch.zeros(nws + GUARD, dtype=torch.uint8, device=DEV)
        self.N = N
        self.status = lib.dccn_capture_acquire(cap.data_ptr(), int(cap.shape[0]) if n_samples is None else n_samples, lo, J, S, K,
                                               CP, sc.data_ptr(), int(sc.numel()), self.first_buf.data_ptr(),
                                               self.cfo_buf.data_ptr(), self.sym_buf.data_ptr(), self.ph_buf.data_ptr(),
                                               self.ws.data_ptr(), nws, stream())
        torch.cuda.synchronize()
        self.nws = nws

    first = property(lambda self: int(self.first_buf[0]))
    cfo = property(lambda self: float(self.cfo_buf[0]))
    sym = property(lambda self: self.sym_buf[:self.N])
    phase = property(lambda self: self.ph_buf[:S])

    def guards_intact(self):
        return (bool((self.first_buf[1:] == -99).all()) and bool((self.cfo_buf[1:] == SENT).all())
                and bool((self.sym_buf[self.N:] == SENT).all()) and bool((self.ph_buf[S:] == SENT).all())
                and bool((self.ws[self.nws:] == 0).all()))

    def untouched(self):
        return (bool((self.first_buf == -99).all()) and bool((self.cfo_buf == SENT).all()) and bool((self.sym_buf == SENT).all())
                and bool((self.ph_buf == SENT).all()) and bool((self.ws == 0).all()))


# ---- 1. against fp64 ---------------------------------------------------------------------------------------------------------------
def check_against_fp64(lib, cap_np, cap, sc_np, sc, lo, J, CP, ref, bpsk_tie=False):
    """one call held to the reference; -> (decidable, ratios)"""
    N = K + CP
    a = Acq(lib, cap, lo, J, CP, sc)
    assert a.status == 0 and a.guards_intact()
    b = Acq(lib, cap, lo, J, CP, sc)
    assert b.first == a.first and same_bits(a.cfo_buf, b.cfo_buf) and same_bits(a.sym_buf, b.sym_buf)      # two runs, the same bits
    assert same_bits(a.ph_buf, b.ph_buf)
    lam = a.sym.cpu().numpy().astype(np.float64)
    m_ratio = float(np.abs(lam - ref["lam"]).max() / (A.lambda_tol(J, S, CP) * ref["phi"].max()))
    assert lo <= a.first < lo + S * N
    rhat, qhat = (a.first - lo) % N, (a.first - lo) // N
    assert rhat == int(np.argmax(lam))                                       # (the kernel's argmax of its own metric, smallest on ties)
    est = np.float64(np.float32(a.cfo))
    g = ref["gamma"][rhat]
    c_ratio = float(F.circle(est - F.cfo_of(g)) / F.cfo_bound(ref["phi"][None, :], np.array([g]))[0])
    # stage B at the GPU's own r^ and eps^
    D, bound = A.stage_b(cap_np, lo, rhat, float(est), J, S, K, CP, sc_np)
    ph = a.phase.cpu().numpy().astype(np.float64)
    d_ratio = float((np.abs(ph - D) / bound).max())
    assert qhat == int(np.argmax(ph))
    assert m_ratio <= 1.0 and c_ratio <= 1.0 and d_ratio <= 1.0, (m_ratio, c_ratio, d_ratio)
    assert abs(est) <= 0.5
    ok = ref["a_ok"] and A.b_decidable(D, bound)
    if ref["a_ok"]:
        assert rhat == ref["r"]
    if bpsk_tie:
        assert qhat in A.tied_maxima(D, bound)
    elif ok:
        assert qhat == int(np.argmax(D)) and a.first == lo + ref["r"] + qhat * N
        if abs(float(est) - ref["eps"]) < 1e-6:                              # (then the reference's own stage B decides alike)
            assert a.first == ref["first"] or not ref["b_ok"]
    return ok, (m_ratio, c_ratio, d_ratio)


@pytest.mark.parametrize("J", A.JS)
@pytest.mark.parametrize("CP", [16, 4])
def test_acquire_against_fp64(lib, CP, J):
    sc_np = A.pilot_sc_of(CP)
    sc = dev(sc_np)
    assert lib.dccn_capture_acquire_supported(S, K, CP, 16, J) == 1
    worst = np.zeros(3)
    caps = {}
    for case in [c for c in A.gpu_cases() if c[0] == CP and c[1] == J]:
        _, _, lo, ch, snr, seed = case
        cap_np, _, _ = A.case_capture(CP, ch, snr, seed)
        if (ch, seed) not in caps:
            caps[(ch, seed)] = dev(cap_np)
        ok, ratios = check_against_fp64(lib, cap_np, caps[(ch, seed)], sc_np, sc, lo, J, CP, A.case_reference(*case))
        worst = np.maximum(worst, ratios)
        _tally["cases"] += 1
        _tally["skipped"] += not ok
    print("CP %d J %d: worst |dLambda| / bound %.3g, |eps^ - eps64| / bound %.3g, |dD| / bound %.3g"
          % (CP, J, worst[0], worst[1], worst[2]))


def test_undecidable_share():
    """(after the cases above: what they skipped as undecidable stays under the cap)"""
    print("%d of %d cases undecidable" % (_tally["skipped"], _tally["cases"]))
    assert _tally["skipped"] <= A.CAP * _tally["cases"]


def test_pilot_cells_outside_the_grid_are_ignored(lib):
    CP, J, lo = 16, 2, 37
    cap_np, _, _ = A.case_capture(CP, "AWGN", 30.0, 0)
    cap = dev(cap_np)
    sc_np = A.pilot_sc_of(CP)
    a = Acq(lib, cap, lo, J, CP, dev(sc_np))
    wild = np.concatenate([[-5], sc_np, [S * K + 7, 1 << 30]]).astype(np.int32)
    b = Acq(lib, cap, lo, J, CP, dev(wild))
    assert a.status == 0 and b.status == 0 and b.guards_intact()
    assert a.first == b.first and same_bits(a.ph_buf, b.ph_buf) and same_bits(a.sym_buf, b.sym_buf) and same_bits(a.cfo_buf, b.cfo_buf)


def test_refused_calls_write_nothing(lib):
    CP, J = 16, 4
    T = S * (K + CP)
    cap = dev(A.case_capture(CP, "AWGN", 30.0, 0)[0])
    sc = dev(A.pilot_sc_of(CP))
    assert Acq(lib, cap, 5, J, CP, sc, n_samples=5 + (J + 2) * T).status == 0
    for kw in (dict(lo=5, n_samples=5 + (J + 2) * T - 1), dict(lo=-1)):
        r = Acq(lib, cap, kw["lo"], J, CP, sc, n_samples=kw.get("n_samples"))
        assert r.status == INVALID and r.untouched(), kw


# ---- 2. J = 1 with BPSK data ---------------------------------------------------------------------------------------------------------
def test_one_bpsk_frame_returns_a_tied_maximum(lib):
    for CP in (16, 4):
        sc_np = A.pilot_sc_of(CP, 1)
        sc = dev(sc_np)
        T = S * (K + CP)
        for seed in range(3):
            cap_np, start = A.build_capture("AWGN", None, CP, 1, 6, (97 * seed + 11) % T, 0.1 * seed, seed=60 + seed)
            lo = 20 + seed
            ref = A.reference(cap_np, lo, 1, S, K, CP, sc_np)
            check_against_fp64(lib, cap_np, dev(cap_np), sc_np, sc, lo, 1, CP, ref, bpsk_tie=True)


# ---- 3. dccn_capture_sync_at = dccn_capture_sync ---------------------------------------------------------------------------------------
class Cut:
    def __init__(self, n, out_kin, W):
        self.out = torch.full((n, S, out_kin, 2), SENT, dtype=torch.float32, device=DEV)
        self.offset = torch.full((n,), -99, dtype=torch.int32, device=DEV)
        self.cfo = torch.full((n,), SENT, dtype=torch.float32, device=DEV)
        self.metric = torch.full((n, 2 * W + 1), SENT, dtype=torch.float32, device=DEV)

    def same(self, o):
        return (same_bits(self.out, o.out) and torch.equal(self.offset, o.offset) and same_bits(self.cfo, o.cfo)
                and same_bits(self.metric, o.metric))


@pytest.mark.parametrize("CP,W", [(16, 3), (4, 4)])
def test_sync_at_gives_capture_syncs_bits(lib, CP, W):
    n, T = 5, S * (K + CP)                                                   # 5 frames: a ragged last block
    cap_np, start, _ = A.case_capture(CP, "ETU", 5.0, 0)
    cap = dev(cap_np)
    ns = int(cap.shape[0])
    for lo in (W, W + 1, 300, 301):                                          # both window parities
        true = A.true_first(start, lo, T)
        for value, clamped in ((true, true), (lo, lo), (lo + T - 1, lo + T - 1), (lo - 7, lo), (lo + 3 * T, lo + T - 1)):
            first_dev = torch.tensor([value], dtype=torch.int64, device=DEV)
            for cfo in (False, True):
                for out_kin in (K + CP, K):
                    a, b = Cut(n, out_kin, W), Cut(n, out_kin, W)
                    sa = lib.dccn_capture_sync_at(cap.data_ptr(), ns, first_dev.data_ptr(), lo, T, n, S, K, CP, W, out_kin,
                                                  a.out.data_ptr(), a.offset.data_ptr(), a.cfo.data_ptr() if cfo else None,
                                                  a.metric.data_ptr(), stream())
                    sb = lib.dccn_capture_sync(cap.data_ptr(), ns, clamped, T, n, S, K, CP, W, out_kin, b.out.data_ptr(),
                                               b.offset.data_ptr(), b.cfo.data_ptr() if cfo else None, b.metric.data_ptr(),
                                               stream())
                    torch.cuda.synchronize()
                    assert sa == 0 and sb == 0
                    assert a.same(b), (lo, value, cfo, out_kin)
                    assert bool((a.offset != -99).all()) and bool((a.out != SENT).any())
                    assert int(first_dev[0]) == value                        # (read, never written)
    # refused on the device as on the host: the last window of the last start must fit
    a = Cut(n, K + CP, W)
    first_dev = torch.tensor([W], dtype=torch.int64, device=DEV)
    st = lib.dccn_capture_sync_at(cap.data_ptr(), W + T - 1 + (n - 1) * T + T + W - 1, first_dev.data_ptr(), W, T, n, S, K, CP, W,
                                  K + CP, a.out.data_ptr(), a.offset.data_ptr(), None, a.metric.data_ptr(), stream())
    torch.cuda.synchronize()
    assert st == INVALID and bool((a.offset == -99).all()) and bool((a.out == SENT).all())


def test_capture_classes(lib):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureSync
    CP, W, n, J, lo = 16, 3, 5, 4, 9
    T = S * (K + CP)
    cap_np, start, _ = A.case_capture(CP, "AWGN", 30.0, 1)
    cap = dev(cap_np)
    acq = CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), J, DEV)
    first = acq.run(cap, lo)
    assert first is acq.first and first.dtype == torch.int64 and tuple(first.shape) == (1,)
    cs = CaptureSync(S, K, CP, W, n, DEV, cfo=True)
    out, off = cs.run(cap, first, lo=lo)
    torch.cuda.synchronize()
    assert int(first[0]) == A.true_first(start, lo, T)
    got = [t.clone() for t in (out, off, cs.cfo, cs.metric)]
    out2, off2 = cs.run(cap, int(first[0]))
    torch.cuda.synchronize()
    assert same_bits(out2, got[0]) and torch.equal(off2, got[1]) and same_bits(cs.cfo, got[2]) and same_bits(cs.metric, got[3])
    assert torch.equal(cs.offsets(cap, first, lo=lo), got[1])
    assert tuple(acq.sym_metric.shape) == (K + CP,) and tuple(acq.phase_metric.shape) == (S,) and tuple(acq.cfo.shape) == (1,)
    with pytest.raises(_lib.DccnError):
        cs.run(cap, first)                                                   # a device first needs lo
    with pytest.raises(_lib.DccnError):
        cs.run(cap, first.to(torch.int32), lo=lo)
    with pytest.raises(_lib.DccnError):
        cs.run(cap, first, lo=W - 1)
    with pytest.raises(_lib.DccnError):
        acq.run(cap_np, lo)                                                  # a host array: no CPU fallback
    with pytest.raises(_lib.DccnError):
        acq.run(cap, int(cap.shape[0]) - (J + 2) * T + 1)
    with pytest.raises(_lib.DccnError):
        CaptureAcquire(S, K, CP, A.pilot_sc_of(CP)[:1], J, DEV)


# ---- 4. the receive calls ------------------------------------------------------------------------------------------------------------
def _clean_capture(CP):
    """12 QPSK frames to receive and room to acquire: the capture begins 211 samples into frame 0"""
    cap_np, start = A.build_capture("AWGN", None, CP, 2, 16, 211, 0.0, seed=77)
    return cap_np, start


@pytest.mark.parametrize("cp", [True, False])
def test_receiver_acquires_then_receives(cp):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    CP, W, nbits, batch, lo = 16, 3, 2, 12, 5
    T = S * (K + CP)
    kin = K + CP if cp else K
    dims = RxDims(S=S, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=kin, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, CP=CP, K=None if cp else K, pilot_sc=A.pilot_sc_of(CP))
    cap_np, start = _clean_capture(CP)
    cap = dev(cap_np)
    true = A.true_first(start, lo, T)
    for cfo in (False, True):
        res = rcv.receive_capture(cap, sync=W, cfo=cfo, acquire=4, lo=lo)
        torch.cuda.synchronize()
        assert int(res.first[0]) == true and res.first.dtype == torch.int64 and tuple(res.acquired_cfo.shape) == (1,)
        assert abs(float(res.acquired_cfo[0])) < 1e-4
        got = [t.clone() for t in (res.packed, res.llr, res.offset, rcv.x)]
        est = res.cfo.clone() if cfo else None
        ref = rcv.receive_capture(cap, true, sync=W, cfo=cfo)
        torch.cuda.synchronize()
        assert ref.first is None and ref.acquired_cfo is None
        assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and torch.equal(got[2], ref.offset)
        assert same_bits(got[3], rcv.x)
        if cfo:
            assert same_bits(est, ref.cfo)
        dev_first = rcv.receive_capture(cap, torch.tensor([true], dtype=torch.int64, device=DEV), sync=W, cfo=cfo, lo=lo)
        torch.cuda.synchronize()
        assert torch.equal(dev_first.packed, got[0]) and same_bits(dev_first.llr, got[1]) and dev_first.acquired_cfo is None
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, sync=W)                                     # neither first nor acquire
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, true, sync=W, acquire=4)                    # both
    with pytest.raises(_lib.DccnError):
        rcv.receive_capture(cap, sync=W, acquire=4, lo=W - 1)
    bare = RxReceiver(dims, batch, p, CP=CP, K=None if cp else K)
    with pytest.raises(_lib.DccnError):
        bare.receive_capture(cap, sync=W, acquire=4, lo=lo)                  # no pilot cells given


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


def test_chain_acquires_then_receives():
    from dl_ofdm_amd import _lib
    CP, W, B, lo = 16, 3, 12, 5
    T = S * (K + CP)
    tx, tr = _trainer(2)
    assert np.array_equal(tx.pilotSc, A.pilot_sc_of(CP))
    cap_np, start = _clean_capture(CP)
    cap = dev(cap_np)
    true = A.true_first(start, lo, T)
    for cfo in (False, True):
        res = tr.receive_capture(cap, sync=W, cfo=cfo, want_llr=True, frames=B, acquire=4, lo=lo)
        torch.cuda.synchronize()
        assert int(res.first[0]) == true and tuple(res.offset.shape) == (B,)
        got = [t.clone() for t in (res.packed, res.llr, res.offset)]
        ref = tr.receive_capture(cap, true, sync=W, cfo=cfo, want_llr=True, frames=B)
        torch.cuda.synchronize()
        assert ref.first is None
        assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and torch.equal(got[2], ref.offset)
        dev_first = tr.receive_capture(cap, torch.tensor([true], dtype=torch.int64, device=DEV), sync=W, cfo=cfo, want_llr=True,
                                       frames=B, lo=lo)
        torch.cuda.synchronize()
        assert torch.equal(dev_first.packed, got[0]) and same_bits(dev_first.llr, got[1])
    # frames=None: with the start on the device, the frames that fit from the last start of [lo, lo + T) on
    auto = tr.receive_capture(cap, sync=W, acquire=4, lo=lo)
    torch.cuda.synchronize()
    assert auto.offset.shape[0] == (int(cap.shape[0]) - (lo + T - 1) - T - W) // T + 1
    with pytest.raises(_lib.DccnError):
        tr.receive_capture(cap, torch.tensor([true], dtype=torch.int64, device=DEV), sync=W, lo=lo)      # frames must be given
