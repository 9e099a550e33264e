"""Host side of carrier offsets beyond half a subcarrier spacing (``dccn_capture_acquire_wide``, ``dccn_capture_sync_wide``,
``dccn_capture_sync_pooled_wide``): the fp64 restatement (tests/capture_wide_ref.py) held to the truth on every capture of the GPU
test, its undecidable share held to the cap, planted wrong estimators caught, and every documented refusal of the three entry
points reached on the host, where nothing can launch."""
import ctypes as C

import numpy as np
import pytest

import capture_acquire_ref as A
import capture_wide_ref as Wd

S, K = Wd.S, Wd.K
INVALID, WORKSPACE = -1, -2
_tally = {"cases": 0, "undecidable": 0}


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def _start_error(first, start, lo, T):
    d = first - A.true_first(start, lo, T)
    return (d + T // 2) % T - T // 2


# ---- 1. the captures of the GPU test ---------------------------------------------------------------------------------------------
def test_grid_is_the_documented_one():
    cases = Wd.gpu_cases()
    assert Wd.n_captures() + 1 <= 64                                          # (+ the synthetic one)
    assert {c[0] for c in cases} == {16, 4} and {c[1] for c in cases} == {1, 2, 16} and {c[6] for c in cases} == {0, 1, 7, 31}
    assert {(c[3], c[4]) for c in cases} == {("AWGN", 30.0), ("ETU", 5.0)}
    for CP in (16, 4):
        for J in Wd.JS:
            assert {c[2] % 2 for c in cases if c[0] == CP and c[1] == J} == {0, 1}
    eps = {c[5] for c in cases}
    assert eps == {0.45, -0.45, 1.45, -1.45, 7.45, -7.45, 31.45, -31.45, 2.49, -3.51, 0.2}
    assert all(abs(c[5]) <= c[6] + 0.5 for c in cases)


@pytest.mark.parametrize("J", Wd.JS)
def test_reference_on_the_gpu_grid(J):
    """every case at this J: decidability counted; with a batch's worth of frames (J = 16) the start is right up to the per-frame
    estimator's bias on a dispersive channel, and the integer is rint(eps - eps^)"""
    for case in [c for c in Wd.gpu_cases() if c[1] == J]:
        CP, _, lo, ch, snr, eps, M = case
        T = S * (K + CP)
        ref = Wd.case_reference(*case)
        assert lo <= ref["first"] < lo + T and -M <= ref["m"] <= M
        _tally["cases"] += 1
        _tally["undecidable"] += not (ref["a_ok"] and ref["b_ok"])
        if J == 16:
            _, start, _ = Wd.case_capture(CP, ch, snr, eps)
            d = _start_error(ref["first"], start, lo, T)
            assert (d == 0) if ch == "AWGN" else (-3 <= d <= 0), (case, d)
            assert ref["m"] == int(np.rint(eps - ref["eps"])), (case, ref["m"], ref["eps"])
            assert abs(ref["m"] + ref["eps"] - eps) < 0.1
            srt = np.sort(ref["D"].reshape(-1))
            assert srt[-2] <= 0.86 * srt[-1], (case, srt[-2] / srt[-1])        # the runner-up stays clear of the maximum


def test_undecidable_share_under_cap():
    """(after the cases above)"""
    print("%d of %d cases undecidable" % (_tally["undecidable"], _tally["cases"]))
    assert _tally["cases"] == len(Wd.gpu_cases())
    assert _tally["undecidable"] <= Wd.CAP * _tally["cases"]


def test_column_zero_is_the_narrow_stage_b():
    """column m = 0 of D(q, m) is capture_acquire_ref's D(q): the same sums"""
    CP, J, lo = 4, 2, 555
    cap, _, _ = Wd.case_capture(CP, "ETU", 5.0, 2.49)
    sc = A.pilot_sc_of(CP)
    rhat, eps, _, _, _ = A.stage_a(cap, lo, J, S, K, CP)
    D, bound = Wd.stage_b_wide(cap, lo, rhat, eps, J, S, K, CP, sc, 7)
    D0, bound0 = A.stage_b(cap, lo, rhat, eps, J, S, K, CP, sc)
    assert np.allclose(D[:, 7], D0, rtol=1e-12, atol=0) and np.allclose(bound[:, 7], bound0, rtol=1e-12, atol=0)


def test_synthetic_frame_whose_bins_wrap():
    """K = 16 with pilots next to both band edges: every shift but 0 wraps some bin mod K"""
    S_, K_, CP, M = (Wd.SYN[k] for k in ("S", "K", "CP", "M"))
    T = S_ * (K_ + CP)
    sc = Wd.synthetic_pilot_sc()
    for seed, eps, cut, lo in ((1, 6.3, 17, 3), (2, -7.45, 40, 10), (3, 0.2, 5, 0), (4, -2.51, 59, 21)):
        cap, start = Wd.synthetic_capture(14, cut, eps, seed)
        ref = Wd.reference(cap, lo, 8, S_, K_, CP, sc, M)
        assert ref["first"] == A.true_first(start, lo, T), (seed, ref["first"])
        assert ref["m"] == int(np.rint(eps - ref["eps"])) and abs(ref["m"] + ref["eps"] - eps) < 0.05
        assert ref["a_ok"] and ref["b_ok"]


# ---- 2. planted errors -----------------------------------------------------------------------------------------------------------
def test_planted_wrong_estimators_are_caught():
    CP, J, lo = 16, 16, 37
    sc = A.pilot_sc_of(CP)
    # the pilots looked for at k_i - m: wrong wherever m != 0
    for eps in (-7.45, -3.51):
        cap, _, _ = Wd.case_capture(CP, "AWGN", 30.0, eps)
        ref = Wd.case_reference(CP, J, lo, "AWGN", 30.0, eps, 7)
        q, m = Wd.stage_b_planted("sign", cap, lo, ref["r"], ref["eps"], J, S, K, CP, sc, 7)
        assert ref["m"] == int(np.rint(eps - ref["eps"])) and m == -ref["m"] and m != ref["m"]
    # the comb taken as uniform across DC: the two halves of a pilot symbol then peak two bins apart, and the maximum is lost
    wrong = 0
    for eps, M in ((7.45, 7), (-7.45, 7), (2.49, 7), (-3.51, 7), (0.2, 7)):
        for ch, snr in A.CHANNELS:
            lo_ = Wd.LOS[CP][0]
            cap, _, _ = Wd.case_capture(CP, ch, snr, eps)
            rhat, e, _, _, _ = A.stage_a(cap, lo_, J, S, K, CP)
            D, _ = Wd.stage_b_wide(cap, lo_, rhat, e, J, S, K, CP, sc, M)
            q, m = Wd.stage_b_planted("uniform", cap, lo_, rhat, e, J, S, K, CP, sc, M)
            wrong += (q, m) != (Wd.decide(D)[0], Wd.decide(D)[1] - M)
    assert wrong >= 3, wrong
    # shifted bins clamped into [0, K), not taken mod K: the synthetic frame's wrapping shifts are lost
    S_, K_, CPs, M = (Wd.SYN[k] for k in ("S", "K", "CP", "M"))
    ssc = Wd.synthetic_pilot_sc()
    lost = 0
    for seed, eps, cut in ((1, 6.3, 17), (2, -7.45, 40), (4, -2.51, 59)):
        cap, _ = Wd.synthetic_capture(14, cut, eps, seed)
        ref = Wd.reference(cap, 3, 8, S_, K_, CPs, ssc, M)
        q, m = Wd.stage_b_planted("clip", cap, 3, ref["r"], ref["eps"], 8, S_, K_, CPs, ssc, M)
        lost += (q, m) != (ref["q"], ref["m"])
    assert lost >= 1, lost                                                    # (a shift that wraps one pair only may still be found)


def test_unwrap():
    # a frame whose own fraction lands on the other side of +-1/2 from acquisition's still gets the right total
    I, ok = Wd.unwrap(2, 0.49, np.array([-0.49, 0.49, 0.45]), K)
    assert list(I) == [3, 2, 2] and ok.all() and np.allclose(I + np.array([-0.49, 0.49, 0.45]), [2.51, 2.49, 2.45])
    I, ok = Wd.unwrap(-4, 0.49, np.array([0.49, -0.5]), K)
    assert list(I) == [-4, -3]
    I, ok = Wd.unwrap(0, 0.0, np.array([0.3, -0.5, 0.5]), K)
    assert list(I) == [0, 0, 0] and list(ok) == [True, False, False]          # (rint: ties to even)
    # the unwrap omitted: the total is off by I whole spacings
    assert abs((3 + -0.49) - 2.51) < 1e-12 and abs(-0.49 - 2.51) > 2.9
    # a wild pair stays inside [-K/2, K/2]
    I, ok = Wd.unwrap(10 ** 9, 0.0, np.array([0.1]), K)
    assert list(I) == [K // 2] and not ok.any()
    assert list(Wd.unwrap(-10 ** 9, 0.0, np.array([0.1]), K)[0]) == [-(K // 2)]
    assert Wd.total_bound(np.array([0, 7]))[1] == Wd.U * 7.5


# ---- 3. the size queries ---------------------------------------------------------------------------------------------------------
def test_wide_supported_answers_as_documented(lib):
    sup, size = lib.dccn_capture_acquire_wide_supported, lib.dccn_capture_acquire_wide_workspace_size
    for CP in (16, 4):
        for J in (1, 2, 16):
            assert size(S, K, CP, 16, J, 0) == lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J)
            for M in (0, 1, 7, 31):
                assert sup(S, K, CP, 16, J, M) == 1
                assert size(S, K, CP, 16, J, M) >= size(S, K, CP, 16, J, 0) + S * 2 * M * J * 4 - 256
    assert sup(S, K, 16, 16, 4, -1) == 0 and sup(S, K, 16, 16, 4, 32) == 0 and size(S, K, 16, 16, 4, 32) == 0
    assert sup(3, 16, 4, 6, 8, 7) == 1 and sup(3, 16, 4, 6, 8, 8) == 0
    assert sup(64, 512, 512, 256, 256, 255) == 1 and sup(1, 2, 1, 2, 1, 0) == 1 and sup(1, 2, 1, 2, 1, 1) == 0
    assert sup(S, 1000, 25, 16, 4, 3) == 0                                    # wherever the narrow call refuses
    pw = lib.dccn_capture_sync_pooled_wide_workspace_size
    assert pw(0) == 0 and all(pw(f) == lib.dccn_capture_sync_pooled_workspace_size(f) + 16 for f in (1, 5, 73))


# ---- 4. refusals, on the host: nothing is launched (there is no device to launch on, and the pointers are host memory) -----------
def _host_buffers():
    store = (C.c_char * 131072)()
    return store, (C.addressof(store) + 255) // 256 * 256


def _p(x):
    return None if x is None else C.c_void_p(x)


def test_capture_acquire_wide_refusals(lib):
    store, a = _host_buffers()
    CP, J, M, T = 16, 4, 7, S * (K + 16)
    nws = lib.dccn_capture_acquire_wide_workspace_size(S, K, CP, 16, J, M)
    assert lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J) < nws < 32768
    ok = dict(cap=a, n_samples=(J + 2) * T + 5, lo=5, J=J, S=S, K=K, CP=CP, pilot_sc=a + 16384, n_pilot=16, M=M,
              first_out=a + 20480, cfo_out=a + 20736, cfo_int_out=a + 20800, sym_metric=a + 20992, phase_metric=a + 24576,
              workspace=a + 32768, workspace_bytes=nws)

    def call(**kw):
        v = dict(ok)
        v.update(kw)
        return lib.dccn_capture_acquire_wide(_p(v["cap"]), v["n_samples"], v["lo"], v["J"], v["S"], v["K"], v["CP"],
                                             _p(v["pilot_sc"]), v["n_pilot"], v["M"], _p(v["first_out"]), _p(v["cfo_out"]),
                                             _p(v["cfo_int_out"]), _p(v["sym_metric"]), _p(v["phase_metric"]), _p(v["workspace"]),
                                             v["workspace_bytes"], None)

    assert call(M=-1) == INVALID and call(M=K // 2) == INVALID and call(M=1 << 30) == INVALID
    for name in ("cap", "pilot_sc", "first_out", "cfo_out", "cfo_int_out", "workspace"):
        assert call(**{name: None}) == INVALID, name
    assert call(cfo_int_out=a + 20800 + 2) == INVALID and call(cap=a + 8) == INVALID and call(first_out=a + 20480 + 4) == INVALID
    for name in ("pilot_sc", "cfo_out", "sym_metric", "phase_metric"):
        assert call(**{name: ok[name] + 2}) == INVALID, name
    assert call(lo=-1) == INVALID and call(lo=6) == INVALID                  # lo + (J + 2) T one sample past the capture
    assert call(n_samples=(J + 2) * T + 4) == INVALID and call(lo=1 << 62) == INVALID and call(n_samples=0) == INVALID
    assert call(J=0) == INVALID and call(n_pilot=1) == INVALID and call(S=65) == INVALID
    assert call(workspace_bytes=nws - 1) == WORKSPACE
    assert call(workspace_bytes=lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J)) == WORKSPACE    # the narrow size is short
    assert bytes(store) == bytes(len(store))                                  # nothing was written


def test_capture_sync_wide_refusals(lib):
    store, a = _host_buffers()
    CP, W, n, T = 16, 3, 5, S * (K + 16)
    lo = W
    ns = lo + T - 1 + (n - 1) * T + T + W                                     # exactly enough for every start in [lo, lo + T - 1]
    pair = dict(cfo_int_dev=a + 33536, cfo_frac_dev=a + 33540)
    ok = dict(cap=a, n_samples=ns, first_dev=a + 32768, lo=lo, stride=T, frames=n, S=S, K=K, CP=CP, W=W, out_kin=K + CP,
              x_out=None, offset=a + 33024, cfo=a + 33280, metric=None, **pair)

    def call(**kw):
        v = dict(ok)
        v.update(kw)
        return lib.dccn_capture_sync_wide(_p(v["cap"]), v["n_samples"], _p(v["first_dev"]), v["lo"], v["stride"], v["frames"],
                                          v["S"], v["K"], v["CP"], v["W"], v["out_kin"], _p(v["x_out"]), _p(v["offset"]),
                                          _p(v["cfo"]), _p(v["metric"]), _p(v["cfo_int_dev"]), _p(v["cfo_frac_dev"]), None)

    assert call(cfo_int_dev=None) == INVALID and call(cfo_frac_dev=None) == INVALID and call(cfo=None) == INVALID
    assert call(cfo_int_dev=a + 33536 + 2) == INVALID and call(cfo_frac_dev=a + 33540 + 1) == INVALID
    # and wherever dccn_capture_sync_at refuses
    assert call(first_dev=None) == INVALID and call(first_dev=a + 32768 + 4) == INVALID
    assert call(lo=W - 1) == INVALID and call(n_samples=ns - 1) == INVALID and call(lo=lo + 1) == INVALID
    assert call(cap=None) == INVALID and call(offset=None) == INVALID and call(stride=T - 1) == INVALID
    assert call(frames=0) == INVALID and call(W=CP + 1) == INVALID and call(out_kin=K + 1) == INVALID
    assert call(x_out=a + 16 * T) == INVALID and call(S=24, W=1) == INVALID

    # the pooled entry: dccn_capture_sync_pooled's refusals, the pair, and its own workspace size
    nws = lib.dccn_capture_sync_pooled_wide_workspace_size(n)
    pok = dict(cap=a, n_samples=ns, first=lo, first_dev=None, lo=0, stride=T, frames=n, S=S, K=K, CP=CP, W=W, out_kin=K + CP,
               x_out=a + 65536, offset=a + 33024, cfo_out=a + 33280, metric=None, workspace=a + 34816, workspace_bytes=nws, **pair)

    def pooled(**kw):
        v = dict(pok)
        v.update(kw)
        return lib.dccn_capture_sync_pooled_wide(_p(v["cap"]), v["n_samples"], v["first"], _p(v["first_dev"]), v["lo"], v["stride"],
                                                 v["frames"], v["S"], v["K"], v["CP"], v["W"], v["out_kin"], _p(v["x_out"]),
                                                 _p(v["offset"]), _p(v["cfo_out"]), _p(v["metric"]), _p(v["cfo_int_dev"]),
                                                 _p(v["cfo_frac_dev"]), _p(v["workspace"]), v["workspace_bytes"], None)

    assert pooled(cfo_int_dev=None) == INVALID and pooled(cfo_frac_dev=None) == INVALID
    assert pooled(cfo_int_dev=a + 33536 + 2) == INVALID
    assert pooled(x_out=None) == INVALID and pooled(cfo_out=None) == INVALID and pooled(workspace=None) == INVALID
    assert pooled(first=W - 1) == INVALID and pooled(first=lo + T) == INVALID and pooled(stride=T - 1) == INVALID
    assert pooled(first_dev=a + 32768, lo=lo + 1) == INVALID and pooled(workspace=a + 34816 + 8) == INVALID
    assert pooled(workspace_bytes=nws - 1) == WORKSPACE
    assert pooled(workspace_bytes=lib.dccn_capture_sync_pooled_workspace_size(n)) == WORKSPACE
    assert bytes(store) == bytes(len(store))


# ---- 5. the Python entry points ----------------------------------------------------------------------------------------------------
def test_bindings_and_python_entry_points():
    import inspect
    from dl_ofdm_amd import _lib, sync
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    from dl_ofdm_amd.receive import ReceiveResult, RxReceiver, chain_receive_capture, group_receive_capture
    for name in ("dccn_capture_acquire_wide", "dccn_capture_acquire_wide_supported", "dccn_capture_acquire_wide_workspace_size",
                 "dccn_capture_sync_wide", "dccn_capture_sync_pooled_wide", "dccn_capture_sync_pooled_wide_workspace_size"):
        assert name in _lib.SIGNATURES
    for fn in (RxReceiver.receive_capture, EqualizerTrainer.receive_capture, chain_receive_capture, group_receive_capture,
               ChainReceiveGroup.receive_capture, sync.CaptureAcquire.__init__, sync.CaptureSync.__init__):
        assert inspect.signature(fn).parameters["cfo_span"].default == 0
    assert inspect.signature(sync.CaptureSync.run).parameters["acquired"].default is None
    r = ReceiveResult(None, None, None, 320, 2)
    assert r.acquired_cfo_int is None and r.acquired_cfo is None
    with pytest.raises(_lib.DccnError):
        sync.CaptureAcquire(S, K, 16, A.pilot_sc_of(16), 4, "cpu", cfo_span=7)  # no CPU fallback
