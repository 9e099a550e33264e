"""Host side of coarse acquisition (``dccn_capture_acquire``, ``dccn_capture_sync_at``): the fp64 restatement
(tests/capture_acquire_ref.py) held to the truth on clean captures, the captures of the GPU test held to the cap on undecidable
cases, and every documented refusal of the two entry points reached on the host, where nothing can launch."""
import ctypes as C

import numpy as np
import pytest

import capture_acquire_ref as A
import frame_sync_ref as R

S, K = A.S, A.K
INVALID, WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


# ---- 1. clean captures: the definition finds the true start ---------------------------------------------------------------------
@pytest.mark.parametrize("CP", [16, 4])
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_clean_capture_gives_the_true_start(nbits, CP):
    """identity channel, no noise; the capture begins at a random sample of frame 0 and the search at a random lo"""
    T = S * (K + CP)
    sc = A.pilot_sc_of(CP, nbits)
    for eps in (0.0, 0.3, -0.45):
        for J in (2, 4):
            rs = np.random.RandomState(1000 * nbits + 10 * CP + J + int(100 * abs(eps)))
            cut, lo = int(rs.randint(0, T)), int(rs.randint(0, 50))
            cap, start = A.build_capture("AWGN", None, CP, nbits, J + 4, cut, eps, seed=5 + J)
            ref = A.reference(cap, lo, J, S, K, CP, sc)
            srt = np.sort(ref["D"])
            print("nbits %d CP %d eps %+.2f J %d cut %d lo %d: first %d, eps^ %+.4f, top D / second %.3f"
                  % (nbits, CP, eps, J, cut, lo, ref["first"], ref["eps"], srt[-1] / srt[-2]))
            assert ref["first"] == A.true_first(start, lo, T)
            assert lo <= ref["first"] < lo + T
            assert abs(ref["eps"] - eps) < 1e-5
            assert ref["a_ok"] and ref["b_ok"]
            assert srt[-1] >= 1.27 * srt[-2]


def test_pilot_symbols_of_the_lte_grid():
    for CP in (16, 4):
        sc = A.pilot_sc_of(CP)
        ps = A.pilot_symbols(sc, S, K)
        assert len(sc) == 16 and [s for s, _ in ps] == [0, 4] and all(len(ks) == 8 for _, ks in ps)
        assert np.array_equal(np.concatenate([s * K + ks for s, ks in ps]), sc)


def test_bounds_come_from_the_term_counts():
    assert A.lambda_tol(1, S, 4) < A.lambda_tol(16, S, 16) < 2.5e-5
    # frame_cfo_ref's bound takes the components of Gamma off by METRIC_TOL Phi: it covers every shape used here
    assert all((J * S + CP + 4) * A.U <= R.METRIC_TOL for J in A.JS for CP in (16, 4))


# ---- 2. the cases of the GPU test: undecidable ones stay under the cap ----------------------------------------------------------
def test_undecidable_cases_under_cap():
    cases = A.gpu_cases()
    assert {c[0] for c in cases} == {16, 4} and {c[1] for c in cases} == {1, 2, 16}
    assert {c[2] % 2 for c in cases} == {0, 1} and {(c[3], c[4]) for c in cases} == {("AWGN", 30.0), ("ETU", 5.0)}
    bad = 0
    for case in cases:
        ref = A.case_reference(*case)
        CP, J, lo = case[:3]
        assert lo <= ref["first"] < lo + S * (K + CP)
        bad += not (ref["a_ok"] and ref["b_ok"])
    print("%d of %d cases undecidable" % (bad, len(cases)))
    assert bad <= A.CAP * len(cases)
    # with a batch's worth of frames the start is right, up to the per-frame estimator's bias on a dispersive channel
    for case in cases:
        CP, J, lo, ch, snr, seed = case
        if J == 16:
            _, start, _ = A.case_capture(CP, ch, snr, seed)
            d = A.case_reference(*case)["first"] - A.true_first(start, lo, S * (K + CP))
            assert (d == 0) if ch == "AWGN" else (-3 <= d <= 0), (case, d)


# ---- 3. dccn_capture_acquire_supported ------------------------------------------------------------------------------------------
def test_supported_answers_as_documented(lib):
    sup, size = lib.dccn_capture_acquire_supported, lib.dccn_capture_acquire_workspace_size
    for CP in (16, 4):
        for J in range(1, 17):
            assert sup(S, K, CP, 16, J) == 1 and size(S, K, CP, 16, J) > 0
    assert sup(64, 512, 512, 256, 256) == 1 and sup(1, 2, 1, 2, 1) == 1
    for bad in ((0, K, 16, 16, 4), (65, K, 16, 16, 4), (S, 1, 1, 16, 4), (S, K, 0, 16, 4), (S, K, K + 1, 16, 4),
                (S, 1000, 25, 16, 4), (S, K, 16, 1, 4), (S, K, 16, 257, 4), (S, K, 16, 16, 0), (S, K, 16, 16, 257)):
        assert sup(*bad) == 0 and size(*bad) == 0, bad


# ---- 4. refusals, on the host: nothing is launched (there is no device to launch on, and the pointers are host memory) ----------
def _host_buffers():
    store = (C.c_char * 65536)()
    return store, (C.addressof(store) + 255) // 256 * 256


def test_capture_acquire_refusals(lib):
    store, a = _host_buffers()
    CP, J, T = 16, 4, S * (K + 16)
    nws = lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J)
    assert 0 < nws < 16384
    ok = dict(cap=a, n_samples=(J + 2) * T + 5, lo=5, J=J, S=S, K=K, CP=CP, pilot_sc=a + 16384, n_pilot=16, first_out=a + 20480,
              cfo_out=a + 20736, sym_metric=a + 20992, phase_metric=a + 24576, workspace=a + 32768, workspace_bytes=nws)

    def call(**kw):
        v = dict(ok)
        v.update(kw)
        p = lambda x: None if x is None else C.c_void_p(x)   # noqa: E731
        return lib.dccn_capture_acquire(p(v["cap"]), v["n_samples"], v["lo"], v["J"], v["S"], v["K"], v["CP"], p(v["pilot_sc"]),
                                        v["n_pilot"], p(v["first_out"]), p(v["cfo_out"]), p(v["sym_metric"]),
                                        p(v["phase_metric"]), p(v["workspace"]), v["workspace_bytes"], None)

    for name in ("cap", "pilot_sc", "first_out", "cfo_out", "workspace"):
        assert call(**{name: None}) == INVALID, name
    assert call(cap=a + 8) == INVALID and call(workspace=a + 32768 + 8) == INVALID
    assert call(first_out=a + 20480 + 4) == INVALID
    for name in ("pilot_sc", "cfo_out", "sym_metric", "phase_metric"):
        assert call(**{name: ok[name] + 2}) == INVALID, name
    assert call(lo=-1) == INVALID
    assert call(lo=6) == INVALID                                              # lo + (J + 2) T one sample past the capture
    assert call(n_samples=(J + 2) * T + 4) == INVALID
    assert call(lo=1 << 62) == INVALID and call(n_samples=0) == INVALID       # (no overflow on the way to the refusal)
    assert call(J=0) == INVALID and call(J=257) == INVALID and call(n_pilot=1) == INVALID and call(CP=K + 1) == INVALID
    assert call(S=65) == INVALID and call(K=1000, CP=25) == INVALID
    assert call(workspace_bytes=nws - 1) == WORKSPACE
    assert bytes(store) == bytes(65536)                                       # nothing was written


def test_capture_sync_at_refusals(lib):
    store, a = _host_buffers()
    CP, W, n, T = 16, 3, 5, S * (K + 16)
    lo = W
    ns = lo + T - 1 + (n - 1) * T + T + W                                     # exactly enough for every start in [lo, lo + T - 1]
    ok = dict(cap=a, n_samples=ns, first_dev=a + 32768, lo=lo, stride=T, frames=n, S=S, K=K, CP=CP, W=W, out_kin=K + CP,
              x_out=None, offset=a + 33024, cfo=None, metric=None)

    def call(**kw):
        v = dict(ok)
        v.update(kw)
        p = lambda x: None if x is None else C.c_void_p(x)   # noqa: E731
        return lib.dccn_capture_sync_at(p(v["cap"]), v["n_samples"], p(v["first_dev"]), v["lo"], v["stride"], v["frames"], v["S"],
                                        v["K"], v["CP"], v["W"], v["out_kin"], p(v["x_out"]), p(v["offset"]), p(v["cfo"]),
                                        p(v["metric"]), None)

    assert call(first_dev=None) == INVALID and call(first_dev=a + 32768 + 4) == INVALID
    assert call(lo=W - 1) == INVALID and call(lo=-5) == INVALID
    assert call(n_samples=ns - 1) == INVALID                                  # the last window of the LAST start past the capture
    assert call(lo=lo + 1) == INVALID
    assert call(lo=1 << 62) == INVALID and call(stride=1 << 62) == INVALID
    # and wherever dccn_capture_sync refuses
    assert call(cap=None) == INVALID and call(offset=None) == INVALID and call(cap=a + 8) == INVALID
    assert call(stride=T - 1) == INVALID and call(frames=0) == INVALID and call(W=CP + 1) == INVALID
    assert call(out_kin=K + 1) == INVALID and call(x_out=a + 16 * T) == INVALID and call(metric=a + 4) == INVALID
    assert call(S=24, W=1) == INVALID                                         # a shape the capture stage does not take
    assert bytes(store) == bytes(65536)


def test_bindings_and_python_entry_points():
    import inspect
    from dl_ofdm_amd import _lib, sync
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.receive import ReceiveResult, RxReceiver, chain_receive_capture
    for name in ("dccn_capture_acquire", "dccn_capture_acquire_supported", "dccn_capture_acquire_workspace_size",
                 "dccn_capture_sync_at"):
        assert name in _lib.SIGNATURES
    with pytest.raises(_lib.DccnError):
        sync.CaptureAcquire(S, K, 16, A.pilot_sc_of(16), 4, "cpu")            # no CPU fallback
    for fn in (RxReceiver.receive_capture, EqualizerTrainer.receive_capture, chain_receive_capture):
        par = inspect.signature(fn).parameters
        assert par["first"].default is None and par["acquire"].default == 0 and par["lo"].default == 0
    r = ReceiveResult(None, None, None, 320, 2)
    assert r.first is None and r.acquired_cfo is None
