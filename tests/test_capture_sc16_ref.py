"""Host side of 16-bit integer I/Q captures (``dccn_capture_sync_sc16``, ``dccn_capture_sync_pooled_sc16``,
``dccn_capture_acquire_sc16``): the NumPy model of the format (``radio.quantize_sc16`` / ``radio.sc16_to_float``) held to its
definition, the three symbols in the header, the library and the binding table, the ``scale`` parameters of the Python entry points,
and the entries' refusals reached on the host, where nothing can launch (the GPU test repeats them against poisoned device
outputs and adds the accepted neighbours)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import capture_acquire_ref as A

S, K = A.S, A.K
INVALID, WORKSPACE = -1, -2
ENTRIES = ("dccn_capture_sync_sc16", "dccn_capture_sync_pooled_sc16", "dccn_capture_acquire_sc16")
SCALES = (np.float32(2.0 ** -15), np.float32(1.0 / 3000.0), np.float32(0.37 / 16384.0))


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


# ---- 1. the format's host model ----------------------------------------------------------------------------------------------------
def test_sc16_to_float_is_one_exact_conversion_and_one_fp32_multiply():
    from dl_ofdm_amd.radio import sc16_to_float
    rs = np.random.RandomState(5)
    q = rs.randint(-32768, 32768, size=(4096, 2)).astype(np.int16)
    q[:4] = [[-32768, 32767], [32767, -32768], [-1, 0], [0, -1]]
    for scale in SCALES:
        got = sc16_to_float(q, scale)
        assert got.dtype == np.float32 and got.shape == q.shape and got.flags["C_CONTIGUOUS"]
        # a 16-bit integer times a 24-bit significand is exact in fp64: rounding that product once is THE fp32 product
        want = (q.astype(np.float64) * np.float64(scale)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got, q.astype(np.float32) * scale)
    assert np.array_equal(sc16_to_float(q, 2.0 ** -15), q.astype(np.float64) / 32768.0)       # a power of two: no rounding at all
    for bad in (q.astype(np.int32), q[:, :1], q.reshape(-1)):
        with pytest.raises(ValueError):
            sc16_to_float(bad, 1.0)


def test_quantize_round_trip_saturation_and_layout():
    from dl_ofdm_amd.radio import quantize_sc16, sc16_to_float
    rs = np.random.RandomState(6)
    x = (0.3 * rs.randn(5000, 2)).astype(np.float32)
    for scale in SCALES:
        q = quantize_sc16(x, scale)
        assert q.dtype == np.int16 and q.shape == x.shape and q.flags["C_CONTIGUOUS"]
        want = np.clip(np.rint(x.astype(np.float64) / float(scale)), -32768, 32767)
        assert np.array_equal(q, want)
        inside = np.abs(want) < 32767
        back = sc16_to_float(q, scale).astype(np.float64)
        # half a count, and the one fp32 rounding of the product
        assert (np.abs(back - x)[inside] <= 0.5 * float(scale) + 2.0 ** -24 * np.abs(back[inside])).all()
        assert np.array_equal(quantize_sc16(sc16_to_float(q, scale), scale), q)                # the grid is a fixed point
    sat = quantize_sc16(np.array([[1e9, -1e9], [1.0, -1.0], [32767.4 / 32768, -32768.6 / 32768]]), 2.0 ** -15)
    assert sat.tolist() == [[32767, -32768], [32767, -32768], [32767, -32768]]
    assert quantize_sc16(np.array([[0.5, -1.5], [2.5, -0.5]]), 1.0).tolist() == [[0, -2], [2, 0]]       # rint: ties to even
    c = (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)
    assert np.array_equal(quantize_sc16(c, SCALES[1]), quantize_sc16(x, SCALES[1]))            # complex [n] is (I, Q) too
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            quantize_sc16(x, bad)
    with pytest.raises(ValueError):
        quantize_sc16(x.reshape(-1), 1.0)


# ---- 2. the symbols and the Python parameters --------------------------------------------------------------------------------------
def test_symbols_in_header_library_and_table(lib):
    from dl_ofdm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dccn.h")).read()
    for name in ENTRIES:
        assert "int %s(const int16_t* cap, long long n_samples, float scale," % name in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args[:3] == [C.c_void_p, C.c_longlong, C.c_float]
    assert len(_lib.SIGNATURES["dccn_capture_sync_sc16"][1]) == len(_lib.SIGNATURES["dccn_capture_sync_at"][1]) + 2
    assert len(_lib.SIGNATURES["dccn_capture_sync_pooled_sc16"][1]) == len(_lib.SIGNATURES["dccn_capture_sync_pooled"][1]) + 1
    assert len(_lib.SIGNATURES["dccn_capture_acquire_sc16"][1]) == len(_lib.SIGNATURES["dccn_capture_acquire"][1]) + 1
    # the public link structs keep their layout
    assert C.sizeof(_lib.CaptureLink) == 80 and C.sizeof(_lib.PooledLink) == 96 and C.sizeof(_lib.AcquireLink) == 80


def test_scale_parameters_default_to_none_and_cpu_is_refused():
    import torch
    from dl_ofdm_amd import _lib, sync
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.receive import RxReceiver, chain_receive_capture
    for fn in (sync.CaptureSync.run, sync.CaptureSync.offsets, sync.CaptureAcquire.run, RxReceiver.receive_capture,
               EqualizerTrainer.receive_capture, chain_receive_capture):
        assert inspect.signature(fn).parameters["scale"].default is None, fn
    assert sync.SC16_DEFAULT_SCALE == 2.0 ** -15
    with pytest.raises(_lib.DccnError):
        sync.CaptureSync(S, K, 16, 3, 9, "cpu")
    with pytest.raises(_lib.DccnError):
        sync.CaptureAcquire(S, K, 16, A.pilot_sc_of(16), 4, "cpu")
    with pytest.raises(_lib.DccnError):                                     # a host tensor: there is no CPU fallback
        sync.capture_format(torch.zeros(64, 2, dtype=torch.int16), None, "CaptureSync")


# ---- 3. refusals, on the host: nothing is launched (there is no device to launch on, and the pointers are host memory) -------------
def _host_buffers():
    store = (C.c_char * 262144)()
    return store, (C.addressof(store) + 255) // 256 * 256


def _p(x):
    return None if x is None else C.c_void_p(x)


BAD_SCALES = (0.0, -0.0, -2.0 ** -15, float("inf"), float("-inf"), float("nan"))


def test_capture_sync_sc16_refusals(lib):
    store, a = _host_buffers()
    CP, W, n, T = 16, 3, 5, S * (K + 16)
    ns = W + (n - 1) * T + T + W
    ok = dict(cap=a, n_samples=ns, scale=2.0 ** -15, first=W, first_dev=None, lo=0, stride=T, frames=n, S=S, K=K, CP=CP, W=W,
              out_kin=K + CP, x_out=None, offset=a + 131072, cfo=None, metric=None)

    def call(**kw):
        v = dict(ok)
        v.update(kw)
        return lib.dccn_capture_sync_sc16(_p(v["cap"]), v["n_samples"], v["scale"], v["first"], _p(v["first_dev"]), v["lo"],
                                          v["stride"], v["frames"], v["S"], v["K"], v["CP"], v["W"], v["out_kin"], _p(v["x_out"]),
                                          _p(v["offset"]), _p(v["cfo"]), _p(v["metric"]), None)

    for bad in BAD_SCALES:
        assert call(scale=bad) == INVALID, bad
    assert call(cap=None) == INVALID and call(cap=a + 4) == INVALID and call(cap=a + 8) == INVALID and call(offset=None) == INVALID
    assert call(n_samples=ns - 1) == INVALID and call(first=W - 1) == INVALID and call(first=W + 1) == INVALID
    assert call(stride=T - 1) == INVALID and call(frames=0) == INVALID and call(out_kin=K + 1) == INVALID
    assert call(W=CP + 1) == INVALID and call(S=24, W=1) == INVALID and call(n_samples=0) == INVALID
    # the capture is 4 n_samples bytes: an output inside them is refused (one that starts right behind them is accepted: GPU test)
    assert call(x_out=a + 16) == INVALID and call(x_out=a + (4 * ns - 1) // 16 * 16) == INVALID
    # first_dev: dccn_capture_sync_at's rules, every start in [lo, lo + T - 1] inside the capture
    ns_at = W + T - 1 + (n - 1) * T + T + W
    at = dict(first_dev=a + 131584, lo=W, n_samples=ns_at)
    assert call(**dict(at, first_dev=a + 131584 + 4)) == INVALID and call(**dict(at, lo=W - 1)) == INVALID
    assert call(**dict(at, n_samples=ns_at - 1)) == INVALID and call(**dict(at, lo=W + 1)) == INVALID
    assert call(**dict(at, scale=float("nan"))) == INVALID
    assert bytes(store) == bytes(len(store))                                  # nothing was written


def test_capture_sync_pooled_and_acquire_sc16_refusals(lib):
    store, a = _host_buffers()
    CP, W, n, J, T = 16, 3, 5, 4, S * (K + 16)
    ns = W + (n - 1) * T + T + W
    nws = lib.dccn_capture_sync_pooled_workspace_size(n)
    pok = dict(cap=a, n_samples=ns, scale=1.0 / 3000.0, first=W, first_dev=None, lo=0, stride=T, frames=n, S=S, K=K, CP=CP, W=W,
               out_kin=K + CP, x_out=a + 65536, offset=a + 131072, cfo_out=a + 131584, metric=None, workspace=a + 132096,
               workspace_bytes=nws)

    def pooled(**kw):
        v = dict(pok)
        v.update(kw)
        return lib.dccn_capture_sync_pooled_sc16(_p(v["cap"]), v["n_samples"], v["scale"], v["first"], _p(v["first_dev"]), v["lo"],
                                                 v["stride"], v["frames"], v["S"], v["K"], v["CP"], v["W"], v["out_kin"],
                                                 _p(v["x_out"]), _p(v["offset"]), _p(v["cfo_out"]), _p(v["metric"]),
                                                 _p(v["workspace"]), v["workspace_bytes"], None)

    for bad in BAD_SCALES:
        assert pooled(scale=bad) == INVALID, bad
    assert pooled(cap=None) == INVALID and pooled(cap=a + 4) == INVALID and pooled(x_out=None) == INVALID
    assert pooled(cfo_out=None) == INVALID and pooled(workspace=None) == INVALID and pooled(workspace=a + 132096 + 8) == INVALID
    assert pooled(n_samples=ns - 1) == INVALID and pooled(first=W - 1) == INVALID and pooled(stride=T - 1) == INVALID
    assert pooled(x_out=a + 4 * ns // 16 * 16 - 16) == INVALID
    assert pooled(workspace_bytes=nws - 1) == WORKSPACE

    naw = lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J)
    aok = dict(cap=a, n_samples=(J + 2) * T + 5, scale=2.0 ** -15, lo=5, J=J, S=S, K=K, CP=CP, pilot_sc=a + 65536, n_pilot=16,
               first_out=a + 66560, cfo_out=a + 66816, sym_metric=a + 67072, phase_metric=a + 68096, workspace=a + 131072,
               workspace_bytes=naw)

    def acquire(**kw):
        v = dict(aok)
        v.update(kw)
        return lib.dccn_capture_acquire_sc16(_p(v["cap"]), v["n_samples"], v["scale"], v["lo"], v["J"], v["S"], v["K"], v["CP"],
                                             _p(v["pilot_sc"]), v["n_pilot"], _p(v["first_out"]), _p(v["cfo_out"]),
                                             _p(v["sym_metric"]), _p(v["phase_metric"]), _p(v["workspace"]), v["workspace_bytes"], None)

    for bad in BAD_SCALES:
        assert acquire(scale=bad) == INVALID, bad
    for name in ("cap", "pilot_sc", "first_out", "cfo_out", "workspace"):
        assert acquire(**{name: None}) == INVALID, name
    assert acquire(cap=a + 4) == INVALID and acquire(lo=-1) == INVALID and acquire(lo=6) == INVALID
    assert acquire(n_samples=(J + 2) * T + 4) == INVALID and acquire(J=0) == INVALID and acquire(n_pilot=1) == INVALID
    assert acquire(workspace_bytes=naw - 1) == WORKSPACE
    assert bytes(store) == bytes(len(store))
