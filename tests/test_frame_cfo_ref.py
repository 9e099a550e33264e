"""Host side of the carrier-frequency-offset tests (no GPU): the fp64 restatement (tests/frame_cfo_ref.py) recovers a known
offset, the impaired inputs of every GPU case are decidable under tests/frame_sync_ref.py's cap, and ``dccn_frame_sync_cfo`` is
declared, exported, bound, and refuses bad arguments without touching a device."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_cfo_ref as F
import frame_sync_ref as R
from dl_ofdm_amd.radio import apply_cfo

NAME = "dccn_frame_sync_cfo"
INVALID = -1                    # DCCN_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- 1. the restatement recovers a known offset -------------------------------------------------------------------
@pytest.mark.parametrize("eps", [-0.45, -0.1, 0.0, 0.03, 0.45])
@pytest.mark.parametrize("CP,W", [(16, 3), (4, 4)])
def test_the_reference_recovers_the_offset_of_exact_prefix_frames(eps, CP, W):
    x = F.exact_prefix_frames(9, R.S, R.K, CP, seed=40 + CP, eps=eps)
    off, lam, phi, gamma, cfo = F.reference(x, R.K, CP, W)
    assert (off == 0).all() and R.decidable(lam, phi).all()
    print("eps %g CP %d: max |cfo64 - eps| = %.3g" % (eps, CP, np.abs(cfo - eps).max()))
    assert np.abs(cfo - eps).max() <= 1e-6
    # and the derotated frame is the frame without the offset, to the float32 rounding of the impaired samples
    clean = F.exact_prefix_frames(9, R.S, R.K, CP, seed=40 + CP)
    assert np.abs(F.derotated(x, off, np.full(9, eps), R.K) - clean).max() <= 4 * 2.0 ** -24 * np.abs(clean).max()


def test_a_zero_offset_leaves_the_frames_as_they_are():
    x = R.case_frames("EVA", 30.0, 16)[:5]
    out = apply_cfo(x, 0, R.K)
    assert out.dtype == np.float32 and np.array_equal(out, x)
    assert np.array_equal(apply_cfo(x, np.zeros(5), R.K), x)
    # per-frame offsets: frame f is turned by its own eps, sample n of the WHOLE frame by 2 pi eps n / K
    eps = np.array([0.25, -0.25, 0.0, 0.5, 0.1])
    y = apply_cfo(x, eps, R.K).astype(np.float64).reshape(5, -1, 2)
    x64 = x.astype(np.float64).reshape(5, -1, 2)
    n = R.K                                                          # one symbol body on: a turn by 2 pi eps
    want = (x64[:, n, 0] + 1j * x64[:, n, 1]) * np.exp(2j * np.pi * eps)
    assert np.abs((y[:, n, 0] + 1j * y[:, n, 1]) - want).max() <= 2.0 ** -23 * np.abs(want).max()


# ---- 2. the cap, on the reference alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("CP,W,channel,snr", R.all_cases())
def test_the_reference_decides_the_impaired_inputs_of_every_gpu_case(CP, W, channel, snr):
    off, lam, phi, ok, gamma, cfo = F.case_reference(channel, snr, CP, W)
    assert (off >= -W).all() and (off <= W).all()
    assert (np.abs(gamma) > 0).all() and (np.abs(cfo) <= 0.5).all()
    for n in R.FRAME_COUNTS:
        bad = int((~ok[:n]).sum())
        print("%s %g dB CP %d W %d: %d of %d impaired frames undecidable" % (channel, snr, CP, W, bad, n))
        assert bad <= R.CAP * n
    # what the estimator is for: on the decidable frames the estimate sits near the offset that was applied
    err = F.circle(cfo - F.case_eps(channel, snr, CP))[ok]
    print("  median |cfo64 - eps| = %.3g, max = %.3g" % (np.median(err), err.max()))


# ---- 3. the entry point: declared, exported, bound; refusals decided on the host ------------------------------------
def test_the_entry_is_declared_exported_and_bound(lib):
    import re
    from dl_ofdm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dccn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "include/dccn.h does not declare %s" % NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* x", "int frames", "int S", "int K", "int CP", "int W", "int out_kin", "float* x_out",
                      "int32_t* offset", "float* cfo", "float* metric", "dccn_stream_t stream"]
    assert hasattr(lib, NAME), "libdccn.so does not export %s" % NAME
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and args == [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 5
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == args


def test_refusals_touch_no_device(lib):
    """host pointers a refused call never dereferences (as tests/test_frame_sync_ref.py does for dccn_frame_sync)"""
    fn = getattr(lib, NAME)
    store = (C.c_char * 8192)()
    p = (C.addressof(store) + 255) // 256 * 256
    x, out, off, cfo, met = p, p + 4096, p + 1024, p + 2048, p + 3072
    ok = dict(x=x, frames=4, S=7, K=64, CP=16, W=3, out_kin=80, x_out=None, offset=off, cfo=cfo, metric=None)

    def call(**over):
        a = dict(ok, **over)
        return fn(a["x"], a["frames"], a["S"], a["K"], a["CP"], a["W"], a["out_kin"], a["x_out"], a["offset"], a["cfo"],
                  a["metric"], None)
    cases = {
        "x NULL": dict(x=None), "offset NULL": dict(offset=None), "cfo NULL": dict(cfo=None),
        "cfo NULL, outputs given": dict(cfo=None, x_out=out, metric=met),
        "frames = 0": dict(frames=0), "frames < 0": dict(frames=-3),
        "W = 0": dict(W=0), "W = CP + 1": dict(W=17), "2 W + CP > 64": dict(K=48, CP=32, W=17, out_kin=80),
        "odd T": dict(K=63, out_kin=79), "S = 0": dict(S=0),
        "out_kin": dict(out_kin=79),
        "x_out off 16 bytes": dict(x_out=out + 4), "x off 16 bytes": dict(x=x + 4), "metric off 16 bytes": dict(metric=met + 4),
        "x_out is x": dict(x_out=x),
    }
    for what, over in cases.items():
        assert call(**over) == INVALID, what
