"""Host side of the frame-sync tests (no GPU): the fp64 restatement of the estimator (tests/frame_sync_ref.py) is a usable
yardstick on the exact inputs of every GPU case, it recovers a pure roll, and the library's host-only shape query and its ctypes
prototypes are there."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_sync_ref as R


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("CP,W,channel,snr", R.all_cases())
def test_the_reference_decides_the_inputs_of_every_gpu_case(CP, W, channel, snr):
    """At most CAP of a case's frames may sit inside the fp32 margin -- at every frame count the GPU test runs (the leading
    frames of the same batch), met by the reference alone."""
    off, lam, phi, ok = R.case_reference(channel, snr, CP, W)
    assert (lam <= 1e-12 * phi.max()).all()                      # Lambda <= 0: |sum p| <= sum |p| <= sum e
    assert (off >= -W).all() and (off <= W).all()
    for n in R.FRAME_COUNTS:
        bad = int((~ok[:n]).sum())
        print("%s %g dB CP %d W %d: %d of %d frames undecidable; offsets %s"
              % (channel, snr, CP, W, bad, n, dict(zip(*[v.tolist() for v in np.unique(off[:n], return_counts=True)]))))
        assert bad <= R.CAP * n


@pytest.mark.parametrize("CP,W", [(16, 16), (16, 3), (4, 4), (4, 1)])
def test_the_reference_recovers_a_pure_roll(CP, W):
    """AWGN, 30 dB: frames delayed by d samples (circularly) give offset0 + d, on the frames that are decidable before and
    after the roll and whose offset stays inside the window."""
    n = 73
    x = R.case_frames("AWGN", 30.0, CP)[:n]
    off0, lam0, phi0 = R.reference(x, R.K, CP, W)
    ok0 = R.decidable(lam0, phi0)
    assert ok0.mean() >= 1 - R.CAP and (off0[ok0] == 0).mean() > 0.9      # the generator's AWGN frames sit on the window
    checked = 0
    for d in range(-W, W + 1):
        off, lam, phi = R.reference(R.roll_frames(x, d), R.K, CP, W)
        use = ok0 & R.decidable(lam, phi) & (np.abs(off0 + d) <= W)
        assert np.array_equal(off[use], off0[use] + d), d
        # and rotating by the estimate undoes the roll
        assert np.array_equal(R.aligned(R.roll_frames(x, d), off)[use], R.aligned(x, off0)[use])
        checked += int(use.sum())
    assert checked >= 0.9 * n * (2 * W + 1)


def test_supported_truth_table(lib):
    q = lib.dccn_frame_sync_supported
    for W in (1, 3, 16):
        assert q(7, 64, 16, W) == 1
    for W in (1, 4):
        assert q(7, 64, 4, W) == 1
    assert q(7, 64, 16, 0) == 0 and q(7, 64, 4, 0) == 0               # W = 0
    assert q(7, 64, 16, 17) == 0 and q(7, 64, 4, 5) == 0              # W = CP + 1
    assert q(7, 1024, 256, 16) == 0                                   # 2 W + CP > 64 (and four frames outgrow the LDS)
    assert q(7, 63, 16, 3) == 0 and q(1, 64, 3, 1) == 0               # odd T
    assert q(0, 64, 16, 3) == 0 and q(7, 0, 16, 3) == 0 and q(7, 64, 0, 1) == 0 and q(-1, 64, 16, 3) == 0
    assert q(7, 64, 32, 16) == 1 and q(7, 64, 32, 17) == 0            # 2 W + CP = 64 is the last that fits
    assert q(2, 63, 16, 3) == 1                                       # an even S makes an odd symbol length fit
    assert q(1, 2030, 16, 3) == 0 and q(1, 1904, 16, 3) == 1          # four frames + lag sums against 64 KB of LDS


def test_lib_carries_the_prototypes(lib):
    from dl_ofdm_amd import _lib
    assert _lib.SIGNATURES["dccn_frame_sync_supported"] == (C.c_int, [C.c_int] * 4)
    res, args = _lib.SIGNATURES["dccn_frame_sync"]
    assert res is C.c_int and args == [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
    assert lib.dccn_frame_sync.argtypes == args and lib.dccn_frame_sync_supported.restype is C.c_int
    # argument validation needs no device: host pointers a refused call never dereferences
    store = (C.c_char * 4096)()
    p = (C.addressof(store) + 255) // 256 * 256
    assert lib.dccn_frame_sync(None, 4, 7, 64, 16, 3, 80, p + 2048, p + 1024, None, None) == -1
    assert lib.dccn_frame_sync(p, 0, 7, 64, 16, 3, 80, None, p + 1024, None, None) == -1
    assert lib.dccn_frame_sync(p, 4, 7, 64, 16, 17, 80, None, p + 1024, None, None) == -1


def test_framesync_refuses_without_a_device():
    import torch
    from dl_ofdm_amd import _lib, sync
    with pytest.raises(_lib.DccnError):
        sync.FrameSync(7, 64, 16, 3, 4, device="cpu")
    if not torch.cuda.is_available():
        return
    with pytest.raises(_lib.DccnError):
        sync.FrameSync(7, 64, 16, 17, 4)
