"""Host side of one carrier offset per capture (include/dccn.h dccn_capture_sync_pooled): the fp64 restatement
(tests/capture_pool_ref.py) held to capture_sync_ref's per-frame estimate, to the estimators it must not be mistaken for and to
the statistical claim it is built on; and the argument checks of the new entries that need no device.  The addresses of those
calls are fabricated (aligned numbers that are never followed) and every call is a REFUSED one: nothing here launches."""
import ctypes as Ct
import os

import numpy as np
import pytest

import capture_pool_ref as P
import capture_sync_ref as C
import frame_cfo_ref as F
import frame_sync_ref as R

S, K = R.S, R.K


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel,snr,CP,W", P.FADING + (("AWGN", 30.0, 16, 16),))
def test_one_frame_is_the_per_frame_estimate(channel, snr, CP, W):
    """frames = 1: the pooled estimate and the derotated frame are capture_sync_ref's, exactly"""
    cap, stride = P.case_capture(channel, snr, CP, 0, P.EPS[0])
    first = C.case_first(CP, 0)
    for f in (0, 1, 17):
        b = first + f * stride
        off, lam, phi, gam, gf, total, eps = P.reference(cap, b, stride, 1, S, K, CP, W)
        o1, _, _, g1 = C.reference(cap, b, stride, 1, S, K, CP, W)
        per_frame = F.cfo_of(C.gamma_at(g1, o1, W))
        assert np.array_equal(off, o1) and total == gf[0] and eps == per_frame[0]
        assert np.array_equal(P.derotated(cap, b, stride, off, eps, S, K, CP), C.derotated(cap, b, stride, o1, per_frame, S, K, CP))


def test_the_stated_order():
    """pooled_sum walks the header's order: in fp64 on integers it is the exact sum, in float32 it is reproducible by hand for a
    count that gives several terms per lane, and DEPTH counts its rounded additions"""
    rs = np.random.RandomState(11)
    for n in (1, 3, 64, 65, 259):
        v = rs.randint(-1000, 1000, n).astype(np.float64)
        assert P.pooled_sum(v) == v.sum()
        assert P.pooled_sum(v + 1j * v[::-1]) == complex(v.sum(), v.sum())
    g = rs.standard_normal(259).astype(np.float32)
    part = np.zeros(64, dtype=np.float32)
    for f in range(259):                                # lane f % 64 takes frame f, ascending
        part[f % 64] = np.float32(part[f % 64] + g[f])
    for d in (1, 2, 4, 8, 16, 32):
        part = np.array([np.float32(part[l] + part[l ^ d]) for l in range(64)], dtype=np.float32)
    assert len(set(part.tolist())) == 1                 # every lane arrives at the same bits
    got = P.pooled_sum(g)
    assert got.dtype == np.float32 and got == part[0]
    assert [P.DEPTH(n) for n in (1, 64, 65, 259, 20000)] == [6, 6, 7, 10, 318]


PLANTED = tuple((ch, snr, CP, W) for ch, snr in (("ETU", 5.0), ("EPA", 5.0), ("EVA", 30.0)) for CP, W in ((16, 3), (4, 4)))


@pytest.mark.parametrize("frames", [3, 5])
@pytest.mark.parametrize("channel,snr,CP,W", PLANTED)
def test_other_estimators_are_told_apart(channel, snr, CP, W, frames):
    """planted errors: the mean of the per-frame angles and the sum of unit vectors each miss the definition by more than
    100 times the bound the GPU is held to -- a kernel that computed either would fail its test.  On the fading channels of the
    GPU test, at the two smallest frame counts above one block's first wave: with few frames the three estimators differ by a
    fraction of one frame's own error.  (With many frames a wrong estimator may land near the right one in a given draw: at 73
    frames the gaps are 34 to 5800 bounds, 34 on ETU 5 dB CP 4 and 43 on EVA 30 dB CP 16 -- still failures of the GPU test,
    but no margin to assert.  On AWGN 30 dB the estimators coincide to 3e-6 and nothing is told apart.)"""
    for eps0 in P.EPS:
        off, lam, phi, gam, gf, total, eps = P.case_reference(channel, snr, CP, W, 0, 0, eps0, frames)
        bound = P.pool_bound(phi, gf, total)
        assert bound < 1e-5
        for wrong in (P.mean_of_angles(gf), P.unit_vector_sum(gf)):
            gap = float(F.circle(wrong - eps))
            print("%s %g dB CP %d W %d frames %d eps %+.3f: gap %.2e bound %.2e" % (channel, snr, CP, W, frames, eps0, gap, bound))
            assert gap > 100.0 * bound


@pytest.mark.parametrize("channel,snr,CP,W", P.FADING)
def test_pooling_beats_the_per_frame_median(channel, snr, CP, W):
    """the claim the stage is built on, on the seeded cases: at 73 frames the pooled estimate is closer to the true offset than
    the median per-frame estimate"""
    for eps0 in P.EPS:
        off, lam, phi, gam, gf, total, eps = P.case_reference(channel, snr, CP, W, 0, 0, eps0)
        per_frame = F.circle(F.cfo_of(gf) - eps0)
        err = float(F.circle(eps - eps0))
        print("%s %g dB CP %d W %d eps %+.3f: per-frame median %.2e max %.2e, pooled %.2e"
              % (channel, snr, CP, W, eps0, np.median(per_frame), per_frame.max(), err))
        assert gf.shape[0] == C.FRAMES == 73 and err < np.median(per_frame)


def test_zero_capture():
    cap = np.zeros((3 * S * (K + 16) + 6, 2), np.float32)
    off, lam, phi, gam, gf, total, eps = P.reference(cap, 3, S * (K + 16), 3, S, K, 16, 3)
    assert total == 0 and eps == 0.0 and not np.signbit(eps)


# ---- the library's host checks ----------------------------------------------------------------------------------------------
INVALID_ARG, WORKSPACE = -1, -2
CP, W = 16, 3
T = S * (K + CP)
FRAMES = 5
MB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def base(i):
    """link i's own 16 MB of fabricated address space (256-byte aligned, like a device allocation)"""
    return 0x7000_0000_0000 + i * 16 * MB


def links(lib, n, metric=True, first=W):
    from dl_ofdm_amd import _lib
    nws = lib.dccn_capture_sync_pooled_workspace_size(FRAMES)
    t = (_lib.PooledLink * max(n, 1))()
    for i in range(n):
        b = base(i)
        t[i] = _lib.PooledLink(b, first + FRAMES * T + W, first, None, 0, T, b + 1 * MB, b + 2 * MB, b + 3 * MB,
                               b + 4 * MB if metric else None, b + 5 * MB, nws)
    return t


def grouped(lib, n, t, shape=(S, K, CP, W), out_kin=K + CP, frames=FRAMES):
    return lib.dccn_capture_sync_pooled_grouped(n, t, frames, *shape, out_kin, None)


def solo(lib, l, shape=(S, K, CP, W), out_kin=K + CP, frames=FRAMES):
    return lib.dccn_capture_sync_pooled(l.cap, l.n_samples, l.first, l.first_dev, l.lo, l.stride, frames, *shape, out_kin, l.x_out,
                                        l.offset, l.cfo, l.metric, l.workspace, l.workspace_bytes, None)


def test_symbols_and_workspace_size(lib):
    for name in ("dccn_capture_sync_pooled_workspace_size", "dccn_capture_sync_pooled", "dccn_capture_sync_pooled_grouped"):
        assert hasattr(lib, name)
    size = lib.dccn_capture_sync_pooled_workspace_size
    assert size(0) == 0 and size(-3) == 0
    sizes = [size(n) for n in (1, 3, 5, 73, 259, 20000)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(set(sizes))
    assert all(s >= 8 * n for s, n in zip(sizes, (1, 3, 5, 73, 259, 20000)))           # Gamma_f as float2 [frames]


def test_struct_size_matches_header():
    from dl_ofdm_amd import _lib
    assert Ct.sizeof(_lib.PooledLink) == 12 * 8
    assert [f[0] for f in _lib.PooledLink._fields_[:10]] == [f[0] for f in _lib.CaptureLink._fields_]


def test_solo_refusals(lib):
    def one(**kw):
        l = links(lib, 1)[0]
        for k, v in kw.items():
            setattr(l, k, v)
        return l
    for field in ("cap", "x_out", "offset", "cfo", "workspace"):                        # required pointers
        assert solo(lib, one(**{field: None})) == INVALID_ARG, field
    l = one()
    assert solo(lib, one(cap=l.cap + 8)) == INVALID_ARG                                 # alignment
    assert solo(lib, one(x_out=l.x_out + 8)) == INVALID_ARG
    assert solo(lib, one(metric=l.metric + 4)) == INVALID_ARG
    assert solo(lib, one(cfo=l.cfo + 2)) == INVALID_ARG
    assert solo(lib, one(workspace=l.workspace + 8)) == INVALID_ARG
    assert solo(lib, one(workspace_bytes=l.workspace_bytes - 1)) == WORKSPACE           # a short workspace
    assert solo(lib, one(workspace_bytes=0)) == WORKSPACE
    assert solo(lib, one(), frames=FRAMES + 1) == INVALID_ARG                           # (the capture is a frame short first)
    size = lib.dccn_capture_sync_pooled_workspace_size
    assert size(FRAMES + 2) > size(FRAMES) == l.workspace_bytes
    assert solo(lib, one(n_samples=l.n_samples + 2 * T), frames=FRAMES + 2) == WORKSPACE    # sized for 5 frames, asked for 7
    assert solo(lib, one(n_samples=l.n_samples - 1)) == INVALID_ARG                     # dccn_capture_sync's rules for `first`
    assert solo(lib, one(first=W - 1)) == INVALID_ARG
    assert solo(lib, one(stride=T - 1)) == INVALID_ARG
    assert solo(lib, one(x_out=l.cap + 16)) == INVALID_ARG                              # x_out inside the capture
    assert solo(lib, one(), frames=0) == INVALID_ARG
    assert solo(lib, one(), out_kin=K + 1) == INVALID_ARG
    assert lib.dccn_capture_sync_supported(S, K, CP, CP + 1) == 0                       # accepted where that query says so
    assert solo(lib, one(), shape=(S, K, CP, CP + 1)) == INVALID_ARG
    # dccn_capture_sync_at's rules once first_dev is given: its alignment, lo >= W, and the LAST start it may clamp to must fit
    dev = base(0) + 7 * MB
    assert solo(lib, one(first_dev=dev + 4, lo=W, n_samples=l.n_samples + T)) == INVALID_ARG
    assert solo(lib, one(first_dev=dev, lo=W - 1, n_samples=l.n_samples + T)) == INVALID_ARG
    assert solo(lib, one(first_dev=dev, lo=W, n_samples=W + T - 1 + FRAMES * T + W - 1)) == INVALID_ARG
    assert solo(lib, one(first_dev=dev, lo=W)) == INVALID_ARG                           # fits `first`, not lo + T - 1


def test_grouped_refusals(lib):
    for k in (0, 9, -1):
        assert grouped(lib, k, links(lib, 8)) == INVALID_ARG
    assert grouped(lib, 2, None) == INVALID_ARG
    t = links(lib, 3)
    t[1].metric = None                                                                  # metric for every link or for none
    assert grouped(lib, 3, t) == INVALID_ARG
    for field in ("x_out", "cfo", "workspace", "offset"):                               # required on every link
        t = links(lib, 3)
        setattr(t[2], field, None)
        assert grouped(lib, 3, t) == INVALID_ARG, field
    t = links(lib, 3)
    t[2].workspace_bytes -= 1                                                           # one link with a short workspace
    assert grouped(lib, 3, t) == WORKSPACE
    t = links(lib, 3)
    t[2].n_samples -= 1                                                                 # each link by the solo rules
    assert grouped(lib, 3, t) == INVALID_ARG
    # an output of one link on an output or an input of another, either order of the two
    for a, b in ((0, 1), (1, 0)):
        for field, target in (("x_out", "cap"), ("x_out", "x_out"), ("offset", "cap"), ("cfo", "metric"), ("workspace", "x_out"),
                              ("workspace", "workspace"), ("cfo", "workspace"), ("workspace", "cap")):
            t = links(lib, 2)
            setattr(t[a], field, getattr(t[b], target) + 16)
            assert grouped(lib, 2, t) == INVALID_ARG, (a, b, field, target)
    t = links(lib, 2)                                                                   # a start on the device is an input
    t[0].first_dev, t[0].lo = t[1].offset, W
    t[0].n_samples = W + T - 1 + FRAMES * T + W
    assert grouped(lib, 2, t) == INVALID_ARG


def test_python_scope_checks_come_first():
    """an unknown scope, and "capture" without cfo: ValueError before a device is looked for"""
    from dl_ofdm_amd import sync
    for kw in (dict(cfo=True, cfo_scope="link"), dict(cfo=False, cfo_scope="capture"), dict(cfo_scope="capture")):
        with pytest.raises(ValueError):
            sync.CaptureSync(S, K, CP, W, FRAMES, device="cpu", **kw)
        with pytest.raises(ValueError):
            sync.CaptureSyncGroup(S, K, CP, W, FRAMES, 2, device="cpu", **kw)
    assert sync.check_cfo_scope(True, "capture") is True and sync.check_cfo_scope(True, "frame") is False
    assert sync.check_cfo_scope(False, "frame") is False
