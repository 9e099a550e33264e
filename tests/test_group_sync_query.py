"""Host side of the grouped receive front end (include/dccn.h dccn_frame_sync_grouped, dccn_capture_sync_grouped,
dccn_capture_acquire_grouped): the argument checks that need no device.  The addresses are fabricated (aligned numbers that are
never followed) and every call here is a REFUSED one: a refused call launches nothing, so nothing here touches a device."""
import ctypes as C
import os

import pytest

INVALID_ARG, WORKSPACE = -1, -2
S, K, CP, W = 7, 64, 16, 3
T = S * (K + CP)
FRAMES, J, NP = 5, 4, 16
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


def frame_links(n, cfo=True, metric=True, x_out=True):
    from dl_ofdm_amd import _lib
    t = (_lib.FrameLink * max(n, 1))()
    for i in range(n):
        b = base(i)
        t[i] = _lib.FrameLink(b, b + 1 * MB if x_out else None, b + 2 * MB, b + 3 * MB if cfo else None, b + 4 * MB if metric else None)
    return t


def capture_links(n, cfo=True, metric=True, x_out=True, n_samples=None, first=W):
    from dl_ofdm_amd import _lib
    ns = first + FRAMES * T + W if n_samples is None else n_samples
    t = (_lib.CaptureLink * max(n, 1))()
    for i in range(n):
        b = base(i)
        t[i] = _lib.CaptureLink(b, ns, first, None, 0, T, b + 1 * MB if x_out else None, b + 2 * MB, b + 3 * MB if cfo else None,
                                b + 4 * MB if metric else None)
    return t


def acquire_links(lib, n, metrics=True):
    from dl_ofdm_amd import _lib
    nws = lib.dccn_capture_acquire_workspace_size(S, K, CP, NP, J)
    assert nws > 0
    t = (_lib.AcquireLink * max(n, 1))()
    for i in range(n):
        b = base(i)
        t[i] = _lib.AcquireLink(b, (J + 2) * T, 0, b + 1 * MB, b + 2 * MB, b + 3 * MB, b + 4 * MB if metrics else None,
                                b + 5 * MB if metrics else None, b + 6 * MB, nws)
    return t


def fs(lib, n, t, shape=(S, K, CP, W), out_kin=K + CP):
    return lib.dccn_frame_sync_grouped(n, t, FRAMES, *shape, out_kin, None)


def cs(lib, n, t, shape=(S, K, CP, W), out_kin=K + CP):
    return lib.dccn_capture_sync_grouped(n, t, FRAMES, *shape, out_kin, None)


def aq(lib, n, t, j=J, shape=(S, K, CP)):
    return lib.dccn_capture_acquire_grouped(n, t, j, *shape, NP, None)


def test_link_counts_and_null_tables(lib):
    assert int(lib.dccn_chain_group_max()) == 8
    for k in (0, 9, -1):
        assert fs(lib, k, frame_links(8)) == INVALID_ARG
        assert cs(lib, k, capture_links(8)) == INVALID_ARG
        assert aq(lib, k, acquire_links(lib, 8)) == INVALID_ARG
    assert fs(lib, 2, None) == INVALID_ARG
    assert cs(lib, 2, None) == INVALID_ARG
    assert aq(lib, 2, None) == INVALID_ARG


@pytest.mark.parametrize("field", ["x_out", "cfo", "metric"])
def test_an_output_given_for_some_links_only(lib, field):
    for make, call in ((frame_links, fs), (capture_links, cs)):
        t = make(3)
        setattr(t[1], field, None)
        assert call(lib, 3, t) == INVALID_ARG, (make.__name__, field)
        t = make(3)
        for i in (0, 2):
            setattr(t[i], field, None)
        assert call(lib, 3, t) == INVALID_ARG, (make.__name__, field)


@pytest.mark.parametrize("field", ["sym_metric", "phase_metric"])
def test_an_acquisition_metric_given_for_some_links_only(lib, field):
    t = acquire_links(lib, 3)
    setattr(t[2], field, None)
    assert aq(lib, 3, t) == INVALID_ARG


def test_outputs_of_one_link_must_not_meet_another_link(lib):
    # frames: link 1's x_out inside link 0's x / x_out / offset; its offset on link 0's metric
    for field, target in (("x_out", "x"), ("x_out", "x_out"), ("offset", "metric"), ("cfo", "offset"), ("metric", "cfo")):
        t = frame_links(2)
        setattr(t[1], field, getattr(t[0], target) + 16)
        assert fs(lib, 2, t) == INVALID_ARG, (field, target)
    # captures: an output against the other link's capture, its outputs -- either order of the two links
    for a, b in ((0, 1), (1, 0)):
        for field, target in (("x_out", "cap"), ("x_out", "x_out"), ("offset", "cap"), ("cfo", "metric")):
            t = capture_links(2)
            setattr(t[a], field, getattr(t[b], target) + 16)
            assert cs(lib, 2, t) == INVALID_ARG, (a, b, field, target)
    # the last byte of a range counts, the first byte behind it does not (that call passes the checks: not made here)
    t = capture_links(2)
    t[1].offset = t[0].cap + (W + FRAMES * T + W) * 8 - 4
    assert cs(lib, 2, t) == INVALID_ARG
    # a start on the device is an input like the capture
    t = capture_links(2)
    t[0].first_dev, t[0].lo = t[1].offset, W
    t[0].n_samples = W + T - 1 + FRAMES * T + W
    assert cs(lib, 2, t) == INVALID_ARG
    # acquisition: outputs and workspaces
    for field, target in (("first_out", "first_out"), ("cfo_out", "sym_metric"), ("workspace", "workspace"), ("sym_metric", "cap"),
                          ("phase_metric", "pilot_sc"), ("workspace", "cap")):
        t = acquire_links(lib, 2)
        setattr(t[1], field, getattr(t[0], target) + (16 if field == "workspace" else 0 if field == "first_out" else 8))
        assert aq(lib, 2, t) == INVALID_ARG, (field, target)


def test_each_link_is_held_to_the_solo_rules(lib):
    # one misaligned pointer, one missing pointer, one capture a sample short -- on the LAST link, the others in order
    t = frame_links(3)
    t[2].x_out += 8
    assert fs(lib, 3, t) == INVALID_ARG
    t = frame_links(3)
    t[2].offset = None
    assert fs(lib, 3, t) == INVALID_ARG
    t = capture_links(3)
    t[2].cap += 8
    assert cs(lib, 3, t) == INVALID_ARG
    t = capture_links(3)
    t[2].n_samples -= 1
    assert cs(lib, 3, t) == INVALID_ARG
    t = capture_links(3)
    t[2].stride = T - 1
    assert cs(lib, 3, t) == INVALID_ARG
    t = capture_links(3)
    t[1].first_dev, t[1].lo = base(1) + 7 * MB + 4, W                        # off its 8-byte boundary
    assert cs(lib, 3, t) == INVALID_ARG
    t = capture_links(3)
    t[1].first_dev, t[1].lo = base(1) + 7 * MB, W                            # the last start the kernel may clamp to must fit
    assert cs(lib, 3, t) == INVALID_ARG
    t = acquire_links(lib, 3)
    t[2].n_samples -= 1
    assert aq(lib, 3, t) == INVALID_ARG
    t = acquire_links(lib, 3)
    t[0].first_out += 4
    assert aq(lib, 3, t) == INVALID_ARG
    t = acquire_links(lib, 3)
    t[1].workspace_bytes -= 1
    assert aq(lib, 3, t) == WORKSPACE


def test_unsupported_shapes(lib):
    assert lib.dccn_frame_sync_supported(S, K, CP, CP + 1) == 0
    assert fs(lib, 2, frame_links(2), shape=(S, K, CP, CP + 1)) == INVALID_ARG
    assert cs(lib, 2, capture_links(2), shape=(S, K, CP, CP + 1)) == INVALID_ARG
    assert fs(lib, 2, frame_links(2), shape=(3, 11, 4, 2)) == INVALID_ARG                 # an odd frame length
    assert fs(lib, 2, frame_links(2), out_kin=K + 1) == INVALID_ARG
    assert cs(lib, 2, capture_links(2), out_kin=K + 1) == INVALID_ARG
    assert lib.dccn_capture_acquire_supported(S, K, CP, NP, 257) == 0
    assert aq(lib, 2, acquire_links(lib, 2), j=257) == INVALID_ARG
    assert aq(lib, 2, acquire_links(lib, 2), shape=(65, K, CP)) == INVALID_ARG
    assert lib.dccn_frame_sync_grouped(2, frame_links(2), 0, S, K, CP, W, K + CP, None) == INVALID_ARG


def test_struct_sizes_match_header():
    from dl_ofdm_amd import _lib
    assert C.sizeof(_lib.FrameLink) == 5 * 8 and C.sizeof(_lib.CaptureLink) == 10 * 8 and C.sizeof(_lib.AcquireLink) == 10 * 8
