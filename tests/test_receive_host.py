"""Host side of the label-free receive path (no GPU): the packed-bit row layout, the new C ABI's struct sizes and
host-side queries, argument validation that happens before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("D,nbits", [(320, 1), (320, 2), (320, 3), (320, 4), (50, 2), (50, 3), (4000, 2)])
def test_pack_unpack_match_numpy(D, nbits):
    from dl_ofdm_amd.receive import pack_bits, row_bytes, unpack_bits
    rng = np.random.RandomState(D + nbits)
    frames = 5
    hard = rng.randint(0, 2, (frames, D, nbits)).astype(np.uint8)
    packed = pack_bits(hard)
    nb = (D * nbits + 7) // 8
    assert row_bytes(D, nbits) == nb
    assert packed.dtype == np.uint8 and packed.shape == (frames, nb)
    for f in range(frames):
        assert np.array_equal(packed[f], np.packbits(hard[f].reshape(-1)))
    # padding bits of the last byte are 0
    pad = nb * 8 - D * nbits
    if pad:
        assert not (packed[:, -1] & ((1 << pad) - 1)).any()
        ones = pack_bits(np.ones((2, D, nbits), np.uint8))
        assert (ones[:, -1] == (0xFF << pad) & 0xFF).all() and (ones[:, :-1] == 0xFF).all()
    # unpack == numpy.unpackbits, and the round trip is the identity
    un = unpack_bits(packed, D, nbits)
    assert un.dtype == np.uint8 and un.shape == hard.shape
    for f in range(frames):
        assert np.array_equal(un[f].reshape(-1), np.unpackbits(packed[f])[:D * nbits])
    assert np.array_equal(un, hard)
    assert np.array_equal(pack_bits(un), packed)
    with pytest.raises(ValueError):
        unpack_bits(packed[:, :-1], D, nbits)


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "dccn.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_struct_sizes_match_header(lib):
    from dl_ofdm_amd import _lib
    # every member of both structs is a pointer or a size_t: 8 bytes each, no padding
    rb = _header_struct_fields("dccn_rx_receive_buffers")
    assert rb == [f for f, _ in _lib.RxReceiveBuffers._fields_]
    assert C.sizeof(_lib.RxReceiveBuffers) == 8 * len(rb) == 88
    ro = _header_struct_fields("dccn_receive_out")
    assert ro == [f for f, _ in _lib.ReceiveOut._fields_]
    assert C.sizeof(_lib.ReceiveOut) == 8 * len(ro) == 24


def test_host_side_queries(lib):
    from dl_ofdm_amd import _lib
    sizes = []
    for batch in (36, 1170, 20000):
        sh = _lib.RxShape(batch, 7, 80, 64, 320, 2)
        sizes.append(lib.dccn_rx_receive_workspace_size(C.byref(sh)))
    assert sizes[0] > 0 and sizes[0] <= sizes[1] <= sizes[2]
    assert lib.dccn_rx_receive_workspace_size(C.byref(_lib.RxShape(1170, 7, 80, 64, 320, 5))) == 0
    assert lib.dccn_dense_decide_supported(1170, 896, 640, 2) == 1
    assert lib.dccn_dense_decide_supported(1170, 896, 640, 5) == 0
    assert lib.dccn_dense_decide_supported(1170, 896, 641, 2) == 0
    # BPSK / QPSK at N = 64: the decision runs inside the dense launch; 16-QAM: dense + decision kernel
    assert lib.dccn_rx_receive_fused(C.byref(_lib.RxShape(1170, 7, 80, 64, 320, 2))) == 1
    assert lib.dccn_rx_receive_fused(C.byref(_lib.RxShape(36, 7, 80, 64, 320, 1))) == 1
    assert lib.dccn_rx_receive_fused(C.byref(_lib.RxShape(1170, 7, 80, 64, 320, 4))) == 0


def test_validation_precedes_device_work(lib):
    """NULL outputs, nbits outside 1..4, non-positive sizes and a short workspace are refused with the existing status
    codes before anything touches a device (this runs on a box without one)."""
    from dl_ofdm_amd import _lib
    one = C.c_void_p(16)            # never dereferenced: validation fails first
    assert lib.dccn_demod_decide(one, one, None, None, None, 4, 320, 2, None) == -1
    assert lib.dccn_demod_decide(one, one, one, None, None, 4, 320, 5, None) == -1
    assert lib.dccn_demod_decide(one, one, one, None, None, 0, 320, 2, None) == -1
    assert lib.dccn_demod_decide(None, one, one, None, None, 4, 320, 2, None) == -1
    assert lib.dccn_dense_decide_fwd(one, one, one, None, one, None, None, None, 1170, 896, 640, 2, None) == -1
    assert lib.dccn_dense_decide_fwd(one, one, one, None, one, one, None, None, 1170, 896, 640, 0, None) == -1
    assert lib.dccn_dense_decide_fwd(one, one, one, None, one, one, None, None, 1170, 896, 640, 3, None) == -1     # z required
    sh = _lib.RxShape(36, 7, 80, 64, 320, 1)
    nws = lib.dccn_rx_receive_workspace_size(C.byref(sh))
    b = _lib.RxReceiveBuffers(16, 16, 16, 16, None, None, None, None, 16, nws, None)
    assert lib.dccn_rx_receive_step(C.byref(sh), C.byref(b), None) == -1                   # packed == NULL
    b = _lib.RxReceiveBuffers(16, 16, 16, 16, None, 16, None, None, 16, nws - 1, None)
    assert lib.dccn_rx_receive_step(C.byref(sh), C.byref(b), None) == -2                   # short workspace
    assert lib.dccn_rx_receive_step(C.byref(_lib.RxShape(36, 7, 80, 64, 320, 5)), C.byref(b), None) == -1
    assert lib.dccn_rx_receive_step(C.byref(sh), None, None) == -1
    es = _lib.EqShape(12, 7, 64, 16, 1, 64, 320, 2, 16, 8)
    assert lib.dccn_eq_receive_step(C.byref(es), None, None, None) == -1
    out = _lib.ReceiveOut(None, None, None)
    eb = _lib.EqBuffers()
    assert lib.dccn_eq_receive_step(C.byref(es), C.byref(eb), C.byref(out), None) == -1    # packed == NULL


def test_receiver_refuses_cpu_device():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    with pytest.raises(_lib.DccnError):
        RxReceiver(RxDims(7, 80, 64, 320, 2), 4, None, device="cpu")
