"""``dccn_classical_receive_supported`` and every refusal of ``dccn_classical_receive`` on a box without a GPU: the pointers are
small host buffers that a refused call never follows (as tests/test_lib_abi.py does it), so ``-1`` here means the call was
judged before any device work; a call that passed validation would try to launch and could not answer ``-1``."""
import ctypes as C
import math
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


GRIDS = [(7, 64, 16, 32, 320, 112), (7, 64, 4, 32, 320, 112), (7, 128, 32, 64, 640, 224)]


def test_struct_size_matches_the_header():
    from dl_ofdm_amd import _lib
    assert C.sizeof(_lib.ClassicalReceiveArgs) == 160
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "sizeof(dccn_classical_receive_args) == 160" in open(os.path.join(root, "include", "dccn.h")).read()


def test_supported_grid(lib):
    q = lib.dccn_classical_receive_supported
    for S, K, CP, P, D, E in GRIDS:
        for nbits in (1, 2, 3, 4):
            assert q(S, K, CP, P, D, E, nbits) == 1
        assert q(S, K, CP, P, D, E, 0) == 0 and q(S, K, CP, P, D, E, 5) == 0
    S, K, CP, P, D, E = GRIDS[0]
    assert q(1, K, CP, P, D, E, 2) == 1 and q(16, K, CP, P, D, E, 2) == 1       # one frame of 16 symbols fills the tile
    assert q(0, K, CP, P, D, E, 2) == 0 and q(17, K, CP, P, D, E, 2) == 0       # a frame must fit the 16-row tile
    assert q(S, 72, CP, P, D, E, 2) == 0 and q(S, 8, CP, P, D, E, 2) == 0       # K: a multiple of 16
    assert q(S, K, 15, P, D, E, 2) == 0 and q(S, K, -1, P, D, E, 2) == 0        # K + CP even: rows stay 16-byte aligned
    assert q(S, K, CP, 0, D, E, 2) == 0 and q(S, K, CP, P, 0, E, 2) == 0 and q(S, K, CP, P, D, 0, 2) == 0
    assert q(S, 256, 64, P, D, E, 2) == 0                                        # LDS: 16 (4 K + 4) floats alone pass 48 KB
    assert q(S, K, CP, 2100, D, E, 2) == 0                                       # ... and so do 2 (16/S) P floats of pilots
    assert q(S, K, CP, P, 317, E, 3) == 1                                        # a ragged row is a supported shape


def host_args(_lib, **over):
    """a call that would be accepted, with every pointer into a small host buffer at the alignment the entry asks for"""
    store = (C.c_char * 4096)()
    base = (C.addressof(store) + 255) // 256 * 256
    S, K, CP, P, D, E = GRIDS[0]
    a = _lib.ClassicalReceiveArgs(3, S, K, CP, P, D, E, 2, 4, CP, 2, 0.0, 3.0, 3.0, *([base] * 13))
    a._keep = store
    for k, v in over.items():
        setattr(a, k, v)
    return a, base


REFUSALS = [("frames", 0), ("frames", -3), ("S", 17), ("K", 60), ("CP", 15), ("P", 0), ("D", 0), ("E", 0), ("nbits", 0), ("nbits", 5),
            ("m", 3), ("m", 8), ("win", -1), ("win", 17), ("mode", 1), ("mode", 3), ("mode", 4), ("mode", -1),
            ("noise_var", -1.0), ("noise_var", math.nan), ("noise_var", math.inf), ("pv_re", math.nan), ("pv_im", math.inf)]


@pytest.mark.parametrize("field,value", REFUSALS)
def test_bad_scalars_are_refused_before_device_work(lib, field, value):
    from dl_ofdm_amd import _lib
    a, _ = host_args(_lib, **{field: value})
    assert lib.dccn_classical_receive(C.byref(a), None) == -1


def test_zero_pilot_value_and_null_struct_are_refused(lib):
    from dl_ofdm_amd import _lib
    a, _ = host_args(_lib, pv_re=0.0, pv_im=0.0)
    assert lib.dccn_classical_receive(C.byref(a), None) == -1
    assert lib.dccn_classical_receive(None, None) == -1


@pytest.mark.parametrize("field", ["dft", "w", "pil", "dat", "empty", "table", "labels", "x", "packed"])
def test_null_required_pointers_are_refused(lib, field):
    from dl_ofdm_amd import _lib
    a, _ = host_args(_lib, **{field: None})
    assert lib.dccn_classical_receive(C.byref(a), None) == -1


@pytest.mark.parametrize("field,off", [("x", 8), ("x", 4), ("chest", 4), ("y_freq", 4), ("table", 4), ("dft", 2), ("w", 1), ("pil", 2),
                                       ("dat", 2), ("empty", 1), ("labels", 2), ("llr", 2), ("noise", 1)])
def test_misaligned_pointers_are_refused(lib, field, off):
    from dl_ofdm_amd import _lib
    a, base = host_args(_lib)
    setattr(a, field, base + off)
    assert lib.dccn_classical_receive(C.byref(a), None) == -1
