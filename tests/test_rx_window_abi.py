"""dccn_gen_static_apply_window -- the fused generator's batch as a cp=False receiver sees it -- is declared in include/dccn.h,
exported by the built library and bound in dl_ofdm_amd/_lib.py with the arguments of dccn_gen_static_apply (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dccn_gen_static_apply_window"


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_windowed_apply_is_declared_exported_and_bound(lib):
    from dl_ofdm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dccn.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert m, "include/dccn.h does not declare %s" % NAME
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 4 and params[0].startswith("const dccn_gen_static*") and params[3].startswith("dccn_stream_t")
    assert hasattr(lib, NAME), "libdccn.so does not export %s" % NAME
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == 4
    assert (restype, argtypes) == _lib.SIGNATURES["dccn_gen_static_apply"]
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == list(argtypes)


def test_windowed_apply_refuses_a_null_descriptor_without_touching_a_device(lib):
    assert getattr(lib, NAME)(None, None, None, None) == -1          # DCCN_ERR_INVALID_ARG, decided on the host
