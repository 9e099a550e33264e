"""Host side of the equaliser's ABI unit (csrc/dccn_abi_eq.hip, csrc/eq_step.h): the workspace layout of the fused step, pinned
byte for byte, and the argument checks of the grouped entry points that need no device.  Nothing here launches.

tests/golden/eq_workspace_layout.json is a recording, not a computation: `python tests/test_eq_abi_host.py --record` writes it from
whatever library dl_ofdm_amd._lib loads (DCCN_LIB_PATH selects another build); it was recorded from the build of the commit before
the layout's description moved into one table (profiles/eq_abi_once.md)."""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eq_workspace_layout.json")

# every name include/dccn.h documents for dccn_eq_workspace_tensor, and the rest of the names the lookup offers
FORWARD = ("x_norm", "ln", "t1", "y", "d1", "d2", "d3", "d4", "T", "be", "eq", "corr", "eqc", "corc", "cat", "fft", "z")
TRAINING = ("dz", "dfft", "dout", "dcat", "deqc", "dcorc", "deq", "dcorr", "dy", "dh", "dT", "dbe", "dd4", "dd3", "dd2", "dd1", "dflat",
            "dt1")
# N = 64, S = 7, F = 64, D = 320, QPSK; pilot_size 12 (2 P = 24) is the case without the bottleneck's partials
BATCHES, PREFIXES, PILOTS = (12, 73, 97), ((1, 16), (0, 16), (1, 4)), (8, 16, 12)


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _cases():
    return list(itertools.product(BATCHES, PREFIXES, PILOTS))


def _key(batch, prefix, pilot):
    return "batch=%d cp=%d CP=%d pilot_size=%d" % (batch, prefix[0], prefix[1], pilot)


def _shape(batch, prefix, pilot):
    from dl_ofdm_amd import _lib
    return _lib.EqShape(batch, 7, 64, prefix[1], prefix[0], 64, 320, 2, pilot, 8)


def _layout(lib, sh):
    offs = (C.c_longlong * 21)()
    assert lib.dccn_eq_param_offsets(C.byref(sh), offs) == 0
    out = dict(workspace_size=[int(lib.dccn_eq_workspace_size(C.byref(sh), t)) for t in (0, 1)], param_offsets=[int(v) for v in offs])
    off, cnt = C.c_size_t(), C.c_size_t()
    for train in (0, 1):
        tensors = {}
        for name in FORWARD + (TRAINING if train else ()):
            assert lib.dccn_eq_workspace_tensor(C.byref(sh), train, name.encode(), C.byref(off), C.byref(cnt)) == 0, name
            tensors[name] = [int(off.value), int(cnt.value)]
        out["tensors_train" if train else "tensors_eval"] = tensors
    return out


def record(lib):
    return {_key(*c): _layout(lib, _shape(*c)) for c in _cases()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_holds_every_case(golden):
    assert sorted(golden) == sorted(_key(*c) for c in _cases()) and len(golden) == 27


@pytest.mark.parametrize("case", _cases(), ids=lambda c: _key(*c).replace(" ", "-"))
def test_workspace_layout_is_the_recorded_one(lib, golden, case):
    """sizes, parameter offsets, and (byte offset, count) of every named tensor: compared exactly"""
    got, want = _layout(lib, _shape(*case)), golden[_key(*case)]
    assert got["workspace_size"] == want["workspace_size"]
    assert got["param_offsets"] == want["param_offsets"]
    for section in ("tensors_eval", "tensors_train"):
        assert sorted(got[section]) == sorted(want[section])
        for name in got[section]:
            assert got[section][name] == want[section][name], (section, name)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: _key(*c).replace(" ", "-"))
def test_lookup_refusals(lib, case):
    """what test_lib_abi.py::test_eq_workspace_tensor_lookup asserts on one shape, on every shape of the recording: a training-only
    name in an evaluation workspace, an unknown name and a NULL name are refused"""
    sh = _shape(*case)
    off, cnt = C.c_size_t(), C.c_size_t()
    for name in TRAINING:
        assert lib.dccn_eq_workspace_tensor(C.byref(sh), 0, name.encode(), C.byref(off), C.byref(cnt)) == -1, name
    for name in (b"nope", b"dtail", b"bn_part", b""):
        assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, name, C.byref(off), C.byref(cnt)) == -1, name
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, None, C.byref(off), C.byref(cnt)) == -1
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, b"y", None, C.byref(cnt)) == -1
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, b"y", C.byref(off), None) == -1


def test_named_tensors_do_not_overlap(lib):
    """inside the sized workspace, on 256-byte boundaries, one after the other in the order of the names"""
    for case in _cases():
        lay = _layout(lib, _shape(*case))
        for train, section in ((0, "tensors_eval"), (1, "tensors_train")):
            end = 0
            for name in FORWARD + (TRAINING if train else ()):
                off, cnt = lay[section][name]
                assert off % 256 == 0 and cnt > 0 and off >= end, (case, name)
                end = off + 4 * cnt
            assert end <= lay["workspace_size"][train], case


# ---- the grouped entry points: the chain count and the tables, before any pointer is followed -------------------------------------
def _tables(n):
    """n zeroed structs of every kind a grouped call takes (and valid shapes): every call below is refused for its chain count or
    its tables, before a pointer inside a struct is followed"""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.equalizer_group import _ptr_array
    keep = dict(shapes=[_shape(73, (1, 16), 8) for _ in range(n)], bufs=[_lib.EqBuffers() for _ in range(n)],
                gens=[_lib.GenStatic() for _ in range(n)], mons=[_lib.EqMonitor() for _ in range(n)])
    ptrs = {k: _ptr_array(v) for k, v in keep.items()}
    ptrs["x"] = (C.c_void_p * n)(*([256] * n))                 # (never dereferenced on the host)
    return keep, ptrs


def _holes(structs):
    """two-entry tables with a NULL entry, at chain 1 and at chain 0"""
    return (C.c_void_p * 2)(C.addressof(structs[0]), None), (C.c_void_p * 2)(None, C.addressof(structs[1]))


def test_grouped_train_step_checks_the_chain_count_and_the_tables(lib):
    from dl_ofdm_amd import _lib
    keep, t = _tables(9)
    hp = _lib.AdamHParams()
    for k in (0, 9, -1):
        assert lib.dccn_eq_train_step_grouped(k, t["shapes"], t["bufs"], hp, None) == -1
    assert lib.dccn_eq_train_step_grouped(2, None, t["bufs"], hp, None) == -1
    assert lib.dccn_eq_train_step_grouped(2, t["shapes"], None, hp, None) == -1
    for hole in _holes(keep["shapes"]):
        assert lib.dccn_eq_train_step_grouped(2, hole, t["bufs"], hp, None) == -1
    for hole in _holes(keep["bufs"]):
        assert lib.dccn_eq_train_step_grouped(2, t["shapes"], hole, hp, None) == -1


def test_grouped_generator_checks_the_chain_count_and_the_tables(lib):
    keep, t = _tables(9)
    for k in (0, 9, -1):
        assert lib.dccn_gen_static_frames_grouped(k, t["gens"], None) == -1
        assert lib.dccn_gen_static_apply_grouped(k, t["gens"], t["x"], None, None) == -1
    assert lib.dccn_gen_static_frames_grouped(2, None, None) == -1
    assert lib.dccn_gen_static_apply_grouped(2, None, t["x"], None, None) == -1
    assert lib.dccn_gen_static_apply_grouped(2, t["gens"], None, None, None) == -1
    for hole in _holes(keep["gens"]):
        assert lib.dccn_gen_static_frames_grouped(2, hole, None) == -1
        assert lib.dccn_gen_static_apply_grouped(2, hole, t["x"], None, None) == -1
    assert lib.dccn_gen_static_apply_grouped(2, t["gens"], (C.c_void_p * 2)(None, 256), None, None) == -1


def test_grouped_monitors_check_the_chain_count_and_the_tables(lib):
    keep, t = _tables(9)
    for k in (0, 9, -1):
        assert lib.dccn_eq_monitor_accumulate_grouped(k, t["mons"], None) == -1
    assert lib.dccn_eq_monitor_accumulate_grouped(2, None, None) == -1
    for hole in _holes(keep["mons"]):
        assert lib.dccn_eq_monitor_accumulate_grouped(2, hole, None) == -1


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_eq_abi_host.py --record")
    sys.path.insert(0, ROOT)
    from dl_ofdm_amd import _lib
    with open(GOLDEN, "w") as f:
        json.dump(record(_lib.load()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d shapes from %s" % (len(_cases()), _lib.LIB_PATH))
