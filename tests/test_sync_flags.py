"""The ``sync`` flag of both harnesses and the host-side half of ``dccn_gen_static_apply_sync`` (apply + cyclic-prefix alignment as
one launch): what can be checked without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dccn_gen_static_apply_sync_supported", "dccn_gen_static_apply_sync")


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_apply_sync_supported_truth_table(lib):
    """= dccn_gen_static_supported && dccn_frame_sync_supported: the generator's two shapes, 1 <= W <= CP"""
    q = lib.dccn_gen_static_apply_sync_supported
    for W in range(0, 18):
        assert q(7, 64, 16, W) == (1 if 1 <= W <= 16 else 0), W
    assert q(7, 64, 4, 4) == 1
    assert q(7, 64, 4, 5) == 0
    assert q(7, 64, 8, 3) == 0                 # the generator has no CP = 8 (the alignment stage alone takes it)
    assert lib.dccn_frame_sync_supported(7, 64, 8, 3) == 1
    assert q(0, 64, 16, 3) == 0
    for S, K, CP, W in [(7, 64, 16, 3), (7, 64, 4, 3), (7, 64, 16, 17), (7, 32, 16, 3), (7, 64, 4, 0)]:
        assert q(S, K, CP, W) == (1 if lib.dccn_gen_static_supported(S, K, CP) and lib.dccn_frame_sync_supported(S, K, CP, W)
                                  else 0)


@pytest.mark.parametrize("harness", ["receiver", "receiver_mp"])
def test_sync_with_align_window_is_refused(harness):
    import importlib
    H = importlib.import_module("dl_ofdm_amd." + harness)
    assert H.Flags().sync == 0
    assert H.Flags(sync=3).sync == 3 and H.parse_flags(["--sync=3"]).sync == 3
    with pytest.raises(ValueError, match="align_window"):
        H.Flags(sync=3, align_window=True)
    with pytest.raises(ValueError, match="sync"):
        H.Flags(sync=-1)
    f = H.Flags(sync=3, device_data=True)
    f.align_window = True                        # set after construction: the harness itself checks before any launch
    with pytest.raises(ValueError, match="align_window"):
        H.train(f, device="cuda", verbose=False, run_test=False, **({"rx_params": {}} if harness == "receiver_mp" else {}))


def test_sync_needs_device_data():
    """there is no host alignment stage: the basic-receiver harness refuses before it builds anything"""
    from dl_ofdm_amd import receiver as R
    with pytest.raises(ValueError, match="device_data"):
        R.train(R.Flags(sync=3, device_data=False), verbose=False, run_test=False)


def test_fused_sync_flag_defaults_to_one_launch():
    from dl_ofdm_amd import receiver_mp as H
    assert H.Flags().fused_sync is True
    assert H.parse_flags(["--sync=3", "--fused_sync=False"]).fused_sync is False


def test_header_declares_and_library_exports_the_two_symbols(lib):
    from dl_ofdm_amd import _lib
    src = open(os.path.join(ROOT, "include", "dccn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dccn_[a-z0-9_]+)\s*\(", src))
    for n in NEW:
        assert n in declared, "include/dccn.h does not declare %s" % n
        assert hasattr(lib, n), "libdccn.so does not export %s" % n
        assert n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dccn_gen_static_apply_sync"][1]) == 9
