"""Every public workspace-size query answers what tests/golden/workspace_sizes.json recorded (no GPU: the queries plan for
256 compute units when no device is visible, which is what an MI355X reports).  The fixture comes from
tests/golden/make_workspace_sizes.py; a layout that changes on purpose regenerates it there."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = {"dccn_rx", "dccn_rx_receive", "dccn_rx_backward", "dccn_batch_moment_norm", "dccn_clip_power", "dccn_dense_bwd_w",
           "dccn_cconv_gemm_bwd_w", "dccn_cconv_patch_bwd_w", "dccn_cconv_patch_bwd_x", "dccn_cconv1d_bwd", "dccn_demod_tail",
           "dccn_dense_tail", "dccn_ingraph_awgn", "dccn_classical", "dccn_channel_awgn", "dccn_channel_doppler_awgn",
           "dccn_channel_groups_awgn", "dccn_eq_monitor"}


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as f:
        return json.load(f)


def _ask(lib, query, args):
    from dl_ofdm_amd import _lib
    if query == "dccn_rx":
        return lib.dccn_rx_workspace_size(C.byref(_lib.RxShape(*args[:6])), args[6])
    if query == "dccn_rx_receive":
        return lib.dccn_rx_receive_workspace_size(C.byref(_lib.RxShape(*args)))
    return getattr(lib, query + "_workspace_size")(*args)


def test_fixture_covers_every_query(recorded):
    assert {r["query"] for r in recorded} == QUERIES
    by = {(r["query"], tuple(r["args"])): r["bytes"] for r in recorded}
    # the sizes the layouts had when the fixture was first recorded
    assert by[("dccn_rx", (36, 7, 80, 64, 320, 2, 1))] == 29600000
    assert by[("dccn_rx", (585, 7, 1096, 1024, 4000, 2, 1))] == 485111296
    assert by[("dccn_dense_bwd_w", (1170, 896, 640))] == 18370560
    assert by[("dccn_channel_awgn", (73, 560, 9))] == 350976
    for q in QUERIES - {"dccn_classical", "dccn_clip_power"}:       # (those two take no argument that can be invalid)
        assert any(r["bytes"] == 0 for r in recorded if r["query"] == q), q
        assert any(r["bytes"] > 0 for r in recorded if r["query"] == q), q


def test_sizes_match_fixture(lib, recorded):
    wrong = [(r["query"], r["args"], r["bytes"], got) for r in recorded
             for got in [_ask(lib, r["query"], r["args"])] if got != r["bytes"]]
    assert not wrong, "query, args, recorded, answered: %r" % (wrong[:10],)
