"""The fused backward launch (csrc/rx_bwd.h) against float64 at every filter count and frame length it accepts (``-m gpu``).

rx_bwd_fused_ok takes any S, any F with 2F a multiple of 64, kin of 64 or 80 and any even D; every other GPU test reaches the
launch at S = 7, F = 64 only: two column tiles per symbol, 14 per row of tiles.  The shapes of rx_backward_ref.SHAPES are the
smallest accepted ones with one, three, four and five tiles per symbol, an odd tile count (xcd_tile), fewer than eight tiles,
S = 1 and S = 14, one live row in the last row tile, no masked row at all, a ragged k-tile of dX (2D = 4), and two and five
(graded) dense dW ranges next to F != 64; tests/test_rx_backward_ref.py shows on the CPU which index errors each of them sees.

Per shape: the plan facts of the table through dccn_rx_bwd_fused_supported and dccn_gemm_route_query, then dccn_rx_backward into
the guarded outputs and the NaN-filled workspace of test_gpu_tile_variants.py -- dfft, dense dW / dbias and the C-Conv dW / dbias
(on the GPU's own dfft) at RTOL of test_gpu_ops.py, as test_rx_backward_fused holds them; a call with dfft = NULL and a third full
call leave the same bits.  Refused geometries launch nothing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rx_backward_ref as R
from test_gemm_route_query import route
from test_gpu_tile_variants import all_nan, check_rx_backward, run_rx_backward, rx_case

pytestmark = pytest.mark.gpu

GRADS = ("dw", "db", "dcw", "dcb")


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def supported(lib, batch, S, kin, F, D):
    from dl_ofdm_amd import _lib
    return lib.dccn_rx_bwd_fused_supported(C.byref(_lib.RxShape(batch, S, kin, F, D, 2)))


@pytest.mark.parametrize("shape", sorted(R.SHAPES), ids=lambda s: "-".join(map(str, s)))
def test_rx_backward_shape(lib, shape):
    batch, S, kin, F, D = shape
    nx, per_symbol, ranges, graded = R.SHAPES[shape]
    # ---- the plan the table states, from the library's own queries ----------------------------------------------------
    assert supported(lib, *shape) == 1
    st, r = route(lib, "rx_backward", *shape)
    assert st == 0 and r["family"] == "rx_fused" and r["tile"] == (64, 64, 64) and r["wtile"] == (64, 64), r
    assert (S * 2 * F) % r["tile"][1] == 0 and (2 * F) % r["tile"][1] == 0
    assert -(-batch // r["tile"][0]) * (S * 2 * F // r["tile"][1]) == nx and 2 * F // r["tile"][1] == per_symbol
    assert (r["splits"], r["nranges"]) == (ranges, ranges if graded else 0), r
    if graded:
        assert r["koff"][0] == 0 and r["koff"][-1] == batch, r
    else:
        assert r["splits"] == -(-batch // r["klen"]), r
    # ---- first call: every output against float64 ---------------------------------------------------------------------
    c = rx_case(batch, kin, D, S, F)
    what = "rx_backward %s" % (shape,)
    st, g, ws = run_rx_backward(lib, c, batch, kin, True, S, F, D)
    assert st == 0
    check_rx_backward(c, g, batch, kin, what, S, F, D)              # (Guarded.get: the NaN bands are untouched)
    first = {k: g[k].get(k).copy() for k in GRADS + ("dfft",)}
    # ---- dfft = NULL: the same gradients, bit for bit, and nothing stored through the missing pointer ------------------
    st, g, ws = run_rx_backward(lib, c, batch, kin, True, S, F, D, want_dfft=False)
    assert st == 0 and all_nan(g["dfft"]), what
    for k in GRADS:
        assert np.array_equal(g[k].get(k), first[k]), "%s: %s differs without the dfft store" % (what, k)
    # ---- fixed-order sums: a third full call is the first -------------------------------------------------------------
    st, g, ws = run_rx_backward(lib, c, batch, kin, True, S, F, D)
    assert st == 0
    for k in GRADS + ("dfft",):
        assert np.array_equal(g[k].get(k), first[k]), "%s: %s differs between two calls" % (what, k)


REFUSED = [(65, 7, 80, 48, 50),        # 2F = 96: a tile would straddle two symbols
           (65, 7, 80, 80, 50),        # 2F = 160: the reference's default filter count -- the grouped backward's
           (65, 7, 72, 64, 50),        # 2kin = 144: neither 128 nor 160
           (65, 7, 80, 64, 51)]        # 2D = 102: no multiple of 4


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "-".join(map(str, s)))
def test_refused_geometry_launches_nothing(lib, shape):
    batch, S, kin, F, D = shape
    assert supported(lib, *shape) == 0
    assert route(lib, "rx_backward", *shape)[0] == -1               # DCCN_ERR_INVALID_ARG: the query agrees
    c = rx_case(batch, kin, D, S, F)
    for want_dfft in (True, False):
        st, g, ws = run_rx_backward(lib, c, batch, kin, True, S, F, D, want_dfft=want_dfft)
        assert st == -1, (shape, st)
        assert all(all_nan(v) for v in g.values()) and bool(torch.isnan(ws).all()), shape
