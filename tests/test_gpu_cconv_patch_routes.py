"""Every launch path of the general-k complex convolutions (csrc/dccn_abi_conv.hip: dccn_cconv_patch_fwd / _bwd_w / _bwd_x,
dccn_cconv1d_bwd) against the fp64 restatement of tests/cconv_patch_ref.py (``-m gpu``), at operator level through ctypes.

tests/test_layer_api.py reaches these kernels through the layers, at shapes on which the persistent kernels never loop, half of
cconv_dx_narrow_kernel's instantiations never launch, the wide input gradient never gathers across a stride and OP_KPATCH never
runs on its large tiles.  The cases of cconv_patch_ref.CASES exist for those paths; each one first asks
dccn_cconv_patch_plan_query -- the plan the operator itself launches from -- and asserts that the path it is written for is
the one its geometry takes on this device.  Then every operator that accepts the geometry runs: the forward, the weight
gradient, the implicit input gradient (bit 1 of dccn_cconv_patch_bwd_supported), dccn_cconv1d_bwd where supported, and for the
strided wide cases dccn_cconv_gemm_bwd_x + dccn_cconv_col2im, the route production takes there.

Per case: outputs are NaN-filled between NaN guard bands (a NaN left behind is a skipped row); every value against fp64 at the
suite's bound (test_gpu_ops.RTOL, max error over max reference); the dx cells no live tap reaches exactly 0.0; the fused 1-D
backward against the separate routes at the same bound; a second call equal to the first bit for bit.  The two control cases
are shapes of test_layer_api.py's parametrisations: what this helper demands is the suite's bound, not one fitted here.
``-s`` prints each case's variant, worst error per output and unreached-cell count.
"""
import numpy as np
import pytest
import torch

import cconv_patch_ref as R
from test_gpu_gemm_operands import Guarded, workspace
from test_gpu_ops import RTOL, dev, relerr

pytestmark = pytest.mark.gpu

STRIDED_WIDE = ("C1", "C2", "C3")          # ... also through GEMM + col2im, the route the layer takes there (bit 2 clear)


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def _twice(run, what):
    """run() -> list of host arrays; two calls, bit for bit the same; no NaN left in any output"""
    a, b = run(), run()
    for k, (u, v) in enumerate(zip(a, b)):
        assert not np.isnan(u).any(), "%s, output %d: %d values never written" % (what, k, int(np.isnan(u).sum()))
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "%s, output %d: a second call differs" % (what, k)
    return a


def run_case(lib, name):
    from dl_ofdm_amd import _lib
    h = R.host_case(name)
    g = h["g"]
    cus = _lib.device_info()[0]
    plan = R.assert_plan(lib, name, " -- device with %d CUs" % cus)
    geo = R.abi_geom(g)
    B, L, Wd, C, Lo, Wo, ntl, ntw, F = g.B, g.L, g.Wd, g.C, g.Lo, g.Wo, g.ntl, g.ntw, g.F
    rows, kin = B * Lo * Wo, ntl * ntw * C
    x, w, bias, dout = dev(h["x"]), dev(h["w"]), dev(h["bias"]), dev(h["dout"])
    xp, wp, bp, dp = x.data_ptr(), w.data_ptr(), bias.data_ptr(), dout.data_ptr()
    un = np.broadcast_to(h["unreached"][None, :, :, None, None], h["dx"].shape)
    err = {}

    def hold(tag, got, ref):
        err[tag] = relerr(got.reshape(ref.shape), ref)
        assert err[tag] <= RTOL, "%s %s: rel err %.3e > %.1e (%s)" % (name, tag, err[tag], RTOL, plan)

    def hold_dx(tag, got):
        hold(tag, got, h["dx"])
        assert np.all(got.reshape(h["dx"].shape)[un] == 0.0), "%s %s: an unreached dx cell is not exactly 0" % (name, tag)

    assert lib.dccn_cconv_patch_supported(B, L, Wd, C, Lo, Wo, ntl, ntw, F) == 1
    mode = lib.dccn_cconv_patch_bwd_supported(B, L, Wd, C, Lo, Wo, ntl, ntw, g.sL, g.sW, F)
    assert (mode & 3) == 3, (name, mode)

    def fwd():
        out = Guarded(rows * 2 * F)
        _lib.check(lib.dccn_cconv_patch_fwd(xp, wp, bp, out.ptr, *geo, F, None), "dccn_cconv_patch_fwd")
        return [out.get("out")]
    hold("out", _twice(fwd, name + " fwd")[0], h["out"])

    nws_w = lib.dccn_cconv_patch_bwd_w_workspace_size(B, Lo, Wo, C, ntl, ntw, F)
    ws_w = workspace(nws_w)

    def bwd_w():
        dw, db = Guarded(kin * 2 * F), Guarded(2 * F)
        _lib.check(lib.dccn_cconv_patch_bwd_w(xp, dp, dw.ptr, db.ptr, *geo, F, ws_w.data_ptr(), nws_w, None), "dccn_cconv_patch_bwd_w")
        return [dw.get("dw"), db.get("dbias")]
    dw_sep, db_sep = _twice(bwd_w, name + " bwd_w")
    hold("dw", dw_sep, h["dw"])
    hold("dbias", db_sep, h["db"])

    nws_x = lib.dccn_cconv_patch_bwd_x_workspace_size(C, ntl, ntw, F)
    ws_x = workspace(nws_x)

    def bwd_x():
        dx = Guarded(B * L * Wd * C * 2)
        _lib.check(lib.dccn_cconv_patch_bwd_x(dp, wp, dx.ptr, *geo, F, ws_x.data_ptr(), nws_x, None), "dccn_cconv_patch_bwd_x")
        return [dx.get("dx")]
    dx_sep = _twice(bwd_x, name + " bwd_x")[0]
    hold_dx("dx", dx_sep)

    fused = R.query(lib, "bwd_1d", g)[0] == 0
    assert fused == bool(Wd == 1 and Wo == 1 and ntw == 1 and g.sW == 1 and lib.dccn_cconv1d_bwd_supported(B, L, C, Lo, ntl, g.sL, F))
    if fused:
        nws_1 = lib.dccn_cconv1d_bwd_workspace_size(F)
        ws_1 = workspace(nws_1)

        def bwd_1d():
            dx, dw, db = Guarded(B * L * C * 2), Guarded(kin * 2 * F), Guarded(2 * F)
            _lib.check(lib.dccn_cconv1d_bwd(xp, dp, wp, dx.ptr, dw.ptr, db.ptr, B, L, C, Lo, ntl, g.tl0, g.sL, g.pl0, F,
                                            ws_1.data_ptr(), nws_1, None), "dccn_cconv1d_bwd")
            return [dx.get("dx"), dw.get("dw"), db.get("dbias")]
        dx1, dw1, db1 = _twice(bwd_1d, name + " bwd_1d")
        hold_dx("1d dx", dx1)
        hold("1d dw", dw1, h["dw"])
        hold("1d dbias", db1, h["db"])
        for tag, a, b in (("dx", dx1, dx_sep), ("dw", dw1, dw_sep), ("dbias", db1, db_sep)):
            e = relerr(a, b)
            assert e <= RTOL, "%s fused 1-D %s vs the separate route: %.3e" % (name, tag, e)

    if name in STRIDED_WIDE:
        assert not (mode & 4), (name, mode)

        def col2im():
            drows, dx = Guarded(rows * kin * 2), Guarded(B * L * Wd * C * 2)
            _lib.check(lib.dccn_cconv_gemm_bwd_x(dp, wp, drows.ptr, rows, kin, F, None), "dccn_cconv_gemm_bwd_x")
            _lib.check(lib.dccn_cconv_col2im(drows.ptr, dx.ptr, *geo, None), "dccn_cconv_col2im")
            return [drows.get("drows"), dx.get("dx")]
        hold_dx("col2im dx", _twice(col2im, name + " gemm_bwd_x + col2im")[1])

    variant = {k: v for k, v in plan.items() if v} if plan["kernel"] != "dx_narrow" else \
        "dx_narrow<%d,%d,%s,%s> phases %d tiles %d grid %d" % (plan["col_tiles"], plan["depth"], "LDS" if plan["bt_lds"] else "global",
                                                               "NMAJ" if plan["taps_fastest"] else "-", plan["phases"], plan["tiles"], plan["grid"])
    print("\n%-4s %s %s | %s | unreached dx cells %d | %s" % (
        name, R.CASES[name].op, variant, "  ".join("%s %.2e" % kv for kv in err.items()), int(h["unreached"].sum()) * B, R.CASES[name].why))
    return err


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "A"])
def test_fused_1d_backward_loops(lib, name):
    """dccn_cconv1d_bwd with blocks that run several chunks: the next-chunk prefetch, the weight-gradient registers carried across
    chunks and the barrier between one chunk's gather and the next chunk's staging"""
    run_case(lib, name)


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "B"])
def test_narrow_input_gradient_variants_and_loops(lib, name):
    """every instantiation of cconv_dx_narrow_kernel, its phase walk at the phase limit and with empty phases, its persistent
    loop within and across phases; B10: one phase too many, the wide gather on four columns"""
    run_case(lib, name)


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "C"])
def test_wide_input_gradient_inverse_stride_gather(lib, name):
    """OP_KPATCH over dout with PatchGeom::isL / isW, on every tile it takes"""
    run_case(lib, name)


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "D"])
def test_forward_tiles(lib, name):
    """OP_KPATCH x OP_CCONV_W on the 64x64x32 and 128x128x32 tiles"""
    run_case(lib, name)


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "X"])
def test_control_shapes_of_the_layer_tests(lib, name):
    """the same helper on two shapes test_layer_api.py already holds to 1e-5 through the layers"""
    run_case(lib, name)
