"""Every knob-selected GEMM tile variant against the float64 oracle (``-m gpu``).

dccn_set_tuning selects compiled kernel instantiations that ship in libdccn.so: the rows of kDenseBwd16, kCconvFwd16, kCconvBw16,
the skinny_launch variants, split counts and the graded dW presets of the fused backward launch.  The defaults were chosen by
timing them against each other; a variant that is fast because it is wrong must not look like a win.

Operator level: every case (1) sets the knobs, (2) asserts through dccn_gemm_route_query -- the route value the operator itself
consumes; tests/test_gemm_route_query.py pins its answers by hand -- that the intended family and tile is what the call will
launch (a mismatch fails: nothing here skips), (3) makes the call through the C ABI into the guarded outputs of
test_gpu_gemm_operands.py (16-byte aligned, NaN-filled, between NaN-filled bands: an out-of-bounds store or an element a ragged
tile leaves unwritten is seen), (4) compares every output with float64 NumPy on the same float32 inputs at
max|gpu - ref64| / max|ref64| <= 1e-5 (RTOL of test_gpu_ops.py; inputs scaled as its test_dense_fwd_bwd /
test_cconv_gemm_fwd_bwd do), (5) restores the knobs.  References are computed once per shape.

Step level: variants that exist only inside the receiver step, through make_case / staged_checks of test_gpu_engine.py at
their own tolerances, the engine built after the knobs are set.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from test_gemm_route_query import CCONV_BW16, CCONV_FWD16, DENSE_BWD16, SKINNY16, knobs, route, snapshot
from test_gpu_engine import make_case, staged_checks
from test_gpu_engine import relerr as step_relerr
from test_gpu_gemm_operands import Guarded, workspace
from test_gpu_ops import RTOL, assert_close, dev

pytestmark = pytest.mark.gpu


def _defaults_at_import():
    from dl_ofdm_amd import _lib
    return snapshot(_lib.load()) if os.path.exists(_lib.LIB_PATH) else None


DEFAULTS = _defaults_at_import()


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def table_is_restored(lib):
    yield
    assert DEFAULTS is not None and snapshot(lib) == DEFAULTS


def routed(lib, op, *dims):
    st, r = route(lib, op, *dims)
    assert st == 0, "route query refused %s %s" % (op, dims)
    return r


def all_nan(g):
    return bool(torch.isnan(g.buf).all())


# ---- inputs and float64 references, once per shape ---------------------------------------------------------------------
_cache = {}


def dense_case(M, K, N):
    key = ("dense", M, K, N)
    if key not in _cache:
        rng = np.random.RandomState(M + K + N)
        x = rng.randn(M, K).astype(np.float32)
        w = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
        b = rng.randn(N).astype(np.float32)
        dy = rng.randn(M, N).astype(np.float32)
        x6, w6, b6, d6 = (a.astype(np.float64) for a in (x, w, b, dy))
        _cache[key] = dict(x=dev(x), w=dev(w), b=dev(b), dy=dev(dy), y=x6 @ w6 + b6, dx=d6 @ w6.T, dw=x6.T @ d6, db=d6.sum(0))
    return _cache[key]


def cconv_case(rows, kin, F):
    key = ("cconv", rows, kin, F)
    if key not in _cache:
        rng = np.random.RandomState(rows + kin + F)
        x = rng.randn(rows, kin, 2).astype(np.float32)
        w = (rng.randn(kin, 2 * F) / np.sqrt(kin)).astype(np.float32)
        b = rng.randn(2 * F).astype(np.float32)
        dout = rng.randn(rows, F, 2).astype(np.float32)
        x6, w6, b6, d6 = (a.astype(np.float64) for a in (x, w, b, dout))
        _, dw, db = O.cconv_gemm_bwd(x6, w6, d6)
        _cache[key] = dict(x=dev(x), w=dev(w), b=dev(b), dout=dev(dout), out=O.cconv_gemm_fwd(x6, w6, b6), dw=dw, db=db)
    return _cache[key]


def rx_case(batch, kin, D=320, S=7, F=64):
    key = ("rx", batch, kin, D, S, F)
    if key not in _cache:
        rng = np.random.RandomState(batch + kin + D + (S - 7) + (F - 64))          # (S = 7, F = 64: the seeds of before)
        xn = rng.randn(batch, S, kin, 2).astype(np.float32)
        a = rng.randn(batch, S * 2 * F).astype(np.float32)
        dz = rng.randn(batch, 2 * D).astype(np.float32)
        w = (rng.randn(S * 2 * F, 2 * D) / 30).astype(np.float32)
        dz6, a6, w6 = dz.astype(np.float64), a.astype(np.float64), w.astype(np.float64)
        _cache[key] = dict(xn=dev(xn), a=dev(a), dz=dev(dz), w=dev(w), xn64=xn.astype(np.float64).reshape(batch * S, kin, 2),
                           dfft=dz6 @ w6.T, dw=a6.T @ dz6, db=dz6.sum(0), conv={})
    return _cache[key]


def call_dense_bwd(lib, c, M, K, N):
    nws = lib.dccn_dense_bwd_w_workspace_size(M, K, N)
    ws = workspace(nws)
    dx, dw, db = Guarded(M * K), Guarded(K * N), Guarded(N)
    st = lib.dccn_dense_bwd(c["x"].data_ptr(), c["dy"].data_ptr(), c["w"].data_ptr(), dx.ptr, dw.ptr, db.ptr, M, K, N,
                            ws.data_ptr(), nws, None)
    torch.cuda.synchronize()
    return st, (dx, dw, db)


def check_dense_bwd(c, outs, M, K, N, what):
    dx, dw, db = outs
    assert_close(dx.get("dx").reshape(M, K), c["dx"], what + ": dx")
    assert_close(dw.get("dw").reshape(K, N), c["dw"], what + ": dw")
    assert_close(db.get("dbias"), c["db"], what + ": dbias")


# ---- knob 1 = 1..6: the dX / dW tile pairs of the grouped dense backward ------------------------------------------------
# (137, 200, 132): ragged against 48 / 64 / 96-row and 64 / 128-column tiles, ragged last k range; (97, 68, 260): one row past
# the few-row grid, K barely above one tile; (300, 896, 640): several blocks on every axis
@pytest.mark.parametrize("splits", [0, 1, 8])
@pytest.mark.parametrize("row", sorted(DENSE_BWD16))
@pytest.mark.parametrize("M,K,N", [(137, 200, 132), (97, 68, 260), (300, 896, 640)])
def test_dense_bwd16_row(lib, M, K, N, row, splits):
    c = dense_case(M, K, N)
    tile, wtile = DENSE_BWD16[row]
    with knobs(lib, {1: row, 4: splits}):
        r = routed(lib, "dense_bwd", M, K, N)
        assert (r["family"], r["variant"], r["tile"], r["wtile"]) == ("gemm16", row, tile, wtile), r
        assert (r["splits"] == 1) if splits == 1 else (1 < r["splits"] <= 8), r
        assert r["klen"] % tile[2] == 0 and r["splits"] == -(-M // r["klen"])
        st, outs = call_dense_bwd(lib, c, M, K, N)
        assert st == 0
        check_dense_bwd(c, outs, M, K, N, "knob 1 = %d, knob 4 = %d, %s, %d ranges" % (row, splits, (M, K, N), r["splits"]))


# ---- knob 2 = 1..6: gemm16 tiles of the C-Conv forward --------------------------------------------------------------------
# (131, 34, 18): K = 68 = three 32-deep k-tiles, the last of 4 (row 5: over two k-slices), 36 columns; (252, 80, 64) and
# (1000, 64, 64): the N = 64 layers with / without the cyclic prefix, several row blocks, a ragged last one
@pytest.mark.parametrize("row", sorted(CCONV_FWD16))
@pytest.mark.parametrize("rows,kin,F", [(131, 34, 18), (252, 80, 64), (1000, 64, 64)])
def test_cconv_fwd16_row(lib, rows, kin, F, row):
    c = cconv_case(rows, kin, F)
    with knobs(lib, {2: row}):
        r = routed(lib, "cconv_fwd", rows, kin, F)
        assert (r["family"], r["variant"], r["tile"]) == ("gemm16", row, CCONV_FWD16[row]), r
        out = Guarded(rows * 2 * F)
        assert lib.dccn_cconv_gemm_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr(), out.ptr, rows, kin, F, None) == 0
        torch.cuda.synchronize()
        assert_close(out.get("out").reshape(c["out"].shape), c["out"], "knob 2 = %d, %s" % (row, (rows, kin, F)))


# ---- knob 8 = 1..4: the skinny tiles of dense_fwd and dense_bwd_x ------------------------------------------------------
# (73, 260, 300): no multiple of 16, so the few-row tiles decline; (96, 256, 644): the last row count and the smallest N / K
# they take; (73, 896, 896) with the few-row tiles switched off (knob 21 = 0): the equaliser's layer
@pytest.mark.parametrize("variant", sorted(SKINNY16))
@pytest.mark.parametrize("M,K,N,extra", [(73, 260, 300, {}), (96, 256, 644, {}), (73, 896, 896, {21: 0})],
                         ids=["73-260-300", "96-256-644", "73-896-896-k21=0"])
def test_skinny_variant(lib, M, K, N, extra, variant):
    c = dense_case(M, K, N)
    with knobs(lib, {**extra, 8: variant}):
        for op in ("dense_fwd", "dense_bwd_x"):
            r = routed(lib, op, M, K, N)
            assert (r["family"], r["variant"], r["tile"]) == ("skinny", variant, SKINNY16[variant]), (op, r)
        y, dx = Guarded(M * N), Guarded(M * K)
        assert lib.dccn_dense_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr(), y.ptr, M, K, N, None) == 0
        assert lib.dccn_dense_bwd_x(c["dy"].data_ptr(), c["w"].data_ptr(), dx.ptr, M, K, N, None) == 0
        torch.cuda.synchronize()
        assert_close(y.get("y").reshape(M, N), c["y"], "knob 8 = %d, dense fwd %s" % (variant, (M, K, N)))
        assert_close(dx.get("dx").reshape(M, K), c["dx"], "knob 8 = %d, dense dX %s" % (variant, (M, K, N)))


# ---- knob 4: split count of the stand-alone dense weight gradient, k-major and 32x32x2 form -----------------------------
@pytest.mark.parametrize("splits", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("form", [7, 0])
@pytest.mark.parametrize("M,K,N", [(600, 260, 132), (2000, 64, 64)])
def test_dense_bwd_w_split_count(lib, M, K, N, form, splits):
    c = dense_case(M, K, N)
    with knobs(lib, {1: form, 4: splits}):
        r = routed(lib, "dense_bwd_w", M, K, N)
        # min(knob, max_splits16 = 8) ranges wanted, ranges of whole 64-row k-tiles (the last one ragged): see the by-hand plans
        # of test_gemm_route_query.py::test_dense_bwd_w_splits
        klen = -(-(-(-M // splits)) // 64) * 64
        assert (r["splits"], r["klen"]) == (-(-M // klen), klen), r
        assert (r["family"], r["tile"]) == ("kmajor" if form == 7 and r["splits"] > 1 else "generic", (64, 64, 64)), r
        nws = lib.dccn_dense_bwd_w_workspace_size(M, K, N)
        ws = workspace(nws)
        dw, db = Guarded(K * N), Guarded(N)
        assert lib.dccn_dense_bwd_w(c["x"].data_ptr(), c["dy"].data_ptr(), dw.ptr, db.ptr, M, K, N, ws.data_ptr(), nws, None) == 0
        torch.cuda.synchronize()
        what = "knob 1 = %d, knob 4 = %d, %s" % (form, splits, (M, K, N))
        assert_close(dw.get("dw").reshape(K, N), c["dw"], what + ": dw")
        assert_close(db.get("dbias"), c["db"], what + ": dbias")


# ---- knob 14: graded k ranges of the dense dW items of the fused backward launch --------------------------------------
def run_rx_backward(lib, c, batch, kin, reduce, S=7, F=64, D=320, want_dfft=True):
    """want_dfft = False: dfft = NULL (the dX tiles only feed their epilogue); its guarded buffer must then stay NaN"""
    nws = lib.dccn_rx_backward_workspace_size(batch, S, kin, F, D)
    ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device="cuda")
    g = dict(dfft=Guarded(batch * S * 2 * F), dw=Guarded(S * 2 * F * 2 * D), db=Guarded(2 * D), dcw=Guarded(kin * 2 * F), dcb=Guarded(2 * F))
    p = (lambda k: g[k].ptr) if reduce else (lambda k: None)
    st = lib.dccn_rx_backward(c["xn"].data_ptr(), c["a"].data_ptr(), c["dz"].data_ptr(), c["w"].data_ptr(),
                              g["dfft"].ptr if want_dfft else None, p("dw"),
                              p("db"), p("dcw"), p("dcb"), batch, S, kin, F, D, 1 if reduce else 0, ws.data_ptr(), nws * 1, None)
    torch.cuda.synchronize()
    return st, g, ws


def check_rx_backward(c, g, batch, kin, what, S=7, F=64, D=320):
    dfft = g["dfft"].get("dfft")
    assert_close(dfft.reshape(batch, -1), c["dfft"], what + ": dfft")
    assert_close(g["dw"].get("dw").reshape(c["dw"].shape), c["dw"], what + ": dense dW")
    assert_close(g["db"].get("db"), c["db"], what + ": dense dbias")
    # the C-Conv gradient on the GPU's own dfft (the stage's input), as test_rx_backward_fused does; the dX tiles do not
    # depend on the dW ranges, so one reference serves every preset that left the same dfft
    key = dfft.tobytes()
    if key not in c["conv"]:
        c["conv"].clear()
        c["conv"][key] = O.cconv_gemm_bwd(c["xn64"], np.zeros((kin, 2 * F)), dfft.astype(np.float64).reshape(batch * S, F, 2))[1:]
    gw, gb = c["conv"][key]
    assert_close(g["dcw"].get("dcw").reshape(gw.shape), gw, what + ": C-Conv dW")
    assert_close(g["dcb"].get("dcb"), gb, what + ": C-Conv dbias")


RX_PRESETS = [(p, 80) for p in range(1, 25)] + [(p, 64) for p in (1, 14, 24)]


@pytest.mark.parametrize("preset,kin", RX_PRESETS)
def test_graded_dw_preset(lib, preset, kin):
    """batch 775 = 13 k-tiles of 64 frames, the last of 7.  The slabs a consumer of the un-reduced launch sees (reduce = 0: the
    head of the workspace, dK x dN floats each) are exactly the ranges the route reports: their sum is dW, the slab behind
    them is untouched."""
    batch, S, F, D = 775, 7, 64, 320
    c = rx_case(batch, kin)
    n_el = S * 2 * F * 2 * D
    with knobs(lib, {14: preset}):
        r = routed(lib, "rx_backward", batch, S, kin, F, D)
        n, off = r["nranges"], r["koff"]
        assert r["family"] == "rx_fused" and 2 <= n <= 8 and r["splits"] == n, r
        assert off[0] == 0 and off[-1] == batch and all(a < b and a % 64 == 0 for a, b in zip(off, off[1:])), off
        what = "knob 14 = %d, kin %d, ranges %s" % (preset, kin, off)
        st, g, ws = run_rx_backward(lib, c, batch, kin, True)
        assert st == 0
        check_rx_backward(c, g, batch, kin, what)
        st, g, ws = run_rx_backward(lib, c, batch, kin, False)
        assert st == 0
        slabs = ws[:(n + 1) * n_el].cpu().numpy().reshape(n + 1, n_el)
        assert not np.isnan(slabs[:n]).any(), what + ": a slab of a reported range holds unwritten elements"
        if n < 8:               # (the workspace holds max_splits16 = 8 slabs)
            assert np.isnan(slabs[n]).all(), what + ": more slabs written than ranges reported"
        assert_close(slabs[:n].astype(np.float64).sum(0).reshape(c["dw"].shape), c["dw"], what + ": sum of the slabs")
        # every slab is its own range's contribution: the first one against its rows alone
        a0 = c["a"][:off[1]].cpu().numpy().astype(np.float64)
        d0 = c["dz"][:off[1]].cpu().numpy().astype(np.float64)
        assert_close(slabs[0].reshape(c["dw"].shape), a0.T @ d0, what + ": slab of range 0")


# ---- values outside the tables ------------------------------------------------------------------------------------------
def test_out_of_range_values_refuse_or_compute(lib):
    """One past the last row (past the last documented value where 7..11 have a meaning): DCCN_ERR_INVALID_ARG with every
    guarded output still NaN, or DCCN_OK with oracle-correct outputs -- and the route query says which."""
    M, K, N = 137, 200, 132
    c = dense_case(M, K, N)
    for v in (8, 1000):
        with knobs(lib, {1: v}):
            assert route(lib, "dense_bwd", M, K, N)[0] == -1
            st, outs = call_dense_bwd(lib, c, M, K, N)
            assert st == -1 and all(all_nan(g) for g in outs), v
            # (the stand-alone weight gradient: not 7, so the 32x32x2 family)
            assert routed(lib, "dense_bwd_w", M, K, N)["family"] == "generic"
    c = cconv_case(131, 34, 18)
    for v in (12, 1000):
        with knobs(lib, {2: v}):
            assert routed(lib, "cconv_fwd", 131, 34, 18)["family"] == "generic"
            out = Guarded(131 * 36)
            assert lib.dccn_cconv_gemm_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr(), out.ptr, 131, 34, 18, None) == 0
            torch.cuda.synchronize()
            assert_close(out.get("out").reshape(c["out"].shape), c["out"], "knob 2 = %d" % v)
    for v in (5, 1000):
        with knobs(lib, {3: v}):            # the stand-alone operator never takes the table rows: 32x32x2 family
            assert route(lib, "cconv_bwd_w", 131, 34, 18)[0] == -1          # (the step's form would: refused)
            nws = lib.dccn_cconv_gemm_bwd_w_workspace_size(131, 34, 18)
            ws = workspace(nws)
            dw, db = Guarded(34 * 36), Guarded(36)
            assert lib.dccn_cconv_gemm_bwd_w(c["x"].data_ptr(), c["dout"].data_ptr(), dw.ptr, db.ptr, 131, 34, 18, ws.data_ptr(), nws, None) == 0
            torch.cuda.synchronize()
            assert_close(dw.get("dw").reshape(c["dw"].shape), c["dw"], "knob 3 = %d: dw" % v)
            assert_close(db.get("db"), c["db"], "knob 3 = %d: dbias" % v)
    M, K, N = 73, 260, 300
    c = dense_case(M, K, N)
    for v in (5, 1000):
        with knobs(lib, {8: v}):
            assert route(lib, "dense_fwd", M, K, N)[0] == -1 and route(lib, "dense_bwd_x", M, K, N)[0] == -1
            y, dx = Guarded(M * N), Guarded(M * K)
            assert lib.dccn_dense_fwd(c["x"].data_ptr(), c["w"].data_ptr(), c["b"].data_ptr(), y.ptr, M, K, N, None) == -1
            assert lib.dccn_dense_bwd_x(c["dy"].data_ptr(), c["w"].data_ptr(), dx.ptr, M, K, N, None) == -1
            torch.cuda.synchronize()
            assert all_nan(y) and all_nan(dx), v
    c = rx_case(775, 80)
    for v in (25, 1000):
        with knobs(lib, {14: v}):
            r = routed(lib, "rx_backward", 775, 7, 80, 64, 320)
            assert (r["nranges"], r["splits"], r["klen"]) == (0, 2, 448)        # the plain plan: two ranges of 448 / 327 rows
            st, g, _ = run_rx_backward(lib, c, 775, 80, True)
            assert st == 0
            check_rx_backward(c, g, 775, 80, "knob 14 = %d" % v)


# ---- step level: variants that exist only inside the receiver step ----------------------------------------------------
def forward_checks(eng, p, x, bits, cfg, rtol=1e-5):
    """The forward half of staged_checks (an evaluation step has no other): x_norm, fft_out, z, prob, ce_mean and the
    decisions against the float64 oracle, with the same tolerances and margins."""
    batch = x.shape[0]
    m = eng.metrics()
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    xn, _, _ = O.batch_moment_norm(x.reshape(batch, -1).astype(np.float64))
    xn = xn.reshape(x.shape)
    _, info = O.rx_forward_backward(p64, xn, bits, cfg)
    sv = info["saved"]
    assert step_relerr(eng.x_norm.cpu().numpy(), xn) <= rtol
    assert step_relerr(eng.fft_out.cpu().numpy().reshape(-1, cfg.F, 2), sv["fft"]) <= rtol
    assert step_relerr(eng.z.cpu().numpy(), sv["z"]) <= rtol
    assert step_relerr(eng.prob.cpu().numpy(), info["prob"]) <= rtol
    assert abs(m["ce_mean"] - info["ce_mean"]) <= rtol * abs(info["ce_mean"])
    pg, pr = eng.prob.cpu().numpy().reshape(-1, 2), info["prob"].reshape(-1, 2)
    safe = np.abs(pr[:, 1] - pr[:, 0]) > 1e-5
    assert np.array_equal((pg[:, 1] > pg[:, 0])[safe], (pr[:, 1] > pr[:, 0])[safe])
    assert np.abs(np.array(m["conf"]) - info["conf"]).sum() <= 2 * int((~safe).sum())
    assert np.array(m["conf"]).sum() == batch * cfg.D * cfg.nbits == m["count"]


def train_and_check(dims, cfg, x, bits, p, batch):
    from dl_ofdm_amd.engine import RxEngine
    eng = RxEngine(dims, batch, params=p, train=True, want_grads=True)
    eng.train_step(x, bits)
    torch.cuda.synchronize()
    staged_checks(eng, p, x, bits, cfg)


STEP_CASES = [(37, 80), (300, 80), (37, 64), (300, 64)]        # (frames, kin): QPSK, F = 64, with / without the cyclic prefix


@pytest.mark.parametrize("row", sorted(CCONV_BW16))
@pytest.mark.parametrize("batch,kin", STEP_CASES)
def test_step_cconv_bw16_row(lib, batch, kin, row):
    """Knob 3 = 1..4 with knob 11 = 0, so that the C-Conv weight gradient is its own launch (with the tail's slab reduction
    riding on it)."""
    dims, cfg, x, bits, p = make_case(batch, 2, kin=kin, seed=31)
    with knobs(lib, {3: row, 11: 0}):
        r = routed(lib, "cconv_bwd_w", batch * 7, kin, 64)
        assert (r["family"], r["variant"], r["tile"]) == ("gemm16", row, CCONV_BW16[row]), r
        assert r["splits"] == -(-(batch * 7) // r["klen"]) and r["klen"] % 32 == 0
        train_and_check(dims, cfg, x, bits, p, batch)


@pytest.mark.parametrize("splits", [1, 7, 128])
@pytest.mark.parametrize("form", [7, 2])
@pytest.mark.parametrize("batch,kin", STEP_CASES)
def test_step_cconv_bw_split_count(lib, batch, kin, form, splits):
    """Knob 5 under the k-major form (ranges of whole 64-row k-tiles) and under a table row (row 2: 32-deep k-tiles)."""
    dims, cfg, x, bits, p = make_case(batch, 2, kin=kin, seed=32)
    rows, bk = batch * 7, 64 if form == 7 else 32
    with knobs(lib, {3: form, 5: splits, 11: 0}):
        r = routed(lib, "cconv_bwd_w", rows, kin, 64)
        klen = -(-(-(-rows // splits)) // bk) * bk
        assert (r["family"], r["splits"], r["klen"]) == ("kmajor" if form == 7 else "gemm16", -(-rows // klen), klen), r
        train_and_check(dims, cfg, x, bits, p, batch)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("k13", [0, 1, 2, 3])
@pytest.mark.parametrize("batch,nbits,kin", [(100, 3, 64), (73, 4, 80)])
def test_step_tail_fusion_bits(lib, batch, nbits, kin, k13, train):
    """Knob 13: which 8-QAM / 16-QAM steps take the fused dense + tail launch (bit 0: the lane-per-cell forms -- 8-QAM, and
    16-QAM evaluation; bit 1: the quad-lane form of 16-QAM training)."""
    from dl_ofdm_amd.engine import RxEngine
    dims, cfg, x, bits, p = make_case(batch, nbits, kin=kin, seed=33)
    with knobs(lib, {13: k13}):
        eng = RxEngine(dims, batch, params=p, train=train)
        fused = bool(k13 & 2) if (nbits == 4 and train) else bool(k13 & 1)
        assert lib.dccn_rx_dense_tail_fused(C.byref(eng.shape), 1 if train else 0) == (1 if fused else 0)
        if train:
            eng.train_step(x, bits)
            torch.cuda.synchronize()
            staged_checks(eng, p, x, bits, cfg)
        else:
            eng.eval_step(x, bits)
            torch.cuda.synchronize()
            forward_checks(eng, p, x, bits, cfg)


def test_zz_knob_table_is_the_one_recorded_at_import(lib):
    """(last in the module) every case restored the process-wide table, even a failing one"""
    assert DEFAULTS is not None and snapshot(lib) == DEFAULTS
