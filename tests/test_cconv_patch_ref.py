"""tests/cconv_patch_ref.py (the fp64 restatement the GPU tests of the general-k convolutions are held to) on the CPU:

(a) the restatement against the literal layers of the oracle -- ``O.layers_conv2d_complex_literal`` /
    ``layers_conv1d_complex_literal`` and their autograd twins in oracle/torch_ref.py -- at 1e-12, on a reduced-size twin of
    every case (same kernel, strides, padding, channel and filter counts; small B and extent);
(b) the plan of every case, from dccn_cconv_patch_plan_query at the 256 CUs device_cus() answers without a device: a case
    exists for one kernel variant, and a moved threshold must fail here rather than turn the case into one more test of the
    default path;
(c) the cases discriminate: four index errors planted in a copy of the restatement -- chunk ownership off by one row, the
    first live tap of a stride phase off by one, the last tile of a phase dropped, later grid-stride rounds working at the first
    round's row origin -- each move at least one case of the family they belong to by more than 100 x the GPU tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cconv_patch_ref as R
from oracle import dccn_oracle as O
from oracle.torch_ref import layers_conv1d_complex_literal_t, layers_conv2d_complex_literal_t

TOL_GPU = 1e-5                  # test_gpu_ops.RTOL, what tests/test_gpu_cconv_patch_routes.py demands
MOVED = 100 * TOL_GPU


def relerr(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


# ---- (a) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_the_literal_layers_on_a_twin(name):
    c, g = R.CASES[name], R.twin_geom(name)
    rng = np.random.RandomState(len(name) + g.L * 7 + g.C)
    x = rng.randn(g.B, g.L, g.Wd, g.C, 2)
    full = rng.randn(g.kL, g.kW, 1, g.C, 2 * g.F)                     # dead taps (they only ever see padding): any value
    live = np.stack([np.stack([full[a, b, 0] for b in g.tw]) for a in g.tl])
    w = live.reshape(g.ntl * g.ntw * g.C, 2 * g.F)
    bias = rng.randn(2 * g.F)
    out = R.forward(x, w, bias, g).reshape(g.B, g.Lo, g.Wo, g.F, 2)
    ref = O.layers_conv2d_complex_literal(x, full, bias, (g.sL, g.sW), g.padding)
    assert relerr(out, ref) <= 1e-12
    one_d = g.Wd == 1 and g.kW == 1
    if one_d:
        assert relerr(out[:, :, 0], O.layers_conv1d_complex_literal(x[:, :, 0], full[:, 0], bias, g.sL, g.padding)) <= 1e-12
    dout = rng.randn(g.B * g.Lo * g.Wo, g.F, 2)
    dx, dw, db = R.backward(x, w, dout, g)
    x64 = torch.tensor(x, requires_grad=True)
    k64, b64 = torch.tensor(full, requires_grad=True), torch.tensor(bias, requires_grad=True)
    gt = torch.tensor(dout.reshape(g.B, g.Lo, g.Wo, g.F, 2))
    if one_d:
        layers_conv1d_complex_literal_t(x64[:, :, 0], k64[:, 0], b64, g.sL, g.padding).backward(gt[:, :, 0])
    else:
        layers_conv2d_complex_literal_t(x64, k64, b64, (g.sL, g.sW), g.padding).backward(gt)
    kg = k64.grad.numpy()
    glive = np.stack([np.stack([kg[a, b, 0] for b in g.tw]) for a in g.tl])
    assert np.abs(kg).sum() - np.abs(glive).sum() <= 1e-12 * np.abs(glive).sum()          # dead taps never meet data
    assert relerr(dx, x64.grad.numpy()) <= 1e-12
    assert relerr(dw, glive.reshape(dw.shape)) <= 1e-12
    assert relerr(db, b64.grad.numpy()) <= 1e-12
    # the mask of unreached cells: exactly the cells whose gradient is identically zero, whatever dout holds
    un = R.unreached(g)
    assert np.all(dx[:, un] == 0.0)
    reach = np.abs(R.scatter(np.ones((g.B, g.Lo, g.Wo, g.ntl, g.ntw, g.C, 2)), g)).min(axis=(0, 3, 4))
    assert np.array_equal(reach == 0.0, un)
    # the by-phase form of the input gradient (what the planted tap error is applied to) is the same function
    assert relerr(R.dx_by_phase(R.patch_grad(w, dout, g), g), dx) <= 1e-12


# ---- (b) -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_runs_the_plan_it_exists_for(lib, name):
    got = R.assert_plan(lib, name, " (256 CUs)")
    c, g = R.CASES[name], R.case_geom(name)
    # the forward and the weight gradient accept every case; the fused 1-D backward exactly the A cases and the first control
    assert R.query(lib, "fwd", g)[0] == 0 and R.query(lib, "bwd_w", g)[0] == 0 and R.query(lib, "bwd_x", g)[0] == 0
    assert (R.query(lib, "bwd_1d", g)[0] == 0) == (c.op == "bwd_1d")
    if got["kernel"] == "dx_narrow":
        tiles, first = R.narrow_tiles(g)                              # the work list the planted errors are applied to
        assert tiles.shape[0] == got["tiles"] and len(first) == got["phases"]
        assert got["grid"] == min(got["tiles"], 6 * 256)
        assert np.array_equal(np.sort(tiles[tiles >= 0]), np.arange(g.B * g.L * g.Wd))
    if got["kernel"] == "conv1d_fused":
        ch = R.chunk_rows(g, got["positions"], got["chunks"])
        assert got["items"] == g.B * got["chunks"] and got["grid"] == min(512, got["items"])
        # consecutive position ranges covering [0, L), consecutive row ranges covering [0, Lo), a chunk's rows fit its 64-row tile
        assert ch[0][0] == 0 and ch[-1][1] == g.L and ch[0][2] == 0 and ch[-1][3] == g.Lo
        assert all(a[3] == b[2] and a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(q1 - q0 <= 64 for _, _, q0, q1 in ch)


def test_plan_facts_the_case_table_quotes(lib):
    """the numbers in the cases' descriptions, from the plans"""
    got = R.assert_plan(lib, "A1")
    assert 500 - 8 * got["positions"] == 28 and -(-1179 // 512) == 3 and 1179 // 512 == 2
    got = R.assert_plan(lib, "A2")
    assert got["items"] - got["grid"] == 188
    got = R.assert_plan(lib, "A4")
    assert got["items"] - got["grid"] == 8
    assert [p1 - p0 for p0, p1, _, _ in R.chunk_rows(R.case_geom("A5"), 57, 3)] == [57, 57, 6]
    got = R.assert_plan(lib, "B11")
    assert got["tiles"] - got["grid"] == 39 and (180 * 560) % 64 == 0          # (its last tile is full; B12's are ragged)
    assert (180 * 561) % 64 == 52 and (180 * 560) % 64 == 0
    tiles, first = R.narrow_tiles(R.case_geom("B12"))
    assert first == [0, 1578] and tiles.shape[0] == 3153 and first[1] - 1536 < 1536 < first[1]       # round 2 crosses the phases
    g = R.case_geom("B8")                                            # five taps at stride 4: one phase per axis meets two taps, three meet one
    combos = {len(range((pl + g.pl0 - g.tl0) % 4, 5, 4)) * len(range((pw + g.pw0 - g.tw0) % 4, 5, 4)) for pl in range(4) for pw in range(4)}
    assert combos == {1, 2, 4}
    g = R.case_geom("B9")
    assert R.unreached(g).sum() == 5 and g.Lo == 1 and g.Wo == 1
    assert 16 * ((9 * 128 + 31) // 32 * 32 + 16) * 4 == 74752         # B4's Bt rows in LDS would be 74 752 B > 64 KB


def test_query_refuses_where_the_operators_do(lib):
    from dl_ofdm_amd import _lib
    g = R.case_geom("A1")
    p = _lib.CconvPatchPlan()
    C.memset(C.byref(p), 0x5a, C.sizeof(p))
    before = bytes(p)

    def q(op, B=g.B, L=g.L, Wd=1, Cc=2, Lo=g.Lo, Wo=1, ntl=5, ntw=1, sL=1, sW=1, F=32, plan=p):
        return lib.dccn_cconv_patch_plan_query(op, B, L, Wd, Cc, Lo, Wo, ntl, ntw, sL, sW, F, None if plan is None else C.byref(plan))
    assert q(0, plan=None) == -1 and q(4) == -1 and q(-1) == -1
    for op in range(4):
        assert q(op, Cc=3) == -1 and q(op, F=0) == -1 and q(op, B=0) == -1 and q(op, sL=0) == -1      # odd channel count, empty axes
    assert q(3, F=16) == -1 and q(3, ntl=8) == -1 and q(3, Wd=2) == -1 and q(3, ntw=2) == -1 and q(3, sW=2) == -1
    assert q(0, F=33) == -1 and q(1, F=33) == -1 and q(2, F=33) == -1
    assert q(0, B=1 << 20, L=1 << 10) == -1                           # 32-bit element offsets into x
    assert bytes(p) == before                                         # refused: the struct is untouched
    for op in range(4):
        assert q(op) == 0
    assert C.sizeof(_lib.CconvPatchPlan) == 64


# ---- (c) -------------------------------------------------------------------------------------------------------------
def _fused1d_errors(lib, name):
    """-> {error: how far it moves the case}: 'boundary' (chunk ownership off by one row: the weight and bias gradient count the
    boundary rows twice), 'rounds' (a block's second and later chunks computed at its first chunk's origin)"""
    h, g = R.host_case(name), R.case_geom(name)
    plan = R.query(lib, "bwd_1d", g)[1]
    PL, nch, grid, items = plan["positions"], plan["chunks"], plan["grid"], plan["items"]
    own = R.chunk_rows(g, PL, nch)
    w1 = np.zeros((g.B, g.Lo))
    for p0, p1, q0, q1 in own:
        w1[:, q0:q1] += 1
    assert np.all(w1 == 1.0)                                          # unplanted: every row counted once
    moved = {}
    wb = np.zeros((g.B, g.Lo))
    for p0, p1, q0, q1 in R.chunk_rows(g, PL, nch, upper_shift=1):
        wb[:, q0:q1] += 1
    dw, db = R.weight_grads(h["x"], h["w"], h["dout"], g, wb.reshape(-1))
    moved["boundary"] = max(relerr(dw, h["dw"]), relerr(db, h["db"]))
    wr, dx = np.zeros((g.B, g.Lo)), h["dx"].copy()
    for ch in range(items):
        src = ch if ch < grid else ch % grid
        (b, j), (bs, js) = divmod(ch, nch), divmod(src, nch)
        wr[bs, own[js][2]:own[js][3]] += 1
        n = min(own[j][1] - own[j][0], own[js][1] - own[js][0])
        dx[b, own[j][0]:own[j][0] + n] = h["dx"][bs, own[js][0]:own[js][0] + n]
    dw, db = R.weight_grads(h["x"], h["w"], h["dout"], g, wr.reshape(-1))
    moved["rounds"] = max(relerr(dx, h["dx"]), relerr(dw, h["dw"]), relerr(db, h["db"]))
    return moved


def _narrow_errors(lib, name):
    """-> {error: how far it moves the case's dx}: 'first_tap' (first live tap of every phase off by one), 'last_tile' (the last
    tile of every phase never written: zeros here), 'rounds' (a block's later tiles computed at its first tile's rows)"""
    h, g = R.host_case(name), R.case_geom(name)
    plan = R.query(lib, "bwd_x", g)[1]
    assert plan["kernel"] == "dx_narrow"
    tiles, first = R.narrow_tiles(g)
    ref = h["dx"].reshape(g.B * g.L * g.Wd, 2 * g.C)
    moved = {}
    pg = R.patch_grad(h["w"], h["dout"], g)
    assert relerr(R.dx_by_phase(pg, g), h["dx"]) <= 1e-12
    moved["first_tap"] = relerr(R.dx_by_phase(pg, g, first_tap_shift=1), h["dx"])
    dx = ref.copy()
    for t in [f - 1 for f in first[1:] if f > 0] + [tiles.shape[0] - 1]:
        dx[tiles[t][tiles[t] >= 0]] = 0.0
    moved["last_tile"] = relerr(dx, ref)
    dx = ref.copy()
    for t in range(plan["grid"], tiles.shape[0]):
        ok = (tiles[t] >= 0) & (tiles[t % plan["grid"]] >= 0)
        dx[tiles[t][ok]] = ref[tiles[t % plan["grid"]][ok]]
    moved["rounds"] = relerr(dx, ref)
    return moved


def test_planted_index_errors_move_the_cases_of_their_family(lib):
    seen = {}
    for name, c in R.CASES.items():
        if c.op == "bwd_1d":
            seen[name] = _fused1d_errors(lib, name)
        elif c.plan["kernel"] == "dx_narrow":
            seen[name] = _narrow_errors(lib, name)
        else:
            seen[name] = {}
    hit = {name: sorted(k for k, v in m.items() if v > MOVED) for name, m in seen.items()}
    print("\n".join("%-4s %s" % (n, "  ".join("%s %.2e" % kv for kv in sorted(seen[n].items())) or "-") for n in seen))
    fam = {"A": [n for n in R.CASES if n[0] == "A"], "B": [n for n in R.CASES if n[0] == "B"]}
    assert any("boundary" in hit[n] for n in fam["A"]) and any("rounds" in hit[n] for n in fam["A"])
    assert any("first_tap" in hit[n] for n in fam["B"]) and any("last_tile" in hit[n] for n in fam["B"])
    assert any("rounds" in hit[n] for n in fam["B"])
    # every case of the looping families notices at least one of the errors ...
    for n in fam["A"] + [n for n in fam["B"] if R.CASES[n].plan["kernel"] == "dx_narrow"]:
        assert hit[n], (n, seen[n])
    # ... the persistent loops notice 'rounds' exactly where a block runs more than one item, and one chunk per item has no boundary
    assert "boundary" not in hit["A4"] and all("boundary" in hit[n] for n in ("A1", "A2", "A3", "A5"))
    assert all("rounds" in hit[n] for n in fam["A"] + ["B11", "B12"]) and "rounds" not in hit["X1"] and "rounds" not in hit["X2"]
    assert all("rounds" not in hit[n] for n in fam["B"] if n not in ("B10", "B11", "B12"))
    # a case that sees none of the four is in the table for the tile it runs, and says so
    for n in R.CASES:
        if not hit[n]:
            assert R.CASES[n].plan["kernel"] == "gemm" and R.CASES[n].why, n
