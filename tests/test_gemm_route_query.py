"""dccn_gemm_route_query (host only, no device work): which launch every stand-alone GEMM-shaped operator issues under the knob
table.  The operators consume the same route value, so what is pinned here is what runs.

Routes are worked out by hand from the comments and predicates of csrc/dccn_abi.hip / csrc/abi_impl.h with 256 CUs (what
device_cus() answers without a device and on an MI355X), as test_lib_abi.py::test_dense_tail_grid_query does for the dense + tail
launch.  tests/test_gpu_tile_variants.py imports `knobs` and `route` from here and asserts a route before every call it makes.
"""
import contextlib
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def snapshot(lib):
    n = lib.dccn_tuning_count()
    t = (C.c_int * n)()
    assert lib.dccn_tuning_snapshot(t, n) == n
    return list(t)


@contextlib.contextmanager
def knobs(lib, values):
    """Set knobs {key: value} of the process-wide table; whatever happens inside, put every one of them back."""
    old = {k: lib.dccn_get_tuning(k) for k in values}
    try:
        for k, v in values.items():
            assert lib.dccn_set_tuning(k, v) == 0, (k, v)
        yield
    finally:
        for k, v in old.items():
            lib.dccn_set_tuning(k, v)


def route(lib, op, *dims):
    """(status, route as a dict or None).  A refused query must leave the struct as it was."""
    from dl_ofdm_amd import _lib
    r = _lib.GemmRoute()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    d = tuple(dims) + (0,) * (5 - len(dims))
    st = lib.dccn_gemm_route_query(_lib.ROUTE_OPS[op], *d, C.byref(r))
    if st != 0:
        assert st == -1 and bytes(r) == before, "a refused query wrote its output"
        return st, None
    fam = {v: k for k, v in _lib.ROUTE_FAMILIES.items()}[r.family]
    return 0, dict(family=fam, variant=r.variant, tile=(r.tile_rows, r.tile_cols, r.tile_k), wtile=(r.w_tile_rows, r.w_tile_cols),
                   splits=r.splits, klen=r.klen, nranges=r.nranges, koff=list(r.koff)[:r.nranges + 1] if r.nranges else [],
                   stage=r.stage)


def ok(lib, op, *dims):
    st, r = route(lib, op, *dims)
    assert st == 0, (op, dims, st)
    assert r["stage"] == 1
    return r


def brief(r):
    return (r["family"], r["variant"], r["tile"])


@pytest.fixture(scope="module")
def defaults(lib):
    return snapshot(lib)


@pytest.fixture(autouse=True)
def table_is_restored(lib, defaults):
    yield
    assert snapshot(lib) == defaults
    assert [lib.dccn_get_tuning(k) for k in range(len(defaults))] == defaults


# gemm16 table rows: (dX / output tile rows, cols, k depth), dW tile
DENSE_BWD16 = {1: ((64, 64, 32), (64, 64)), 2: ((48, 64, 32), (64, 64)), 3: ((64, 64, 64), (64, 64)), 4: ((96, 64, 32), (64, 64)),
               5: ((64, 128, 32), (64, 128)), 6: ((64, 64, 32), (64, 128))}
CCONV_FWD16 = {1: (32, 128, 32), 2: (32, 128, 32), 3: (16, 128, 32), 4: (64, 64, 32), 5: (16, 128, 32), 6: (32, 64, 32)}
CCONV_BW16 = {1: (64, 64, 32), 2: (32, 64, 32), 3: (80, 128, 32), 4: (32, 128, 32)}
SKINNY16 = {1: (16, 64, 64), 2: (32, 64, 64), 3: (32, 32, 64), 4: (16, 64, 64)}


def test_default_routes(lib):
    """The default table at the flagship shapes (C2: 1170 frames, S = 7, kin = 80, F = 64, D = 320) and the equaliser's 73 frames."""
    assert brief(ok(lib, "cconv_fwd", 8190, 80, 64)) == ("staged", 7, (64, 64, 160))        # 64 x 1 = 64 < 512
    assert brief(ok(lib, "cconv_fwd", 8190, 64, 64)) == ("staged", 7, (64, 64, 128))
    assert brief(ok(lib, "cconv_fwd", 131, 34, 18)) == ("generic", 0, (64, 64, 64))         # K = 68: no staged form, no 32-deep
    assert brief(ok(lib, "cconv_fwd", 131, 48, 18)) == ("generic", 0, (64, 64, 32))         # K = 96 = 32 * 3
    assert brief(ok(lib, "dense_fwd", 1170, 896, 640)) == ("gemm16", 0, (48, 64, 64))       # knob 10
    assert brief(ok(lib, "dense_fwd", 73, 896, 896)) == ("fewrow", 0, (16, 16, 896))        # 56 k-groups: 14 slots of 64
    assert brief(ok(lib, "dense_bwd_x", 73, 896, 640)) == ("fewrow", 0, (16, 16, 640))
    r = ok(lib, "dense_bwd", 73, 896, 640)
    assert brief(r) == ("fewrow", 0, (16, 16, 640)) and r["wtile"] == (64, 64) and r["splits"] == 1
    # grouped dense backward at C2: plan_splitk(896, 640, 1170): 140 tiles >= 32 -> want 4 -> klen 320 > 256, so the k-major
    # form asks for ceil(1170 / 256) = 5 ranges (<= max_splits16 = 8): klen 234 -> 256, 5 ranges
    r = ok(lib, "dense_bwd", 1170, 896, 640)
    assert brief(r) == ("grouped_kmajor", 0, (64, 64, 64)) and r["wtile"] == (64, 64) and (r["splits"], r["klen"]) == (5, 256)
    r = ok(lib, "dense_bwd_w", 1170, 896, 640)
    assert brief(r) == ("kmajor", 0, (64, 64, 64)) and (r["splits"], r["klen"]) == (5, 256)
    # C-Conv weight gradient in the step: plan_splitk(160, 128, 2100): 6 tiles -> 256 / 6 = 42, at most ceil(2100 / 128) = 17
    # ranges: klen 124 -> 128, 17 ranges
    r = ok(lib, "cconv_bwd_w", 2100, 80, 64)
    assert brief(r) == ("kmajor", 0, (64, 64, 64)) and (r["splits"], r["klen"]) == (17, 128)
    # refused: non-positive extents, unknown operator, no output
    assert route(lib, "dense_fwd", 0, 896, 640)[0] == -1
    assert lib.dccn_gemm_route_query(99, 4, 4, 4, 0, 0, None) == -1
    assert lib.dccn_gemm_route_query(0, 4, 4, 4, 0, 0, None) == -1


@pytest.mark.parametrize("row", sorted(DENSE_BWD16))
def test_dense_bwd16_rows(lib, row):
    """Knob 1 = 1..6 at (137, 200, 132): 2 x 2 = 4 < 512 tiles of 128x128.  dX tiles nx <= 15, dW tiles tw <= 12: the automatic
    count (768 - nx + tw / 2) / tw >= 63 is cut to max_splits16(200, 132) = min(8, ceil(1024 / 12)) = 8; ranges of
    ceil(137 / 8) = 18 rows rounded up to the k-tile depth: 32 -> 5 ranges, 64 (row 3) -> 3 ranges."""
    tile, wtile = DENSE_BWD16[row]
    with knobs(lib, {1: row}):
        r = ok(lib, "dense_bwd", 137, 200, 132)
        assert brief(r) == ("gemm16", row, tile) and r["wtile"] == wtile
        assert (r["splits"], r["klen"]) == ((3, 64) if row == 3 else (5, 32))
        with knobs(lib, {4: 1}):            # one range: 137 rounded up to the k-tile depth
            r = ok(lib, "dense_bwd", 137, 200, 132)
            assert brief(r) == ("gemm16", row, tile) and (r["splits"], r["klen"]) == (1, 192 if row == 3 else 160)
        with knobs(lib, {4: 3}):            # ceil(137 / 3) = 46 -> 64: 3 ranges either way
            assert (ok(lib, "dense_bwd", 137, 200, 132)["splits"], ok(lib, "dense_bwd", 137, 200, 132)["klen"]) == (3, 64)
        # few rows come first: M <= 96 runs dX on the few-row / skinny tiles with the unsplit dW in one grid
        assert ok(lib, "dense_bwd", 96, 200, 132)["family"] == "skinny"
        assert brief(ok(lib, "dense_bwd", 97, 200, 132)) == ("gemm16", row, tile)
        # the table rows have no scalar loaders: K % 4 != 0 leaves them (x is not vector-legal)
        assert ok(lib, "dense_bwd", 137, 202, 132)["family"] != "gemm16"


@pytest.mark.parametrize("row", sorted(CCONV_FWD16))
def test_cconv_fwd16_rows(lib, row):
    with knobs(lib, {2: row}):
        assert brief(ok(lib, "cconv_fwd", 131, 34, 18)) == ("gemm16", row, CCONV_FWD16[row])
        assert brief(ok(lib, "cconv_fwd", 1000, 64, 64)) == ("gemm16", row, CCONV_FWD16[row])
        # odd kin or F: the float2 / float4 loaders do not apply
        assert brief(ok(lib, "cconv_fwd", 131, 33, 18)) == ("generic", 0, (64, 64, 64))
        assert brief(ok(lib, "cconv_fwd", 131, 34, 17)) == ("generic", 0, (64, 64, 64))
        # 128x128 tiles: 511 x 1 < 512 stays, 512 x 1 leaves for the 128x128x32 tiles (M, N > 64)
        assert brief(ok(lib, "cconv_fwd", 511 * 128, 80, 64)) == ("gemm16", row, CCONV_FWD16[row])
        assert brief(ok(lib, "cconv_fwd", 511 * 128 + 1, 80, 64)) == ("generic", 0, (128, 128, 32))


def test_cconv_fwd_staged_and_big_threshold(lib):
    for v, tile in ((7, (64, 64, 160)), (8, (64, 64, 160)), (9, (64, 64, 160)), (10, (32, 128, 160)), (11, (32, 128, 160))):
        with knobs(lib, {2: v}):
            assert brief(ok(lib, "cconv_fwd", 511 * 128, 80, 64)) == ("staged", v, tile)
            assert brief(ok(lib, "cconv_fwd", 511 * 128 + 1, 80, 64)) == ("generic", 0, (128, 128, 32))
            assert brief(ok(lib, "cconv_fwd", 1000, 34, 64)) == ("generic", 0, (64, 64, 64))         # K = 68
    with knobs(lib, {2: 0}):
        assert brief(ok(lib, "cconv_fwd", 1000, 80, 64)) == ("generic", 0, (64, 64, 160))            # whole-k tile (knob 7)
        with knobs(lib, {7: 0}):
            assert brief(ok(lib, "cconv_fwd", 1000, 80, 64)) == ("generic", 0, (64, 64, 32))         # 160 = 5 x 32


@pytest.mark.parametrize("row", sorted(CCONV_BW16))
def test_cconv_bw16_rows(lib, row):
    """Knob 3 = 1..4 in the step's form at rows = 2100 (300 frames x 7 symbols), kin = 80, F = 64: output 160 x 128.
    tiles t = ceil(160 / rows) * ceil(128 / cols); want = ceil(512 / t), at most 128 ranges; ranges of ceil(2100 / want)
    rows rounded up to 32."""
    expect = {1: (66, 32),      # t = 3 x 2 = 6 -> want 86 -> 25 -> 32: ceil(2100 / 32) = 66
              2: (33, 64),      # t = 5 x 2 = 10 -> want 52 -> 41 -> 64: 33
              3: (66, 32),      # t = 2 x 1 = 2 -> want 256 -> 128 -> 17 -> 32: 66
              4: (66, 32)}      # t = 5 x 1 = 5 -> want 103 -> 21 -> 32: 66
    with knobs(lib, {3: row}):
        r = ok(lib, "cconv_bwd_w", 2100, 80, 64)
        assert brief(r) == ("gemm16", row, CCONV_BW16[row]) and (r["splits"], r["klen"]) == expect[row]
        with knobs(lib, {5: 7}):            # ceil(2100 / 7) = 300 -> 320: 7 ranges
            r = ok(lib, "cconv_bwd_w", 2100, 80, 64)
            assert brief(r) == ("gemm16", row, CCONV_BW16[row]) and (r["splits"], r["klen"]) == (7, 320)
        # outputs above 512 x 512 floats stay on the 32x32x2 family
        assert ok(lib, "cconv_bwd_w", 2100, 520, 512)["family"] == "generic"


def test_cconv_bwd_w_step_forms(lib):
    with knobs(lib, {3: 0}):
        r = ok(lib, "cconv_bwd_w", 2100, 80, 64)            # 17 ranges of 128 rows, each as one k-tile (knob 7)
        assert brief(r) == ("generic", 0, (64, 64, 128)) and (r["splits"], r["klen"]) == (17, 128)
        with knobs(lib, {7: 0}):
            assert brief(ok(lib, "cconv_bwd_w", 2100, 80, 64)) == ("generic", 0, (64, 64, 64))
    for want, plan in ((1, (1, 2112)), (7, (7, 320)), (128, (33, 64)), (1000, (33, 64))):
        with knobs(lib, {5: want}):
            r = ok(lib, "cconv_bwd_w", 2100, 80, 64)
            assert brief(r) == ("kmajor", 0, (64, 64, 64)) and (r["splits"], r["klen"]) == plan, want
            with knobs(lib, {3: 2}):
                r = ok(lib, "cconv_bwd_w", 2100, 80, 64)
                assert r["family"] == "gemm16" and r["splits"] == -(-2100 // r["klen"]) and r["klen"] % 32 == 0


@pytest.mark.parametrize("v", sorted(SKINNY16))
def test_skinny_variants(lib, v):
    """Knob 8 = 1..4 at (73, 260, 300): N = 300 (dense_fwd) / K = 260 (dense_bwd_x: its output columns) are no multiples of 16,
    so the few-row tiles decline; M <= 96, N and K >= 256 and multiples of 4: the skinny tiles."""
    with knobs(lib, {8: v}):
        assert brief(ok(lib, "dense_fwd", 73, 260, 300)) == ("skinny", v, SKINNY16[v])
        assert brief(ok(lib, "dense_bwd_x", 73, 260, 300)) == ("skinny", v, SKINNY16[v])
        assert brief(ok(lib, "dense_fwd", 96, 256, 644)) == ("skinny", v, SKINNY16[v])
        assert brief(ok(lib, "dense_bwd_x", 96, 260, 644)) == ("skinny", v, SKINNY16[v])
        assert brief(ok(lib, "dense_fwd", 73, 896, 896)) == ("fewrow", 0, (16, 16, 896))
        with knobs(lib, {21: 0}):
            assert brief(ok(lib, "dense_fwd", 73, 896, 896)) == ("skinny", v, SKINNY16[v])
            assert brief(ok(lib, "dense_bwd_x", 73, 896, 896)) == ("skinny", v, SKINNY16[v])
            # the grouped backward's few-row grid runs dX on variant 1 whatever the knob says
            r = ok(lib, "dense_bwd", 73, 896, 896)
            assert brief(r) == ("skinny", 1, (16, 64, 64)) and r["wtile"] == (64, 64) and (r["splits"], r["klen"]) == (1, 128)


def test_few_row_thresholds(lib):
    # M = 96 / 97
    assert brief(ok(lib, "dense_fwd", 96, 256, 644)) == ("skinny", 1, (16, 64, 64))
    assert brief(ok(lib, "dense_fwd", 97, 256, 644)) == ("gemm16", 0, (48, 64, 64))
    assert brief(ok(lib, "dense_fwd", 96, 896, 640)) == ("fewrow", 0, (16, 16, 896))
    assert brief(ok(lib, "dense_fwd", 97, 896, 640)) == ("gemm16", 0, (48, 64, 64))
    assert brief(ok(lib, "dense_bwd_x", 96, 640, 896)) == ("fewrow", 0, (16, 16, 896))
    assert brief(ok(lib, "dense_bwd_x", 97, 640, 896)) == ("generic", 0, (64, 64, 64))
    assert ok(lib, "dense_bwd", 96, 896, 640)["family"] == "fewrow"
    assert ok(lib, "dense_bwd", 97, 896, 640)["family"] in ("two_launch", "grouped_kmajor")
    # K = 1152 / 1168 (multiples of 16): the deepest few-row instantiation covers 18 slots of 64
    assert brief(ok(lib, "dense_fwd", 73, 1152, 640)) == ("fewrow", 0, (16, 16, 1152))
    assert brief(ok(lib, "dense_fwd", 73, 1168, 640)) == ("skinny", 1, (16, 64, 64))
    assert brief(ok(lib, "dense_bwd_x", 73, 640, 1152)) == ("fewrow", 0, (16, 16, 1152))
    assert brief(ok(lib, "dense_bwd_x", 73, 640, 1168)) == ("skinny", 1, (16, 64, 64))
    # the slot counts instantiated: 3, 4, 10, 14, 18
    for K, slots in ((128, 3), (192, 3), (208, 4), (256, 4), (272, 10), (640, 10), (656, 14), (896, 14), (912, 18)):
        assert brief(ok(lib, "dense_fwd", 73, K, 640)) == ("fewrow", 0, (16, 16, 64 * slots)), K
    # N % 16
    assert brief(ok(lib, "dense_fwd", 73, 896, 896)) == ("fewrow", 0, (16, 16, 896))
    assert brief(ok(lib, "dense_fwd", 73, 896, 900)) == ("skinny", 1, (16, 64, 64))
    assert brief(ok(lib, "dense_fwd", 73, 896, 898)) == ("generic", 0, (64, 64, 64))         # N % 4 != 0: scalar loaders
    # skinny wants N, K >= 256; below, the 48x64 tiles (K >= 128) or the 32x32x2 family
    assert brief(ok(lib, "dense_fwd", 73, 260, 252)) == ("gemm16", 0, (48, 64, 64))
    assert brief(ok(lib, "dense_fwd", 73, 100, 300)) == ("generic", 0, (64, 64, 64))
    with knobs(lib, {8: 0}):
        assert brief(ok(lib, "dense_fwd", 73, 896, 896)) == ("gemm16", 0, (48, 64, 64))
        assert brief(ok(lib, "dense_bwd_x", 73, 896, 896)) == ("generic", 0, (64, 64, 64))
    # big = 511 / 512 for the 48x64 tiles of knob 10
    assert brief(ok(lib, "dense_fwd", 511 * 128, 128, 128)) == ("gemm16", 0, (48, 64, 64))
    assert brief(ok(lib, "dense_fwd", 511 * 128 + 1, 128, 128)) == ("generic", 0, (128, 128, 32))
    with knobs(lib, {10: 0}):
        assert brief(ok(lib, "dense_fwd", 511 * 128, 128, 128)) == ("generic", 0, (64, 64, 64))


def test_dense_bwd_w_splits(lib):
    """Knob 4 on the stand-alone weight gradient at (600, 260, 132): plan_splitk(260, 132, 600): 5 x 3 = 15 tiles < 32 ->
    256 / 15 = 17, at most ceil(600 / 128) = 5 ranges -> klen 120 -> 128: 5 ranges (128 <= 256: the k-major form keeps them).
    Knob 4 = n: min(n, max_splits16 = 8) ranges of ceil(600 / n) rounded up to 64."""
    for k1, fam in ((7, "kmajor"), (0, "generic")):
        with knobs(lib, {1: k1}):
            r = ok(lib, "dense_bwd_w", 600, 260, 132)
            assert (r["family"], r["tile"], r["splits"], r["klen"]) == (fam, (64, 64, 64), 5, 128)
            for n, plan in ((1, (1, 640)), (2, (2, 320)), (3, (3, 256)), (5, (5, 128)), (8, (5, 128))):
                with knobs(lib, {4: n}):
                    r = ok(lib, "dense_bwd_w", 600, 260, 132)
                    # (one range: the 32x32x2 family writes dw itself)
                    assert (r["family"], r["splits"], r["klen"]) == ("generic" if n == 1 else fam, ) + plan, (k1, n)
    # (knob 4 = 8 above: ceil(600 / 8) = 75 -> 128 rows: ceil(600 / 128) = 5 ranges, not 8)
    # (2000, 64, 64): one tile -> 256 ranges wanted, at most ceil(2000 / 128) = 16: klen 125 -> 128, 16 ranges
    r = ok(lib, "dense_bwd_w", 2000, 64, 64)
    assert (r["family"], r["splits"], r["klen"]) == ("kmajor", 16, 128)
    with knobs(lib, {4: 5}):
        assert (ok(lib, "dense_bwd_w", 2000, 64, 64)["splits"], ok(lib, "dense_bwd_w", 2000, 64, 64)["klen"]) == (5, 448)


RX = (7, 80, 64, 320)          # S, kin, F, D: dense layer 896 x 640, max_splits16 = min(8, ceil(1024 / 140)) = 8
# the plain plan of the fused backward launch: ceil(batch / 448) ranges wanted, ceil(batch / want) rows rounded up to 64
PLAIN = {767: (2, 384), 768: (2, 384), 775: (2, 448), 1170: (3, 448), 1536: (4, 384)}


@pytest.mark.parametrize("preset", range(1, 25))
def test_graded_presets(lib, preset):
    with knobs(lib, {14: preset}):
        for batch in (768, 775, 1170, 1536):
            r = ok(lib, "rx_backward", batch, *RX)
            assert brief(r) == ("rx_fused", 0, (64, 64, 64)) and r["wtile"] == (64, 64)
            off, n = r["koff"], r["nranges"]
            assert 2 <= n <= 8 and n == r["splits"] and len(off) == n + 1, (batch, r)
            assert off[0] == 0 and off[-1] == batch and all(a < b for a, b in zip(off, off[1:])), (batch, off)
            assert all(o % 64 == 0 for o in off[1:-1]), (batch, off)
            assert r["klen"] == PLAIN[batch][1]


def test_graded_presets_by_hand_and_outside_their_range(lib):
    # preset 14 = {9, 5, 2, 2, 1} / 19 of 13 k-tiles: cumulative 9, 14, 16, 18, 19 -> floor(x * 13 / 19) = 6, 9, 10, 12, then all 13
    assert ok(lib, "rx_backward", 775, *RX)["koff"] == [0, 384, 576, 640, 768, 775]
    with knobs(lib, {14: 4}):           # {10, 9}: floor(10 * 13 / 19) = 6
        assert ok(lib, "rx_backward", 775, *RX)["koff"] == [0, 384, 775]
    with knobs(lib, {14: 24}):          # {10, 4, 2, 1, 1, 1} / 19 of 12 k-tiles: 6, 8, 10, 10 (no tile: dropped), 11, 12
        assert ok(lib, "rx_backward", 768, *RX)["koff"] == [0, 384, 512, 640, 704, 768]
    for preset, batch in ((0, 775), (25, 775), (1000, 775), (14, 767), (1, 767)):
        with knobs(lib, {14: preset}):
            r = ok(lib, "rx_backward", batch, *RX)
            assert brief(r) == ("rx_fused", 0, (64, 64, 64))
            assert (r["nranges"], r["koff"], r["splits"], r["klen"]) == (0, [], ) + PLAIN[batch], (preset, batch)
    # refused where dccn_rx_backward refuses: kin other than 64 / 80, the launch switched off, dW not in the k-major form
    assert route(lib, "rx_backward", 775, 7, 72, 64, 320)[0] == -1
    assert route(lib, "rx_backward", 775, 7, 80, 64, 0)[0] == -1
    for off in ({11: 0}, {1: 0}, {1: 3}):
        with knobs(lib, off):
            assert route(lib, "rx_backward", 775, *RX)[0] == -1


def test_out_of_range_knob_values(lib):
    """One past the last table row and a large number: refusal or a documented fallback family, never a table index.
    (Knob 1 = 7 and knob 3 = 7 are the k-major forms, knob 2 = 7..11 the staged forms: one past THOSE is meant as well.)"""
    for v in (8, 9, 1000, 2 ** 31 - 1):
        with knobs(lib, {1: v}):
            assert route(lib, "dense_bwd", 137, 200, 132)[0] == -1                   # where a row would have run: refused
            assert ok(lib, "dense_bwd", 73, 896, 640)["family"] == "fewrow"          # few rows never read the knob
            assert ok(lib, "dense_bwd", 137, 202, 132)["family"] in ("two_launch", "grouped")     # nor do scalar loaders
            assert ok(lib, "dense_bwd_w", 600, 260, 132)["family"] == "generic"      # not 7: no k-major form
    for v in (12, 13, 1000, 2 ** 31 - 1):
        with knobs(lib, {2: v}):                                                     # as 0: the 32x32x2 family
            assert brief(ok(lib, "cconv_fwd", 131, 34, 18)) == ("generic", 0, (64, 64, 64))
            assert brief(ok(lib, "cconv_fwd", 1000, 80, 64)) == ("generic", 0, (64, 64, 160))
    for v in (5, 6, 8, 1000, 2 ** 31 - 1):
        with knobs(lib, {3: v}):
            assert route(lib, "cconv_bwd_w", 2100, 80, 64)[0] == -1
            assert ok(lib, "cconv_bwd_w", 2100, 520, 512)["family"] == "generic"     # large outputs never read the rows
    for v in (5, 6, 1000, 2 ** 31 - 1):
        with knobs(lib, {8: v}):
            assert route(lib, "dense_fwd", 73, 260, 300)[0] == -1
            assert route(lib, "dense_bwd_x", 73, 260, 300)[0] == -1
            assert ok(lib, "dense_fwd", 73, 896, 896)["family"] == "fewrow"          # any value > 0 switches the few-row tiles on
            assert ok(lib, "dense_fwd", 97, 256, 644)["family"] == "gemm16"
    assert lib.dccn_set_tuning(1, -1) == -1 and lib.dccn_set_tuning(8, -5) == -1
