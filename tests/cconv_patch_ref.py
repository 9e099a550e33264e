"""Plain NumPy float64 restatement of the general-k complex convolutions' contract, and the case tables of their launch paths.

The contract is written in ``ops.cconv_patch``: what ``cconv_gemm(cconv_im2col(x, ...), w, bias)`` computes.  Restated here:
``gather`` (the patch rows, zeros where the padding lies), ``forward`` / ``backward`` (``O.cconv_gemm_fwd`` / ``O.cconv_gemm_bwd``
on the gathered rows, the patch gradient scattered back into dx) and ``unreached`` (the dx cells no live tap reaches: exact
zeros).  The geometry arguments come from ``complex.tf_padding`` and ``complex._live_taps``, so a case hands the C ABI what the
layer would hand it.  tests/test_cconv_patch_ref.py ties this file to the literal restatement of the reference layers
(oracle/dccn_oracle.py, oracle/torch_ref.py) at 1e-12; tests/test_gpu_cconv_patch_routes.py holds the kernels to it.

``dx_by_phase`` is the same input gradient gathered position by position, one stride phase at a time (the order the few-channel
kernel works in); ``narrow_tiles`` and ``chunk_rows`` lay out which rows a tile / a chunk of the persistent kernels owns.  They
exist so that an index error can be planted in a copy of the restatement (test_cconv_patch_ref.py: every case family must
notice the error that belongs to it).

CASES: every case exists for the kernel variant its ``plan`` names -- what dccn_cconv_patch_plan_query must answer at 256 CUs.
"""
import collections

import numpy as np

from dl_ofdm_amd.complex import _live_taps, tf_padding
from oracle import dccn_oracle as O

Geom = collections.namedtuple("Geom", "B L Wd C F kL kW sL sW padding Lo Wo pl0 pw0 tl tw ntl ntw tl0 tw0")


def geometry(shape, F, kern, strides, padding):
    """(B, L, Wd, C) -> F, kernel (kL, kW), strides (sL, sW), 'same' / 'valid' -> what complex._cconv_lower derives"""
    B, L, Wd, C = shape
    (kL, kW), (sL, sW) = kern, strides
    Lo, pl0, _ = tf_padding(L, kL, sL, padding)
    Wo, pw0, _ = tf_padding(Wd, kW, sW, padding)
    tl, tw = _live_taps(L, kL, sL, Lo, pl0), _live_taps(Wd, kW, sW, Wo, pw0)
    assert tl == list(range(tl[0], tl[0] + len(tl))) and tw == list(range(tw[0], tw[0] + len(tw)))
    return Geom(B, L, Wd, C, F, kL, kW, sL, sW, padding, Lo, Wo, pl0, pw0, tl, tw, len(tl), len(tw), tl[0], tw[0])


def abi_geom(g):
    """the (B, L, Wd, C, Lo, Wo, ntl, ntw, tl0, tw0, sL, sW, pl0, pw0) run of the C ABI's patch operators"""
    return (g.B, g.L, g.Wd, g.C, g.Lo, g.Wo, g.ntl, g.ntw, g.tl0, g.tw0, g.sL, g.sW, g.pl0, g.pw0)


def _span(n_in, n_out, stride, off):
    """outputs o in [o0, o1) whose input index o * stride + off lies inside [0, n_in)"""
    o0 = max(0, -(off // stride))                    # ceil(-off / stride)
    o1 = min(n_out, (n_in - 1 - off) // stride + 1)
    return o0, max(o0, o1)


def _taps(g):
    """every live tap pair: (ti, tj, output slices, input slices)"""
    for ti in range(g.ntl):
        offl = g.tl0 + ti - g.pl0
        a0, a1 = _span(g.L, g.Lo, g.sL, offl)
        for tj in range(g.ntw):
            offw = g.tw0 + tj - g.pw0
            b0, b1 = _span(g.Wd, g.Wo, g.sW, offw)
            if a1 > a0 and b1 > b0:
                yield (ti, tj, slice(a0, a1), slice(b0, b1),
                       slice(a0 * g.sL + offl, (a1 - 1) * g.sL + offl + 1, g.sL),
                       slice(b0 * g.sW + offw, (b1 - 1) * g.sW + offw + 1, g.sW))


def gather(x, g):
    """x [B, L, Wd, C, 2] -> patch rows [B, Lo, Wo, ntl, ntw, C, 2], zeros where the padding lies"""
    rows = np.zeros((g.B, g.Lo, g.Wo, g.ntl, g.ntw, g.C, 2), dtype=np.float64)
    for ti, tj, so_l, so_w, si_l, si_w in _taps(g):
        rows[:, so_l, so_w, ti, tj] = x[:, si_l, si_w]
    return rows


def scatter(drows, g):
    """the adjoint of gather: patch gradient [B, Lo, Wo, ntl, ntw, C, 2] summed into dx [B, L, Wd, C, 2]"""
    dx = np.zeros((g.B, g.L, g.Wd, g.C, 2), dtype=np.float64)
    for ti, tj, so_l, so_w, si_l, si_w in _taps(g):
        dx[:, si_l, si_w] += drows[:, so_l, so_w, ti, tj]
    return dx


def unreached(g):
    """[L, Wd] bool: input cells that no live tap of any output position reads -- their dx is exactly 0"""
    n = np.zeros((g.L, g.Wd), dtype=np.int64)
    for ti, tj, so_l, so_w, si_l, si_w in _taps(g):
        n[si_l, si_w] += 1
    return n == 0


def forward(x, w, bias, g):
    """-> out [B*Lo*Wo, F, 2]"""
    rows = gather(np.asarray(x, np.float64), g).reshape(g.B * g.Lo * g.Wo, g.ntl * g.ntw * g.C, 2)
    return O.cconv_gemm_fwd(rows, np.asarray(w, np.float64), None if bias is None else np.asarray(bias, np.float64))


def patch_grad(w, dout, g):
    """dout [B*Lo*Wo, F, 2] -> the gradient of the patch rows [B, Lo, Wo, ntl, ntw, C, 2]"""
    zero = np.zeros((dout.shape[0], g.ntl * g.ntw * g.C, 2))
    return O.cconv_gemm_bwd(zero, np.asarray(w, np.float64), np.asarray(dout, np.float64))[0].reshape(
        g.B, g.Lo, g.Wo, g.ntl, g.ntw, g.C, 2)


def backward(x, w, dout, g):
    """-> dx [B, L, Wd, C, 2], dw [ntl*ntw*C, 2F], dbias [2F]"""
    rows = gather(np.asarray(x, np.float64), g).reshape(g.B * g.Lo * g.Wo, g.ntl * g.ntw * g.C, 2)
    dr, dw, db = O.cconv_gemm_bwd(rows, np.asarray(w, np.float64), np.asarray(dout, np.float64))
    return scatter(dr.reshape(g.B, g.Lo, g.Wo, g.ntl, g.ntw, g.C, 2), g), dw, db


def weight_grads(x, w, dout, g, row_weight):
    """dw, dbias of backward() with output row r counted row_weight[r] times (all ones: the contract; the planted errors count
    some rows twice or never)"""
    rows = gather(np.asarray(x, np.float64), g).reshape(g.B * g.Lo * g.Wo, g.ntl * g.ntw * g.C, 2)
    d = np.asarray(dout, np.float64) * np.asarray(row_weight, np.float64)[:, None, None]
    return O.cconv_gemm_bwd(rows, np.asarray(w, np.float64), d)[1:]


def dx_by_phase(drows, g, first_tap_shift=0):
    """scatter(drows, g) restated as a gather: the positions of stride phase (pl, pw) = (l mod sL, w mod sW) meet data at every
    sL-th / sW-th tap from a first live tap on.  first_tap_shift = 1 plants the error 'first live tap of a phase off by one'."""
    dx = np.zeros((g.B, g.L, g.Wd, g.C, 2), dtype=np.float64)
    for pl in range(g.sL):
        for pw in range(g.sW):
            l, w = np.arange(pl, g.L, g.sL), np.arange(pw, g.Wd, g.sW)
            t0l = (pl + g.pl0 - g.tl0) % g.sL + first_tap_shift
            t0w = (pw + g.pw0 - g.tw0) % g.sW + first_tap_shift
            for ti in range(t0l, g.ntl, g.sL):
                lo = (l + g.pl0 - g.tl0 - ti) // g.sL
                vl = (lo >= 0) & (lo < g.Lo)
                for tj in range(t0w, g.ntw, g.sW):
                    wo = (w + g.pw0 - g.tw0 - tj) // g.sW
                    vw = (wo >= 0) & (wo < g.Wo)
                    dx[:, l[vl][:, None], w[vw][None, :]] += drows[:, lo[vl][:, None], wo[vw][None, :], ti, tj]
    return dx


def narrow_tiles(g):
    """The few-channel input gradient's work list: per stride phase, its positions (b, lq, wq) in row-major order cut into
    tiles of 64; -> (tiles [n, 64] of linear positions into [B*L*Wd], -1 behind a phase's last row; first tile of each phase)"""
    tiles, first = [], []
    for pl in range(g.sL):
        for pw in range(g.sW):
            l, w = np.arange(pl, g.L, g.sL), np.arange(pw, g.Wd, g.sW)
            pos = ((np.arange(g.B)[:, None, None] * g.L + l[None, :, None]) * g.Wd + w[None, None, :]).reshape(-1)
            n = -(-pos.size // 64)
            first.append(sum(t.shape[0] for t in tiles))
            tiles.append(np.concatenate([pos, np.full(n * 64 - pos.size, -1, dtype=pos.dtype)]).reshape(n, 64))
    return np.concatenate(tiles), first


def chunk_rows(g, PL, nch, upper_shift=0):
    """The fused 1-D backward's ownership: chunk j of a batch item owns the positions [j PL, min((j + 1) PL, L)) and the output
    rows below the first row the next chunk holds completely; -> per chunk (p0, p1, q0, q1).  upper_shift = 1 plants the error
    'ownership boundary off by one row' (the boundary row is counted by both neighbours)."""
    o, out, q0 = g.tl0 - g.pl0, [], 0
    for j in range(nch):
        p0, p1 = j * PL, min((j + 1) * PL, g.L)
        q1 = g.Lo if j + 1 == nch else min(g.Lo, max(0, -((-(p1 - o - (g.ntl - 1))) // g.sL)))
        out.append((p0, p1, q0, min(g.Lo, q1 + (upper_shift if j + 1 < nch else 0))))
        q0 = q1
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "shape F kern strides padding op plan twin why")
_N, _G, _K, _F1 = "dx_narrow", "gemm", "kmajor", "conv1d_fused"


def _nar(col_tiles, depth, lds, nmaj, **kw):
    return dict(kernel=_N, col_tiles=col_tiles, depth=depth, bt_lds=lds, taps_fastest=nmaj, **kw)


def _tile(r, c, k):
    return dict(kernel=_G, tile_rows=r, tile_cols=c, tile_k=k)


# name -> geometry (B, L, Wd, C) -> F, kernel, strides, padding; the operator the case exists for and the plan fields its
# query must report at 256 CUs; its reduced-size twin (B, L, Wd) for the CPU tie to the literal layers; what it is for
CASES = collections.OrderedDict([
    # A. fused 1-D backward loop (dccn_cconv1d_bwd): min(2 CUs, 1024, items) = 512 persistent blocks
    ("A1", Case((131, 500, 1, 2), 32, (5, 1), (1, 1), "same", "bwd_1d", dict(kernel=_F1, positions=59, chunks=9, items=1179, grid=512),
                (2, 70, 1), "blocks run 2 and 3 chunks, a block's sequence crosses batch items, the last chunk of an item owns 28 positions")),
    ("A2", Case((70, 560, 1, 2), 64, (5, 1), (1, 1), "same", "bwd_1d", dict(kernel=_F1, positions=59, chunks=10, items=700, grid=512),
                (2, 70, 1), "2F = 128; 188 blocks run two chunks, the rest one")),
    ("A3", Case((200, 333, 1, 2), 64, (5, 1), (2, 1), "same", "bwd_1d", dict(kernel=_F1, positions=121, chunks=3, items=600, grid=512),
                (2, 135, 1), "strided ownership across the loop")),
    ("A4", Case((520, 40, 1, 6), 32, (2, 1), (1, 1), "same", "bwd_1d", dict(kernel=_F1, positions=62, chunks=1, items=520, grid=512),
                (3, 40, 1), "even kernel, 24 patch columns; 8 blocks run a second item: the smallest looping shape")),
    ("A5", Case((260, 120, 1, 2), 32, (7, 1), (1, 1), "valid", "bwd_1d", dict(kernel=_F1, positions=57, chunks=3, items=780, grid=512),
                (2, 70, 1), "VALID: o = 0, Lo = 114 < L, chunks of 57, 57 and 6 positions")),
    # B. few-channel input gradient (cconv_dx_narrow_kernel<col tiles, depth, LDS, NMAJ>), min(tiles, 6 CUs) persistent blocks
    ("B1", Case((3, 41, 1, 12), 16, (3, 1), (1, 1), "same", "bwd_x", _nar(2, 2, 1, 1, phases=1, tiles=2, grid=2),
                (2, 9, 1), "<2,2,LDS,NMAJ>: 24 columns, the second column tile half masked")),
    ("B2", Case((3, 41, 1, 10), 4, (3, 1), (2, 1), "same", "bwd_x", _nar(2, 2, 1, 0, phases=2),
                (2, 9, 1), "<2,2,LDS,->, two phases")),
    ("B3", Case((3, 41, 1, 10), 6, (3, 1), (1, 1), "same", "bwd_x", _nar(2, 1, 1, 0, phases=1),
                (2, 9, 1), "<2,1,LDS,->: k groups span taps (2F = 12)")),
    ("B4", Case((3, 37, 1, 8), 64, (9, 1), (1, 1), "same", "bwd_x", _nar(1, 2, 0, 0, phases=1),
                (2, 11, 1), "<1,2,global,->: Bt is 74 752 B, over the LDS limit")),
    ("B5", Case((2, 12, 12, 8), 6, (9, 10), (1, 1), "same", "bwd_x", _nar(1, 1, 0, 0, phases=1),
                (1, 5, 6), "<1,1,global,->: 90 taps, most of them in the padding at any position")),
    ("B6", Case((3, 50, 1, 16), 64, (5, 1), (2, 1), "same", "bwd_x", _nar(2, 2, 0, 0, phases=2, tiles=4, grid=4),
                (2, 9, 1), "<2,2,global,->, two phases")),
    ("B7", Case((2, 11, 13, 16), 6, (7, 7), (1, 1), "same", "bwd_x", _nar(2, 1, 0, 0, phases=1),
                (1, 5, 6), "<2,1,global,->")),
    ("B8", Case((2, 19, 21, 2), 8, (5, 5), (4, 4), "same", "bwd_x", _nar(1, 2, 1, 0, phases=16, tiles=16, grid=16),
                (1, 9, 10), "the phase limit: 16 phases with 1, 2 and 4 live-tap combinations")),
    ("B9", Case((1, 2, 3, 2), 4, (1, 1), (3, 3), "same", "bwd_x", _nar(1, 2, 1, 0, phases=9, tiles=6, grid=6),
                (1, 2, 3), "phases with no rows (Lp = 0), unreached dx cells (exact zeros), tiles of fewer than 16 rows")),
    ("B10", Case((2, 19, 21, 2), 8, (5, 7), (3, 6), "same", "bwd_x", _tile(64, 64, 64),
                 (1, 9, 13), "18 phases: not narrow, the wide inverse-stride gather with N = 4 columns")),
    ("B11", Case((180, 560, 1, 2), 16, (5, 1), (1, 1), "same", "bwd_x", _nar(1, 2, 1, 1, phases=1, tiles=1575, grid=1536),
                 (2, 70, 1), "persistent loop: 39 blocks run a second tile (100 800 positions: every tile full)")),
    ("B12", Case((180, 1121, 1, 2), 16, (5, 1), (2, 1), "same", "bwd_x", _nar(1, 2, 1, 1, phases=2, tiles=3153, grid=1536),
                 (2, 71, 1), "blocks run 2-3 tiles and step from phase 0 (561 rows per item, last tile ragged: 52 rows) into phase 1 (560)")),
    # C. wide input gradient (OP_KPATCH over dout, inverse-stride gather)
    ("C1", Case((2, 70, 1, 18), 6, (5, 1), (2, 1), "same", "bwd_x", _tile(64, 64, 64),
                (1, 11, 1), "smallest wide strided shape: K = 60 (one masked k-tile), N = 36, negative fine positions at the left edge")),
    ("C2", Case((2, 70, 1, 18), 6, (5, 1), (3, 1), "valid", "bwd_x", _tile(64, 64, 64),
                (1, 11, 1), "a non-power-of-two inverse stride (il_mul)")),
    ("C3", Case((2, 33, 9, 40), 10, (3, 2), (2, 3), "same", "bwd_x", _tile(64, 64, 64),
                (1, 7, 7), "both inverse strides, two tap axes; N = 80 (second column tile ragged), K = 120")),
    ("C4", Case((3, 64, 1, 20), 16, (3, 1), (1, 1), "same", "bwd_x", _tile(64, 64, 32),
                (1, 9, 1), "the 32-deep k-tile on a patch operand (K = 96)")),
    ("C5", Case((512, 128, 1, 34), 2, (3, 1), (1, 1), "same", "bwd_x", _tile(128, 128, 32),
                (1, 9, 1), "the large tile on a patch operand: 65 536 rows is the fewest at which it exists (K = 12, N = 68)")),
    # D. forward (OP_KPATCH x OP_CCONV_W) tiles
    ("D1", Case((3, 40, 1, 16), 8, (5, 1), (1, 1), "same", "fwd", _tile(64, 64, 32),
                (1, 9, 1), "the forward's 32-deep k-tile (K = 160)")),
    ("D2", Case((512, 128, 1, 2), 34, (3, 1), (1, 1), "same", "fwd", _tile(128, 128, 32),
                (1, 9, 1), "the forward's large tile (N = 68, 65 536 rows)")),
    # control: two shapes of the existing parametrisations of tests/test_layer_api.py
    ("X1", Case((37, 560, 1, 2), 64, (5, 1), (1, 1), "same", "bwd_1d", dict(kernel=_F1, positions=59, chunks=10, items=370, grid=370),
                (2, 70, 1), "control: test_conv1d_fused_backward_vs_separate_routes_and_literal's first shape")),
    ("X2", Case((16, 512, 1, 8), 16, (5, 1), (1, 1), "same", "bwd_x", _nar(1, 2, 1, 1, phases=1, tiles=128, grid=128),
                (2, 70, 1), "control: test_conv1d_implicit_gemm_vs_literal_and_im2col's largest shape")),
])


def case_geom(name):
    c = CASES[name]
    return geometry(c.shape, c.F, c.kern, c.strides, c.padding)


def twin_geom(name):
    c = CASES[name]
    return geometry(c.twin + (c.shape[3],), c.F, c.kern, c.strides, c.padding)


def query(lib, op, g):
    """dccn_cconv_patch_plan_query -> (status, dict of the plan's fields with the kernel by name)"""
    import ctypes as C
    from dl_ofdm_amd import _lib
    p = _lib.CconvPatchPlan()
    st = lib.dccn_cconv_patch_plan_query(_lib.PATCH_OPS[op], g.B, g.L, g.Wd, g.C, g.Lo, g.Wo, g.ntl, g.ntw, g.sL, g.sW, g.F, C.byref(p))
    d = {n: getattr(p, n) for n, _ in _lib.CconvPatchPlan._fields_}
    d["kernel"] = {v: k for k, v in _lib.PATCH_KERNELS.items()}[d["kernel"]]
    return st, d


def assert_plan(lib, name, what=""):
    """the plan the case exists for is what its geometry runs"""
    c, g = CASES[name], case_geom(name)
    st, got = query(lib, c.op, g)
    assert st == 0, "%s %s: query refused%s" % (name, c.op, what)
    for k, v in c.plan.items():
        assert got[k] == v, "%s %s: %s = %r, the case needs %r (%s)%s" % (name, c.op, k, got[k], v, got, what)
    return got


_HOST = {}


def host_case(name):
    """float32 operands and the float64 restatement of a case, built once per process"""
    if name not in _HOST:
        c, g = CASES[name], case_geom(name)
        rng = np.random.RandomState(sum(ord(ch) for ch in name) * 131 + g.L)
        kin = g.ntl * g.ntw * g.C
        x = rng.randn(g.B, g.L, g.Wd, g.C, 2).astype(np.float32)
        w = (rng.randn(kin, 2 * g.F) / np.sqrt(kin)).astype(np.float32)
        bias = rng.randn(2 * g.F).astype(np.float32)
        dout = rng.randn(g.B * g.Lo * g.Wo, g.F, 2).astype(np.float32)
        dx, dw, db = backward(x, w, dout, g)
        _HOST[name] = dict(g=g, x=x, w=w, bias=bias, dout=dout, out=forward(x, w, bias, g), dx=dx, dw=dw, db=db,
                           unreached=unreached(g))
    return _HOST[name]
