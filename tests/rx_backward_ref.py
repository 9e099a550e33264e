"""Float64 NumPy model of what the fused backward launch leaves for the C-Conv weight gradient and of how the fold reads it.

Written from the contract stated in csrc/rx_bwd.h (the dX tiles' epilogue) and csrc/gemm_f32_mfma.h (cconv_fold_body with
tilew = 64), not from the kernels' lane arithmetic:

  * dfft is [batch, S * 2F]; a dX tile is 64 frames x 64 columns, tile q = row_tile * ntn + column_tile with ntn = S * 2F / 64.
    A tile lies inside ONE symbol s = n0 // 2F (2F is a multiple of 64), so there are 2F / 64 tiles per symbol.
  * the tile contracts its 64 dfft columns with x_norm[frame, s, 0 .. 2kin) of its frames (rows past the batch are zero):
    dWeff[m, c] = sum_frames x[frame][m] * dfft[frame][n0 + c], and stores it folded,
    partial[q][n][j] = {dWeff[2n, 2j] - dWeff[2n+1, 2j+1], dWeff[2n, 2j+1] - dWeff[2n+1, 2j]}, next to colsum[q][c].
  * the fold sums `terms` = ceil(batch / 64) * S terms per element: term z = row_tile * S + s, column tile h = 2f // 64 of
    the symbol, at tile z * tiles_per_symbol + h; dbias[f] = sum_z colsum[.][2f] - colsum[.][2f + 1], dbias[F + f] = -dbias[f].

The keyword arguments plant the errors an index rewrite of the launch can make (tests/test_rx_backward_ref.py): with their
defaults the model is the contract.  A read past the last tile returns NaN, as the NaN-filled workspace of
tests/test_gpu_rx_backward_shapes.py would.
"""
import numpy as np

TILE = 64

# (batch, S, kin, F, D) -> (dX tiles nx, tiles per symbol, dense dW ranges, graded): the smallest accepted shapes that reach each
# edge of the launch's index arithmetic (DESIGN.md "Tests: hold the fused backward launch ..." says what each one is for).  The
# plan facts are asserted through dccn_rx_bwd_fused_supported and dccn_gemm_route_query before any of them is launched.
SHAPES = {
    (1, 1, 80, 32, 2): (1, 1, 1, False),
    (65, 7, 64, 32, 50): (14, 1, 1, False),
    (63, 3, 80, 96, 34): (9, 3, 1, False),
    (129, 2, 64, 128, 320): (24, 4, 1, False),
    (70, 1, 64, 160, 10): (10, 5, 1, False),
    (128, 1, 80, 64, 322): (4, 2, 1, False),
    (200, 14, 80, 64, 50): (112, 2, 1, False),
    (500, 7, 64, 32, 50): (56, 1, 2, False),
    (800, 7, 80, 32, 50): (91, 1, 5, True),
    (800, 7, 64, 128, 50): (364, 4, 5, True),
}
# the shapes of test_gpu_ops.py::test_rx_backward_fused: all S = 7, F = 64
OLD_SHAPES = [(1170, 7, 80, 64, 320), (64, 7, 64, 64, 320), (37, 7, 80, 64, 50), (200, 7, 64, 64, 322)]


def geometry(batch, S, F):
    """(row tiles, column tiles per row tile, tiles per symbol)"""
    assert (2 * F) % TILE == 0
    return -(-batch // TILE), S * 2 * F // TILE, 2 * F // TILE


def tile_partials(xn, dfft, batch, S, kin, F, symbol_of=None, zero_past_batch=True):
    """(partial [tiles, kin, 32, 2], colsum [tiles, 64]).  symbol_of(n0): the symbol whose x rows the tile at column n0
    contracts with (default n0 // 2F); zero_past_batch = False: the last row tile keeps the clamped duplicates of the last
    frame that the accumulators and the staged x rows hold past the batch."""
    nrt, ntn, _ = geometry(batch, S, F)
    x = np.asarray(xn, np.float64).reshape(batch, S, 2 * kin)
    d = np.asarray(dfft, np.float64).reshape(batch, S * 2 * F)
    partial = np.empty((nrt * ntn, kin, TILE // 2, 2))
    colsum = np.empty((nrt * ntn, TILE))
    for rt in range(nrt):
        rows = np.arange(rt * TILE, (rt + 1) * TILE)
        rows = rows[rows < batch] if zero_past_batch else np.minimum(rows, batch - 1)
        for ct in range(ntn):
            n0 = ct * TILE
            s = n0 // (2 * F) if symbol_of is None else symbol_of(n0)
            dt = d[rows, n0:n0 + TILE]
            # dWeff of the tile: [2kin, 64] (a symbol past the frame: rows behind x_norm, NaN here)
            w = x[rows, s].T @ dt if 0 <= s < S else np.full((2 * kin, TILE), np.nan)
            q = rt * ntn + ct
            partial[q, :, :, 0] = w[0::2, 0::2] - w[1::2, 1::2]
            partial[q, :, :, 1] = w[0::2, 1::2] - w[1::2, 0::2]
            colsum[q] = dt.sum(0)
    return partial, colsum


def fold(partial, colsum, batch, S, kin, F, tiles_per_symbol=None, symbol_of=None, terms=None):
    """(dWa | dWb [kin, 2F], dbias [2F]).  tiles_per_symbol: the distance between consecutive terms, in tiles (default
    2F / 64); terms: how many are summed (default ceil(batch / 64) * S); symbol_of(n0): a fold that looks the first tile of
    symbol s up by a symbol index of its own -- the first column tile with symbol_of(64 ct) == s -- instead of s * tiles."""
    nrt, ntn, tps_true = geometry(batch, S, F)
    tps = tps_true if tiles_per_symbol is None else tiles_per_symbol
    nz = nrt * S if terms is None else terms
    pad_p = np.full((1,) + partial.shape[1:], np.nan)
    pad_c = np.full((1, TILE), np.nan)
    P, Cs = np.concatenate([partial, pad_p]), np.concatenate([colsum, pad_c])
    last = partial.shape[0]
    first = None
    if symbol_of is not None:
        first = {}
        for ct in range(ntn):
            first.setdefault(symbol_of(ct * TILE), ct)
    dw = np.zeros((kin, 2 * F))
    db = np.zeros(2 * F)
    for f in range(F):
        h, j = (2 * f) // TILE, ((2 * f) % TILE) // 2
        for z in range(nz):
            if first is None:
                q = z * tps + h
            else:
                q = (z // S) * ntn + first.get(z % S, last) + h
            q = q if 0 <= q < last else last
            dw[:, f] += P[q, :, j, 0]
            dw[:, F + f] += P[q, :, j, 1]
            db[f] += Cs[q, 2 * j] - Cs[q, 2 * j + 1]
    db[F:] = -db[:F]
    return dw, db


def moved(planted, true):
    """max-norm relative change; a NaN (a read past the last tile) counts as infinitely far"""
    diff = np.abs(np.asarray(planted) - np.asarray(true))
    return float("inf") if np.isnan(diff).any() else float(diff.max() / np.abs(true).max())
