"""CPU check of tests/rx_backward_ref.py, the float64 model of what the fused backward launch (csrc/rx_bwd.h) leaves for the
C-Conv weight gradient and of how cconv_fold_body reads it -- and of the shape table of tests/test_gpu_rx_backward_shapes.py:

  (a) with the true geometry the model IS the C-Conv weight gradient (O.cconv_gemm_bwd, 1e-12) at every shape of the table and
      at the flagship batch;
  (b) each index error a rewrite of the launch can make moves the gradient by at least 100 RTOL at the table shapes named here
      (the margin of assert_guard in test_optimizer_oracle.py), so the GPU test at those shapes would fail on it;
  (c) the first three of them change not one bit at the four shapes of test_gpu_ops.py::test_rx_backward_fused (S = 7,
      F = 64): why the suite could not see them before.
"""
import numpy as np
import pytest

import rx_backward_ref as R
from oracle import dccn_oracle as O
from test_gpu_ops import RTOL

MARGIN = 100 * RTOL
FLAGSHIP = (1170, 7, 80, 64, 320)

_cache = {}


def case(shape):
    """inputs, the model's tiles and the oracle's gradient, once per shape and left unchanged"""
    if shape not in _cache:
        batch, S, kin, F, D = shape
        rng = np.random.RandomState(batch + S + kin + F)
        xn = rng.randn(batch, S, kin, 2)
        dfft = rng.randn(batch, S * 2 * F)
        _, gw, gb = O.cconv_gemm_bwd(xn.reshape(batch * S, kin, 2), np.zeros((kin, 2 * F)), dfft.reshape(batch * S, F, 2))
        partial, colsum = R.tile_partials(xn, dfft, batch, S, kin, F)
        _cache[shape] = dict(xn=xn, dfft=dfft, gw=gw, gb=gb, partial=partial, colsum=colsum)
    return _cache[shape]


def dims(shape):
    batch, S, kin, F, _ = shape
    return batch, S, kin, F


def two_tiles_per_symbol(c, shape):
    return R.fold(c["partial"], c["colsum"], *dims(shape), tiles_per_symbol=2)


def symbol_128_in_the_tile(c, shape):
    return R.fold(*R.tile_partials(c["xn"], c["dfft"], *dims(shape), symbol_of=lambda n0: n0 // 128), *dims(shape))


def symbol_128_in_the_fold(c, shape):
    return R.fold(c["partial"], c["colsum"], *dims(shape), symbol_of=lambda n0: n0 // 128)


def seven_symbols(c, shape):
    return R.fold(c["partial"], c["colsum"], *dims(shape), terms=-(-shape[0] // 64) * 7)


def rows_past_the_batch_kept(c, shape):
    return R.fold(*R.tile_partials(c["xn"], c["dfft"], *dims(shape), zero_past_batch=False), *dims(shape))


# planted error -> (model run with it, the table shapes that must see it with a FINITE change of the gradient: a NaN -- a read
# past the last tile -- would be seen too, but a wrong finite value is the harder case)
PLANTED = {
    "tiles_per_symbol fixed at 2": (two_tiles_per_symbol, [(63, 3, 80, 96, 34), (129, 2, 64, 128, 320), (70, 1, 64, 160, 10),
                                                            (800, 7, 64, 128, 50)]),
    "symbol = n0 // 128, x rows of the tile": (symbol_128_in_the_tile, [(65, 7, 64, 32, 50), (500, 7, 64, 32, 50),
                                                                        (800, 7, 80, 32, 50)]),
    "symbol = n0 // 128, tiles of a term": (symbol_128_in_the_fold, [(63, 3, 80, 96, 34)]),
    "terms = ceil(batch / 64) * 7": (seven_symbols, [(200, 14, 80, 64, 50)]),
    "rows past the batch not zeroed": (rows_past_the_batch_kept, [(1, 1, 80, 32, 2), (65, 7, 64, 32, 50), (63, 3, 80, 96, 34),
                                                                  (129, 2, 64, 128, 320), (70, 1, 64, 160, 10)]),
}
BLIND_AT_F64_S7 = ["tiles_per_symbol fixed at 2", "symbol = n0 // 128, x rows of the tile", "symbol = n0 // 128, tiles of a term",
                   "terms = ceil(batch / 64) * 7"]


@pytest.mark.parametrize("shape", sorted(R.SHAPES) + [FLAGSHIP], ids=lambda s: "-".join(map(str, s)))
def test_model_is_the_cconv_weight_gradient(shape):
    c = case(shape)
    batch, S, kin, F = dims(shape)
    nrt, ntn, tps = R.geometry(batch, S, F)
    if shape in R.SHAPES:
        assert (nrt * ntn, tps) == R.SHAPES[shape][:2]
    assert c["partial"].shape == (nrt * ntn, kin, 32, 2) and c["colsum"].shape == (nrt * ntn, 64)
    dw, db = R.fold(c["partial"], c["colsum"], batch, S, kin, F)
    assert R.moved(dw, c["gw"]) <= 1e-12 and R.moved(db, c["gb"]) <= 1e-12, (R.moved(dw, c["gw"]), R.moved(db, c["gb"]))


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_planted_error_is_seen_at_its_shapes(name):
    run, witnesses = PLANTED[name]
    assert witnesses and all(s in R.SHAPES for s in witnesses)
    for shape in witnesses:
        c = case(shape)
        far = R.moved(run(c, shape)[0], c["gw"])
        assert np.isfinite(far) and far >= MARGIN, (name, shape, far)


@pytest.mark.parametrize("name", BLIND_AT_F64_S7)
def test_the_old_shapes_could_not_see_it(name):
    run, _ = PLANTED[name]
    for shape in R.OLD_SHAPES:
        c = case(shape)
        true = R.fold(c["partial"], c["colsum"], *dims(shape))
        got = run(c, shape)
        assert np.array_equal(got[0], true[0]) and np.array_equal(got[1], true[1]), (name, shape)


def test_the_old_shapes_do_see_unzeroed_rows():
    """(three of them have a ragged last row tile: that error was covered before, and stays covered)"""
    run, _ = PLANTED["rows past the batch not zeroed"]
    ragged = [s for s in R.OLD_SHAPES if s[0] % 64]
    assert len(ragged) == 3
    for shape in ragged:
        c = case(shape)
        assert R.moved(run(c, shape)[0], c["gw"]) >= MARGIN, shape
