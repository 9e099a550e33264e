"""dccn_dense_fwd_ld: the dense forward on a column window of wider rows (``-m gpu``).

The classical receivers' FFT window and the equaliser's windowed first layer call it with a row stride ldx > K and a start
pointer inside the row: 2 (CP - advance) floats in, 16-byte aligned only when CP - advance is even, so one call site
moves between the vector tile families and the scalar-loader GEMM with the channel profile.  Here x lives in a
[M, ldx] array whose columns outside the window are NaN (a loader that strays over the window's edge poisons the
result), `off` floats behind a 16-byte boundary; y lies between NaN guard bands.  Every case is held to float64
x . w (+ bias) with the tolerance of test_gpu_ops.py, with and without bias, and to dccn_dense_fwd on a packed copy of
the same rows.
  (35, 128, 128, 160, 0 / 4 / 2)    the classical window at few rows: aligned, aligned further in, misaligned
  (1393, 128, 128, 160, 0 / 2)      the 48x64 tiles against the scalar loaders
  (37, 260, 256, 264, 0)            skinny, with a k tail
  (37, 896, 640, 900, 0)            few rows at depth 14
  (65, 132, 68, 133, 1)             nothing vector-legal: odd stride, odd offset
"""
import numpy as np
import pytest
import torch

from test_gpu_gemm_operands import Guarded, operand
from test_gpu_ops import RTOL, assert_close, relerr

pytestmark = pytest.mark.gpu

INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)
CASES = [(35, 128, 128, 160, 0), (35, 128, 128, 160, 4), (35, 128, 128, 160, 2), (1393, 128, 128, 160, 0),
         (1393, 128, 128, 160, 2), (37, 260, 256, 264, 0), (37, 896, 640, 900, 0), (65, 132, 68, 133, 1)]


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def window(x, ldx, off):
    """(buffer, pointer): the rows of x [M, K] as a column window of a NaN-filled [M, ldx] array that starts `off` floats
    behind a 16-byte boundary"""
    M, K = x.shape
    assert off + K <= ldx
    buf = torch.full((M * ldx + 8,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and off + (M - 1) * ldx + K <= buf.numel()
    buf[off:off + M * ldx].view(M, ldx)[:, :K] = torch.from_numpy(x).cuda()
    assert int(torch.isnan(buf).sum()) == buf.numel() - M * K
    return buf, buf.data_ptr() + 4 * off


@pytest.mark.parametrize("M,K,N,ldx,off", CASES)
def test_dense_fwd_ld(lib, M, K, N, ldx, off):
    from dl_ofdm_amd import _lib
    rng = np.random.RandomState(M + K + N + ldx + off)
    x = rng.randn(M, K).astype(np.float32)
    w = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    b = rng.randn(N).astype(np.float32)
    ref0 = x.astype(np.float64) @ w.astype(np.float64)
    buf, xptr = window(x, ldx, off)
    assert xptr % 16 == (4 * off) % 16
    dw, db, packed = operand(w, 0), operand(b, 0), operand(x, 0)
    for bias, ref in ((None, ref0), (db, ref0 + b.astype(np.float64))):
        bptr = None if bias is None else bias.data_ptr()
        y, yp = Guarded(M * N), Guarded(M * N)
        _lib.check(lib.dccn_dense_fwd_ld(xptr, ldx, dw.data_ptr(), bptr, y.ptr, M, K, N, None), "dccn_dense_fwd_ld")
        _lib.check(lib.dccn_dense_fwd(packed.data_ptr(), dw.data_ptr(), bptr, yp.ptr, M, K, N, None), "dccn_dense_fwd")
        torch.cuda.synchronize()
        tag = "dense_fwd_ld %s%s" % ((M, K, N, ldx, off), "" if bias is None else " + bias")
        got, gotp = y.get("y").reshape(M, N), yp.get("y packed").reshape(M, N)
        print("measured %-52s rel err vs fp64 %.3e, vs packed dccn_dense_fwd %.3e" % (tag, relerr(got, ref), relerr(got, gotp)))
        assert_close(got, ref, tag + " vs oracle", tol=RTOL)
        assert_close(got, gotp, tag + " vs dccn_dense_fwd on packed rows", tol=RTOL)


def test_dense_fwd_ld_refuses_a_stride_shorter_than_the_row(lib):
    M, K, N = 35, 128, 128
    x = operand(np.ones((M, K)), 0)
    w = operand(np.ones((K, N)), 0)
    y = Guarded(M * N)
    for ldx in (K - 1, 1, 0, -K):
        assert lib.dccn_dense_fwd_ld(x.data_ptr(), ldx, w.data_ptr(), None, y.ptr, M, K, N, None) == INVALID_ARG, ldx
    torch.cuda.synchronize()
    assert np.isnan(y.get("refused y")).all()
