"""The six stand-alone GEMM operators of the C ABI with each input operand moved one float off a 16-byte boundary
(``-m gpu``).

The launch planning describes every GEMM role once (csrc/dccn_abi.hip: dense_fwd_params ... cconv_bwd_w_params); the
description computes, from pointer alignment, divisibility and size, whether the fast loaders may read an operand as
vectors.  A misaligned operand must take the operator off every tile family that has no scalar loaders -- the few-row,
skinny and 48x64 tiles, the staged whole-k C-Conv forward, the k-major weight gradient -- and the result must still be
right.  Shapes: dense (65, 132, 68) has several ragged tiles and only multiples of 4, so the pointer alone decides;
dense (73, 896, 896) takes the few-row / skinny tiles when aligned; C-Conv (129, 34, 18) is ragged everywhere;
C-Conv (511, 80, 64) takes the staged forward and the k-major weight gradient when aligned.

Every result is held to the float64 oracle with the helper and tolerance of test_gpu_ops.py; the aligned and the
misaligned call on equal values agree within the same tolerance (not bitwise: the k order differs between tile
families).  Outputs lie between NaN-filled guard bands of 64 floats that must stay untouched.
"""
import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from test_gpu_ops import RTOL, assert_close

pytestmark = pytest.mark.gpu

GUARD = 64
DENSE = [(65, 132, 68), (73, 896, 896)]
CCONV = [(129, 34, 18), (511, 80, 64)]


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def operand(a, shift):
    """Device copy of `a` whose first element lies `shift` floats behind a 16-byte boundary: a view into a larger allocation."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * shift
    return v


class Guarded:
    """An output of n floats, 16-byte aligned, between two NaN-filled bands of GUARD floats."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def get(self, what):
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + self.n:]).all(), "%s: guard band written" % what
        return h[GUARD:GUARD + self.n]


def workspace(nbytes):
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def sweep(run, inputs, refs, what):
    """run(ptrs) -> list of output arrays.  Once with every input aligned, then with each input in turn misaligned; every
    result against the float64 references, and the misaligned against the aligned."""
    base = None
    for moved in [None] + list(range(len(inputs))):
        ops = [operand(a, 1 if i == moved else 0) for i, a in enumerate(inputs)]
        outs = run([o.data_ptr() for o in ops])
        torch.cuda.synchronize()
        tag = "%s, %s" % (what, "aligned" if moved is None else "input %d off by one float" % moved)
        for k, (got, ref) in enumerate(zip(outs, refs)):
            assert_close(got.reshape(ref.shape), ref, "%s, output %d vs oracle" % (tag, k))
        if base is None:
            base = outs
        else:
            for k, (got, ref) in enumerate(zip(outs, base)):
                assert_close(got, ref, "%s, output %d vs aligned" % (tag, k), tol=RTOL)


@pytest.fixture(scope="module")
def dense_case():
    cache = {}

    def make(M, K, N):
        if (M, K, N) not in cache:
            rng = np.random.RandomState(M + K + N)
            x = rng.randn(M, K).astype(np.float32)
            w = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
            b = rng.randn(N).astype(np.float32)
            dy = rng.randn(M, N).astype(np.float32)
            x6, w6, b6, d6 = (a.astype(np.float64) for a in (x, w, b, dy))
            cache[(M, K, N)] = dict(x=x, w=w, b=b, dy=dy, y=x6 @ w6 + b6, dx=d6 @ w6.T, dw=x6.T @ d6, db=d6.sum(0))
        return cache[(M, K, N)]
    return make


@pytest.fixture(scope="module")
def cconv_case():
    cache = {}

    def make(rows, kin, F):
        if (rows, kin, F) not in cache:
            rng = np.random.RandomState(rows + kin + F)
            x = rng.randn(rows, kin, 2).astype(np.float32)
            w = (rng.randn(kin, 2 * F) / np.sqrt(kin)).astype(np.float32)
            b = rng.randn(2 * F).astype(np.float32)
            dout = rng.randn(rows, F, 2).astype(np.float32)
            x6, w6, b6, d6 = (a.astype(np.float64) for a in (x, w, b, dout))
            dx, dw, db = O.cconv_gemm_bwd(x6, w6, d6)
            cache[(rows, kin, F)] = dict(x=x, w=w, b=b, dout=dout, out=O.cconv_gemm_fwd(x6, w6, b6), dx=dx, dw=dw, db=db)
        return cache[(rows, kin, F)]
    return make


@pytest.mark.parametrize("M,K,N", DENSE)
def test_dense_fwd(lib, dense_case, M, K, N):
    from dl_ofdm_amd import _lib
    c = dense_case(M, K, N)

    def run(p):
        y = Guarded(M * N)
        _lib.check(lib.dccn_dense_fwd(p[0], p[1], p[2], y.ptr, M, K, N, None), "dccn_dense_fwd")
        return [y.get("y")]
    sweep(run, [c["x"], c["w"], c["b"]], [c["y"]], "dense fwd %s" % ((M, K, N),))


@pytest.mark.parametrize("M,K,N", DENSE)
def test_dense_bwd_x(lib, dense_case, M, K, N):
    from dl_ofdm_amd import _lib
    c = dense_case(M, K, N)

    def run(p):
        dx = Guarded(M * K)
        _lib.check(lib.dccn_dense_bwd_x(p[0], p[1], dx.ptr, M, K, N, None), "dccn_dense_bwd_x")
        return [dx.get("dx")]
    sweep(run, [c["dy"], c["w"]], [c["dx"]], "dense dX %s" % ((M, K, N),))


@pytest.mark.parametrize("M,K,N", DENSE)
def test_dense_bwd_w(lib, dense_case, M, K, N):
    from dl_ofdm_amd import _lib
    c = dense_case(M, K, N)
    nws = lib.dccn_dense_bwd_w_workspace_size(M, K, N)
    ws = workspace(nws)

    def run(p):
        dw, db = Guarded(K * N), Guarded(N)
        _lib.check(lib.dccn_dense_bwd_w(p[0], p[1], dw.ptr, db.ptr, M, K, N, ws.data_ptr(), nws, None), "dccn_dense_bwd_w")
        return [dw.get("dw"), db.get("dbias")]
    sweep(run, [c["x"], c["dy"]], [c["dw"], c["db"]], "dense dW %s" % ((M, K, N),))


@pytest.mark.parametrize("rows,kin,F", CCONV)
def test_cconv_gemm_fwd(lib, cconv_case, rows, kin, F):
    from dl_ofdm_amd import _lib
    c = cconv_case(rows, kin, F)

    def run(p):
        out = Guarded(rows * 2 * F)
        _lib.check(lib.dccn_cconv_gemm_fwd(p[0], p[1], p[2], out.ptr, rows, kin, F, None), "dccn_cconv_gemm_fwd")
        return [out.get("out")]
    sweep(run, [c["x"], c["w"], c["b"]], [c["out"]], "C-Conv fwd %s" % ((rows, kin, F),))


@pytest.mark.parametrize("rows,kin,F", CCONV)
def test_cconv_gemm_bwd_x(lib, cconv_case, rows, kin, F):
    from dl_ofdm_amd import _lib
    c = cconv_case(rows, kin, F)

    def run(p):
        dx = Guarded(rows * 2 * kin)
        _lib.check(lib.dccn_cconv_gemm_bwd_x(p[0], p[1], dx.ptr, rows, kin, F, None), "dccn_cconv_gemm_bwd_x")
        return [dx.get("dx")]
    sweep(run, [c["dout"], c["w"]], [c["dx"]], "C-Conv dX %s" % ((rows, kin, F),))


@pytest.mark.parametrize("rows,kin,F", CCONV)
def test_cconv_gemm_bwd_w(lib, cconv_case, rows, kin, F):
    from dl_ofdm_amd import _lib
    c = cconv_case(rows, kin, F)
    nws = lib.dccn_cconv_gemm_bwd_w_workspace_size(rows, kin, F)
    ws = workspace(nws)

    def run(p):
        dw, db = Guarded(kin * 2 * F), Guarded(2 * F)
        _lib.check(lib.dccn_cconv_gemm_bwd_w(p[0], p[1], dw.ptr, db.ptr, rows, kin, F, ws.data_ptr(), nws, None),
                   "dccn_cconv_gemm_bwd_w")
        return [dw.get("dw"), db.get("dbias")]
    sweep(run, [c["x"], c["dout"]], [c["dw"], c["db"]], "C-Conv dWeff %s" % ((rows, kin, F),))
