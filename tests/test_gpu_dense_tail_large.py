"""The fused dense + tail launch on the grids of LARGE layers, at operator level against the float64 oracle (``-m gpu``).

dense_tail_route (csrc/dccn_abi.hip) puts dccn_dense_tail_fwd[_bwd] on 80x64 tiles once ceil(M / 48) * ceil(N / 64) reaches
4 x 256 tiles, and -- BPSK / QPSK, 1 <= M % 80 <= 32 -- on the ragged grid: 80x64 tiles plus one row of 32x64 blocks.  The
shapes below are the smallest at which each of those routes exists (about 1.5 M cells whatever the shape; K is small, so
the GEMM costs nothing).  Every case first asks dccn_dense_tail_grid which grid it is about to run and asserts the answer:
if the threshold moved, a case would fail instead of quietly becoming one more 48x64 test.

Inputs: the construction of test_gpu_ops.py::test_dense_tail_fused.  Rows of x are re-drawn until NO cell has a
pre-activation within 2e-4 of a leaky-ReLU kink or a probability pair within 2e-5 of a tie, so no cell is excluded from any
comparison.  Each round evaluates the oracle on the re-drawn rows alone (the conditions are per cell); the oracle of record
is one evaluation over the final inputs.  Tolerances are those of test_gpu_ops.py: 1e-5 (z, prob, ce_mean), 2e-5 (dz, tail
gradients), 5e-6 (fused against dense-then-tail prob); confusion counts exact.  The same helper runs on two 48x64 shapes of
test_dense_tail_fused's parametrisation (the control): what it asks is the suite's own bound, not one fitted to the large
grids.  z, prob and dz lie between NaN-filled guard bands of 64 floats.

A case is built once (module-level cache) and never modified; tests/test_gpu_receive.py holds the decision launch to the
same operands.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from test_gpu_gemm_operands import Guarded
from test_gpu_ops import RTOL, _tail_params, relerr

pytestmark = pytest.mark.gpu

TILES, RAGGED = 0, 2               # dccn_dense_tail_grid's grid (1 = few-row tiles: at most 96 rows, not met here)
TUNE_DENSE_RAGGED = 27
# (M, K, N, nbits) -> what dccn_dense_tail_grid must say: (grid, tile rows, ragged rows, blocks)
LARGE = {
    (4960, 192, 640, 1): (TILES, 80, 0, 620),        # uniform 80x64, interior tiles only, 3 k-tiles
    (4960, 192, 640, 2): (TILES, 80, 0, 620),
    (4960, 192, 640, 3): (TILES, 80, 0, 620),        # ... the LDS-staged tail over an 80-row tile
    (4960, 192, 640, 4): (TILES, 80, 0, 620),
    (4961, 192, 640, 2): (RAGGED, 80, 1, 630),       # one row in the 32x64 blocks
    (4992, 192, 640, 1): (RAGGED, 80, 32, 630),      # a full 32-row block
    (4993, 192, 640, 2): (TILES, 80, 0, 630),        # 33 rows left: uniform 80x64 with a masked last tile row
    (4976, 896, 580, 2): (RAGGED, 80, 16, 630),      # the workload's K, a last column tile of 4 columns
    (4976, 192, 640, 4): (TILES, 80, 0, 630),        # nbits >= 3 never runs ragged: masked 16-row last tile, LDS-staged
}
CONTROL = {
    (53, 192, 100, 2): (TILES, 48, 0, 4),
    (300, 896, 640, 4): (TILES, 48, 0, 70),
}
# the cases tests/test_gpu_receive.py runs the decision launch on (kept in the cache when this module is done)
DECIDE = [(4960, 192, 640, 1), (4960, 192, 640, 2), (4961, 192, 640, 2), (4992, 192, 640, 1), (4960, 192, 640, 4)]

_cases = {}


def grid_of(lib, M, K, N, nbits):
    g = [C.c_int(-1) for _ in range(4)]
    assert lib.dccn_dense_tail_grid(M, K, N, nbits, *[C.byref(v) for v in g]) == 0
    return tuple(v.value for v in g)


def _ill_conditioned(r, cells):
    pr = r["prob"].reshape(cells, -1, 2)
    return (np.abs(r["pre1"]).min(1) < 2e-4) | (np.abs(r["pre2"]).min(1) < 2e-4) | \
           (np.abs(pr[..., 1] - pr[..., 0]).min(1) < 2e-5)


def host_case(M, K, N, nbits):
    """Inputs and float64 references of one case, on the host."""
    rng = np.random.RandomState(100 * nbits + M)
    D = N // 2
    tp = {k: v.astype(np.float32).astype(np.float64) for k, v in _tail_params(nbits, rng).items()}
    flat = np.concatenate([tp[k].reshape(-1) for k in ("w1", "b1", "w2", "b2")]).astype(np.float32)
    w = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    b = (rng.randn(N) * 0.5).astype(np.float32)
    x = (rng.randn(M, K) * 2.0).astype(np.float32)
    bits = rng.randint(0, 2, (M, D, nbits)).astype(np.int32)
    w6, b6 = w.astype(np.float64), b.astype(np.float64)

    def oracle(rows):
        z6 = x[rows].astype(np.float64) @ w6 + b6
        return z6, O.tail_forward_backward(z6.reshape(-1, 2), bits[rows].reshape(-1, nbits), tp["w1"], tp["b1"], tp["w2"],
                                           tp["b2"], nbits)

    rows = np.arange(M)
    for _ in range(60):
        _, r = oracle(rows)
        rows = rows[np.unique(np.nonzero(_ill_conditioned(r, rows.size * D))[0] // D)]
        if rows.size == 0:
            break
        x[rows] = (rng.randn(rows.size, K) * 2.0).astype(np.float32)
    else:
        raise AssertionError("could not build a well-conditioned case")
    z6, r = oracle(np.arange(M))
    assert not _ill_conditioned(r, M * D).any()                 # the share of cells left out of a comparison is 0
    conf = np.asarray(r["conf"]).reshape(-1)
    assert (conf > 0).all() and int(conf.sum()) == M * D * nbits, conf
    pr = r["prob"].reshape(M, D, nbits, 2)
    gref = np.concatenate([r["grads"][k].reshape(-1) for k in ("w1", "b1", "w2", "b2")])
    return dict(M=M, K=K, N=N, nbits=nbits, x=x, w=w, b=b, flat=flat, bits=bits, z=z6, prob=pr, hard=pr[..., 1] > pr[..., 0],
                dz=r["dz"].reshape(M, N), dtailp=gref, ce_mean=float(r["ce_mean"]), conf=conf)


def large_case(M, K, N, nbits):
    """host_case plus device copies of the operands; built once per process."""
    key = (M, K, N, nbits)
    if key not in _cases:
        c = host_case(M, K, N, nbits)
        for k in ("x", "w", "b", "flat"):
            c["d_" + k] = torch.as_tensor(c[k]).cuda()
        c["d_bits"] = torch.as_tensor(c["bits"]).cuda()
        _cases[key] = c
    return _cases[key]


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    cu, wf, hbm, arch = _lib.device_info()
    assert wf == 64 and arch.startswith("gfx950"), (cu, wf, arch)
    yield _lib.load()
    for key in [k for k in _cases if k not in DECIDE]:
        del _cases[key]


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.ptr if isinstance(t, Guarded) else t.data_ptr())


def run_tail(lib, c, bwd=True, want_z=True, want_prob=True):
    """One call of dccn_dense_tail_fwd_bwd (bwd) / dccn_dense_tail_fwd on the case's operands.  Returns host arrays
    (None for an output that was not asked for); the guard bands of z, prob and dz are checked on the way out."""
    from dl_ofdm_amd import _lib, ops
    M, K, N, nbits = c["M"], c["K"], c["N"], c["nbits"]
    D = N // 2
    nws = lib.dccn_dense_tail_workspace_size(M, N, nbits)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    z = Guarded(M * N) if want_z else None
    prob = Guarded(M * D * nbits * 2) if want_prob else None
    dz = Guarded(M * N) if bwd else None
    dt = torch.full((c["flat"].size,), float("nan"), device="cuda") if bwd else None
    mbuf = torch.zeros(_lib.METRICS_BYTES, dtype=torch.uint8, device="cuda")
    head = [_ptr(c["d_x"]), _ptr(c["d_w"]), _ptr(c["d_b"]), _ptr(z), _ptr(c["d_bits"]), _ptr(c["d_flat"]), _ptr(prob), _ptr(mbuf)]
    tail = [M, K, N, nbits, _ptr(ws), nws, ops._stream()]
    if bwd:
        _lib.check(lib.dccn_dense_tail_fwd_bwd(*(head + [_ptr(dz), _ptr(dt)] + tail)), "dccn_dense_tail_fwd_bwd")
    else:
        _lib.check(lib.dccn_dense_tail_fwd(*(head + tail)), "dccn_dense_tail_fwd")
    torch.cuda.synchronize()
    return dict(z=z.get("z").reshape(M, N) if want_z else None,
                prob=prob.get("prob").reshape(M, D, nbits, 2) if want_prob else None,
                dz=dz.get("dz").reshape(M, N) if bwd else None, dtailp=dt.cpu().numpy() if bwd else None,
                m=ops.read_metrics(mbuf))


def two_launch_prob(lib, c):
    """dccn_dense_fwd, then dccn_demod_tail_loss_fwd on its z."""
    from dl_ofdm_amd import _lib, ops
    M, K, N, nbits = c["M"], c["K"], c["N"], c["nbits"]
    cells = M * (N // 2)
    z = torch.empty(M, N, device="cuda")
    prob = torch.empty(cells * nbits * 2, device="cuda")
    mbuf = torch.zeros(_lib.METRICS_BYTES, dtype=torch.uint8, device="cuda")
    nws = lib.dccn_demod_tail_workspace_size(cells, nbits)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dccn_dense_fwd(_ptr(c["d_x"]), _ptr(c["d_w"]), _ptr(c["d_b"]), _ptr(z), M, K, N, ops._stream()), "dccn_dense_fwd")
    _lib.check(lib.dccn_demod_tail_loss_fwd(_ptr(z), _ptr(c["d_bits"]), _ptr(c["d_flat"]), _ptr(prob), _ptr(mbuf), cells, nbits,
                                            _ptr(ws), nws, ops._stream()), "dccn_demod_tail_loss_fwd")
    torch.cuda.synchronize()
    return prob.cpu().numpy()


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (what, a.shape, b.shape)
    n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert n == 0, "%s: %d of %d values differ in their bits" % (what, n, a.size)


def check_against_oracle(c, got, what):
    """The outputs of one dccn_dense_tail_fwd_bwd call against the float64 references of the case; every cell takes part."""
    M, N, nbits = c["M"], c["N"], c["nbits"]
    m = got["m"]
    conf = np.asarray(m["conf"]).reshape(-1)
    e = dict(z=relerr(got["z"], c["z"]), prob=relerr(got["prob"], c["prob"]), dz=relerr(got["dz"], c["dz"]),
             dtailp=relerr(got["dtailp"], c["dtailp"]), ce=abs(m["ce_mean"] - c["ce_mean"]) / abs(c["ce_mean"]))
    print("%s: z %.2e  prob %.2e  ce_mean %.2e  dz %.2e  dtailp %.2e | conf %s" % (what, e["z"], e["prob"], e["ce"], e["dz"],
                                                                               e["dtailp"], conf.tolist()))
    assert e["z"] <= RTOL and e["prob"] <= RTOL and e["ce"] <= RTOL, (what, e)
    assert np.array_equal(conf, c["conf"]) and m["count"] == M * (N // 2) * nbits, (what, conf, c["conf"], m["count"])
    assert np.array_equal(got["prob"][..., 1] > got["prob"][..., 0], c["hard"]), what
    assert e["dz"] <= 2e-5 and e["dtailp"] <= 2e-5, (what, e)


def check_case(lib, c, what):
    """Everything this module asks of one shape."""
    full = run_tail(lib, c)
    check_against_oracle(c, full, what)
    # the BWD = false instantiation: prob, z and the confusion counts bit for bit
    fwd = run_tail(lib, c, bwd=False)
    assert_same_bits(fwd["z"], full["z"], what + ": z of the evaluation instantiation")
    assert_same_bits(fwd["prob"], full["prob"], what + ": prob of the evaluation instantiation")
    assert fwd["m"]["conf"] == full["m"]["conf"] and fwd["m"]["count"] == full["m"]["count"], what
    # z = NULL, prob = NULL: dz, the tail gradients and the metrics bit for bit (on the ragged grid the second shape's
    # offsets of the two are then NULL as well)
    lean = run_tail(lib, c, want_z=False, want_prob=False)
    assert_same_bits(lean["dz"], full["dz"], what + ": dz without z and prob")
    assert_same_bits(lean["dtailp"], full["dtailp"], what + ": tail gradients without z and prob")
    assert lean["m"] == full["m"], (what, lean["m"], full["m"])
    # dense forward, then the stand-alone tail: to rounding
    e = relerr(two_launch_prob(lib, c), full["prob"].reshape(-1))
    print("%s: fused against dense-then-tail prob %.2e" % (what, e))
    assert e <= 5e-6, (what, e)
    return full


@pytest.mark.parametrize("M,K,N,nbits", sorted(LARGE))
def test_large_grids_against_the_oracle(lib, M, K, N, nbits):
    assert grid_of(lib, M, K, N, nbits) == LARGE[(M, K, N, nbits)]
    check_case(lib, large_case(M, K, N, nbits), "%s nbits %d" % ((M, K, N), nbits))


@pytest.mark.parametrize("M,K,N,nbits", sorted(CONTROL))
def test_control_the_same_helper_on_48x64_tiles(lib, M, K, N, nbits):
    assert grid_of(lib, M, K, N, nbits) == CONTROL[(M, K, N, nbits)]
    check_case(lib, large_case(M, K, N, nbits), "control %s nbits %d" % ((M, K, N), nbits))


def test_ragged_grid_switched_off_runs_uniform_tiles_with_the_same_bits(lib):
    """Knob 27 = 0 puts (4976, 896, 580, 2) on uniform 80x64 tiles (63 x 10 blocks, the last tile row masked).  Same oracle
    bounds; and z and prob are the ragged grid's bit for bit: a row's k order does not depend on the height of its tile."""
    M, K, N, nbits = key = (4976, 896, 580, 2)
    c = large_case(*key)
    assert grid_of(lib, *key) == LARGE[key]
    ragged = run_tail(lib, c)
    default = lib.dccn_get_tuning(TUNE_DENSE_RAGGED)
    try:
        assert lib.dccn_set_tuning(TUNE_DENSE_RAGGED, 0) == 0
        assert grid_of(lib, *key) == (TILES, 80, 0, 630)
        uniform = check_case(lib, c, "%s nbits %d, knob 27 = 0" % ((M, K, N), nbits))
    finally:
        lib.dccn_set_tuning(TUNE_DENSE_RAGGED, default)
    print("uniform against ragged: z max|diff| %.2e  prob max|diff| %.2e" % (float(np.abs(uniform["z"] - ragged["z"]).max()),
                                                                          float(np.abs(uniform["prob"] - ragged["prob"]).max())))
    assert_same_bits(uniform["z"], ragged["z"], "z, uniform against ragged grid")
    assert_same_bits(uniform["prob"], ragged["prob"], "prob, uniform against ragged grid")
