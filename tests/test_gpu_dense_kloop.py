"""The k-loop of the fused dense + tail launch, one case per path it can take (``-m gpu``).

gemm16_block (csrc/gemm16.h) runs the dense forward's k range on one of several schedules: k-tiles of 64, global loads two
k-tiles ahead when the whole range is full tiles (the "deep" path: a first k-tile with late LDS stores, a loop of two
k-tiles with the stores early and the barrier inside the k-tile, and one to three remainder tiles), loads one k-tile ahead
otherwise, and a masked loader for a ragged last k-tile.  A schedule that lets a wave read an LDS buffer before every
store to it has landed, or overwrite one that is still being read, gives wrong sums in some rows of some tiles only, so
every case is compared element by element.

Small layer, M = 146 rows (3 x 48 + 2: interior and ragged 48x64 tiles, above the 96 rows of the few-row plan), N = 128:
  K = 128, 192, 256, 320, 384   deep path, 2 ... 6 k-tiles: every remainder length, zero / one pass of the paired loop
  K = 64                        one k-tile: the schedule with loads one k-tile ahead
  K = 196                       three full k-tiles and a ragged one: the masked loader
Large layer, K = 128, N = 4096: M = 768 (uniform 80x64 tiles) and M = 745 (80x64 tiles plus the 25-row ragged row).
Each for BPSK and QPSK (the large ones: QPSK), training (dccn_dense_tail_fwd_bwd) and evaluation (dccn_dense_tail_fwd).

Two comparisons.  Against the float64 oracle at the project's bar of 1e-5 (relative to the largest magnitude) for z, prob,
ce_mean, dz and the tail-parameter gradients; confusion counts exact.  Inputs are built as in
tests/test_gpu_dense_tail_large.py (rows re-drawn until no cell sits at a leaky-ReLU kink or a tie; the 2048-cell rows of
the large layer with narrower margins, see _wide_case).  And against the
stand-alone tail run on the fused launch's own z: dz and prob bit for bit, confusion counts equal, ce_mean and the
gradients (another block order of the same terms) within 3e-5 as in tests/test_gpu_dense_tail_fastpath.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_dense_tail_large import RAGGED, TILES, assert_same_bits, grid_of, host_case, run_tail
from oracle import dccn_oracle as O
from test_gpu_ops import RTOL, _tail_params, relerr

pytestmark = pytest.mark.gpu

SMALL = [(146, k, 128) for k in (64, 128, 192, 196, 256, 320, 384)]
# (M, K, N) -> what dccn_dense_tail_grid must say for QPSK: (grid, tile rows, ragged rows, blocks)
LARGE = {
    (768, 128, 4096): (TILES, 80, 0, 640),
    (745, 128, 4096): (RAGGED, 80, 25, 640),
}
CASES = [(m, k, n, nb) for (m, k, n) in SMALL for nb in (1, 2)] + [(m, k, n, 2) for (m, k, n) in sorted(LARGE)]

_cases = {}


def _wide_case(M, K, N, nbits, kink=2e-5, tie=2e-6):
    """host_case of tests/test_gpu_dense_tail_large.py for rows of 2048 cells.  That construction re-draws a whole row of x
    while one of its cells is within 2e-4 of a kink; about one cell in a thousand is, so a row of 2048 cells practically
    always holds one and the re-drawing never ends.  Here the margins are 2e-5 (kink) and 2e-6 (tie of a probability pair):
    K = 128 products of magnitude <= 1 summed in fp32 leave z, and the pre-activations formed from it, within about
    sqrt(K) * 2^-24 * |z| ~ 2e-6 of the float64 values, a tenth of the margin; the probabilities are within 1e-7."""
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

    def ill(r, cells):
        pr = r["prob"].reshape(cells, -1, 2)
        return (np.abs(r["pre1"]).min(1) < kink) | (np.abs(r["pre2"]).min(1) < kink) | \
               (np.abs(pr[..., 1] - pr[..., 0]).min(1) < tie)

    rows = np.arange(M)
    for _ in range(60):
        _, r = oracle(rows)
        rows = rows[np.unique(np.nonzero(ill(r, rows.size * D))[0] // D)]
        if rows.size == 0:
            break
        x[rows] = (rng.randn(rows.size, K) * 2.0).astype(np.float32)
    else:
        raise AssertionError("could not build a well-conditioned case")
    z6, r = oracle(np.arange(M))
    assert not ill(r, M * D).any()
    conf = np.asarray(r["conf"]).reshape(-1)
    assert (conf > 0).all() and int(conf.sum()) == M * D * nbits, conf
    pr = r["prob"].reshape(M, D, nbits, 2)
    gref = np.concatenate([r["grads"][k].reshape(-1) for k in ("w1", "b1", "w2", "b2")])
    return dict(M=M, K=K, N=N, nbits=nbits, x=x, w=w, b=b, flat=flat, bits=bits, z=z6, prob=pr, hard=pr[..., 1] > pr[..., 0],
                dz=r["dz"].reshape(M, N), dtailp=gref, ce_mean=float(r["ce_mean"]), conf=conf)


def _case(M, K, N, nbits):
    """Operands and float64 references of one shape: built once, shared by its tests, never modified."""
    key = (M, K, N, nbits)
    if key not in _cases:
        c = _wide_case(M, K, N, nbits) if (M, K, N) in LARGE else host_case(M, K, N, nbits)
        for k in ("x", "w", "b", "flat"):
            c["d_" + k] = torch.as_tensor(c[k]).cuda()
        c["d_bits"] = torch.as_tensor(c["bits"]).cuda()
        _cases[key] = c
    return _cases[key]


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    yield _lib.load()
    _cases.clear()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _standalone_tail(lib, c, z, bwd):
    """dccn_demod_tail_loss_fwd[_bwd] on z (host array [M, N])."""
    from dl_ofdm_amd import _lib, ops
    M, N, nbits = c["M"], c["N"], c["nbits"]
    D = N // 2
    cells = M * D
    zd = torch.as_tensor(z).cuda()
    prob = torch.full((M, D, nbits, 2), float("nan"), device="cuda")
    mbuf = torch.zeros(_lib.METRICS_BYTES, dtype=torch.uint8, device="cuda")
    nws = lib.dccn_demod_tail_workspace_size(cells, nbits)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    dz = dt = None
    if bwd:
        dz = torch.full((M, N), float("nan"), device="cuda")
        dt = torch.full((c["flat"].size,), float("nan"), device="cuda")
        _lib.check(lib.dccn_demod_tail_loss_fwd_bwd(_ptr(zd), _ptr(c["d_bits"]), _ptr(c["d_flat"]), _ptr(prob), _ptr(mbuf),
                                                    _ptr(dz), _ptr(dt), cells, nbits, _ptr(ws), nws, ops._stream()),
                   "dccn_demod_tail_loss_fwd_bwd")
    else:
        _lib.check(lib.dccn_demod_tail_loss_fwd(_ptr(zd), _ptr(c["d_bits"]), _ptr(c["d_flat"]), _ptr(prob), _ptr(mbuf), cells,
                                                nbits, _ptr(ws), nws, ops._stream()), "dccn_demod_tail_loss_fwd")
    torch.cuda.synchronize()
    return dict(prob=prob.cpu().numpy(), dz=dz.cpu().numpy() if bwd else None, dtailp=dt.cpu().numpy() if bwd else None,
                m=ops.read_metrics(mbuf))


@pytest.mark.parametrize("bwd", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("M,K,N,nbits", CASES)
def test_every_kloop_path_against_oracle_and_standalone_tail(lib, M, K, N, nbits, bwd):
    if (M, K, N) in LARGE:
        assert grid_of(lib, M, K, N, nbits) == LARGE[(M, K, N)]
    else:
        assert grid_of(lib, M, K, N, nbits) == (TILES, 48, 0, 4 * (N // 64))
    c = _case(M, K, N, nbits)
    what = "%s nbits %d %s" % ((M, K, N), nbits, "train" if bwd else "eval")
    got = run_tail(lib, c, bwd=bwd)               # z, prob and dz between NaN guard bands, checked on the way out
    alone = _standalone_tail(lib, c, got["z"], bwd)
    m, m2 = got["m"], alone["m"]
    conf, conf2 = (np.asarray(q["conf"]).reshape(-1) for q in (m, m2))
    count = M * (N // 2) * nbits

    # ---- the float64 oracle, 1e-5 ----
    e = dict(z=relerr(got["z"], c["z"]), prob=relerr(got["prob"], c["prob"]),
             ce=abs(m["ce_mean"] - c["ce_mean"]) / abs(c["ce_mean"]))
    if bwd:
        e.update(dz=relerr(got["dz"], c["dz"]), dtailp=relerr(got["dtailp"], c["dtailp"]))
    print("%s: against the oracle %s" % (what, "  ".join("%s %.2e" % kv for kv in sorted(e.items()))))
    assert not np.isnan(got["z"]).any() and not np.isnan(got["prob"]).any(), what       # every element was written
    assert all(v <= RTOL for v in e.values()), (what, e)
    assert np.array_equal(conf, c["conf"]) and m["count"] == count and int(conf.sum()) == count, (what, conf, c["conf"])
    assert np.array_equal(got["prob"][..., 1] > got["prob"][..., 0], c["hard"]), what

    # ---- the stand-alone tail on the fused launch's own z ----
    assert_same_bits(got["prob"], alone["prob"], what + ": prob against the stand-alone tail")
    assert np.array_equal(conf, conf2) and m2["count"] == count, (what, conf, conf2)
    assert abs(m["ce_mean"] - m2["ce_mean"]) <= 3e-5 * abs(m2["ce_mean"]), (what, m["ce_mean"], m2["ce_mean"])
    if bwd:
        assert not np.isnan(got["dz"]).any(), what
        assert_same_bits(got["dz"], alone["dz"], what + ": dz against the stand-alone tail")
        e2 = relerr(got["dtailp"], alone["dtailp"])
        print("%s: tail gradients against the stand-alone tail %.2e" % (what, e2))
        assert e2 <= 3e-5, (what, e2)
