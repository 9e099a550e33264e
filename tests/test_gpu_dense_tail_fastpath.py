"""The fused dense + tail launch against the two-launch route (dense forward, then the stand-alone tail) on shapes that
mix interior and ragged 48x64 tiles (``-m gpu``).

Interior tiles run the tail without validity masks and with tile-relative store addresses; ragged tiles keep the masked
form; both pack the four confusion tallies into one word.  A missing mask or a wrong field shows up as a count that
differs from the stand-alone tail's, or as a dz / prob cell written to the wrong place.

Shapes (N=64 / CP=16: K = 896, D = 320 data cells): 50 frames = row tiles 48 + 2 (nbits 1, 2), 48 frames = interior tiles
only, 7 frames = ragged tiles only, 50 frames at nbits 3 = the LDS-staged tail.  Batches of up to 96 frames are planned
onto the few-row 16x16 tiles by default, so every case runs twice: as planned, and with that plan switched off
(tuning knob 21), which puts the same shapes on the 48x64 tiles this file is about.

Comparisons: prob at 5e-6 (what test_gpu_ops.py::test_dense_tail_fused uses for this pair of routes).  dz, ce_mean and the
tail-parameter gradients: both routes are held to the float64 oracle at 1e-5 (stand-alone tail) and 2e-5 (fused launch) by
test_gpu_ops.py, so they differ from each other by at most 3e-5 of the largest magnitude; inputs are re-drawn until no
pre-activation sits within 2e-4 of a leaky-ReLU kink (there a rounding-level difference in z flips a derivative).  With z
taken from the fused launch itself the per-cell outputs of the two routes must be EQUAL bit for bit (same tail_cells code,
any batch width gives the same bits).  Confusion counts: exactly equal, and they sum to frames * D * nbits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O

pytestmark = pytest.mark.gpu

K, D = 896, 320
N = 2 * D
TUNE_FEWROW = 21
SHAPES = [(50, 1), (50, 2), (48, 2), (7, 2), (50, 3)]


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def relerr(got, ref):
    got = got.double().cpu().numpy()
    ref = ref.double().cpu().numpy()
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


_cases = {}


def _case(frames, nbits):
    """Inputs of one shape (built once, shared by its four tests, never modified)."""
    key = (frames, nbits)
    if key in _cases:
        return _cases[key]
    rng = np.random.RandomState(1000 * nbits + frames)
    m = 1 << nbits
    tp = dict(w1=rng.uniform(-1, 1, (2, m)), b1=rng.uniform(-.3, .3, m), w2=rng.uniform(-1, 1, (m + 2, 2 * nbits)),
              b2=rng.uniform(-.3, .3, 2 * nbits))
    tp = {k: v.astype(np.float32).astype(np.float64) for k, v in tp.items()}
    flat = np.concatenate([tp[k].reshape(-1) for k in ("w1", "b1", "w2", "b2")]).astype(np.float32)
    w = (rng.randn(K, N) / np.sqrt(K)).astype(np.float32)
    b = (rng.randn(N) * 0.5).astype(np.float32)
    x = (rng.randn(frames, K) * 2.0).astype(np.float32)
    bits = rng.randint(0, 2, (frames, D, nbits)).astype(np.int32)
    w6, b6 = w.astype(np.float64), b.astype(np.float64)
    for _ in range(60):
        z6 = x.astype(np.float64) @ w6 + b6
        r = O.tail_forward_backward(z6.reshape(-1, 2), bits.reshape(-1, nbits), tp["w1"], tp["b1"], tp["w2"], tp["b2"], nbits)
        pr = r["prob"].reshape(frames * D, -1, 2)
        bad = (np.abs(r["pre1"]).min(1) < 2e-4) | (np.abs(r["pre2"]).min(1) < 2e-4) | \
              (np.abs(pr[..., 1] - pr[..., 0]).min(1) < 2e-5)
        rows = np.unique(np.nonzero(bad)[0] // D)
        if rows.size == 0:
            break
        x[rows] = (rng.randn(rows.size, K) * 2.0).astype(np.float32)
    else:
        raise AssertionError("could not build a well-conditioned case")
    conf = np.asarray(r["conf"]).reshape(-1)
    assert (conf > 0).all(), conf                   # random bits, random weights: all four confusion cells are hit
    _cases[key] = dict(x=dev(x), w=dev(w), b=dev(b), flat=dev(flat), bits=dev(bits, torch.int32), conf=conf)
    return _cases[key]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fused(lib, ops, c, frames, nbits, want_prob):
    from dl_ofdm_amd._lib import check
    nws = lib.dccn_dense_tail_workspace_size(frames, N, nbits)
    ws = ops.workspace(nws, c["x"].device, "fastpath_fused")
    z = torch.full((frames, N), float("nan"), device="cuda")
    dz = torch.full((frames, N), float("nan"), device="cuda")
    prob = torch.full((frames, D, nbits, 2), float("nan"), device="cuda") if want_prob else None
    dt = torch.empty_like(c["flat"])
    mbuf = torch.zeros(ops._lib.METRICS_BYTES, dtype=torch.uint8, device="cuda")
    check(lib.dccn_dense_tail_fwd_bwd(_ptr(c["x"]), _ptr(c["w"]), _ptr(c["b"]), _ptr(z), _ptr(c["bits"]), _ptr(c["flat"]),
                                      _ptr(prob), _ptr(mbuf), _ptr(dz), _ptr(dt), frames, K, N, nbits, _ptr(ws), nws,
                                      ops._stream()), "dccn_dense_tail_fwd_bwd")
    return z, dz, prob, dt, ops.read_metrics(mbuf)


def _tail(lib, ops, c, z, frames, nbits, want_prob):
    from dl_ofdm_amd._lib import check
    cells = frames * D
    nws = lib.dccn_demod_tail_workspace_size(cells, nbits)
    ws = ops.workspace(nws, z.device, "fastpath_tail")
    dz = torch.full((frames, N), float("nan"), device="cuda")
    prob = torch.full((frames, D, nbits, 2), float("nan"), device="cuda") if want_prob else None
    dt = torch.empty_like(c["flat"])
    mbuf = torch.zeros(ops._lib.METRICS_BYTES, dtype=torch.uint8, device="cuda")
    check(lib.dccn_demod_tail_loss_fwd_bwd(_ptr(z), _ptr(c["bits"]), _ptr(c["flat"]), _ptr(prob), _ptr(mbuf), _ptr(dz),
                                           _ptr(dt), cells, nbits, _ptr(ws), nws, ops._stream()),
          "dccn_demod_tail_loss_fwd_bwd")
    return dz, prob, dt, ops.read_metrics(mbuf)


@pytest.mark.parametrize("fewrow", [0, 1], ids=["tiles48x64", "planned"])
@pytest.mark.parametrize("want_prob", [True, False], ids=["prob", "noprob"])
@pytest.mark.parametrize("frames,nbits", SHAPES)
def test_fused_launch_matches_dense_then_tail(frames, nbits, want_prob, fewrow):
    from dl_ofdm_amd import _lib, ops
    lib = _lib.load()
    c = _case(frames, nbits)
    default = lib.dccn_get_tuning(TUNE_FEWROW)
    try:
        assert lib.dccn_set_tuning(TUNE_FEWROW, fewrow) == 0
        z, dz, prob, dt, m = _fused(lib, ops, c, frames, nbits, want_prob)
        # the two-launch route: stand-alone dense forward, stand-alone tail
        z2 = ops.dense(c["x"], c["w"], c["b"])
    finally:
        lib.dccn_set_tuning(TUNE_FEWROW, default)
    dz2, prob2, dt2, m2 = _tail(lib, ops, c, z2, frames, nbits, want_prob)
    # ... and the tail alone on the fused launch's own z: per-cell results are the same bits
    dz3, prob3, dt3, m3 = _tail(lib, ops, c, z, frames, nbits, want_prob)
    torch.cuda.synchronize()
    count = frames * D * nbits
    conf, conf2, conf3 = (np.asarray(q["conf"]).reshape(-1) for q in (m, m2, m3))
    print("frames %d nbits %d prob %d fewrow %d: conf %s | dz %.2e  dt %.2e  ce %.2e (vs two launches) | dt %.2e (same z)"
          % (frames, nbits, want_prob, fewrow, conf.tolist(), relerr(dz, dz2), relerr(dt, dt2),
             abs(m["ce_mean"] - m2["ce_mean"]) / abs(m2["ce_mean"]), relerr(dt, dt3)))
    assert not torch.isnan(z).any() and not torch.isnan(dz).any()           # every element was written
    assert np.array_equal(conf, conf2) and np.array_equal(conf, conf3) and np.array_equal(conf, c["conf"])
    assert int(conf.sum()) == count and m["count"] == count
    assert (conf > 0).all()
    if want_prob:
        assert not torch.isnan(prob).any()
        assert relerr(prob, prob2) <= 5e-6
        assert torch.equal(prob, prob3)
    assert torch.equal(dz, dz3)
    assert relerr(dz, dz2) <= 3e-5
    assert relerr(dt, dt2) <= 3e-5 and relerr(dt, dt3) <= 3e-5
    assert abs(m["ce_mean"] - m2["ce_mean"]) <= 3e-5 * abs(m2["ce_mean"])
    assert abs(m["ce_mean"] - m3["ce_mean"]) <= 3e-5 * abs(m3["ce_mean"])
