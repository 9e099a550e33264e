"""The plan that is timed against the plan that is checked (``-m gpu``).

bench.py and receiver.train build the engine with ``want_prob=False, want_grads=False, want_z=False, want_dfft=False``: the
null-``prob`` tail instantiations, ``skip_dw_grad`` in the optimizer launch, a dense + tail launch without a ``z`` store, a
backward without a ``dfft`` store.  include/dccn.h documents all four as nullable STORES (``keep_dense_grad``, ``prob``, ``z``,
``dfft``): nothing the step computes may depend on them.  Engine A here is the full plan, the one tests/test_gpu_engine.py holds
to the oracle stage by stage (``staged_checks``, repeated below as the anchor); engine B is exactly bench.py's.  Both start
from the same parameters and the same resumed, non-zero optimizer state with amplified L2 coefficients
(tests/test_gpu_optimizer.py: a wrong gate or gradient moves ``m`` / ``v``), take the same fresh batches, and must agree after
every step: parameters, both Adam slots and the optimizer state bit for bit, the metrics with ``==``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from test_gpu_engine import make_case, staged_checks
from test_gpu_optimizer import _batches, resume, snapshot
from test_optimizer_oracle import F32, assert_guard

pytestmark = pytest.mark.gpu
N_STEPS = 3
METRIC_KEYS = ("ce_mean", "conf", "count", "berlin", "tx_power")
# (frames, nbits, kin), D = 320: 50 frames: few-row tiles; 130: 48x64 tiles, interior plus ragged; 500: two slabs of the dense dW
SHAPES = [(frames, nbits, 80) for nbits in (1, 2, 3, 4) for frames in (50, 130, 500)] + [(130, 2, 64)]
LEAN = dict(want_prob=False, want_grads=False, want_z=False, want_dfft=False)


def _pair(frames, nbits, kin, seed=0):
    """A (full plan) and B (bench.py's), same parameters, same resumed optimizer state, same amplified coefficients"""
    from dl_ofdm_amd.engine import RxEngine
    dims, cfg, x, bits, p = make_case(frames, nbits, kin=kin, D=320, seed=seed)
    a = RxEngine(dims, frames, params=p, train=True, want_prob=True, want_grads=True, want_tx_power=True)
    b = RxEngine(dims, frames, params=p, train=True, want_tx_power=True, **LEAN)
    assert b.prob is None and b.buffers.keep_dense_grad == -1
    coef = resume(a, p, x, bits, seed + 5)
    for name in ("params", "adam_m", "adam_v", "adam_state", "reg_coef"):
        getattr(b, name).copy_(getattr(a, name))
    torch.cuda.synchronize()
    return a, b, cfg, x, bits, p, coef


def _same(a, b, what):
    torch.cuda.synchronize()
    for name in ("params", "adam_m", "adam_v", "adam_state"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    ma, mb = a.metrics(), b.metrics()
    for k in METRIC_KEYS:
        assert ma[k] == mb[k], (what, k, ma[k], mb[k])


@pytest.mark.parametrize("mode", ["plain", "pipe", "pipe-graph"])
@pytest.mark.parametrize("frames,nbits,kin", SHAPES)
def test_lean_plan_is_bitwise_the_full_plan(frames, nbits, kin, mode):
    """B as train_step, as train_step_pipelined (eager) and as its captured replay, against A's plain train_step."""
    a, b, cfg, x, bits, p, coef = _pair(frames, nbits, kin)
    assert b.lib.dccn_rx_bwd_fused_supported(C.byref(b.shape)) == 1 and b.dfft is None        # the backward is one launch
    assert (b.z is None) == bool(b.lib.dccn_rx_dense_tail_fused(C.byref(b.shape), 1))
    xs, bs = _batches(x, bits, N_STEPS + 1, 23)
    if mode != "plain":
        b.prime(xs[0])
    for t in range(N_STEPS):
        before = snapshot(a) if t == 0 else None
        a.train_step(xs[t], bs[t])
        if mode == "plain":
            b.train_step(xs[t], bs[t])
        elif mode == "pipe":
            b.train_step_pipelined(next_x=xs[t + 1], bits=bs[t], last=(t == N_STEPS - 1))
        else:
            b.train_step_pipelined(next_x=xs[t + 1], bits=bs[t], graph=True)
        if t == 0:                                               # the inputs can see a wrong gate / a missing term
            s0 = before["state"]
            assert_guard(before["p"], a.get_grads(), coef, a.metrics()["berlin"],
                         O.AdamState(before["m"], before["v"], F32(s0[1]), F32(s0[2]), F32(s0[0])))
        _same(a, b, (frames, nbits, kin, mode, t))
    assert float(a.adam_state[0]) == 498.0 + N_STEPS
    b.drop_prefetch()


@pytest.mark.parametrize("frames,nbits,kin", SHAPES)
def test_eval_step_without_prob_reports_the_same_metrics(frames, nbits, kin):
    from dl_ofdm_amd.engine import RxEngine
    dims, cfg, x, bits, p = make_case(frames, nbits, kin=kin, D=320, seed=1)
    a = RxEngine(dims, frames, params=p, train=False, want_prob=True)
    b = RxEngine(dims, frames, params=p, train=False, want_prob=False)
    a.eval_step(x, bits)
    b.eval_step(x, bits)
    torch.cuda.synchronize()
    ma, mb = a.metrics(), b.metrics()
    for k in METRIC_KEYS:
        assert ma[k] == mb[k], (k, ma[k], mb[k])
    assert ma["count"] == frames * 320 * nbits == int(np.sum(ma["conf"]))


def test_full_plan_anchor_matches_the_oracle():
    """What the bitwise comparisons above hang on: engine A's step from the resumed state, held to the float64 oracle end to end
    and stage by stage (tests/test_gpu_engine.py staged_checks) at (QPSK, 130 frames)."""
    a, b, cfg, x, bits, p, coef = _pair(130, 2, 80)
    xs, bs = _batches(x, bits, 1, 23)
    a.train_step(xs[0], bs[0])
    b.train_step(xs[0], bs[0])
    torch.cuda.synchronize()
    staged_checks(a, p, xs[0], bs[0], cfg)
    _same(a, b, "anchor")
