"""The optimizer half of the CPU oracle, held to a float64 restatement, and the inputs of tests/test_gpu_optimizer.py
held to a sensitivity guard (no GPU).

The GPU tests of the fused optimizer launch compare Adam's slots after a step with ``O.adam_tf_step`` applied to the GPU's own
gradient.  That comparison is only worth something where a wrong gradient, a wrong BER gate or a missing L2 term MOVES the
slots by much more than the tolerance: from ``m = v = 0`` the first update is ``+-lr`` whatever ``|g|`` is, and at the
production coefficient (2e-6) the L2 term changes ``m`` by ~1e-8 of its scale.  ``l2_sensitivity`` measures exactly that on a
given set of inputs; the helpers below build the resumed, non-zero optimizer state and the amplified coefficients the GPU tests
run from, and ``test_chosen_inputs_pass_the_guard`` checks them here, on the oracle's own gradients.
"""
import copy

import numpy as np
import pytest

from oracle import dccn_oracle as O

F32 = np.float32
M_TOL = 2e-6                 # tests/test_gpu_ops.py::test_adam_tf_steps' bound on m / v / parameters (of each tensor's max)
GUARD_FACTOR = 100.0         # a dropped L2 term / a gate forced to 1 must move m by >= GUARD_FACTOR * M_TOL
START_STEP = 498             # four steps from here run at global_step 498, 499 | 500, 501: across the first stair
# amplified L2 coefficients (production: 2e-6 on all four): one value per tensor, different ones on the two kernels so that a
# coefficient read at the wrong tensor's offset shows as well
REG_AMPLIFIED = {"demodulation/dense/kernel": 5e-3, "demodulation/dense/bias": 1e-2,
                 "demodulation/dense_1/kernel": 4e-3, "demodulation/dense_1/bias": 1e-1}


def relmax(a, b):
    """max-norm distance of a from b, relative to max|b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


def beta_powers(steps: int):
    """beta1^(steps+1), beta2^(steps+1) as the float32 running products a run of `steps` optimizer steps leaves behind"""
    b1p, b2p = F32(O.ADAM_BETA1), F32(O.ADAM_BETA2)
    for _ in range(steps):
        b1p, b2p = F32(b1p * F32(O.ADAM_BETA1)), F32(b2p * F32(O.ADAM_BETA2))
    return b1p, b2p


def resumed_state(grad_scale, shapes, rng, step: int = START_STEP) -> O.AdamState:
    """An optimizer state as a checkpoint taken after `step` steps holds it: m ~ N(0, s), v ~ U(0.25, 4) s^2 per tensor (s its
    gradient scale: sqrt(v) stays far from eps and m / sqrt(v) is O(1) like in a running optimizer), beta powers as float32
    running products, global_step = step."""
    st = O.AdamState()
    for k, shp in shapes.items():
        s = F32(grad_scale[k])
        st.m[k] = (rng.standard_normal(shp) * s).astype(F32)
        st.v[k] = (rng.uniform(0.25, 4.0, shp) * s * s).astype(F32)
    st.beta1_power, st.beta2_power = beta_powers(step)
    st.global_step = F32(step)
    return st


def grad_scales(grads):
    """per tensor: RMS of the gradient"""
    return {k: max(float(np.sqrt(np.mean(np.asarray(g, np.float64) ** 2))), 1e-12) for k, g in grads.items()}


def effective_grads(grads, params, reg, gate):
    """what the optimizer kernels feed to Adam: g + (gate * reg) * p in float32, in that association (norm_adam.h)"""
    out = {}
    for k, g in grads.items():
        c = reg.get(k)
        if c is None:
            out[k] = np.asarray(g, F32)
        else:
            out[k] = (np.asarray(g, F32) + (F32(gate) * np.asarray(c, F32)) * np.asarray(params[k], F32)).astype(F32)
    return out


def oracle_step(params, grads, reg, gate, state: O.AdamState):
    """One TF-Adam step of the oracle on copies: (params', state', alpha)."""
    p = {k: np.array(v, F32) for k, v in params.items()}
    st = copy.deepcopy(state)
    alpha = O.adam_tf_step(p, effective_grads(grads, params, reg, gate), st)
    return p, st, alpha


def l2_sensitivity(params, grads, reg, gate, state: O.AdamState):
    """The guard: how far would m land from the true update if the kernel (a) dropped the L2 term, (b) took the gate as 1?
    name -> (relative max-norm distance of (a), of (b)) for every regularised tensor.  Both must be >> the comparison
    tolerance for a comparison of m to see those faults; this is a property of the inputs, measured on the oracle alone."""
    params, grads = {k: params[k] for k in reg}, {k: grads[k] for k in reg}        # (the other tensors carry no term)
    state = O.AdamState({k: state.m[k] for k in reg}, {k: state.v[k] for k in reg}, state.beta1_power, state.beta2_power,
                        state.global_step)
    _, true, _ = oracle_step(params, grads, reg, gate, state)
    _, no_l2, _ = oracle_step(params, grads, {}, gate, state)
    _, gate1, _ = oracle_step(params, grads, reg, 1.0, state)
    return {k: (relmax(no_l2.m[k], true.m[k]), relmax(gate1.m[k], true.m[k])) for k in reg}


def assert_guard(params, grads, reg, gate, state, tol=M_TOL, what=""):
    sens = l2_sensitivity(params, grads, reg, gate, state)
    for k, (d_l2, d_gate) in sens.items():
        assert d_l2 >= GUARD_FACTOR * tol and d_gate >= GUARD_FACTOR * tol, (what, k, d_l2, d_gate)
    return sens


# ---- the oracle itself -----------------------------------------------------------------------------------------------------
def test_learning_rate_staircase():
    """lr = 1e-3 * 0.98^floor(step / 500) in float32: flat up to 499, one factor at 500 .. 999, two at 1000"""
    lr0, r = F32(1e-3), F32(0.98)
    want = {0: lr0, 499: lr0, 500: F32(lr0 * r), 501: F32(lr0 * r), 999: F32(lr0 * r), 1000: F32(lr0 * F32(r * r))}
    for step, w in want.items():
        got = O.learning_rate(F32(step))
        assert got.dtype == np.float32 and got == w, (step, got, w)
    assert want[499] > want[500] > want[1000]


def _adam64(p, g, m, v, b1p, b2p, step):
    """TF ApplyAdam (training_ops.cc) restated in float64 from the formula"""
    lr = 1e-3 * 0.98 ** np.floor(step / 500.0)
    alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    m = m + (g - m) * (1.0 - 0.9)
    v = v + (g * g - v) * (1.0 - 0.999)
    return p - m * alpha / (np.sqrt(v) + 1e-8), m, v, alpha


@pytest.mark.parametrize("step", [7, 499, 500, 1203])
def test_adam_tf_step_from_a_resumed_state_matches_float64(step):
    rng = np.random.RandomState(step)
    shapes = {"a": (37, 5), "b": (11,)}
    scale = {"a": 3e-3, "b": 0.2}
    p = {k: rng.uniform(-0.1, 0.1, s).astype(F32) for k, s in shapes.items()}
    st = resumed_state(scale, shapes, rng, step)
    for it in range(3):
        g = {k: (rng.standard_normal(s) * scale[k]).astype(F32) for k, s in shapes.items()}
        ref = {k: _adam64(p[k].astype(np.float64), g[k].astype(np.float64), st.m[k].astype(np.float64),
                          st.v[k].astype(np.float64), float(st.beta1_power), float(st.beta2_power), float(st.global_step))
               for k in shapes}
        b1p, b2p, gs = float(st.beta1_power), float(st.beta2_power), float(st.global_step)
        p_before = {k: v.copy() for k, v in p.items()}
        alpha = O.adam_tf_step(p, g, st)
        for k in shapes:
            assert abs(float(alpha) - ref[k][3]) <= 1e-6 * ref[k][3]
            assert relmax(st.m[k], ref[k][1]) <= 1e-6 and relmax(st.v[k], ref[k][2]) <= 1e-6, (step, it, k)
            assert relmax(p[k], ref[k][0]) <= 1e-6, (step, it, k)
            # ... and the update itself, not only the parameter it is a small part of
            assert relmax(p[k] - p_before[k], ref[k][0] - p_before[k].astype(np.float64)) <= 1e-4, (step, it, k)
        assert float(st.global_step) == gs + 1.0
        assert abs(float(st.beta1_power) - b1p * 0.9) <= 1e-7 and abs(float(st.beta2_power) - b2p * 0.999) <= 1e-7


def test_beta_powers_are_running_products():
    b1p, b2p = beta_powers(0)
    assert b1p == F32(0.9) and b2p == F32(0.999)
    b1p, b2p = beta_powers(START_STEP)
    assert abs(float(b2p) - 0.999 ** (START_STEP + 1)) <= 1e-4 * 0.999 ** (START_STEP + 1)
    assert 0.0 < float(b1p) < 1e-20                     # (1 - beta1_power rounds to 1: alpha = lr * sqrt(1 - beta2_power))


def test_guard_sees_what_the_production_coefficients_hide():
    """At reg = 2e-6 and from m = v = 0 -- what every GPU test of the fused optimizer launch ran before -- dropping the L2 term
    moves m by less than the comparison tolerance; the guard must say so, and must pass on the amplified coefficients."""
    rng = np.random.RandomState(1)
    shapes = {k: (64, 10) for k in REG_AMPLIFIED}
    p = {k: rng.uniform(-0.08, 0.08, s).astype(F32) for k, s in shapes.items()}
    g = {k: (rng.standard_normal(s) * 1e-3).astype(F32) for k, s in shapes.items()}
    st = resumed_state(grad_scales(g), shapes, rng)
    prod = {k: F32(2e-6) for k in shapes}
    sens = l2_sensitivity(p, g, prod, 0.25, st)
    assert all(d_l2 < GUARD_FACTOR * M_TOL for d_l2, _ in sens.values())
    with pytest.raises(AssertionError):
        assert_guard(p, g, prod, 0.25, st)
    assert_guard(p, g, {k: F32(1e-2) for k in shapes}, 0.25, st)


@pytest.mark.parametrize("kin,batch", [(80, 300), (64, 300), (80, 13)])
def test_chosen_inputs_pass_the_guard(kin, batch):
    """The small-layer geometries of tests/test_gpu_optimizer.py (F = 64, S = 7, D = 50), the oracle's gradients standing in for
    the GPU's: with REG_AMPLIFIED, the resumed state and the BER gate of an untrained receiver (~0.5), both guard distances
    clear GUARD_FACTOR * M_TOL = 2e-4 with room to spare (the GPU tests assert the same on the GPU's own gradients)."""
    cfg = O.RxConfig(S=7, kin=kin, F=64, D=50, nbits=2)
    rng = np.random.RandomState(0)
    x = rng.standard_normal((batch, 7, kin, 2)).astype(np.float32)
    bits = rng.randint(0, 2, (batch, 50, 2)).astype(np.int32)
    p = O.init_params(cfg, seed=1)
    for k in p:
        if k.endswith("bias"):
            p[k] = rng.uniform(-0.05, 0.05, p[k].shape).astype(np.float32)
    xn, _, _ = O.batch_moment_norm(x.reshape(batch, -1).astype(np.float64))
    grads, info = O.rx_forward_backward({k: v.astype(np.float64) for k, v in p.items()}, xn.reshape(x.shape), bits, cfg)
    grads = {k: v.astype(np.float32) for k, v in grads.items()}
    st = resumed_state(grad_scales(grads), {k: v.shape for k, v in p.items()}, rng)
    reg = {k: F32(v) for k, v in REG_AMPLIFIED.items()}
    sens = assert_guard(p, grads, reg, float(info["berlin"]), st)
    print("guard margins (x tolerance) kin=%d batch=%d gate=%.3f: %s" % (
        kin, batch, float(info["berlin"]), {k: (round(a / M_TOL), round(b / M_TOL)) for k, (a, b) in sens.items()}))
    assert min(min(v) for v in sens.values()) >= 5 * GUARD_FACTOR * M_TOL          # (room for the GPU's other batches)
