"""Shared checker of the equaliser step's optimizer launch (``eq_opt_kernel``, csrc/eq_opt.h; the riders of csrc/eq_step.h):
TF-Adam of the oracle applied to the GPU's own gradient arena, from the GPU's own pre-step parameters, slots and state.  No GPU,
not a conftest: tests/test_eq_optimizer_checker.py holds it on the CPU, tests/test_gpu_eq_optimizer.py applies it to the kernels.

The gradient arena of the equaliser step holds the DATA term; the L2 term enters in the optimizer as ``g + c * p`` with gate 1
(``eq_adam_one``: the equaliser has no BER gate), so the oracle runs on ``effective_grads(g, p, coef, 1.0)``.  A snapshot is
``dict(p=.., m=.., v=.. (name -> array), state=[global_step, beta1_power, beta2_power, alpha], pad=..)`` with ``pad`` the
padding floats of the four arenas (``arena name -> array``; include/dccn.h dccn_eq_param_offsets: they must stay zero).

Every bound is one the project already has: alpha 1e-6 relative, beta powers 1e-7, m / v / parameters ``M_TOL`` of each tensor's
max over EVERY element, the guard ``GUARD_FACTOR * M_TOL`` (tests/test_optimizer_oracle.py).
"""
import numpy as np

from oracle import dccn_oracle as O
from test_optimizer_oracle import (F32, GUARD_FACTOR, M_TOL, START_STEP, beta_powers, grad_scales, oracle_step,  # noqa: F401
                                   relmax, resumed_state)

KAPPA = 0.3
ARENAS = ("params", "adam_m", "adam_v", "grads")
ORACLE_HP = dict(lr0=O.LR0, decay_steps=O.LR_DECAY_STEPS, decay_rate=O.LR_DECAY, beta1=O.ADAM_BETA1, beta2=O.ADAM_BETA2,
                 eps=O.ADAM_EPS)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def regularized(names):
    """the tensors keras puts l2(0.01) on: every dense kernel and bias, no C-Conv (oracle/equalizer_oracle.py regularized)"""
    return [n for n in names if "/dense" in n]


def eq_coefficients(params, grad_scale, kappa=KAPPA, *, form, rng=None):
    """The L2 coefficients a case runs with, name -> what the oracle applies (a float32 scalar, or an array per element).
    ``c_n = kappa * rms(g_n) / rms(p_n)``: the term is ~kappa of each tensor's gradient scale and no two tensors share a value, so a
    coefficient read at another tensor's offset shows.
      uniform      dense kernels and biases only, one value per tensor (reg_uniform = 1: the production form)
      per_element  U(0, 2 c_n) per element on EVERY tensor, C-Conv kernels, their biases and the (S,K) kernel included
                   (reg_uniform = 0)
      null         {}: no coefficients (reg_coef = NULL)
    The arena's padding floats are not named here: they stay 0 in every form."""
    if form == "null":
        return {}
    c = {n: F32(kappa * float(grad_scale[n]) / max(_rms(params[n]), 1e-30)) for n in params}
    if form == "uniform":
        out = {n: c[n] for n in regularized(params)}
        assert len(set(float(v) for v in out.values())) == len(out), "two tensors share a coefficient"
        return out
    assert form == "per_element", form
    rng = rng or np.random.RandomState(0)
    return {n: rng.uniform(0.0, 2.0 * float(c[n]), np.shape(params[n])).astype(F32) for n in params}


def l2_sensitivity(params, grads, coef, state):
    """name -> (distance of m, of v) from the true update if the optimizer dropped the L2 term, for every tensor that carries a
    coefficient -- a property of the inputs, measured on the oracle alone (the L2 half of test_optimizer_oracle.l2_sensitivity)"""
    names = list(coef)
    p, g = {k: params[k] for k in names}, {k: grads[k] for k in names}
    st = O.AdamState({k: state.m[k] for k in names}, {k: state.v[k] for k in names}, state.beta1_power, state.beta2_power,
                     state.global_step)
    _, true, _ = oracle_step(p, g, coef, 1.0, st)
    _, no_l2, _ = oracle_step(p, g, {}, 1.0, st)
    return {k: (relmax(no_l2.m[k], true.m[k]), relmax(no_l2.v[k], true.v[k])) for k in names}


def assert_l2_guard(params, grads, coef, state, tol=M_TOL, what="", factor=1.0):
    """Dropping the L2 term must move m by >= factor * GUARD_FACTOR * tol on every tensor that carries a coefficient (the gate
    half of assert_guard does not apply: the equaliser's gate is the constant 1)."""
    sens = l2_sensitivity(params, grads, coef, state)
    for k, (d_m, _) in sens.items():
        assert d_m >= factor * GUARD_FACTOR * tol, (what, k, d_m)
    return sens


def _hp_dict(hp):
    if hp is None:
        return dict(ORACLE_HP)
    if isinstance(hp, dict):
        return {k: float(hp[k]) for k in ORACLE_HP}
    return {k: float(getattr(hp, k)) for k in ORACLE_HP}


def _step_hp(params, eff, state, hp):
    """adam_tf_step restated in float32 with the trainer's own hyper-parameters (only used where they differ from the oracle's)"""
    f = F32
    lr = f(f(hp["lr0"]) * np.power(f(hp["decay_rate"]), np.floor(f(state.global_step) / f(hp["decay_steps"])), dtype=f))
    alpha = f(lr * np.sqrt(f(1.0) - state.beta2_power, dtype=f) / (f(1.0) - state.beta1_power))
    p, m, v = {}, {}, {}
    for k in params:
        g = eff[k]
        m[k] = state.m[k] + (g - state.m[k]) * (f(1.0) - f(hp["beta1"]))
        v[k] = state.v[k] + (g * g - state.v[k]) * (f(1.0) - f(hp["beta2"]))
        p[k] = np.asarray(params[k], f) - (m[k] * alpha) / (np.sqrt(v[k]) + f(hp["eps"]))
    st = O.AdamState(m, v, f(state.beta1_power * f(hp["beta1"])), f(state.beta2_power * f(hp["beta2"])),
                     f(state.global_step + f(1.0)))
    return p, st, alpha


def reference_step(before, grads, coef, hp=None):
    """(params', state', alpha, lr) of one step from the snapshot `before` on the data-term gradients `grads`"""
    from test_optimizer_oracle import effective_grads
    hp = _hp_dict(hp)
    s0 = np.asarray(before["state"], F32)
    st = O.AdamState({k: np.asarray(v, F32) for k, v in before["m"].items()}, {k: np.asarray(v, F32) for k, v in before["v"].items()},
                     F32(s0[1]), F32(s0[2]), F32(s0[0]))
    if all(F32(hp[k]) == F32(ORACLE_HP[k]) for k in ORACLE_HP):
        p, st1, alpha = oracle_step(before["p"], grads, coef, 1.0, st)
        lr = O.learning_rate(F32(s0[0]))
    else:
        p, st1, alpha = _step_hp(before["p"], effective_grads(grads, before["p"], coef, 1.0), st, hp)
        lr = F32(F32(hp["lr0"]) * np.power(F32(hp["decay_rate"]), np.floor(F32(s0[0]) / F32(hp["decay_steps"])), dtype=F32))
    return p, st1, alpha, lr


def check_eq_step(before, after, grads, coef, hp=None):
    """The oracle against the step the GPU took.  Returns name -> (passed, measured, bound); the checks are
      alpha          1e-6 relative, of the PRE-step state (state'[3])
      lr             the stair in float32 -- lr0 * (decay_rate if step >= decay_steps else 1) below the second stair -- and the
                     rate the GPU's alpha implies (alpha / (sqrt(1 - beta2_power) / (1 - beta1_power))) within 1e-6 of it
      global_step    exactly + 1
      beta_powers    1e-7
      m/<t> v/<t> p/<t>   relmax <= M_TOL of the tensor's max, every element, for each of the tensors
      padding        the padding floats of params, adam_m, adam_v and grads are exactly 0.0 after the step"""
    hpd = _hp_dict(hp)
    p_or, st_or, alpha, lr = reference_step(before, grads, coef, hpd)
    s0, s1 = np.asarray(before["state"], F32), np.asarray(after["state"], F32)
    out = {}
    e = abs(float(s1[3]) - float(alpha)) / float(alpha)
    out["alpha"] = (e <= 1e-6, e, 1e-6)
    step = float(s0[0])
    stairs = np.floor(F32(step) / F32(hpd["decay_steps"]))
    want = F32(hpd["lr0"]) * (F32(hpd["decay_rate"]) if stairs == 1 else F32(1.0)) if stairs <= 1 else lr
    corr = float(np.sqrt(F32(1.0) - F32(s0[2]), dtype=F32) / (F32(1.0) - F32(s0[1])))
    e = abs(float(s1[3]) / corr - float(want)) / float(want)
    out["lr"] = (bool(lr == want) and e <= 1e-6, e, 1e-6)
    out["global_step"] = (float(s1[0]) == step + 1.0, float(s1[0]) - step, 1.0)
    e = max(abs(float(s1[1]) - float(st_or.beta1_power)), abs(float(s1[2]) - float(st_or.beta2_power)))
    out["beta_powers"] = (e <= 1e-7, e, 1e-7)
    for n in before["p"]:
        for slot, ref in (("m", st_or.m[n]), ("v", st_or.v[n]), ("p", p_or[n])):
            e = relmax(np.asarray(after[slot][n]).reshape(np.shape(ref)), ref)
            out["%s/%s" % (slot, n)] = (e <= M_TOL, e, M_TOL)
    worst = max([float(np.abs(np.asarray(after["pad"][a], np.float64)).max()) if np.size(after["pad"][a]) else 0.0 for a in ARENAS])
    out["padding"] = (worst == 0.0 and all(a in after["pad"] for a in ARENAS), worst, 0.0)
    return out


def failed(checks):
    return sorted(k for k, (ok, _, _) in checks.items() if not ok)


def worst_errors(checks):
    """(worst m, worst v, worst parameter error) over the tensors, as fractions of each tensor's max"""
    return tuple(max(e for k, (_, e, _) in checks.items() if k.startswith(s + "/")) for s in "mvp")


def padding_floats(flat, layout):
    """the floats of a flat arena that no tensor of `layout` (name -> (offset, shape)) covers"""
    flat = np.asarray(flat).ravel()
    mask = np.ones(flat.shape[0], bool)
    for o, shp in layout.values():
        mask[o:o + int(np.prod(shp))] = False
    return flat[mask].copy()
