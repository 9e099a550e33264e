"""tests/eq_optimizer_ref.py held on the CPU (no GPU): the guard on the inputs the GPU cases run with, the checker on the oracle's
own step, and every fault the checker is there to catch planted into the "after" values -- each must fail exactly the checks it
has to and no other.

Gradients: ``LiteralEqualizer.forward_backward`` (float64 autograd) on ``E.init_params(bias_scale=0.05)`` with the production L2
part subtracted, i.e. the data term the GPU's gradient arena holds.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E
from oracle.torch_ref import LiteralEqualizer, LiteralRx
import eq_optimizer_ref as R
from eq_optimizer_ref import F32, GUARD_FACTOR, M_TOL, START_STEP
from test_gpu_equalizer import _trainer_config

GEOMETRIES = [(64, 16, 8), (64, 16, 73), (128, 9, 12)]          # (K, CP, frames), cp=True, QPSK
_CACHE = {}


def data_term(K, CP, B):
    """(params, data-term gradients) of one batch, float32, computed once per geometry"""
    if (K, CP, B) not in _CACHE:
        _, tx, ecfg, rcfg, pe, pr = _trainer_config(2, 21, cp=True, nfft=K, longcp=(4 * CP == K))
        assert (tx.K, tx.CP) == (K, CP)
        rng = np.random.RandomState(100 + B)
        x = (rng.standard_normal((B, 7, K + CP, 2)) * 2).astype(np.float64)
        bits = rng.randint(0, 2, (B, tx.frame_size, 2)).astype(np.int32)
        lit_rx = LiteralRx({k: v.astype(np.float64) for k, v in pr.items()}, rcfg, dtype=torch.float64, literal_conv=False)
        g, _ = LiteralEqualizer({k: v.astype(np.float64) for k, v in pe.items()}, lit_rx, ecfg).forward_backward(x, bits)
        prod = E.EQ_REG_COEFF * 2 * O.REG_L2
        g = {n: (g[n] - (prod * pe[n].astype(np.float64) if "/dense" in n else 0.0)).astype(F32) for n in pe}
        _CACHE[(K, CP, B)] = (pe, g)
    return _CACHE[(K, CP, B)]


def snapshot_before(p, g, step, seed=5):
    st = R.resumed_state(R.grad_scales(g), {n: v.shape for n, v in p.items()}, np.random.RandomState(seed), step)
    return dict(p={n: v.copy() for n, v in p.items()}, m=st.m, v=st.v,
                state=np.array([st.global_step, st.beta1_power, st.beta2_power, 0.0], F32))


def snapshot_after(before, g, coef, alpha=None, v_grads=None):
    """the step as the oracle takes it; alpha: another rate for the parameter update (and state[3]); v_grads: v formed from
    these gradients instead of the effective ones"""
    p1, st1, a, _ = R.reference_step(before, g, coef)
    if v_grads is not None:
        for n in p1:
            gg = np.asarray(v_grads[n], F32)
            st1.v[n] = before["v"][n] + (gg * gg - before["v"][n]) * (F32(1.0) - F32(O.ADAM_BETA2))
    if alpha is not None or v_grads is not None:
        a = F32(a if alpha is None else alpha)
        p1 = {n: before["p"][n] - (st1.m[n] * a) / (np.sqrt(st1.v[n]) + F32(O.ADAM_EPS)) for n in p1}
    return dict(p=p1, m=st1.m, v=st1.v, state=np.array([st1.global_step, st1.beta1_power, st1.beta2_power, a], F32),
                pad={k: np.zeros(2, F32) for k in R.ARENAS})


@pytest.mark.parametrize("K,CP,B", GEOMETRIES)
def test_guard_on_the_oracle_alone(K, CP, B):
    """With kappa = 0.3 a dropped L2 term moves m by thousands of tolerances on every tensor that carries a coefficient, in
    both forms (measured: 6.1e3, 6.0e3, 5.6e3 x M_TOL at the three geometries, the smallest of the 20 tensors; v >= 117 x)."""
    p, g = data_term(K, CP, B)
    scale = R.grad_scales(g)
    before = snapshot_before(p, g, START_STEP)
    st = O.AdamState(before["m"], before["v"], F32(before["state"][1]), F32(before["state"][2]), F32(before["state"][0]))
    for form, n_coef in (("uniform", 12), ("per_element", 20)):
        coef = R.eq_coefficients(p, scale, form=form, rng=np.random.RandomState(3))
        assert len(coef) == n_coef
        sens = R.assert_l2_guard(p, g, coef, st, what=(K, CP, B, form), factor=5.0)
        m_min, v_min = min(a for a, _ in sens.values()), min(b for _, b in sens.values())
        print("guard margins K=%d CP=%d B=%d %s: m >= %.0f x M_TOL, v >= %.0f x M_TOL" % (K, CP, B, form, m_min / M_TOL, v_min / M_TOL))
        assert m_min >= 5 * GUARD_FACTOR * M_TOL and v_min >= GUARD_FACTOR * M_TOL
    assert R.eq_coefficients(p, scale, form="null") == {}


@pytest.mark.parametrize("form", ["uniform", "per_element", "null"])
@pytest.mark.parametrize("step", [START_STEP, 500])
def test_checker_passes_on_the_oracles_own_step(form, step):
    p, g = data_term(64, 16, 8)
    coef = R.eq_coefficients(p, R.grad_scales(g), form=form, rng=np.random.RandomState(3))
    before = snapshot_before(p, g, step)
    checks = R.check_eq_step(before, snapshot_after(before, g, coef), g, coef)
    assert len(checks) == 5 + 3 * 20 and not R.failed(checks), R.failed(checks)
    # hyper-parameters other than the oracle's are read from hp: a step taken with them passes, and fails against the defaults
    hp = dict(R.ORACLE_HP, lr0=2e-3, beta2=0.99)
    p1, st1, a, _ = R.reference_step(before, g, coef, hp)
    after = dict(p=p1, m=st1.m, v=st1.v, state=np.array([st1.global_step, st1.beta1_power, st1.beta2_power, a], F32),
                 pad={k: np.zeros(0, F32) for k in R.ARENAS})
    assert not R.failed(R.check_eq_step(before, after, g, coef, hp))
    assert {"alpha", "lr", "beta_powers"} <= set(R.failed(R.check_eq_step(before, after, g, coef)))


def _tensors(prefix, names):
    return {"%s/%s" % (s, n) for s in prefix for n in names}


def test_each_planted_fault_fails_exactly_its_checks():
    p, g = data_term(64, 16, 8)
    names, reg = list(p), R.regularized(p)
    coef = R.eq_coefficients(p, R.grad_scales(g), form="uniform")
    b498, b500 = snapshot_before(p, g, START_STEP), snapshot_before(p, g, 500)
    good498, good500 = snapshot_after(b498, g, coef), snapshot_after(b500, g, coef)
    W3, W4 = "Equalizer/dense_3/kernel", "Equalizer/dense_4/kernel"
    cases = {}                                          # name -> (before, after, must fail, may fail as well)

    cases["L2 term dropped"] = (b498, snapshot_after(b498, g, {}), _tensors("mv", reg), _tensors("p", reg))

    swapped = dict(coef)
    swapped[W3] = coef["Equalizer/dense_3/bias"]
    cases["coefficient of the neighbouring tensor"] = (b498, snapshot_after(b498, g, swapped), {"m/" + W3}, {"v/" + W3, "p/" + W3})

    a500 = float(good500["state"][3])
    cases["lr not decayed at step 500"] = (b500, snapshot_after(b500, g, coef, alpha=a500 / float(F32(0.98))),
                                            {"alpha", "lr"} | _tensors("p", names), set())

    b1p, b2p = R.beta_powers(137)
    a137 = F32(O.learning_rate(F32(137)) * np.sqrt(F32(1.0) - b2p, dtype=F32) / (F32(1.0) - b1p))
    cases["alpha of the chain at step 137"] = (b498, snapshot_after(b498, g, coef, alpha=a137), {"alpha", "lr"} | _tensors("p", names), set())

    twice = copy.deepcopy(good498)
    eff = (g[W4] + coef[W4] * twice["p"][W4]).astype(F32)            # the second visit reads the updated parameter
    q = (slice(3, 4), slice(8, 12))                                      # one quad of a row
    twice["m"][W4][q] += (eff[q] - twice["m"][W4][q]) * (F32(1.0) - F32(O.ADAM_BETA1))
    twice["v"][W4][q] += (eff[q] * eff[q] - twice["v"][W4][q]) * (F32(1.0) - F32(O.ADAM_BETA2))
    twice["p"][W4][q] -= (twice["m"][W4][q] * good498["state"][3]) / (np.sqrt(twice["v"][W4][q]) + F32(O.ADAM_EPS))
    cases["one quad updated twice"] = (b498, twice, {"m/" + W4, "p/" + W4}, {"v/" + W4})

    cases["v from g without the L2 term"] = (b498, snapshot_after(b498, g, coef, v_grads=g), _tensors("v", reg), _tensors("p", reg))

    stuck = copy.deepcopy(good498)
    stuck["state"][1:3] = b498["state"][1:3]
    cases["beta powers not advanced"] = (b498, stuck, {"beta_powers"}, set())

    dirty = copy.deepcopy(good498)
    dirty["pad"]["adam_v"][1] = F32(1e-30)
    cases["a non-zero padding float"] = (b498, dirty, {"padding"}, set())

    assert not R.failed(R.check_eq_step(b498, good498, g, coef)) and not R.failed(R.check_eq_step(b500, good500, g, coef))
    for what, (before, after, must, may) in cases.items():
        got = set(R.failed(R.check_eq_step(before, after, g, coef)))
        print("%-40s fails %d checks: %s" % (what, len(got), sorted(k.split("/")[0] for k in got)[:6]))
        assert must <= got, (what, "not caught", sorted(must - got))
        assert got <= must | may, (what, "fails checks it should pass", sorted(got - must - may))
