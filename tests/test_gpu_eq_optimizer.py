"""The equaliser step's optimizer launch (``eq_opt_kernel``, csrc/eq_opt.h) and its riders (``eq_ride_body``, csrc/eq_step.h) held to
Adam's oracle mid-run (``-m gpu``) -- what tests/test_gpu_optimizer.py does for the receiver.

Every earlier test of this launch starts from ``m = v = 0`` at ``global_step = 0`` with the production coefficient, where the first
update is ``+-lr`` whatever ``|g|`` is; ``v`` was never compared, the stair at step 500 never reached, ``reg_uniform = 0`` and
``reg_coef = NULL`` never run.  Here every case follows the recipe of ``test_gpu_optimizer.resume``: one dry step for the gradient
scales, parameters put back, slots and state as after ``START_STEP = 498`` steps (``m ~ N(0, s)``, ``v ~ U(0.25, 4) s^2``), L2
coefficients from ``eq_optimizer_ref.eq_coefficients`` (the term is ~30 % of each tensor's gradient scale, one value per tensor),
then FOUR steps on fresh batches at global steps 498, 499 | 500, 501, captured graphs on the odd ones.  After each step the guard
runs on the GPU's own gradients and ``check_eq_step`` holds alpha, the rate, the state, and m / v / parameter of all 20 tensors
-- every element, ``M_TOL`` of the tensor's max -- and the arenas' padding to the oracle.

Each case first proves the branch it is written for through the host-only queries (``dccn_gemm_route_query``,
``dccn_eq_bottleneck_supported``, ``dccn_eq_norm_rides``); what no query reports is derived from the line that fixes it:

  * bottleneck partial count: ``eq_bn_parts`` (eq_step.h) ``tiles = ceil(B / 16)``, the ``splits`` of the four EQJ_SUM jobs
    ``eq_issue_update`` adds for dense_1 / dense_2: 5 at 73 frames (``splits <= 8`` branch of eq_opt_sum), 13 at 200 (``> 8``).
  * riders: ``eq_issue_backward`` lets dense_4 / dense_3 ride when their grouped backward left no slabs (route ``splits == 1``)
    and the fold of the smoothing kernel whenever ``dsT.dw_slabs == nullptr`` -- which the lines above it ENSURE: slabs of dT are
    summed by a launch of their own first.  So with the bottleneck launch present the fold always runs with ``splits == 1``, at 200
    frames too; its ``splits > 1`` loop (eq_opt_conv2d / slab_sum) is not reachable from the step.  The general (non-gather) loop
    runs where ``S * K > 512``: N = 128 (896 cells).
  * ``J.vec == 0``: ``EqOptBuilder::slabs`` with ``slab % 4 != 0`` -- the bias slabs of dense_5 at N = 128 / CP = 9 (2 (K + CP) = 274
    floats apart) once the layer is split, i.e. from 73 frames on; at 12 frames nothing is split (query: ``splits == 1``
    everywhere) and the N = 128 case runs plain jobs with an element-wise tail (274 % 4 = 2), the bottleneck as GEMMs and the
    general fold loop.  Case E (129 frames, 8 slabs) takes ``J.vec == 0``.
  * split counts above 8 on a dense layer need no knob: dense / dense_5 at 200 frames are split 11 ways (query).  Knob 4 CUTS counts
    (``dense_dw_plan``: at most ``max_splits16``); set to 12 it leaves dense_5 with exactly 8 slabs -- the last count of the
    unrolled branch -- which is the case kept here; knob 5 does not reach the equaliser's grouped C-Conv backward.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import eq_optimizer_ref as R
from eq_optimizer_ref import F32, START_STEP
from oracle import dccn_oracle as O
from test_gemm_route_query import route
from test_gpu_equalizer import _trainer

pytestmark = pytest.mark.gpu
N_STEPS = 4
GEOM = {"A": dict(nfft=64, longcp=True, cp=True, B=73), "B": dict(nfft=64, longcp=True, cp=True, B=200),
        "C": dict(nfft=64, longcp=True, cp=False, B=12), "D": dict(nfft=128, longcp=False, cp=True, B=12),
        "E": dict(nfft=128, longcp=False, cp=True, B=129)}


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


class knobs:
    """dccn_set_tuning for a block; every knob back to what it was afterwards"""

    def __init__(self, lib, values):
        self.lib, self.values = lib, values

    def __enter__(self):
        self.old = {k: self.lib.dccn_get_tuning(k) for k in self.values}
        for k, v in self.values.items():
            assert self.lib.dccn_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.dccn_set_tuning(k, v)
        assert all(self.lib.dccn_get_tuning(k) == v for k, v in self.old.items())


def splits(lib, op, *dims):
    st, r = route(lib, op, *dims)
    assert st == 0, (op, dims)
    return r["splits"]


def prove_branch(lib, case, tx, shape):
    """the branch the case is written for, from the host-only queries, before anything is launched"""
    g = GEOM[case]
    B, K, CP = g["B"], tx.K, tx.CP
    R_, SK2, Pp, N2 = 7 * B, 7 * K * 2, 2 * tx.pilot_size, 2 * (K + CP)
    bn, rides = lib.dccn_eq_bottleneck_supported(B, SK2, Pp), lib.dccn_eq_norm_rides(C.byref(shape))
    s_sq, s_d5 = splits(lib, "dense_bwd", B, SK2, SK2), splits(lib, "dense_bwd", R_, 4 * K, N2)
    s_d0 = splits(lib, "dense_bwd_w", R_, N2 if g["cp"] else 2 * K, 2 * K)
    facts = dict(bottleneck=bn, norm_rides=rides, partials=-(-B // 16), dense34_smooth=s_sq, dense_5=s_d5, dense=s_d0, cells=7 * K)
    if case == "A":          # riders carry the gather fold and dense_3 / dense_4; 5 partials and 4 dense slabs: the <= 8 branch
        assert bn == 1 and rides == 1 and s_sq == 1 and 7 * K <= 512 and 1 < facts["partials"] <= 8 and 1 < s_d5 <= 8, facts
    elif case == "B":        # dense_3 / dense_4 split; 13 partials and 11 dense slabs: the > 8 branch
        assert bn == 1 and s_sq > 1 and facts["partials"] > 8 and s_d5 > 8 and s_d0 > 8, facts
    elif case == "C":        # nothing split: the dense layers' gradients are finished in the arena (plain jobs)
        assert bn == 1 and s_sq == 1 and s_d5 == 1 and s_d0 == 1, facts
    elif case == "D":        # no bottleneck launch (so no riders), nothing split, fold of 896 cells, 274-float rows
        assert bn == 0 and rides == 0 and s_sq == 1 and s_d5 == 1 and s_d0 == 1 and 7 * K > 512 and N2 % 4 == 2, facts
    else:                    # dense_5 split with bias slabs 274 floats apart: J.vec == 0 with splits > 1
        assert bn == 0 and s_d5 > 1 and N2 % 4 == 2, facts
    return facts


def snapshot(tr):
    torch.cuda.synchronize()
    named = lambda arena: {n: tr.view(n, arena).detach().cpu().numpy().copy() for n in tr.names}          # noqa: E731
    pad = {a: R.padding_floats(getattr(tr, a).cpu().numpy(), tr.layout) for a in R.ARENAS}
    return dict(p=named(tr.params), m=named(tr.adam_m), v=named(tr.adam_v), state=tr.adam_state.cpu().numpy().copy(), pad=pad)


def _load(tr, arena, values):
    with torch.no_grad():
        for n, v in values.items():
            tr.view(n, arena).copy_(torch.as_tensor(np.array(np.broadcast_to(np.asarray(v, np.float32), tr.layout[n][1]))))


def load_resumed(tr, p0, seed, form, step=START_STEP, fill=True):
    """steps 2-4 of the recipe, after the dry step: parameters back, slots and state of a run of `step` steps, coefficients.
    form 'null' with fill: the arena holds the uniform form's values, which a launch given reg_coef = NULL must not read."""
    torch.cuda.synchronize()
    scale = R.grad_scales(tr.get_grads())
    rng = np.random.RandomState(seed)
    st = R.resumed_state(scale, {n: tr.layout[n][1] for n in tr.names}, rng, step)
    tr.load_params(p0)
    _load(tr, tr.adam_m, st.m)
    _load(tr, tr.adam_v, st.v)
    tr.adam_state.copy_(torch.tensor([float(st.global_step), float(st.beta1_power), float(st.beta2_power), 0.0]))
    p_named = tr.get_params()
    coef = R.eq_coefficients(p_named, scale, form=form, rng=rng)
    tr.reg_coef.zero_()
    if form != "null" or fill:
        _load(tr, tr.reg_coef, coef if form != "null" else R.eq_coefficients(p_named, scale, form="uniform"))
    assert not np.any(R.padding_floats(tr.reg_coef.cpu().numpy(), tr.layout))
    tr.__dict__.pop("_normalised_ahead", None)
    torch.cuda.synchronize()
    return coef


def set_form(bufs, form):
    if form == "per_element":
        bufs.reg_uniform = 0
    elif form == "null":
        bufs.reg_coef = None


def check(tr, before, coef, step, what):
    g = tr.get_grads()
    assert before["state"][0] == step, (what, before["state"])
    st = O.AdamState(before["m"], before["v"], F32(before["state"][1]), F32(before["state"][2]), F32(before["state"][0]))
    margin = None
    if coef:
        sens = R.assert_l2_guard(before["p"], g, coef, st, what=(what, step))
        margin = min(a for a, _ in sens.values()) / R.M_TOL
    after = snapshot(tr)
    checks = R.check_eq_step(before, after, g, coef, tr.hp)
    print("%s step %d: worst m %.2e v %.2e p %.2e of max | alpha %.1e | guard %s x M_TOL | fails %s" % (
        (what, step) + R.worst_errors(checks) + (checks["alpha"][1], "%.0f" % margin if margin else "-", R.failed(checks))))
    bad = R.failed(checks)
    assert not bad, (what, step, "%d checks fail" % len(bad), {k: checks[k][1] for k in bad[:9]})
    return after


def batches(tr, B, tx, n, seed):
    rng = np.random.RandomState(seed)
    xs = [(rng.standard_normal((B, 7, tx.K + tx.CP, 2)) * 2).astype(np.float32) for _ in range(n)]
    bs = [rng.randint(0, 2, (B, tx.frame_size, 2)).astype(np.int32) for _ in range(n)]
    return xs, bs


def run_case(lib, case, form="uniform", seed=0, checked=True, fill=True, what=""):
    """The recipe at one geometry under the knobs currently set.  Returns the final (params, m, v) arenas."""
    g = GEOM[case]
    B = g["B"]
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer(seed=21 + seed, cp=g["cp"], nfft=g["nfft"], longcp=g["longcp"])
    pl = tr.resident(B)
    facts = prove_branch(lib, case, tx, pl.shape) if lib.dccn_get_tuning(20) == 1 and lib.dccn_get_tuning(4) == 0 else {}
    what = ("%s %s %s" % (case, form, what)).strip()
    print("%s: routes as the queries answer %s" % (what, facts))
    set_form(pl.buffers, form)
    xs, bs = batches(tr, B, tx, N_STEPS + 1, 100 + seed)
    tr.train_step(xs[N_STEPS], bs[N_STEPS], fused=True, graph=False)                  # the dry step
    coef = load_resumed(tr, tr_params0(tr, pe), 5 + seed, form, fill=fill)
    before = snapshot(tr) if checked else None
    for t in range(N_STEPS):
        tr.train_step(xs[t], bs[t], fused=True, graph=(t % 2 == 1))
        if checked:
            before = check(tr, before, coef, START_STEP + t, what)
    torch.cuda.synchronize()
    assert float(tr.adam_state[0]) == START_STEP + N_STEPS
    return tr.params.clone(), tr.adam_m.clone(), tr.adam_v.clone()


def tr_params0(tr, pe):
    return {n: np.asarray(pe[n], np.float32).reshape(tr.layout[n][1]) for n in tr.names}


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


_DEFAULT = {}


def default_run(lib, case, form="uniform"):
    """the checked run of a case under the default knobs, once per module (other tests compare their bits with it)"""
    if (case, form) not in _DEFAULT:
        _DEFAULT[(case, form)] = run_case(lib, case, form)
    return _DEFAULT[(case, form)]


# ---- the geometries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(GEOM))
def test_geometry(lib, case):
    """A: 64 / long / cp, 73 frames -- riders carry the smoothing fold (gather fast path, 448 cells) and dense_3 / dense_4, five
       bottleneck partials and four dense slabs (splits <= 8), C-Conv folds
    B: 200 frames -- dense_3 / dense_4 as split-K slabs inside the launch, 13 partials and 11 dense slabs (splits > 8)
    C: cp=False, 12 frames -- direct gradients: plain jobs
    D: 128 / short, 12 frames -- no bottleneck launch and no riders, fold of 896 cells (general loop), element-wise tails
    E: 128 / short, 129 frames -- element-wise branch (J.vec == 0) with 8 slabs"""
    assert lib.dccn_get_tuning(20) == 1 and lib.dccn_get_tuning(24) == 1 and lib.dccn_get_tuning(4) == 0
    default_run(lib, case)


# ---- knobs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 2, 3, 4])
def test_riders_leave_the_same_bits(lib, value):
    """knob 24: 0 no riders, 2 only dense_3 rides, 3 only dense_4, 4 no fold -- each held to the oracle, and parameters, m and v
    bit-equal to the default run (1: all three ride) from the same state (eq_opt.h: "bit-identical parameters")"""
    ref = default_run(lib, "A")
    with knobs(lib, {24: value}):
        got = run_case(lib, "A", what="knob24=%d" % value)
    assert same_bits(got, ref)


@pytest.mark.parametrize("case", ["A", "B"])
@pytest.mark.parametrize("value", [0, 3])
def test_step_plans(lib, case, value):
    """knob 20: 0 = launch per stage (adam_impl over the whole arena), 3 = the job table without the bottleneck launch (dense_1 /
    dense_2 as GEMM slabs or plain jobs, no riders)"""
    with knobs(lib, {20: value}):
        run_case(lib, case, what="knob20=%d" % value)


def test_eight_dense_slabs(lib):
    """knob 4 = 12 at 200 frames: the query confirms exactly 8 slabs for dense_5 -- the last count of the unrolled branch of
    eq_opt_sum (counts above 8 are the default there: test_geometry[B])"""
    with knobs(lib, {4: 12}):
        n = splits(lib, "dense_bwd", 7 * 200, 256, 160)
        if n != 8:
            pytest.fail("the route query no longer reports 8 slabs under knob 4 = 12 (%d): pick the knob value that does" % n)
        run_case(lib, "B", what="knob4=12")


# ---- coefficient forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_per_element_coefficients(lib, case):
    """reg_uniform = 0: a coefficient per element on all 20 tensors, the C-Conv kernels, their biases and the (S,K) kernel included
    (eq_adam_one in the two folds; adjacent plain jobs merge in this form: C)"""
    run_case(lib, case, "per_element")


@pytest.mark.parametrize("case", ["A", "B", "D"])
def test_no_coefficients(lib, case):
    """reg_coef = NULL with a FILLED arena: held to the oracle without a term, and bit-equal to a run with a zero arena"""
    a = run_case(lib, case, "null", fill=True)
    b = run_case(lib, case, "null", fill=False, checked=False)
    assert same_bits(a, b)


# ---- the pipelined pair ---------------------------------------------------------------------------------------------------------
def test_pipelined_pair_across_the_stair(lib):
    """pipe_with / x_next at A: every step's optimizer launch normalises the next batch (EQJ_NORM_NEXT in front of the table) and
    the next step's bookkeeping runs on eq_prep_kernel.  The step at 500 must use the decayed rate although its normalisation ran
    on the launch of step 499."""
    from dl_ofdm_amd.equalizer import _FusedPlan
    g = GEOM["A"]
    B = g["B"]
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer(seed=29, cp=True)
    a = _FusedPlan(tr, B)
    b = _FusedPlan(tr, B, twin_of=a)
    assert lib.dccn_eq_norm_rides(C.byref(a.shape)) == 1
    a.pipe_with(b, 0)
    b.pipe_with(a, 1)
    xs, bs = batches(tr, B, tx, N_STEPS + 1, 300)
    a.set_batch(xs[N_STEPS], bs[N_STEPS])
    a.run(True, graph=False)                                             # the dry step
    coef = load_resumed(tr, tr_params0(tr, pe), 31, "uniform")
    before = snapshot(tr)
    plans = [a, b, a, b]
    plans[0].set_batch(xs[0], bs[0])
    for t in range(N_STEPS):
        if t + 1 < N_STEPS:
            plans[t + 1].set_batch(xs[t + 1], bs[t + 1])                 # (its previous reader was issued on this stream)
        plans[t].run(True, graph=(t % 2 == 1), pipe=0 if t == 0 else (2 if t == N_STEPS - 1 else 1))
        before = check(tr, before, coef, START_STEP + t, "pipelined")
    a.close()
    b.close()


# ---- a chain group ----------------------------------------------------------------------------------------------------------------
def test_chain_group_with_chains_at_different_steps(lib, tmp_path):
    """Three chains (BPSK, QPSK, 16-QAM; N = 64 / long, 73 frames) in one launch sequence, resumed at DIFFERENT steps -- 137, 498,
    499 -- each with its own slots and coefficients: a kernel or rider that read chain 0's state (chain_at / move_to_chain /
    EqRideArgs::at_chain) would pass every bitwise chain-versus-solo test and fails alpha and every parameter of chains 1 and 2
    here.  Three group steps (own normalisation, pipelined, last of the epoch), the next batch's generator and the monitors
    riding as in the training loop; check_eq_step per chain on that chain's own snapshot."""
    from dl_ofdm_amd import ofdm, receiver as Rx, receiver_mp as H
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer_group import EqualizerChainGroup, _eq_shape
    B, starts = 73, (137, START_STEP, START_STEP + 1)
    fl = [H.Flags(nbits=nb, nfilter=64, channel="mixRayleigh", device_data=True, seed=10 + 7 * i + nb, max_epoch_num=2, early_stop=200,
                  msg_length=7 * B * 3, eval_frames=128, token="opt%d_%d" % (i, nb), save_dir=os.path.join(str(tmp_path), "ck%d/" % i))
          for i, nb in enumerate((1, 2, 4))]
    assert all(lib.dccn_eq_group_supported(C.byref(_eq_shape(F, ofdm.ofdm_tx(F), B, F.nbits))) == 1 for F in fl)
    grp = EqualizerChainGroup(fl, [glorot_init(Rx.rx_dims(F, ofdm.ofdm_tx(F)), 3 + i) for i, F in enumerate(fl)])
    chains = grp.chains
    assert chains[0].steps == 3 and chains[0].B == B
    rng = np.random.RandomState(9)
    p0 = [c.tr.get_params() for c in chains]
    for c, p in zip(chains, p0):                                           # non-zero biases (a zero tensor carries no L2 term at all)
        for n in p:
            if n.endswith("bias"):
                p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
        c.tr.load_params(p)
    for c in chains:                                                       # the dry epoch: gradient scales
        c.begin_epoch()
    for i in range(3):
        grp.step(chains, i)
    coefs = [load_resumed(c.tr, p0[i], 40 + i, "uniform", step=starts[i]) for i, c in enumerate(chains)]
    assert len({float(co["Equalizer/dense_3/kernel"]) for co in coefs}) == 3
    before = [snapshot(c.tr) for c in chains]
    for c in chains:
        c.epoch += 1
        c.begin_epoch()
    for i in range(3):
        grp.step(chains, i)
        before = [check(c.tr, before[k], coefs[k], starts[k] + i, "group chain %d" % k) for k, c in enumerate(chains)]
