"""The optimizer launches held to the oracle where Adam can see them (``-m gpu``).

Every earlier GPU test of ``adam_rx_kernel`` (norm_adam.h) starts from ``m = v = 0`` at ``global_step = 0`` with the production
L2 coefficient: the first update is ``+-lr`` whatever ``|g|`` is, the L2 term is ~1e-5 of the gradient, and the learning-rate
stair at step 500 is never reached.  Here every case resumes from a non-zero state at ``global_step = 498`` (``m ~ N(0, s)``,
``v ~ U(0.25, 4) s^2``, ``s`` the tensor's gradient scale from a dry step), runs FOUR steps on fresh batches -- 498, 499 | 500,
501 -- with amplified L2 coefficients, and after each step applies ``O.adam_tf_step`` in float32 to the GPU's own gradient, from
the GPU's own pre-step parameters and slots.  Before anything is compared, the sensitivity guard of
tests/test_optimizer_oracle.py must say that a dropped L2 term and a gate forced to 1 would each move ``m`` by at least 100
tolerances on these very inputs.

Tolerances are the ones of the existing tests of the same quantities: alpha 1e-6 relative
(test_trainer_step_gradients_and_adam), beta powers 1e-7 and m / v / parameters 2e-6 of each tensor's max (test_adam_tf_steps),
the dense kernel's gradient against ``fft_out.T @ dz`` in float64 at 1e-5 (staged_checks) -- the last one holds the sum of the
split-K slabs itself.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from test_gpu_engine import make_case, relerr
from test_optimizer_oracle import (F32, M_TOL, REG_AMPLIFIED, START_STEP, assert_guard, beta_powers, grad_scales,
                                   oracle_step, resumed_state)

pytestmark = pytest.mark.gpu
N_STEPS = 4
DENSE_W = "demodulation/dense/kernel"


def _batches(x, bits, n, seed):
    rng = np.random.RandomState(seed)
    xs = [(x + 0.3 * rng.standard_normal(x.shape)).astype(np.float32) for _ in range(n)]
    bs = [rng.randint(0, 2, bits.shape).astype(np.int32) for _ in range(n)]
    return xs, bs


def _tensors(eng, arena):
    return {n: eng.view(n, arena).detach().cpu().numpy().copy() for n in eng.layout}


def _load(eng, arena, values):
    for n, v in values.items():
        eng.view(n, arena).copy_(torch.as_tensor(np.asarray(v, np.float32)).reshape(eng.layout[n][1]))


def resume(eng, p, x, bits, seed, reg="uniform"):
    """Steps 2-3 of the recipe: one dry step for the gradient scales, then parameters back to `p`, slots and state as a run
    of START_STEP steps would leave them, amplified L2 coefficients.  Returns name -> coefficient (scalar or array) as the
    oracle applies it, {} for the reg_coef = NULL form."""
    eng.train_step(x, bits)
    torch.cuda.synchronize()
    scale = grad_scales(eng.get_grads())
    rng = np.random.RandomState(seed)
    st = resumed_state(scale, {n: shp for n, (_, shp) in eng.layout.items()}, rng)
    eng.load_params(p)
    _load(eng, eng.adam_m, st.m)
    _load(eng, eng.adam_v, st.v)
    eng.adam_state.copy_(torch.tensor([float(st.global_step), float(st.beta1_power), float(st.beta2_power), 0.0]))
    coef = {n: F32(c) for n, c in REG_AMPLIFIED.items()}
    if reg == "nonuniform":          # a coefficient per element of the dense kernel: the launch must stream reg_coef there
        coef[DENSE_W] = rng.uniform(0.0, 2.0 * REG_AMPLIFIED[DENSE_W], eng.layout[DENSE_W][1]).astype(np.float32)
        eng.buffers.reg_uniform_dense = 0
    eng.reg_coef.zero_()
    _load(eng, eng.reg_coef, {n: np.array(np.broadcast_to(c, eng.layout[n][1])) for n, c in coef.items()})
    if reg == "null":                # no coefficients at all: gate 1, no term (the arena above stays filled: it must not be read)
        eng.buffers.reg_coef = None
        coef = {}
    eng._pipe_bufs.clear()
    torch.cuda.synchronize()
    return coef


def snapshot(eng):
    return dict(p=_tensors(eng, eng.params), m=_tensors(eng, eng.adam_m), v=_tensors(eng, eng.adam_v),
                state=eng.adam_state.cpu().numpy().copy())


def check_step(eng, before, coef, step, what):
    """The oracle on the GPU's own gradient, from the GPU's own pre-step state; every assertion of the module docstring."""
    torch.cuda.synchronize()
    g = eng.get_grads()
    gate = eng.metrics()["berlin"] if coef else 1.0
    s0 = before["state"]
    assert s0[0] == START_STEP + step, (what, step, s0)
    st = O.AdamState(before["m"], before["v"], F32(s0[1]), F32(s0[2]), F32(s0[0]))
    if coef:
        assert_guard(before["p"], g, coef, gate, st, what=(what, step))
    p_or, st_or, alpha = oracle_step(before["p"], g, coef, gate, st)
    s1 = eng.adam_state.cpu().numpy()
    lr = O.learning_rate(F32(START_STEP + step))
    assert lr == F32(1e-3) * (F32(0.98) if START_STEP + step >= 500 else F32(1.0))          # the stair is crossed at step 2
    # alpha belongs to the pre-step state; the state advances by exactly one step
    assert abs(float(s1[3]) - float(alpha)) <= 1e-6 * float(alpha), (what, step, s1[3], alpha)
    assert s1[0] == s0[0] + 1.0, (what, step, s1)
    assert abs(float(s1[1]) - float(st_or.beta1_power)) <= 1e-7 and abs(float(s1[2]) - float(st_or.beta2_power)) <= 1e-7
    after = snapshot(eng)
    for n in eng.layout:
        for slot, ref in (("m", st_or.m[n]), ("v", st_or.v[n]), ("p", p_or[n])):
            err = relerr(after[slot][n], ref)
            assert err <= M_TOL, (what, step, slot, n, err)
    # the sum of the split-K slabs (or the unsplit GEMM) against the float64 contraction of the GPU's own operands
    a64 = eng.fft_out.cpu().numpy().astype(np.float64).reshape(eng.batch, -1)
    err = relerr(g[DENSE_W], a64.T @ eng.dz.cpu().numpy().astype(np.float64))
    assert err <= 1e-5, (what, step, "dense dW", err)
    return after


def check_conv_grads(eng, x_norm, what):
    """The C-Conv gradient of the step just run -- in the fused plans the sum adam_rx_kernel takes over the per-tile partials of
    the backward launch -- against O.cconv_gemm_bwd on the GPU's own dfft and on `x_norm`, the normalised batch that step ran
    on: staged_checks' own check at its own tolerance (check_step does not look at this gradient)."""
    torch.cuda.synchronize()
    g = eng.get_grads()
    batch, S, kin, _ = x_norm.shape
    F = eng.dfft.shape[-2]
    _, gw, gb = O.cconv_gemm_bwd(x_norm.cpu().numpy().astype(np.float64).reshape(batch * S, kin, 2), np.zeros((kin, 2 * F)),
                                 eng.dfft.cpu().numpy().astype(np.float64).reshape(batch * S, F, 2))
    for name, ref in (("fft_like/conv3d/kernel", gw), ("fft_like/conv3d/bias", gb)):
        err = relerr(g[name], ref)
        assert err <= 1e-5, (what, name, err)


def run_case(batch, kin=80, F=64, D=50, mode="plain", reg="uniform", fused_bwd=True, seed=0, what="", check=True, S=7,
             each_step=None):
    """mode: plain | pipe (train_step_pipelined, eager) | pipe-graph.  Returns the engine after N_STEPS steps, each one checked
    (check=False: the same run, unchecked -- for a second engine that is compared with a checked one bit by bit).
    each_step(eng, x_norm, what): called after every step with the normalised batch that step ran on (a pipelined step leaves
    the NEXT batch in the engine's buffer, so a copy is taken before it)."""
    from dl_ofdm_amd.engine import RxEngine
    dims, cfg, x, bits, p = make_case(batch, 2, kin, F, D, S=S, seed=seed)
    eng = RxEngine(dims, batch, params=p, train=True, want_prob=True, want_grads=True)
    assert bool(eng.lib.dccn_rx_bwd_fused_supported(C.byref(eng.shape))) == fused_bwd
    xs, bs = _batches(x, bits, N_STEPS + 1, seed + 17)
    coef = resume(eng, p, x, bits, seed + 5, reg)
    before = snapshot(eng)
    if mode != "plain":
        eng.prime(xs[0])
    for t in range(N_STEPS):
        xn = eng._norm_bufs[eng._norm_parity].clone() if (each_step and mode != "plain") else None
        if mode == "plain":
            eng.train_step(xs[t], bs[t])
        elif mode == "pipe":
            eng.train_step_pipelined(next_x=xs[t + 1], bits=bs[t], last=(t == N_STEPS - 1))
        else:
            eng.train_step_pipelined(next_x=xs[t + 1], bits=bs[t], graph=True)
        if check:
            before = check_step(eng, before, coef, t, (what, batch, kin, mode, reg))
        if each_step:
            each_step(eng, eng.x_norm if xn is None else xn, (what, batch, S, kin, F, mode, t))
    torch.cuda.synchronize()
    eng.drop_prefetch()
    return eng


# ---- slab counts of the fused backward -------------------------------------------------------------------------------------
# (D = 50, dK = 896: dense_dw_plan with 448-row ranges gives 1 slab at 300 frames -- summed by the runtime-count kernel with
# dw_slabs set --, 2 at 500; from 768 frames on the graded presets of knob 14 decide: the default 14 has 5 ranges, presets 2 / 1 /
# 21 have 3 / 4 / 6; knob 4 = 7 with the grading off asks for seven 128-row ranges, past the largest instantiation)
SLAB_CASES = [("1slab", 300, 80, {}), ("2slabs", 500, 64, {}), ("graded-default", 800, 80, {}),
              ("3ranges", 800, 80, {14: 2}), ("4ranges", 800, 64, {14: 1}), ("6ranges", 800, 80, {14: 21}),
              ("7slabs-runtime", 800, 80, {14: 0, 4: 7})]


@pytest.mark.parametrize("name,batch,kin,knobs", SLAB_CASES, ids=[c[0] for c in SLAB_CASES])
def test_slab_counts_of_the_fused_backward(name, batch, kin, knobs):
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    defaults = {k: lib.dccn_get_tuning(k) for k in knobs}
    try:
        for k, v in knobs.items():
            assert lib.dccn_set_tuning(k, v) == 0
        run_case(batch, kin=kin, what=name)
    finally:
        for k, v in defaults.items():
            lib.dccn_set_tuning(k, v)
    assert all(lib.dccn_get_tuning(k) == v for k, v in defaults.items())


# ---- filter counts and frame lengths other than F = 64, S = 7 ------------------------------------------------------------------
# adam_rx_kernel folds the per-tile partials of the fused backward launch (cw_tilew = 64, cw_slab = (2F / 64) tiles,
# cw_splits = ceil(batch / 64) * S terms) and applies Adam in the same pass: one, three and four tiles per symbol, S = 3, one /
# two / graded dense dW ranges, and -- pipe -- R0 of the next batch on the same launch.  F = 80 is the receiver's default filter
# count: 2F = 160 is no multiple of 64, the grouped backward's split-K fold.  tests/test_rx_backward_ref.py: what these see.
GEOMETRY_CASES = [("F32-1slab", 300, dict(kin=80, F=32)), ("F32-2slabs", 500, dict(kin=64, F=32)),
                  ("F128", 300, dict(kin=64, F=128)), ("F96-S3", 300, dict(kin=80, F=96, S=3)),
                  ("F32-graded-pipe", 800, dict(kin=80, F=32, mode="pipe")),
                  ("F80-grouped", 300, dict(kin=80, F=80, fused_bwd=False))]


@pytest.mark.parametrize("name,batch,kw", GEOMETRY_CASES, ids=[c[0] for c in GEOMETRY_CASES])
def test_other_filter_counts_and_frame_lengths(name, batch, kw):
    """check_step holds the dense kernel's gradient and every Adam slot of every tensor, from the resumed state; the C-Conv
    gradient itself -- the fold -- is held by check_conv_grads after each of the four steps."""
    run_case(batch, D=50, what=name, each_step=check_conv_grads, **kw)


# ---- who advances the state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,mode", [(300, "plain"), (2000, "plain"), (300, "pipe"), (300, "pipe-graph")])
def test_every_plan_advances_the_state_once_per_step(batch, mode):
    """300 frames: the single-pass R0; 2000: the two-kernel R0 (> 1536 frames); pipelined, eager and captured: R0 of the next
    batch rides on this very launch.  In each, global_step advances by exactly one per step and alpha is the pre-step one."""
    run_case(batch, mode=mode, seed=2, what="state")


# ---- regulariser forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", ["nonuniform", "null"])
@pytest.mark.parametrize("batch", [300, 500])
def test_regulariser_forms(reg, batch):
    """reg_uniform_dense = 0 with a random non-negative coefficient per element of the dense kernel; reg_coef = NULL: gate 1, no
    term (uniform, the default, is every other case of this file)."""
    run_case(batch, reg=reg, seed=3, what="reg")


# ---- scalar segment path -------------------------------------------------------------------------------------------------------
def _grouped_dw_splits(lib, M, K, N):
    """the slab count the grouped (un-fused) dense backward leaves for the optimizer launch: dccn_dense_bwd_slabs' own answer"""
    nws = lib.dccn_dense_bwd_w_workspace_size(M, K, N)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    x, dy, w = torch.zeros(M, K, device="cuda"), torch.zeros(M, N, device="cuda"), torch.zeros(K, N, device="cuda")
    dx, dw, db = torch.zeros(M, K, device="cuda"), torch.zeros(K, N, device="cuda"), torch.zeros(N, device="cuda")
    splits = C.c_int(0)
    assert lib.dccn_dense_bwd_slabs(x.data_ptr(), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                    M, K, N, ws.data_ptr(), nws, C.byref(splits), None) == 0
    torch.cuda.synchronize()
    return splits.value


@pytest.mark.parametrize("batch,split", [(13, False), (300, True)])
def test_scalar_segment_path(batch, split):
    """kin = 20, F = 12, D = 51: 2D = 102 is no multiple of 4, so the dense segments are not float4-aligned (seg4 false) and the
    backward is not fused.  13 frames: unsplit dW, plain gradient loads; 300 frames: the grouped backward defers its slabs
    (dccn_dense_bwd_slabs reports how many for the same (M, K, N)) and the element-wise slab sum of kernel AND bias runs."""
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    assert (_grouped_dw_splits(lib, batch, 7 * 12 * 2, 102) > 1) == split
    run_case(batch, kin=20, F=12, D=51, fused_bwd=False, seed=4, what="scalar")


# ---- large layers: the dense kernel's segment on the second stream -------------------------------------------------------------
def test_large_layer_pair_of_launches():
    """kin = 1096, F = 1024, D = 260, 40 frames: 112 x 5 weight tiles (>= 512) and an unsplit dW, so the dense kernel's update
    runs as its own launch on the library's second stream with non-temporal accesses (skip_hi, nt = 2) and the main launch
    skips that segment (skip_lo / skip_hi).  Same assertions; with knob 25 = 0 (one stream, one launch) the same bits."""
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    assert lib.dccn_get_tuning(25) == 2
    kw = dict(kin=1096, F=1024, D=260, fused_bwd=False, seed=6, what="large")
    a = run_case(40, **kw)
    try:
        assert lib.dccn_set_tuning(25, 0) == 0
        b = run_case(40, check=False, **kw)
    finally:
        lib.dccn_set_tuning(25, 2)
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)


# ---- the stand-alone optimizer -----------------------------------------------------------------------------------------------
def test_standalone_adam_from_a_resumed_state():
    """dccn_adam_tf_step as test_adam_tf_steps calls it (n = 10007: the arena's tail is no multiple of 4), resumed at step 498
    with non-zero slots, gate 0.25 and a coefficient the guard can see."""
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    dev = lambda a: torch.as_tensor(np.asarray(a, np.float32)).cuda()          # noqa: E731
    rng = np.random.RandomState(5)
    n, gate = 10007, 0.25
    p = {"w": rng.randn(n).astype(np.float32)}
    reg = np.zeros(n, np.float32)
    reg[1000:6000] = 0.2
    reg[n - 3:] = 0.3                                       # (the scalar tail carries a term too)
    st = resumed_state({"w": 0.1}, {"w": (n,)}, rng)
    pt, mt, vt = dev(p["w"]), dev(st.m["w"]), dev(st.v["w"])
    state = dev([float(st.global_step), float(st.beta1_power), float(st.beta2_power), 0.0])
    gt_gate, regt = dev([gate]), dev(reg)
    hp = _lib.AdamHParams.default()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    on = reg > 0
    for it in range(N_STEPS):
        g = {"w": (rng.randn(n) * 0.1).astype(np.float32)}
        assert_guard({"w": p["w"][on]}, {"w": g["w"][on]}, {"w": reg[on]}, gate,
                     O.AdamState({"w": st.m["w"][on]}, {"w": st.v["w"][on]}, st.beta1_power, st.beta2_power, st.global_step))
        p, st, alpha = oracle_step(p, g, {"w": reg}, gate, st)
        _lib.check(lib.dccn_adam_tf_step(pt.data_ptr(), dev(g["w"]).data_ptr(), mt.data_ptr(), vt.data_ptr(), regt.data_ptr(),
                                         gt_gate.data_ptr(), state.data_ptr(), hp, n, s))
        torch.cuda.synchronize()
        sv = state.cpu().numpy()
        assert sv[0] == START_STEP + it + 1 and abs(float(sv[3]) - float(alpha)) <= 1e-6 * float(alpha), (it, sv, alpha)
        assert abs(float(sv[1]) - float(st.beta1_power)) <= 1e-7 and abs(float(sv[2]) - float(st.beta2_power)) <= 1e-7
        for got, ref, name in ((pt, p["w"], "p"), (mt, st.m["w"], "m"), (vt, st.v["w"], "v")):
            assert relerr(got.cpu().numpy(), ref) <= M_TOL, (it, name)


# ---- the equaliser trainer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused-graph", "fused-eager", "composed"])
def test_equaliser_trainer_crosses_the_stair(mode):
    """The equaliser step's own copy of the schedule (equalizer.h prep, the job-table optimizer launch, dccn_adam_tf_step in the
    composed plan): state resumed at step 498, four steps; per step the assertions of test_trainer_step_gradients_and_adam
    (alpha 1e-6 relative, global_step exact, m at 1e-6), the oracle applied to the GPU's own gradients and pre-step slots."""
    from oracle import equalizer_oracle as E
    from test_gpu_equalizer import _trainer
    fused, graph = mode != "composed", mode == "fused-graph"
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer()
    b1p, b2p = beta_powers(START_STEP)
    tr.adam_state.copy_(torch.tensor([float(START_STEP), float(b1p), float(b2p), 0.0]))
    rng = np.random.RandomState(7)
    B = 8
    coef = {n: F32(E.EQ_REG_COEFF * 2 * O.REG_L2) for n in tr.names if "/dense" in n}
    for step in range(N_STEPS):
        x = (rng.standard_normal((B, 7, 80, 2)) * 2).astype(np.float32)
        bits = rng.randint(0, 2, (B, tx.frame_size, 2)).astype(np.int32)
        p0 = tr.get_params()
        m0 = {n: tr.view(n, tr.adam_m).detach().cpu().numpy().copy() for n in tr.names}
        v0 = {n: tr.view(n, tr.adam_v).detach().cpu().numpy().copy() for n in tr.names}
        s0 = tr.adam_state.cpu().numpy().copy()
        tr.train_step(x, bits, fused=fused, graph=graph)
        torch.cuda.synchronize()
        st = O.AdamState(m0, v0, F32(s0[1]), F32(s0[2]), F32(s0[0]))
        _, st_or, alpha = oracle_step(p0, tr.get_grads(), coef, 1.0, st)
        a = tr.adam()
        assert a["global_step"] == START_STEP + step + 1, (step, a)
        assert abs(a["alpha"] - float(alpha)) <= 1e-6 * float(alpha), (step, a["alpha"], alpha)
        assert abs(a["beta1_power"] - float(st_or.beta1_power)) <= 1e-7 and abs(a["beta2_power"] - float(st_or.beta2_power)) <= 1e-7
        for n in tr.names:
            m_or, m_gpu = st_or.m[n].ravel(), tr.view(n, tr.adam_m).detach().cpu().numpy().ravel()
            assert np.abs(m_or - m_gpu).max() <= 1e-6 * max(np.abs(m_or).max(), 1e-30) + 1e-12, (step, n)
    lr_ratio = float(O.learning_rate(F32(START_STEP + N_STEPS - 1)) / O.learning_rate(F32(START_STEP)))
    assert abs(lr_ratio - 0.98) <= 1e-6
