"""CPU check of the stage-by-stage checker of tests/test_gpu_equalizer_stages.py: fed with the float64 intermediates and
gradients of the end-to-end autograd oracle (every intermediate of the whole graph retained) in the place of the GPU's
workspace tensors, every stage must agree to rounding (1e-11) -- i.e. the per-stage formulas, reshapes, upstream-gradient
layouts, the window behind the cyclic prefix, the receiver's crop, the zero prefix of its input gradient and the loss scale
of O.tail_forward_backward are the whole graph's own, at every geometry the GPU cases run; a perturbed intermediate must be
caught by exactly the stages that consume or produce it; and the two margins the GPU cases state stay inside their caps on
the float64 oracle alone, with the cases' own seeds."""
import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E
from oracle.torch_ref import LiteralRx, conv2d_complex_literal
from test_gpu_equalizer import _trainer_config
from test_gpu_equalizer_stages import (GEOMETRY_CASES, H_CAP, KINK_CAP, Stage, _window, check_stages, h_margin, kink_margin)

# (K, CP, cp): N = 64 with the long and the short prefix, N = 128 with the short one (rows of 274 floats)
GEOMETRIES = [(64, 16, True), (64, 16, False), (64, 4, True), (64, 4, False), (128, 9, False)]


def oracle_values(K=64, CP=16, cp=True, B=5, nbits=2, seed=3):
    rng = np.random.RandomState(seed)
    _, tx, c, rc, pe, pr = _trainer_config(nbits, seed, cp=cp, nfft=K, longcp=(4 * CP == K), rx_bias=0.05)
    assert (c.K, c.CP, c.cp) == (K, CP, cp)
    pe = {k: v.astype(np.float64) for k, v in pe.items()}
    pr = {k: v.astype(np.float64) for k, v in pr.items()}
    S, nsc, pc = c.S, c.n_sc, c.pilot_carriers
    lo, kin = _window(c)
    x = rng.standard_normal((B, S, nsc, 2)) * 2
    bits = rng.randint(0, 2, (B, rc.D, nbits)).astype(np.int32)
    lit_rx = LiteralRx(pr, rc, dtype=torch.float64, literal_conv=False)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in pe.items()}
    keep = {}

    def k(name, t):
        t.retain_grad()
        keep[name] = t
        return t
    conv = lambda x5, n, pad: conv2d_complex_literal(x5, P[n + "/kernel"], P[n + "/bias"], pad)      # noqa: E731
    xt = torch.tensor(x, dtype=torch.float64)
    x_norm = k("x_norm", lit_rx.normalise(xt).clone().requires_grad_(True))
    mean = x_norm.mean(dim=(1, 2, 3), keepdim=True)
    var = ((x_norm - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    inv = torch.rsqrt(var + E.LN_EPS)
    ln = k("ln", x_norm * inv + (-mean * inv))
    t1 = k("t1", ln[:, :, lo:lo + kin, :].reshape(B, S, -1) @ P["Equalizer/dense/kernel"] + P["Equalizer/dense/bias"])      # model.py:364-371
    y = k("y", conv(t1.reshape(B, S, K, 1, 2), "Equalizer/conv3d", "valid").permute(0, 1, 3, 2, 4).reshape(B, S, K, 2))
    d1 = k("d1", y.reshape(B, S * K * 2) @ P["Equalizer/dense_1/kernel"] + P["Equalizer/dense_1/bias"])
    d2 = k("d2", d1 @ P["Equalizer/dense_2/kernel"] + P["Equalizer/dense_2/bias"])
    d3 = k("d3", d2 @ P["Equalizer/dense_3/kernel"] + P["Equalizer/dense_3/bias"])
    pre4 = k("pre4", d3 @ P["Equalizer/dense_4/kernel"] + P["Equalizer/dense_4/bias"])
    d4 = k("d4", torch.tanh(pre4))
    h = k("h", conv(d4.reshape(B, S, K, 1, 2), "Equalizer/conv3d_1", "same").reshape(B, S, K, 2))
    yc, hc = torch.view_as_complex(y.contiguous()), torch.view_as_complex(h.contiguous())
    e = yc * (torch.conj(hc) / torch.abs(hc))
    eq = k("eq", torch.view_as_real(e))
    corr = k("corr", torch.view_as_real(torch.view_as_complex(eq.contiguous()) * torch.conj(torch.view_as_complex(eq.contiguous()))))
    eqc = k("eqc", conv(eq.reshape(B, S, K, 1, 2), "Equalizer/conv3d_3", "valid")[:, :, 0, :, :])
    corc = k("corc", conv(corr.reshape(B, S, K, 1, 2), "Equalizer/conv3d_2", "valid")[:, :, 0, :, :])
    cat = k("cat", torch.cat([eqc, corc], dim=-1))
    out_eq = k("out_eq", (cat.reshape(B, S, 4 * K) @ P["Equalizer/dense_5/kernel"] + P["Equalizer/dense_5/bias"]).reshape(B, S, nsc, 2))
    prob, _, z = lit_rx.receiver(out_eq[:, :, lo:, :])              # the frozen receiver crops the prefix itself (model.py:1236-1240)
    z.retain_grad()
    ce_mean, conf, _, _ = lit_rx.losses(prob, bits)
    ce_mean.backward(retain_graph=True)
    v = {n: t.detach().numpy().copy() for n, t in keep.items() if n not in ("pre4", "eqc", "corc")}
    grads = {n: t.grad.numpy().copy() for n, t in keep.items()}      # (copied now: retained gradients accumulate on later calls)
    G = {n: t.grad.numpy().copy() for n, t in P.items()}
    dz = z.grad.numpy().copy()
    g = lambda n: grads[n]      # noqa: E731
    # "deq" of the step is the gradient through the :443 C-Conv alone (eq also feeds the autocorrelation; the equalise
    # stage's backward adds that path itself)
    (deq_direct,) = torch.autograd.grad(eqc, eq, grad_outputs=torch.tensor(grads["eqc"]), retain_graph=True)
    v.update(x=x, snr_db=E.pilot_snr(eq.detach().numpy(), pc), dz=dz, dout=g("out_eq"), deqc=g("eqc"),
             dcorc=g("corc"), deq=deq_direct.numpy().copy(), dcorr=g("corr"), dh=g("h"), dd4=g("pre4"), dd3=g("d3"), dd2=g("d2"),
             dflat=g("y"), dt1=g("t1"))
    # dy = the equalise stage's own contribution to dy (the total, dflat, also carries the pilot branch)
    v["dy"] = v["dflat"] - (g("d1") @ pe["Equalizer/dense_1/kernel"].T).reshape(B, S, K, 2)
    return v, pe, G, c, lit_rx, bits, float(ce_mean.detach()), conf.numpy()


@pytest.fixture(scope="module")
def values():
    """the whole-graph oracle once per geometry, shared and left unchanged (the mutation tests copy what they change)"""
    cache = {}

    def get(K, CP, cp):
        if (K, CP, cp) not in cache:
            cache[(K, CP, cp)] = oracle_values(K, CP, cp)
        return cache[(K, CP, cp)]
    return get


@pytest.mark.parametrize("K,CP,cp", GEOMETRIES)
def test_stage_checker_agrees_with_the_whole_graph_oracle(values, K, CP, cp):
    v, pe, G, c, lit_rx, bits, ce, conf = values(K, CP, cp)
    st = Stage()
    ce2, conf2, _ = check_stages(v, pe, G, c, lit_rx, bits, st)
    worst = max(e for _, e, _ in st.rows)
    assert worst <= 1e-11, sorted(st.rows, key=lambda r: -r[1])[:3]
    assert "tail dz" in [n for n, _, _ in st.rows]
    assert len(st.rows) >= 46 and abs(ce - ce2) <= 1e-14 and np.array_equal(conf, conf2)
    if not cp:                                        # the whole graph leaves exact zeros where the checker demands them
        assert not v["dout"][:, :, :CP, :].any() and v["dout"][:, :, CP:, :].any()
        assert not G["Equalizer/dense_5/kernel"][:, :2 * CP].any() and not G["Equalizer/dense_5/bias"][:2 * CP].any()


def _flagged(v, pe, G, c, lit_rx, bits):
    st = Stage()
    check_stages(v, pe, G, c, lit_rx, bits, st)
    return {n for n, e, tol in st.rows if e > tol}


def test_stage_checker_localises_a_wrong_intermediate():
    v, pe, G, c, lit_rx, bits, _, _ = oracle_values(seed=4)
    v = dict(v)
    v["d3"] = v["d3"] * (1 + 1e-4)                     # one stage's output off by 1e-4
    bad = _flagged(v, pe, G, c, lit_rx, bits)
    assert bad == {":408 dense_3", ":421 dense_4 + tanh", "dense_4 dW", "dense_3 dX"} or \
        bad == {":408 dense_3", ":421 dense_4 + tanh", "dense_4 dW"}, bad


@pytest.mark.parametrize("K,CP,cp", [(64, 16, True), (128, 9, False)])
def test_stage_checker_catches_a_wrong_loss_scale(values, K, CP, cp):
    """dz off by 1e-4 (a loss scale other than 1 / (B D nbits)): the stage that produces dz and the one that consumes it"""
    v, pe, G, c, lit_rx, bits, _, _ = values(K, CP, cp)
    v = dict(v)
    v["dz"] = v["dz"] * (1 + 1e-4)
    assert _flagged(v, pe, G, c, lit_rx, bits) == {"tail dz", "receiver dX (dz -> d equalized)"}


@pytest.mark.parametrize("K,CP,cp", [(64, 16, False), (64, 4, False), (128, 9, False)])
def test_stage_checker_catches_a_shifted_window(values, K, CP, cp):
    """FLAGS.cp off, ln rolled by one sample along the subcarrier axis (a window read one sample off): the stage that produces
    ln and the two that read its window"""
    v, pe, G, c, lit_rx, bits, _, _ = values(K, CP, cp)
    v = dict(v)
    v["ln"] = np.roll(v["ln"], 1, axis=2)
    assert _flagged(v, pe, G, c, lit_rx, bits) == {":363 layer_norm", ":371 dense", "dense dW"}


def test_stage_checker_demands_exact_zeros_in_the_prefix(values):
    v, pe, G, c, lit_rx, bits, _, _ = values(64, 4, False)
    v = dict(v)
    v["dout"] = v["dout"].copy()
    v["dout"][0, 0, 0, 0] = 1e-30                      # far below any relative bar: only the exact check sees it
    assert _flagged(v, pe, G, c, lit_rx, bits) == {"receiver dX: exact zeros in the prefix"}
    G = dict(G, **{"Equalizer/dense_5/bias": G["Equalizer/dense_5/bias"].copy()})
    G["Equalizer/dense_5/bias"][2 * c.CP - 1] = -1e-30
    assert _flagged(v, pe, G, c, lit_rx, bits) == {"receiver dX: exact zeros in the prefix", "dense_5 db: exact zeros in the prefix"}


# the (nbits, frames) pairs of test_fused_step_stage_by_stage_at_1e5 (N = 64, long prefix, FLAGS.cp on, a bias-free receiver)
MARGIN_CASES = dict(GEOMETRY_CASES, **{"%d-%d" % (nbits, B): dict(nbits=nbits, B=B, geometry={})
                                       for nbits, B in ((2, 73), (2, 12), (2, 200), (4, 73), (1, 73))})


@pytest.mark.parametrize("case", sorted(MARGIN_CASES))
def test_margins_of_the_gpu_cases_stay_inside_their_caps(case):
    """every case of tests/test_gpu_equalizer_stages.py with its own seeds, float64 oracle alone: the cells the |h| margin and
    the kink margin leave out are within their caps (3 % each; the GPU's fp32 intermediates move a cell across a margin only
    next to it, the fractions printed here are far from the caps)"""
    cs = MARGIN_CASES[case]
    nbits, B = cs["nbits"], cs["B"]
    _, tx, c, rc, pe, pr = _trainer_config(nbits, 51 + B, **cs["geometry"])
    pe = {k: v.astype(np.float64) for k, v in pe.items()}
    pr = {k: v.astype(np.float64) for k, v in pr.items()}
    rng = np.random.RandomState(300 + B + nbits)
    lo, _ = _window(c)
    batches = [(rng.standard_normal((B, c.S, c.n_sc, 2)) * 2).astype(np.float32)]
    rng.randint(0, 2, (B, tx.frame_size, nbits))                                  # (the labels: drawn to keep the stream in step)
    if cs.get("evaluate"):
        batches.append((rng.standard_normal(batches[0].shape) * 2).astype(np.float32))
    for i, x in enumerate(batches):
        out, _, h = E.equalizer_forward(pe, O.batch_moment_norm(x.astype(np.float64))[0], c)
        left = 1.0 - float(h_margin(h).mean())
        print("%s batch %d: |h| margin leaves out %.4f %%" % (case, i, 100 * left))
        assert left <= H_CAP
        if i == 0:                                     # (the evaluation step runs no backward)
            _, t = O.rx_forward(pr, out[:, :, lo:, :], rc, keep=True)
            left = 1.0 - float(kink_margin(t["pre1"], t["pre2"]).mean())
            print("%s: kink margin leaves out %.4f %%" % (case, 100 * left))
            assert left <= KINK_CAP
