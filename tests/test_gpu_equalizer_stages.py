"""Stage-by-stage parity of the FUSED equaliser training step (dccn_eq_train_step: what receiver_mp / config 5 run) at
north_star's tolerance: every stage of ``equalizer_ofdm`` (dev/py/model.py:349-478) is compared with the float64 oracle
evaluated on the GPU's OWN inputs to that stage -- forward, input gradient and parameter gradients -- to **1e-5 of the
reference tensor's scale**, the way tests/test_gpu_engine.py checks the basic receiver (an end-to-end fp32-vs-fp64 comparison
through twelve layers measures the conditioning of the chain, 5e-5..3e-4 here, not any kernel; test_gpu_equalizer.py keeps the
end-to-end direction check, cosine >= 1 - 1e-6).

The GPU's stage inputs are the step's own intermediates, read out of its workspace through dccn_eq_workspace_tensor
(include/dccn.h); the oracle side is oracle/equalizer_oracle.py (NumPy, literal tap-by-tap C-Conv) for the forward stages and
float64 autograd over oracle/torch_ref.py::conv2d_complex_literal (the zero-padded conv3d formulation) for the gradients.
Every extent comes from the case's EqConfig: N = 64 and 128, the long and the short cyclic prefix, FLAGS.cp on and off (the
first dense layer and the frozen receiver then read the K-sample window behind the prefix, and nothing flows back into it).

Stated margins (everything else is held to 1e-5 flat):
  * equalise (:431-438) divides by |h|: cells with |h| below 2 % of the batch's median |h| are left out of the comparison of
    that stage's outputs and gradients (d(1/|h|) ~ 1/|h|^2 amplifies the GPU's own 6e-8 input rounding past any fixed bar);
  * Equalizer/conv3d_1/bias is d = sum_c (dbe[2c] - dbe[2c+1]), a difference of two nearly equal sums: it is held to 1e-5 of
    the SUM OF MAGNITUDES of its terms (the forward error bound of a float32 sum), not of the cancelled result;
  * tail dz (the frozen receiver's tail backward, z -> dz, with the loss scale 1 / (B D nbits)): the derivative of a leaky ReLU
    jumps 1 <-> 0.2 at zero, and the step's fp32 z is within about 1e-6 of its scale of the float64 z the reference starts
    from, so a pre-activation that close to zero may fall on the other side.  Cells with a hidden pre-activation below
    1e-4 max|pre1| or a logit below 1e-4 max|pre2| (the oracle's own pre1 / pre2: two orders above that distance) are left
    out, at most 3 % of the cells (asserted, the count is printed).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E
from oracle.torch_ref import LiteralRx, conv2d_complex_literal

pytestmark = pytest.mark.gpu
TOL = 1e-5
H_MARGIN, H_CAP = 0.02, 0.03              # |h| below 2 % of the median; at most 3 % of the cells
KINK_MARGIN, KINK_CAP = 1e-4, 0.03        # |pre| below 1e-4 of its maximum; at most 3 % of the cells
TAIL_NAMES = ("demodulation/conv2d/kernel", "demodulation/conv2d/bias", "demodulation/dense_1/kernel", "demodulation/dense_1/bias")


def rel(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    s = float(np.abs(want).max()) if scale is None else float(scale)
    return float(np.abs(got - want).max()) / max(s, 1e-300)


class Stage:
    """collects (name, error) and asserts them together, so one run shows every stage's margin"""

    def __init__(self):
        self.rows = []

    def check(self, name, got, want, scale=None, tol=TOL):
        self.rows.append((name, rel(got, want, scale), tol))

    def finish(self):
        bad = ["%s %.2e > %.0e" % r for r in self.rows if not r[1] <= r[2]]
        print("\n".join("%-34s %.2e" % (n, e) for n, e, _ in self.rows))
        print("worst stage: %-34s %.2e" % max(((n, e) for n, e, _ in self.rows), key=lambda r: r[1]))
        assert not bad, "; ".join(bad)


def _trainer(nbits, B, seed, **geometry):
    from test_gpu_equalizer import _trainer as mk
    return mk(nbits=nbits, seed=seed, **geometry)


def _ws(tr, pl, name, train=1):
    off, cnt = C.c_size_t(), C.c_size_t()
    rc = tr.lib.dccn_eq_workspace_tensor(C.byref(pl.shape), train, name.encode(), C.byref(off), C.byref(cnt))
    assert rc == 0, (name, rc)
    t = pl.ws[off.value:off.value + 4 * cnt.value].view(torch.float32)
    return t.cpu().numpy().astype(np.float64)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def _vjp(fn, inputs, upstream):
    """float64 autograd: gradients of sum(fn(*inputs) * upstream) with respect to every input"""
    ts = [_t(a, True) for a in inputs]
    out = fn(*ts)
    gs = torch.autograd.grad(out, ts, grad_outputs=_t(upstream), allow_unused=True)
    return [None if g is None else g.numpy() for g in gs]


def h_margin(h):
    """cells the equalise stage is compared on: |h| at least 2 % of the batch's median (h: [B,S,K,2])"""
    habs = np.sqrt((h ** 2).sum(-1))
    return habs >= H_MARGIN * np.median(habs)


def kink_margin(pre1, pre2):
    """cells (rows of pre1 [cells, m] / pre2 [cells, 2 nbits]) the tail's backward is compared on: no pre-activation within
    1e-4 of its tensor's largest magnitude of the leaky-ReLU kink"""
    return (np.abs(pre1) >= KINK_MARGIN * np.abs(pre1).max()).all(axis=1) & \
           (np.abs(pre2) >= KINK_MARGIN * np.abs(pre2).max()).all(axis=1)


def _window(ecfg):
    """(first sample, number of samples) of a row that the first dense layer and the frozen receiver read (model.py:364-366,
    1236-1240): the whole row, or the K samples behind the cyclic prefix"""
    return (0, ecfg.n_sc) if ecfg.cp else (ecfg.CP, ecfg.K)


def _cconv_1k(P, B, S, K):
    def f(inp, name):                   # (1,K) valid C-Conv of [B,S,K,2] -> [B,S,K(filters),2]  (:378-380, :439-449)
        o = O.layers_conv2d_complex_literal(inp.reshape(B, S, K, 1, 2), P[name + "/kernel"], P[name + "/bias"], (1, 1), "valid")
        return o[:, :, 0, :, :]
    return f


def check_forward(v, P, ecfg, lit_rx, bits, st):
    """the forward stages on the values `v` holds for their inputs (R0 through dense_5, the pilot SNR), then the frozen receiver
    in float64 on v["out_eq"].  Returns what check_backward and the callers need of it: the equalise margin's cells, out_eq as
    the autograd leaf, the receiver's z, and the oracle's (ce_mean, confusion matrix, number of near-tie decisions)."""
    S, K, nsc = ecfg.S, ecfg.K, ecfg.n_sc
    lo, kin = _window(ecfg)
    B = v["x"].shape[0]
    R, SK2, K2, N2 = B * S, S * K * 2, 2 * K, 2 * nsc
    assert lit_rx.cfg.kin == kin and lit_rx.cfg.S == S, (lit_rx.cfg, ecfg)

    x_norm = v["x_norm"].reshape(B, S, nsc, 2)
    st.check("R0 batch-moment norm", x_norm, O.batch_moment_norm(v["x"].astype(np.float64))[0])
    ln = v["ln"].reshape(B, S, nsc, 2)
    st.check(":363 layer_norm", ln, E.layer_norm(x_norm))
    t1 = v["t1"].reshape(R, K2)
    st.check(":371 dense", t1, ln[:, :, lo:lo + kin, :].reshape(R, 2 * kin) @ P["Equalizer/dense/kernel"] + P["Equalizer/dense/bias"])
    y = v["y"].reshape(B, S, K, 2)
    cconv_1k = _cconv_1k(P, B, S, K)
    st.check(":378 C-Conv (1,K)", y, cconv_1k(t1.reshape(B, S, K, 2), "Equalizer/conv3d"))
    d1, d2 = v["d1"].reshape(B, -1), v["d2"].reshape(B, SK2)
    st.check(":394 dense_1 (pilots)", d1, y.reshape(B, SK2) @ P["Equalizer/dense_1/kernel"] + P["Equalizer/dense_1/bias"])
    st.check(":402 dense_2", d2, d1 @ P["Equalizer/dense_2/kernel"] + P["Equalizer/dense_2/bias"])
    d3, d4 = v["d3"].reshape(B, SK2), v["d4"].reshape(B, SK2)
    st.check(":408 dense_3", d3, d2 @ P["Equalizer/dense_3/kernel"] + P["Equalizer/dense_3/bias"])
    st.check(":421 dense_4 + tanh", d4, np.tanh(d3 @ P["Equalizer/dense_4/kernel"] + P["Equalizer/dense_4/bias"]))
    h = v["h"].reshape(B, S, K, 2)
    h_ref = O.layers_conv2d_complex_literal(d4.reshape(B, S, K, 1, 2), P["Equalizer/conv3d_1/kernel"],
                                            P["Equalizer/conv3d_1/bias"], (1, 1), "same")[:, :, :, 0, :]
    st.check(":428 C-Conv (S,K) same", h, h_ref)
    eq, corr = v["eq"].reshape(B, S, K, 2), v["corr"].reshape(B, S, K, 2)
    ok = h_margin(h)                                      # stated margin: cells next to the 1/|h| pole
    # (how many cells the margin leaves out: printed so that the number is on record -- DESIGN.md section 4 quotes it)
    print("equalise margin: %d of %d cells (%.4f %%) below 2 %% of the median |h| left out [B=%d]"
          % (int((~ok).sum()), ok.size, 100.0 * float((~ok).mean()), B))
    assert ok.mean() > 1.0 - H_CAP
    eq_ref, corr_ref = E.equalize(y, h)
    st.check(":431-436 equalise", eq[ok], eq_ref[ok])
    st.check(":438 autocorrelation", corr[ok], corr_ref[ok])
    cat = v["cat"].reshape(B, S, K, 4)
    st.check(":443 C-Conv of eq -> cat", cat[..., 0:2], cconv_1k(eq, "Equalizer/conv3d_3"))
    st.check(":439 C-Conv of corr -> cat", cat[..., 2:4], cconv_1k(corr, "Equalizer/conv3d_2"))
    out_eq = v["out_eq"].reshape(B, S, nsc, 2)
    st.check(":458 dense_5", out_eq.reshape(R, N2), cat.reshape(R, 4 * K) @ P["Equalizer/dense_5/kernel"] + P["Equalizer/dense_5/bias"])
    snr_ref = E.pilot_snr(eq, ecfg.pilot_carriers)
    st.check(":465-475 pilot SNR", v["snr_db"].reshape(B, 1), snr_ref, scale=max(np.abs(snr_ref).max(), 1.0))

    # ---- the frozen receiver (on the window behind the prefix when FLAGS.cp is off): loss and decisions ---------------
    o_t = _t(out_eq, True)
    prob, _, z = lit_rx.receiver(o_t[:, :, lo:, :])
    ce_mean, conf, _, _ = lit_rx.losses(prob, bits)
    pr = prob.detach().numpy().reshape(-1, 2)
    return dict(ok=ok, o_t=o_t, z=z, ce_mean=float(ce_mean.detach()), conf=conf.numpy(),
                ties=int((np.abs(pr[:, 1] - pr[:, 0]) < 2e-5).sum()))


def check_backward(v, P, G, ecfg, lit_rx, bits, st, fw):
    """the backward stages, last stage first, each on the GPU's own upstream gradient; fw: what check_forward returned for
    the same values"""
    S, K, nsc, CP = ecfg.S, ecfg.K, ecfg.n_sc, ecfg.CP
    lo, kin = _window(ecfg)
    B = v["x"].shape[0]
    R, SK2, K2, N2 = B * S, S * K * 2, 2 * K, 2 * nsc
    D, nbits = lit_rx.cfg.D, lit_rx.cfg.nbits
    ok, o_t, z = fw["ok"], fw["o_t"], fw["z"]
    ln, t1, y = v["ln"].reshape(B, S, nsc, 2), v["t1"].reshape(R, K2), v["y"].reshape(B, S, K, 2)
    d1, d2, d3, d4 = v["d1"].reshape(B, -1), v["d2"].reshape(B, SK2), v["d3"].reshape(B, SK2), v["d4"].reshape(B, SK2)
    h, eq, corr = v["h"].reshape(B, S, K, 2), v["eq"].reshape(B, S, K, 2), v["corr"].reshape(B, S, K, 2)
    cat = v["cat"].reshape(B, S, K, 4)

    # ---- the frozen receiver's tail: z -> dz, loss scale included.  The fused dense + tail routes store no z, so the stage
    # starts from the float64 z of the GPU's own out_eq (the nearest tensor every route materialises)
    tl = O.tail_forward_backward(z.detach().numpy().reshape(B * D, 2), np.asarray(bits).reshape(B * D, nbits),
                                 *[lit_rx.p[n].detach().numpy() for n in TAIL_NAMES], nbits)
    keep = kink_margin(tl["pre1"], tl["pre2"])
    print("kink margin: %d of %d cells (%.4f %%) within 1e-4 of a leaky-ReLU kink left out [B=%d, nbits=%d]"
          % (int((~keep).sum()), keep.size, 100.0 * float((~keep).mean()), B, nbits))
    assert (~keep).mean() <= KINK_CAP
    st.check("tail dz", v["dz"].reshape(B * D, 2)[keep], tl["dz"][keep])

    # ---- the receiver's linear part, on the GPU's dz: the gradient handed to the equaliser --------------------------------
    dout = v["dout"].reshape(B, S, nsc, 2)
    (dout_ref,) = torch.autograd.grad(z, o_t, grad_outputs=_t(v["dz"].reshape(z.shape)))
    dout_ref = dout_ref.numpy()
    st.check("receiver dX (dz -> d equalized)", dout, dout_ref)
    if lo:
        # nothing flows back into the cyclic-prefix samples: exact zeros there, and through them in the prefix columns of
        # dense_5's gradients (eq_issue_backward: "the zero rows of Mf leave zeros in the cyclic-prefix samples")
        # (asserted with the other stages by Stage.finish, at tolerance 0 on an absolute scale: any non-zero value fails)
        assert not dout_ref[:, :, :lo, :].any()
        for name, got in (("receiver dX: exact zeros in the prefix", dout[:, :, :lo, :]),
                          ("dense_5 dW: exact zeros in the prefix", G["Equalizer/dense_5/kernel"][:, :2 * lo]),
                          ("dense_5 db: exact zeros in the prefix", G["Equalizer/dense_5/bias"][:2 * lo])):
            st.check(name, got, np.zeros_like(got), scale=1.0, tol=0.0)

    do2 = dout.reshape(R, N2)
    dcat_ref = (do2 @ P["Equalizer/dense_5/kernel"].T).reshape(B, S, K, 4)
    deqc, dcorc = v["deqc"].reshape(B, S, K, 2), v["dcorc"].reshape(B, S, K, 2)
    st.check("dense_5 dX -> d(C-Conv eq)", deqc, dcat_ref[..., 0:2], scale=np.abs(dcat_ref).max())
    st.check("dense_5 dX -> d(C-Conv corr)", dcorc, dcat_ref[..., 2:4], scale=np.abs(dcat_ref).max())
    st.check("dense_5 dW", G["Equalizer/dense_5/kernel"], cat.reshape(R, 4 * K).T @ do2)
    st.check("dense_5 db", G["Equalizer/dense_5/bias"], do2.sum(0))

    def conv_fn(padding):
        return lambda inp, kern, bias: conv2d_complex_literal(inp, kern, bias, padding)

    def bias_scale(gb, up):
        # the bias pair (ba - bb, bb - ba) of complex.py:187-188: db = +-sum(d re - d im), a signed sum over every row --
        # held to 1e-5 of its value or of 1e-3 of the sum of magnitudes, whichever is larger (cancellation)
        return max(np.abs(gb).max(), np.abs(up).sum() * 1e-3)
    deq, dcorr = v["deq"].reshape(B, S, K, 2), v["dcorr"].reshape(B, S, K, 2)
    for tag, name, inp, up, dx_gpu in (("eq", "Equalizer/conv3d_3", eq, deqc, deq), ("corr", "Equalizer/conv3d_2", corr, dcorc, dcorr)):
        # input [B,S,K,1,2] -> output [B,S,1,K,2]: the upstream gradient is indexed by filter on the last-but-one axis
        gx, gk, gb = _vjp(conv_fn("valid"), [inp.reshape(B, S, K, 1, 2), P[name + "/kernel"], P[name + "/bias"]],
                          up.reshape(B, S, 1, K, 2))
        st.check("C-Conv(%s) dX" % tag, dx_gpu, gx.reshape(B, S, K, 2))
        st.check("C-Conv(%s) dW" % tag, G[name + "/kernel"], gk)
        st.check("C-Conv(%s) db" % tag, G[name + "/bias"], gb, scale=bias_scale(gb, up))

    def equalize_t(yt, ht):
        yc, hc = torch.view_as_complex(yt.contiguous()), torch.view_as_complex(ht.contiguous())
        hn = torch.conj(hc) / torch.abs(hc)
        e = yc * hn
        return torch.cat([torch.view_as_real(e), torch.view_as_real(e * torch.conj(e))], dim=-1)
    dy, dh = v["dy"].reshape(B, S, K, 2), v["dh"].reshape(B, S, K, 2)
    gy, gh = _vjp(equalize_t, [y, h], np.concatenate([deq, dcorr], axis=-1))
    st.check("equalise dy", dy[ok], gy[ok])
    st.check("equalise dh", dh[ok], gh[ok])

    dd4 = v["dd4"].reshape(B, SK2)
    gd4, gk1, gb1 = _vjp(conv_fn("same"), [d4.reshape(B, S, K, 1, 2), P["Equalizer/conv3d_1/kernel"], P["Equalizer/conv3d_1/bias"]],
                         dh.reshape(B, S, K, 1, 2))
    st.check("C-Conv (S,K) dX . tanh'", dd4, gd4.reshape(B, SK2) * (1.0 - d4 ** 2))
    st.check("C-Conv (S,K) dW", G["Equalizer/conv3d_1/kernel"], gk1)
    st.check("C-Conv (S,K) db", G["Equalizer/conv3d_1/bias"], gb1, scale=np.abs(dh).sum())      # stated margin (cancellation)
    dd3, dd2 = v["dd3"].reshape(B, SK2), v["dd2"].reshape(B, SK2)
    st.check("dense_4 dX", dd3, dd4 @ P["Equalizer/dense_4/kernel"].T)
    st.check("dense_4 dW", G["Equalizer/dense_4/kernel"], d3.T @ dd4)
    st.check("dense_4 db", G["Equalizer/dense_4/bias"], dd4.sum(0))
    st.check("dense_3 dX", dd2, dd3 @ P["Equalizer/dense_3/kernel"].T)
    st.check("dense_3 dW", G["Equalizer/dense_3/kernel"], d2.T @ dd3)
    st.check("dense_3 db", G["Equalizer/dense_3/bias"], dd3.sum(0))
    # pilot bottleneck (dense_2 then dense_1 backwards, one launch per direction in the default plan); its input gradient
    # lands on top of the equalise stage's dy: dflat = total gradient of y
    dd1_ref = dd2 @ P["Equalizer/dense_2/kernel"].T
    dflat = v["dflat"].reshape(B, S, K, 2)
    st.check("bottleneck dX + dy", dflat.reshape(B, SK2), dy.reshape(B, SK2) + dd1_ref @ P["Equalizer/dense_1/kernel"].T)
    st.check("dense_2 dW", G["Equalizer/dense_2/kernel"], d1.T @ dd2)
    st.check("dense_2 db", G["Equalizer/dense_2/bias"], dd2.sum(0))
    st.check("dense_1 dW", G["Equalizer/dense_1/kernel"], y.reshape(B, SK2).T @ dd1_ref)
    st.check("dense_1 db", G["Equalizer/dense_1/bias"], dd1_ref.sum(0))
    dt1 = v["dt1"].reshape(R, K2)
    gt1, gk0, gb0 = _vjp(conv_fn("valid"), [t1.reshape(B, S, K, 1, 2), P["Equalizer/conv3d/kernel"], P["Equalizer/conv3d/bias"]],
                         dflat.reshape(B, S, 1, K, 2))
    st.check("C-Conv (1,K) dX", dt1, gt1.reshape(R, K2))
    st.check("C-Conv (1,K) dW", G["Equalizer/conv3d/kernel"], gk0)
    st.check("C-Conv (1,K) db", G["Equalizer/conv3d/bias"], gb0, scale=bias_scale(gb0, dflat))
    st.check("dense dW", G["Equalizer/dense/kernel"], ln[:, :, lo:lo + kin, :].reshape(R, 2 * kin).T @ dt1)
    st.check("dense db", G["Equalizer/dense/bias"], dt1.sum(0))


def check_stages(v, P, G, ecfg, lit_rx, bits, st):
    """every stage of the step on the values `v` holds for its inputs (v: name -> float64 array, the names of
    dccn_eq_workspace_tensor + "x", "h", "out_eq", "snr_db"); P / G: parameters the step ran with / gradients it left
    (TF shapes).  Returns the oracle's (ce_mean, confusion matrix, number of near-tie decisions) of the frozen receiver on
    v["out_eq"]."""
    fw = check_forward(v, P, ecfg, lit_rx, bits, st)
    check_backward(v, P, G, ecfg, lit_rx, bits, st, fw)
    return fw["ce_mean"], fw["conf"], fw["ties"]


FWD_NAMES = ("x_norm", "ln", "t1", "y", "d1", "d2", "d3", "d4", "eq", "corr", "cat")
WS_NAMES = FWD_NAMES + ("dz", "dout", "deqc", "dcorc", "deq", "dcorr", "dy", "dh", "dd4", "dd3", "dd2", "dflat", "dt1")


def _outputs(v, pl):
    v["h"] = pl.chest.detach().cpu().numpy().astype(np.float64)
    v["out_eq"] = pl.out_eq.detach().cpu().numpy().astype(np.float64)
    v["snr_db"] = pl.snr_db.detach().cpu().numpy().astype(np.float64)
    return v


def _check_metrics(m, ce_mean, conf, ties):
    assert abs(m["ce_mean"] - ce_mean) <= TOL * abs(ce_mean), (m["ce_mean"], ce_mean)
    # hard decisions: exact outside a 1e-5 probability margin (|p1 - p0| < 2e-5: float32 and float64 may fall on either side
    # of a tie; such a cell moves one count between two cells of a row of the confusion matrix)
    got = np.asarray(m["conf"]).reshape(2, 2)
    assert got.sum() == conf.sum() and np.array_equal(got.sum(1), conf.sum(1))
    assert np.abs(got - conf).sum() <= 2 * ties, (got, conf, ties)


def eq_shape(B, ecfg, rcfg):
    from dl_ofdm_amd import _lib
    return _lib.EqShape(B, ecfg.S, ecfg.K, ecfg.CP, 1 if ecfg.cp else 0, rcfg.F, rcfg.D, rcfg.nbits, ecfg.pilot_size,
                        len(ecfg.pilot_carriers))


def route_of(lib, B, ecfg, rcfg):
    """what the library's own queries (host only) say a training step of this shape launches, under the knobs set now:
    rides: `input:0` by the single-pass kernel (else the multi-launch norm); bn: the shape of the pilot bottleneck fits its
    one-launch-per-direction kernels (the shape alone: the launch-per-stage plan runs GEMM launches all the same); group:
    rides and bn and the few-row receiver folded into one matrix; tail / tail_eval: the receiver's dense layer and tail as
    one launch (training / evaluation instantiation); splits: split counts of the weight gradients of (dense, dense_5, the
    SK2 x SK2 layers, dense_1, dense_2) as stand-alone GEMMs of these shapes (dccn_gemm_route_query); fold_k: the folded
    matrix's row count S * 2 n_sc, read back from dccn_eq_rx_folded_floats; window: byte offset, modulo 16, of the window
    behind the prefix"""
    from dl_ofdm_amd import _lib
    sh = eq_shape(B, ecfg, rcfg)
    rsh = _lib.RxShape(B, rcfg.S, rcfg.kin, rcfg.F, rcfg.D, rcfg.nbits)
    SK2, dN = ecfg.S * ecfg.K * 2, 2 * rcfg.D
    R, K2, N2, Pp = B * ecfg.S, 2 * ecfg.K, 2 * ecfg.n_sc, 2 * ecfg.pilot_size

    def splits(op, m, k, n):
        gr = _lib.GemmRoute()
        assert lib.dccn_gemm_route_query(_lib.ROUTE_OPS[op], m, k, n, 0, 0, C.byref(gr)) == 0, (op, m, k, n)
        return int(gr.splits)
    n = int(lib.dccn_eq_rx_folded_floats(C.byref(sh)))
    assert (n - dN) % dN == 0
    return dict(rides=int(lib.dccn_eq_norm_rides(C.byref(sh))), bn=int(lib.dccn_eq_bottleneck_supported(B, SK2, Pp)),
                group=int(lib.dccn_eq_group_supported(C.byref(sh))), tail=int(lib.dccn_rx_dense_tail_fused(C.byref(rsh), 1)),
                tail_eval=int(lib.dccn_rx_dense_tail_fused(C.byref(rsh), 0)),
                splits=(splits("dense_bwd_w", R, 2 * _window(ecfg)[1], K2), splits("dense_bwd", R, 4 * ecfg.K, N2),
                        splits("dense_bwd", B, SK2, SK2), splits("dense_bwd", B, SK2, Pp), splits("dense_bwd", B, Pp, SK2)),
                fold_k=(n - dN) // dN, window=(0 if ecfg.cp else 8 * ecfg.CP) % 16)


def run_case(nbits, B, plan, knobs, geometry=None, route=None, evaluate=False):
    """one training step of the planned sequence under tuning key 20 = plan and the further keys `knobs` (set before the
    trainer builds its plan and put back whatever happens), every stage against the oracle; geometry: keyword arguments of
    test_gpu_equalizer._trainer (nfft, longcp, cp, rx_bias); route: what route_of must answer for the case, asserted before
    the step is issued; evaluate: also one evaluation step on a second batch, its forward stages, ce_mean and decisions"""
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    geometry = dict(geometry or {})
    saved = {k: lib.dccn_get_tuning(k) for k in knobs}
    ev = None
    try:
        for k, val in knobs.items():
            assert lib.dccn_set_tuning(k, val) == 0, (k, val)
        F, tx, ecfg, rcfg, pe, pr, tr = _trainer(nbits, B, seed=51 + B, **geometry)
        rng = np.random.RandomState(300 + B + nbits)
        x = (rng.standard_normal((B, ecfg.S, ecfg.n_sc, 2)) * 2).astype(np.float32)
        bits = rng.randint(0, 2, (B, tx.frame_size, nbits)).astype(np.int32)
        shp = E.param_shapes(ecfg)
        P = {n: a.astype(np.float64).reshape(shp[n]) for n, a in tr.get_params().items()}     # the step's own parameters
        try:
            assert lib.dccn_set_tuning(20, plan) == 0
            if route is not None:
                got = route_of(lib, B, ecfg, rcfg)
                assert got == route, "route: the library answers %r, the case expects %r" % (got, route)
            tr.train_step(x, bits, fused=True, graph=False)
            torch.cuda.synchronize()
            pl = tr._plan(B)
            m_train = dict(tr.last)
            G = {n: a.astype(np.float64).reshape(shp[n]) for n, a in tr.get_grads().items()}      # without the L2 term (reg_coef)
            v = _outputs({n: _ws(tr, pl, n) for n in WS_NAMES}, pl)
            if evaluate:
                # the evaluation plan on a second batch, with the parameters the training step left: no riding normalisation,
                # the evaluation instantiations of the tail and of dense + tail.  Every forward tensor the checker reads is
                # written by eq_issue_forward on this plan too (x_norm .. cat into the workspace, carved without the
                # training-only tensors: the names are looked up again; chest / out_eq / snr_db into the caller's buffers),
                # so no stage has to be checked together with the next one; eq_issue_rx stores no z where dense + tail are
                # one launch (tail_eval of the case's route), and the forward half does not read it
                x2 = (rng.standard_normal(x.shape) * 2).astype(np.float32)
                bits2 = rng.randint(0, 2, bits.shape).astype(np.int32)
                P2 = {n: a.astype(np.float64).reshape(shp[n]) for n, a in tr.get_params().items()}
                m_eval = dict(tr.eval_step(x2, bits2, fused=True, graph=False))
                torch.cuda.synchronize()
                v2 = _outputs({n: _ws(tr, pl, n, train=0) for n in FWD_NAMES}, pl)
                v2["x"] = x2
                ev = (v2, P2, bits2, m_eval)
        finally:
            lib.dccn_set_tuning(20, 1)
    finally:
        for k, val in saved.items():
            lib.dccn_set_tuning(k, val)
    assert all(lib.dccn_get_tuning(k) == val for k, val in saved.items()) and lib.dccn_get_tuning(20) == 1
    v["x"] = x
    if plan != 1:
        # without the fused bottleneck the pilot branch's input gradient is a GEMM of its own: it lands in "dflat" and is
        # then either added onto "dy" in place (dy = total, dflat = branch) or the sum rides on that GEMM's store (dflat =
        # total, dy untouched: the layout of the shipped plan).  Bring the first form to the second.
        SK2 = ecfg.S * ecfg.K * 2
        branch = (v["dd2"].reshape(B, SK2) @ P["Equalizer/dense_2/kernel"].T) @ P["Equalizer/dense_1/kernel"].T
        if rel(v["dflat"].reshape(B, SK2), branch) < 1e-3:
            total = v["dy"]
            v["dy"] = total - v["dflat"]
            v["dflat"] = total
    lit_rx = LiteralRx({k: a.astype(np.float64) for k, a in pr.items()}, rcfg, dtype=torch.float64, literal_conv=False)
    st = Stage()
    ce_mean, conf, ties = check_stages(v, P, G, ecfg, lit_rx, bits, st)
    st.finish()
    _check_metrics(m_train, ce_mean, conf, ties)
    if ev is not None:
        v2, P2, bits2, m_eval = ev
        st2 = Stage()
        fw = check_forward(v2, P2, ecfg, lit_rx, bits2, st2)
        print("evaluation step:")
        st2.finish()
        _check_metrics(m_eval, fw["ce_mean"], fw["conf"], fw["ties"])


def _case(nbits, B, plan, knobs=None):
    """(a case without knobs keeps the id it always had: nbits-B-plan)"""
    knobs = dict(knobs or {})
    return pytest.param(nbits, B, plan, knobs, id="-".join(["%d-%d-%d" % (nbits, B, plan)] + ["k%d=%d" % kv for kv in sorted(knobs.items())]))


# knobs (all on the shipped plan): 21 = 0: the skinny 16x64 tiles carry the tanh / equalise stages, the few-row dense backward
# runs launch_dense_bwd16 with the tanh-gradient / add stage; with 19 = 0 the stages are launches of their own; 17 = 0: dX and
# dW of the few-row backward as two launches; 8 = 0: no skinny / few-row tiles at all; 24: the Adam riders of the bottleneck
# backward launch; at 200 frames 19 = 1 / 0: the k-major grouped launch without the tanh-gradient / add column maps
@pytest.mark.parametrize("nbits,B,plan,knobs", [
    _case(2, 73, 1), _case(2, 12, 1), _case(2, 200, 1), _case(4, 73, 1), _case(2, 73, 0), _case(2, 73, 3), _case(2, 200, 0), _case(1, 73, 1),
    _case(2, 73, 1, {21: 0}), _case(2, 73, 1, {21: 0, 19: 0}), _case(2, 73, 1, {17: 0}), _case(2, 73, 1, {8: 0}),
    _case(2, 73, 1, {24: 0}), _case(2, 73, 1, {24: 2}), _case(2, 73, 1, {24: 3}), _case(2, 73, 1, {24: 4}),
    _case(2, 200, 1, {19: 1}), _case(2, 200, 1, {19: 0})])
def test_fused_step_stage_by_stage_at_1e5(nbits, B, plan, knobs):
    """plan = tuning key 20: 1 the shipped launch plan (few-row tiles, fused pilot bottleneck, grouped C-Conv pairs, job-table
    optimizer launch), 0 the launch-per-stage plan, 3 the re-plan without the fused bottleneck; 73 frames = the reference's
    training batch (few-row kernels, folded receiver), 200 = split-K gradients, 12 = direct ones.  knobs: further tuning keys,
    set before the trainer builds its plan and put back whatever happens.  N = 64, the long prefix, FLAGS.cp on."""
    run_case(nbits, B, plan, knobs)


# ---- the other geometries of the reference driver's grid (cp x longcp, N = 64 and 128): each case starts from its route ----
# route_of's answers, from the predicates of csrc/eq_step.h (row = 2 (K + CP) floats, cols = S rows):
#   rides  the single-pass norm: cols % 4 == 0 (and a re-plan: key 20 != 0)
#   bn     one launch per direction for P = 2 pilots in {16, 32}: 32 at N = 64, 64 at N = 128
#   group  1 only where the few-row receiver (B <= 96, S * 2F <= 1152) is folded into one matrix (fold_k % 16 == 0, <= 1152)
#          on top of rides and bn
#   tail   dense + tail as one launch on the receiver's own dense layer: every modulation in evaluation, all but 16-QAM in
#          training (few-row steps with 8-QAM / 16-QAM then run the stand-alone tail all the same: eq_step_plan, cls_fused)
#   splits what dccn_gemm_route_query answers; 1: a direct gradient.  Row layers (dense, dense_5: B S rows) split from 19
#          frames on, the frame layers from 129 (N = 64: all three kinds; N = 128: dense_1 / dense_2 only)
# The expected values are the queries' own answers where they differ from what the predicates suggested beforehand (tail at
# 16-QAM, the split onsets): a case that falls onto another route than the one written here fails before its step is issued.
def _geo(nfft, longcp, cp):
    return dict(nfft=nfft, longcp=longcp, cp=cp, rx_bias=0.05)


GEOMETRY_CASES = {
    # a: window reads at 128 B, folded few-row receiver, zero prefix in dout
    "a": dict(nbits=2, B=73, plan=1, geometry=_geo(64, True, False), evaluate=True,
              route=dict(rides=1, bn=1, group=1, tail=1, tail_eval=1, splits=(4, 4, 1, 1, 1), fold_k=1120, window=0)),
    # b: window + split-K gradients in every layer; no few-row receiver (200 > 96 frames): the general dense forward at
    # kin = 64 and the stand-alone quad-lane tail (the query: a 16-QAM training step has no dense + tail launch; z is stored)
    "b": dict(nbits=4, B=200, plan=1, geometry=_geo(64, True, False),
              route=dict(rides=1, bn=1, group=0, tail=0, tail_eval=1, splits=(11, 11, 2, 2, 2), fold_k=1120, window=0)),
    # c: 136-float rows, few-row receiver NOT folded (952 % 16 = 8): its own C-Conv launch at ld = 2 n_sc
    "c": dict(nbits=2, B=73, plan=1, geometry=_geo(64, False, True), evaluate=True,
              route=dict(rides=1, bn=1, group=0, tail=1, tail_eval=1, splits=(4, 4, 1, 1, 1), fold_k=952, window=0)),
    # d: 32 B window, 8-QAM: few-row dense + stand-alone tail (z is stored here)
    "d": dict(nbits=3, B=73, plan=1, geometry=_geo(64, False, False),
              route=dict(rides=1, bn=1, group=0, tail=1, tail_eval=1, splits=(4, 4, 1, 1, 1), fold_k=952, window=0)),
    # e: direct gradients, BPSK
    "e": dict(nbits=1, B=12, plan=1, geometry=_geo(64, False, True),
              route=dict(rides=1, bn=1, group=0, tail=1, tail_eval=1, splits=(1, 1, 1, 1, 1), fold_k=952, window=0)),
    # f: 274-float rows (masked loaders), multi-launch norm (1918 % 4 = 2), bottleneck as GEMMs, no few-row receiver
    "f": dict(nbits=2, B=12, plan=1, geometry=_geo(128, False, True), evaluate=True,
              route=dict(rides=0, bn=0, group=0, tail=1, tail_eval=1, splits=(1, 1, 1, 1, 1), fold_k=1918, window=0)),
    # g: the 72 B window that is not 16-byte aligned; 16-QAM: dense, then the stand-alone tail in training, one launch in
    # evaluation
    "g": dict(nbits=4, B=12, plan=1, geometry=_geo(128, False, False), evaluate=True,
              route=dict(rides=0, bn=0, group=0, tail=0, tail_eval=1, splits=(1, 1, 1, 1, 1), fold_k=1918, window=8)),
    # h: unaligned split-K slabs (dense_5's 274-float bias slabs), elsewhere only compared plan against plan; 129 frames: the
    # smallest batch at which dccn_gemm_route_query also splits the bottleneck's two GEMMs (128: one range; the SK2 x SK2
    # layers stay unsplit at N = 128 up to 200 frames and beyond)
    "h": dict(nbits=2, B=129, plan=1, geometry=_geo(128, False, True),
              route=dict(rides=0, bn=0, group=0, tail=1, tail_eval=1, splits=(8, 8, 1, 2, 2), fold_k=1918, window=0)),
    # i: aligned 320-float rows, SK2 = 1792
    "i": dict(nbits=2, B=73, plan=1, geometry=_geo(128, True, True),
              route=dict(rides=1, bn=0, group=0, tail=1, tail_eval=1, splits=(4, 4, 1, 1, 1), fold_k=2240, window=0)),
    # j: the launch-per-stage plan through the window (key 20 = 0: no single-pass norm, hence no group; bn answers for the
    # shape alone)
    "j": dict(nbits=2, B=73, plan=0, geometry=_geo(64, True, False),
              route=dict(rides=0, bn=1, group=0, tail=1, tail_eval=1, splits=(4, 4, 1, 1, 1), fold_k=1120, window=0)),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY_CASES))
def test_fused_step_stage_by_stage_at_every_prefix_and_window(case):
    """the step away from N = 64 / CP = 16 / FLAGS.cp on: the routes only these geometries reach (GEOMETRY_CASES), each asserted
    through the library's own queries first, then every stage at 1e-5 with the margins of the module docstring; the frozen
    receiver carries non-zero biases.  Cases a, c, f and g also hold an evaluation step on a second batch: its forward stages,
    ce_mean and the confusion counts with tie accounting."""
    c = GEOMETRY_CASES[case]
    run_case(c["nbits"], c["B"], c["plan"], {}, c["geometry"], c["route"], c.get("evaluate", False))
