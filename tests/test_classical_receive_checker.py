"""The checker of ``dccn_classical_receive`` held to account on the CPU (``-m "not gpu"``): tests/classical_receive_ref.py is
what tests/test_gpu_classical_receive.py holds the kernel to, so this file shows that (a) its restatement decides like the
project's oracle of the classical receivers (``benchmark.ClassicalReceiver.receive``), (b) its decidable-cell rule leaves at most
1 % of the cells out, (c) the empty-carrier noise estimate is the noise variance, (d) the comparison sees planted errors, and
(e) a float32 NumPy emulation of the kernel's expressions stays inside every derived bound.

(c) at the short prefix: with CP = 4 on ETU at 30 dB the empty cells also hold the inter-symbol interference the prefix does
not cover, and the estimate reads 1.8 times the noise variance (24 frames, seed 13).  That is what the frame contains, not an error of the
estimator; it is documented (include/dccn.h) and not asserted."""
import functools

import numpy as np
import pytest

import classical_receive_ref as R

CHANNELS = [("EPA", 10.0), ("ETU", 30.0), ("AWGN", 5.0)]
METHODS = ("LS-Spline", "LS-Linear", "ALMMSE")
CAP = 0.01


@functools.lru_cache(maxsize=None)
def case(nbits, channel, snr, method, longcp=True, nfft=64):
    return R.make_case(nbits, channel, snr, n=24, seed=11 + nbits, nfft=nfft, longcp=longcp, method=method)


@functools.lru_cache(maxsize=None)
def restated(nbits, channel, snr, method, known=True):
    c = case(nbits, channel, snr, method)
    return R.restate_case(c, c["known_noise"] if known else 0.0)


@pytest.mark.parametrize("channel,snr", CHANNELS)
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
@pytest.mark.parametrize("method", METHODS)
def test_restatement_decides_like_the_oracle_on_every_decidable_cell(method, nbits, channel, snr):
    c = case(nbits, channel, snr, method)
    r = restated(nbits, channel, snr, method)
    ref = c["host"].receive(c["x"], method, snr, advance=c["advance"], aligned=True)
    dec = r["decidable"]
    assert 1.0 - dec.mean() <= CAP, 1.0 - dec.mean()                                    # (b)
    assert np.array_equal(r["hard"][dec], (np.asarray(ref) != 0).astype(np.uint8)[dec])
    # the restatement is not a copy of the oracle's answer by construction of `decidable`: most cells are held
    assert dec.mean() >= 1.0 - CAP
    # and its packed rows are its hard bits in the receive path's layout
    from dl_ofdm_amd.receive import pack_bits
    assert np.array_equal(r["packed"], pack_bits(r["hard"]))


@pytest.mark.parametrize("channel,snr", CHANNELS)
@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_estimated_noise_leaves_at_most_one_percent_undecidable(nbits, channel, snr):
    for method in ("LS-Spline", "ALMMSE"):
        r = restated(nbits, channel, snr, method, known=False)
        assert 1.0 - r["decidable"].mean() <= CAP
        assert np.all(np.isfinite(r["llr"]))


@pytest.mark.parametrize("channel,snr", [("AWGN", 5.0), ("EPA", 10.0)])
def test_empty_carrier_noise_estimate_is_the_noise_variance(channel, snr):
    c = case(2, channel, snr, "ALMMSE")
    r = restated(2, channel, snr, "ALMMSE", known=False)
    assert len(c["empty"]) == 112
    ratio = float(np.median(r["noise"]) / c["known_noise"])
    print("median nv / (K sigma^2) on %s %g dB: %.4f" % (channel, snr, ratio))
    assert 0.95 <= ratio <= 1.05, ratio


@pytest.mark.parametrize("plant", R.PLANTS)
def test_the_comparison_sees_a_planted_error(plant):
    c = case(3, "EPA", 10.0, "ALMMSE")
    clean = restated(3, "EPA", 10.0, "ALMMSE", known=False)
    assert R.failures(R.compare(clean, R.as_device_result(clean), c["D"], c["nbits"])) == []
    bad = R.restate_case(c, 0.0, plant=plant)
    fig = R.compare(clean, R.as_device_result(bad), c["D"], c["nbits"])
    assert R.failures(fig), (plant, fig)
    expect = {"window": "share_y_freq", "conj_pv": "share_chest", "no_mean": "share_chest", "bit_order": "bit_mismatch",
              "llr_sign": "llr_sign"}[plant]
    assert expect in R.failures(fig), (plant, fig)


# ---- (e) the kernel's expressions in float32 NumPy, sums in the kernel's order where NumPy allows -----------------------
def emulate32(c, noise_var):
    f = np.float32
    x, dft, w = c["x"], c["dft"], c["w"]
    n, S, _, _ = x.shape
    K, SK, win = c["K"], c["S"] * c["K"], c["win"]
    xw = x[:, :, win:win + K, :].reshape(n * S, 2 * K)
    Y = np.zeros((n * S, 2 * K), f)
    for i in range(2 * K):                                    # one product at a time: more roundings than the MFMA's
        Y = (Y + xw[:, i:i + 1] * dft[i:i + 1, :]).astype(f)
    Y = Y.reshape(n, SK, 2)
    pvx, pvy = c["pv"]
    pd = f(pvx * pvx + pvy * pvy)
    yp = Y[:, c["pil"], :]
    gp = np.stack([(yp[..., 0] * pvx + yp[..., 1] * pvy) / pd, (yp[..., 1] * pvx - yp[..., 0] * pvy) / pd], -1).astype(f)
    G = np.zeros((n, SK, 2), f)
    for j in range(w.shape[0]):
        G = (G + gp[:, j:j + 1, :] * w[j][None, :, None]).astype(f)
    if noise_var > 0:
        nv = np.full(n, f(noise_var), f)
    else:
        ye = Y[:, c["empty"], :]
        a = np.zeros(n, f)
        for e in range(ye.shape[1]):
            a = (a + (ye[:, e, 0] * ye[:, e, 0] + ye[:, e, 1] * ye[:, e, 1])).astype(f)
        nv = np.maximum(a / f(ye.shape[1]), f(1e-20)).astype(f)
    if c["mode"] == 2:
        g3 = G.reshape(n, S, K, 2)
        v = np.zeros((n, K, 2), f)
        for s in range(S):
            v = (v + g3[:, s]).astype(f)
        v = (v / f(S)).astype(f)
        pe = np.zeros(n, f)
        for k in range(K):
            pe = (pe + (v[:, k, 0] * v[:, k, 0] + v[:, k, 1] * v[:, k, 1])).astype(f)
        e = (pe / f(S)).astype(f)
        wgt = (e / (e + nv / pd)).astype(f)
        G = np.repeat((v * wgt[:, None, None]).astype(f)[:, None], S, axis=1).reshape(n, SK, 2)
    yd, gd = Y[:, c["dat"], :], G[:, c["dat"], :]
    d = (gd[..., 0] * gd[..., 0] + gd[..., 1] * gd[..., 1]).astype(f)
    xh = np.stack([(yd[..., 0] * gd[..., 0] + yd[..., 1] * gd[..., 1]) / d, (yd[..., 1] * gd[..., 0] - yd[..., 0] * gd[..., 1]) / d],
                  -1).astype(f)
    dx = (xh[..., None, 0] - c["table"][None, None, :, 0]).astype(f)
    dy = (xh[..., None, 1] - c["table"][None, None, :, 1]).astype(f)
    dq = (dx * dx + dy * dy).astype(f)
    best = np.argmin(dq, axis=-1)
    hard = (c["labels"][best] != 0).astype(np.uint8)
    lab = c["labels"] != 0
    nb = c["nbits"]
    m0 = np.stack([np.where(~lab[None, None, :, b], dq, f(3e38)).min(axis=-1) for b in range(nb)], -1)
    m1 = np.stack([np.where(lab[None, None, :, b], dq, f(3e38)).min(axis=-1) for b in range(nb)], -1)
    llr = ((d / nv[:, None])[..., None] * (m0 - m1)).astype(f)
    return dict(packed=R.pack_rows(hard), y_freq=Y, chest=G, noise=nv, llr=llr)


@pytest.mark.parametrize("method,nbits,channel,snr,known", [("ALMMSE", 2, "EPA", 10.0, False), ("LS-Spline", 4, "ETU", 30.0, True),
                                                           ("LS-Linear", 3, "AWGN", 5.0, False), ("ALMMSE", 1, "ETU", 30.0, True)])
def test_float32_emulation_stays_inside_every_bound(method, nbits, channel, snr, known):
    c = case(nbits, channel, snr, method)
    r = restated(nbits, channel, snr, method, known=known)
    with np.errstate(all="ignore"):
        got = emulate32(c, c["known_noise"] if known else 0.0)
    fig = R.compare(r, got, c["D"], c["nbits"])
    print(method, nbits, channel, fig)
    assert R.failures(fig) == [], fig
