"""oracle/classical_oracle.py (the stage-by-stage float64 restatement the GPU stage tests compare with) against
dl_ofdm_amd.benchmark.ClassicalReceiver (the whole-receiver restatement, itself pinned by closed forms in
tests/test_benchmark.py) at the product geometry: two restatements of one estimator family that must not drift apart."""
import numpy as np
import pytest

from dl_ofdm_amd import benchmark as B
from dl_ofdm_amd.receiver import Flags
from oracle import classical_oracle as CO

N_FRAMES = 5
METHOD_MODE = [("LS-Spline", CO.LS), ("LMMSE", CO.LMMSE), ("ALMMSE", CO.ALMMSE), ("Perfect", CO.PERFECT)]


def rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.fixture(scope="module", params=[2, 4])
def case(request):
    nb = request.param
    r = B.ClassicalReceiver(Flags(nbits=nb, channel="EPA", nfilter=64))
    rng = np.random.RandomState(40 + nb)
    SK = r.S * r.K
    cplx = lambda *s: rng.randn(*s) + 1j * rng.randn(*s)          # noqa: E731
    H = cplx(N_FRAMES, SK)
    Y = (0.7 - 0.4j) * H * (r.pilot_value + 0.3 * cplx(N_FRAMES, SK))         # a gain that is not real, and noise
    gp = CO.pilot_ls(Y, r.pil, r.pilot_value)                      # [2, n, P]
    Gls = np.stack([gp[0] @ r.W_spline.T, gp[1] @ r.W_spline.T], 0)      # the interpolation, plane by plane as on the device
    return dict(r=r, nb=nb, Y=Y, H=H, gp=gp, Gls=Gls, noise_var=0.37 * abs(r.pilot_value) ** 2, rng=rng)


def test_pilot_ls_and_interpolation(case):
    r = case["r"]
    g_p = case["Y"][:, r.pil] / r.pilot_value
    assert case["gp"].shape == (2, N_FRAMES, len(r.pil))
    assert rel(CO.from_planes(case["gp"]), g_p) <= 1e-12
    assert rel(CO.from_planes(case["Gls"]), g_p @ r.W_spline.T) <= 1e-12


def test_gain_scalar_is_the_one_receive_computes(case):
    r, Y, H = case["r"], case["Y"], case["H"]
    sums, scales = CO.gain_sums(Y, H, case["Gls"], r.pil, r.pilot_value)
    a = np.sum(Y[:, r.pil] * np.conj(H[:, r.pil] * r.pilot_value)) / np.sum(np.abs(H[:, r.pil] * r.pilot_value) ** 2)
    assert abs(CO.gain_scalar(sums) - a) <= 1e-12 * abs(a)
    assert abs(sums[3] - np.sum(np.abs(CO.from_planes(case["Gls"])) ** 2)) <= 1e-12 * sums[3]
    assert (scales >= np.abs(sums)).all() and scales[2] == sums[2] and scales[3] == sums[3]
    s0, _ = CO.gain_sums(Y, None, case["Gls"], r.pil, r.pilot_value)
    assert (s0[:3] == 0.0).all() and s0[3] == sums[3]


@pytest.mark.parametrize("method,mode", METHOD_MODE)
def test_estimate_matches_the_receiver(case, method, mode):
    r, Y, H = case["r"], case["Y"], case["H"]
    a = CO.gain_scalar(CO.gain_sums(Y, H, case["Gls"], r.pil, r.pilot_value)[0])
    c = case["noise_var"] / abs(r.pilot_value) ** 2
    ref = r.estimate(Y, method, case["noise_var"], G_true=H * a)
    got = CO.estimate(case["Gls"].reshape(2, N_FRAMES, r.S, r.K), H.reshape(N_FRAMES, r.S, r.K), mode, c, a)
    assert rel(got, ref) <= 1e-12, method
    if mode in (CO.LMMSE, CO.ALMMSE):                                   # the noise term is not a bystander in this case
        assert rel(got, r.estimate(Y, method, 0.0, G_true=H * a)) >= 1e-3


def test_frame_mean_is_the_pdp_branch_input(case):
    r = case["r"]
    V = CO.estimate(case["Gls"].reshape(2, N_FRAMES, r.S, r.K), None, CO.FRAME_MEAN, 0.0)
    G_ls = (case["Y"][:, r.pil] / r.pilot_value) @ r.W_spline.T
    assert V.shape == (N_FRAMES, r.K)
    assert rel(V, G_ls.reshape(N_FRAMES, r.S, r.K).mean(axis=1)) <= 1e-12


def test_detect_is_demap(case):
    r, Y, rng = case["r"], case["Y"], case["rng"]
    SK = r.S * r.K
    G = CO.from_planes(case["Gls"])
    bits = rng.randint(0, 2, (N_FRAMES, len(r.dat), case["nb"])).astype(np.int32)
    ref = r.demap(Y[:, r.dat] / G[:, r.dat])
    det, errors = CO.detect(Y, G, r.dat, r.table, r.labels, bits, SK, 0)
    assert det.shape == ref.shape and np.array_equal(det, ref)
    assert errors == int(np.count_nonzero(ref != bits))
    # the one-row-per-frame form of the PDP variants
    V = G.reshape(N_FRAMES, r.S, r.K).mean(axis=1)
    full = np.repeat(V[:, None, :], r.S, axis=1).reshape(N_FRAMES, SK)
    det1, err1 = CO.detect(Y, V, r.dat, r.table, r.labels, bits, r.K, r.K)
    assert np.array_equal(det1, r.demap(Y[:, r.dat] / full[:, r.dat])) and err1 == int(np.count_nonzero(det1 != bits))
    assert (CO.decision_margin(Y, G, r.dat, r.table, SK, 0) >= 0.0).all()
