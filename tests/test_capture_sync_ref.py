"""Host side of the capture stage (``dccn_capture_sync``): the linear fp64 restatement (tests/capture_sync_ref.py) held to the
circular one where the two must agree, the captures of the GPU tests held to the cap on undecidable frames, and the host
impairment model that builds captures (``rayleigh_chan_lte.run_stream``, ``apply_cfo_stream``) held to ``run`` / ``apply_cfo``."""
import numpy as np
import pytest

import capture_sync_ref as CR
import frame_cfo_ref as F
import frame_sync_ref as R


# ---- 1. padded captures: the linear reference IS the circular one ---------------------------------------------------------
@pytest.mark.parametrize("CP,W", [(16, 3), (16, 16), (4, 3), (4, 1)])
def test_padded_capture_agrees_with_circular_reference(CP, W):
    xs = R.case_frames("ETU", 5.0, CP)[:40]
    cap, first, stride = CR.padded_capture(xs, W)
    off, lam, phi, gam = CR.reference(cap, first, stride, xs.shape[0], R.S, R.K, CP, W)
    off0, lam0, phi0 = R.reference(xs, R.K, CP, W)
    assert np.array_equal(off, off0) and np.array_equal(lam, lam0) and np.array_equal(phi, phi0)
    assert np.array_equal(CR.gamma_at(gam, off, W), F.gamma_at(xs, R.K, CP, off0))
    assert len(set(off.tolist())) > 1                                         # (the case moves frames both ways)
    # and the cut is the rotation: the slot's padding holds exactly the samples that wrap
    assert np.array_equal(CR.cut(cap, first, stride, off, R.S, R.K, CP), R.aligned(xs, off0))


def test_small_shape_padded_capture():
    """(S, K, CP, W) = (3, 12, 4, 2): T = 48"""
    xs = F.exact_prefix_frames(9, 3, 12, 4, seed=5, eps=0.17, roll=1)
    cap, first, stride = CR.padded_capture(xs, 2)
    off, lam, phi, _ = CR.reference(cap, first, stride, 9, 3, 12, 4, 2)
    off0, lam0, phi0 = R.reference(xs, 12, 4, 2)
    assert np.array_equal(off, off0) and np.array_equal(lam, lam0) and np.array_equal(phi, phi0)
    assert (off == 1).all()


# ---- 2. the captures of the GPU tests: undecidable frames stay under the cap -----------------------------------------------
@pytest.mark.parametrize("CP,W,channel,snr", CR.CASES)
def test_undecidable_frames_under_cap(CP, W, channel, snr):
    assert (CP, W, channel, snr) in R.all_cases()
    for cfo in (False, True):
        for spare, shift in CR.LAYOUTS:
            off, lam, phi, gam, ok = CR.case_reference(channel, snr, CP, W, spare, shift, cfo)
            bad = int((~ok).sum())
            print("%s %g dB CP %d W %d spare %d shift %d cfo %d: %d of %d undecidable, offsets %s"
                  % (channel, snr, CP, W, spare, shift, cfo, bad, CR.FRAMES, sorted(set(off.tolist()))))
            assert bad <= R.CAP * CR.FRAMES


def test_cases_cover_the_grid():
    assert len(CR.CASES) == 8 and {c[0] for c in CR.CASES} == {16, 4}
    assert any(ch != "AWGN" and snr == 5.0 for (_, _, ch, snr) in CR.CASES)
    assert any(ch != "AWGN" and snr == 30.0 for (_, _, ch, snr) in CR.CASES)


# ---- 3. the host impairment model ------------------------------------------------------------------------------------------
def _tx(channel, frames, seed):
    from dl_ofdm_amd import ofdm, util
    from dl_ofdm_amd.radio import rayleigh_chan_lte
    Fl = R._flags(channel, 16)
    o = ofdm.ofdm_tx(Fl)
    np.random.seed(seed)
    bits = util.bit_source(Fl.nbits, o.frame_size, frames)
    iq, _, _ = o.ofdm_tx_frame_np(bits)
    return iq, rayleigh_chan_lte(Fl, o.Fs)


@pytest.mark.parametrize("channel", ["EPA", "EVA", "ETU", "AWGN", "mixRayleigh"])
def test_run_stream_agrees_with_run(channel):
    iq, fading = _tx(channel, 9, seed=4)
    n_fr, S, N = iq.shape
    T = S * N
    np.random.seed(77)
    y, H = fading.run(iq)
    after_run = np.random.random()
    np.random.seed(77)
    lead = 40
    cap, Hs = fading.run_stream(iq, lead)
    assert np.random.random() == after_run                                    # (the random stream consumed exactly as run does)
    assert np.array_equal(H, Hs) and Hs.dtype == H.dtype
    assert np.iscomplexobj(cap) and cap.shape == (2 * lead + n_fr * T,)
    L = max(p.alpha.shape[1] for p in fading.profiles)
    yc = (y[..., 0] + 1j * y[..., 1]).reshape(n_fr, T)
    body = cap[lead:lead + n_fr * T].reshape(n_fr, T)
    assert np.array_equal(body[:, L:T - L], yc[:, L:T - L])                   # away from a frame's borders: run's samples exactly
    assert np.abs(cap[:lead - L]).max() == 0 and np.abs(cap[lead + n_fr * T + L:]).max() == 0
    if L > 1:
        assert not np.array_equal(body[1:-1], yc[1:-1])                       # at the borders the neighbours' tails fall in
    if L > 1 and len(fading.profiles) == 1:
        assert np.abs(cap[lead - L:lead]).max() > 0 and np.abs(cap[lead + n_fr * T:lead + n_fr * T + L]).max() > 0
    # every frame's full convolution is in the capture: total energy at least that of run's truncated frames
    assert np.sum(np.abs(cap) ** 2) >= np.sum(np.abs(yc) ** 2) * (1 - 1e-6)


def test_run_stream_refusals():
    from dl_ofdm_amd.radio import rayleigh_chan_lte
    iq, fading = _tx("ETU", 3, seed=1)
    with pytest.raises(ValueError):
        fading.run_stream(iq, 2)                                              # no room for the tails
    mobile = rayleigh_chan_lte(R._flags("ETU", 16), fading.sample_rate, mobile=True)
    with pytest.raises(ValueError):
        mobile.run_stream(iq, 40)                                             # Doppler frames
    with pytest.raises(AssertionError):
        fading.run_stream(np.zeros((3, 7, 80)), 40)


def test_apply_cfo_stream():
    from dl_ofdm_amd.radio import apply_cfo, apply_cfo_stream
    rs = np.random.RandomState(2)
    x = rs.standard_normal((5, 7, 80, 2)).astype(np.float32)
    cap = x.reshape(-1, 2)
    eps = 0.137
    got = apply_cfo_stream(cap, eps, 64)
    assert got.dtype == np.float32 and got.shape == cap.shape
    assert np.array_equal(got[:560], apply_cfo(x[:1], eps, 64).reshape(-1, 2))       # frame 0: the per-frame form
    c = got[:, 0].astype(np.float64) + 1j * got[:, 1]
    c0 = cap[:, 0].astype(np.float64) + 1j * cap[:, 1]
    n = np.arange(c.shape[0])
    assert np.abs(c - c0 * np.exp(2j * np.pi * eps * n / 64)).max() < 1e-6           # continuous over the capture
    per_frame = apply_cfo(x, eps, 64).reshape(-1, 2)
    assert not np.allclose(got[560:], per_frame[560:], atol=1e-3)                    # (apply_cfo restarts the phase)
    z = apply_cfo_stream(c0, eps, 64)
    assert np.iscomplexobj(z) and np.allclose(z, c0 * np.exp(2j * np.pi * eps * n / 64), atol=1e-12)
    with pytest.raises(ValueError):
        apply_cfo_stream(x, eps, 64)
