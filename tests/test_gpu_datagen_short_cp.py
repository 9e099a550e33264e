"""The fused generator launch at the short cyclic prefix (csrc/datagen.h gen_static_frames_kernel<7,64,4> /
gen_doppler_frames_kernel<7,64,4>; N = 64, CP = round(0.07 * 64) = 4: 68 samples per symbol, 476 per frame -- the
``longcp=False`` half of the reference driver's grid), ``-m gpu``.  The prefix is half a 16-column MFMA tile there, so the ifft
tiles are anchored behind it and the prefix copy is a per-lane condition inside the last tile; ETU's 9 taps reach past the
4-sample prefix into the previous symbol's body in the per-symbol Doppler FIR.

Order of trust: the launch-per-stage device chain is held to the host substrate at THIS shape first (the substrate is pinned to
the reference by the ``n64s_b2`` golden of tests/test_golden_substrate.py); the fused launch is then held to that chain at the
same (seed, offset) with the bounds tests/test_gpu_datagen.py and tests/test_gpu_datagen_mobile.py use at the long prefix."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)


def flags(**kw):
    from dl_ofdm_amd.receiver import Flags
    f = Flags(channel="EPA", nfilter=64, nbits=2, SNR=5.0, longcp=False)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def gens(chan, nbits, seed, mobile=False, mix=False, count=2, **kw):
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    F = flags(nbits=nbits, channel=chan, **kw)
    o = ofdm.ofdm_tx(F)
    assert o.CP == 4 and o.K == 64 and o.frame_size == 320
    return [DeviceDataGen(F, o, seed=seed, mobile=mobile, mix=mix) for _ in range(count)]


def doppler_frames(gen, n):
    if gen.mixed:
        return [dop for _, dop in gen.frame_plan(n)]
    return [bool(gen.doppler)] * n


# ---- 1. the comparator first ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chan", ["EPA", "ETU"])
def test_launch_per_stage_chain_matches_the_host_substrate_at_the_short_prefix(chan):
    """dccn_ofdm_tx_frames + dccn_channel_awgn at N = 64 / CP = 4 against ofdm.py / radio.py fed the same bits, tap draws and
    noise draws (ETU: the longest response against the 4-sample prefix).  Bounds: tests/test_gpu_datagen.py
    test_transmitter_and_awgn_at_other_fft_sizes (tx 2e-5, received 3e-5, noise power 1e-5) and
    test_channel_and_awgn_match_host_given_the_same_draws (H 2e-5)."""
    from dl_ofdm_amd import ofdm, radio
    from dl_ofdm_amd.datagen import DeviceDataGen
    F = flags(channel=chan)
    o = ofdm.ofdm_tx(F)
    assert o.CP == 4
    gen = DeviceDataGen(F, o, seed=5)
    n = 6
    bits = np.random.RandomState(64).randint(0, 2, (n, o.frame_size, 2))
    iq, want, _ = o.ofdm_tx_frame_np(bits)
    tx, _ = gen.transmit(n, bits=bits)
    assert tx.shape == want.shape == (n, 7, 68, 2)
    e_tx = float(np.abs(tx.cpu().numpy() - want).max() / np.abs(want).max())
    snr = np.linspace(-3, 25, n).reshape(n, 1)
    np.random.seed(3)
    y_host, H_host = radio.rayleigh_chan_lte(F, o.Fs).run(iq)
    out_host, npow_host = radio.AWGN_channel_np(y_host, snr)
    np.random.seed(3)                                               # replay numpy's draws: taps per frame, then the noise
    taps = np.stack([np.random.normal(loc=0.0, scale=1.0, size=[gen.n_taps, 2]) for _ in range(n)])
    noise = np.random.randn(*want.shape)
    out, npow, H = gen.channel(tx, snr, taps=taps, noise=noise.reshape(n, -1, 2), want_H=True)
    e_x = float(np.abs(out.cpu().numpy() - out_host).max() / np.abs(out_host).max())
    e_np = abs(float(npow) - npow_host) / npow_host
    Hh = H_host[:, 0, :]
    e_H = float(np.abs(H.cpu().numpy() - Hh).max() / max(np.abs(Hh).max(), 1.0))
    print("launch-per-stage vs host, CP = 4", chan, dict(tx=e_tx, x=e_x, npow=e_np, H=e_H))
    assert e_tx <= 2e-5
    assert e_x <= 3e-5
    assert e_np <= 1e-5
    assert e_H <= 2e-5


# ---- 2. fused static against launch-per-stage -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chan,nbits,n,cp", [("EPA", 2, 73, True), ("ETU", 3, 9, True), ("EVA", 4, 37, True), ("AWGN", 1, 1, True),
                                              ("EPA", 2, 2, False), ("mixRayleigh", 2, 7, True), ("mixAll", 1, 9, True)])
def test_fused_static_generator_matches_the_launch_per_stage_chain_at_the_short_prefix(chan, nbits, n, cp):
    """what test_fused_static_generator_matches_the_launch_per_stage_chain and
    test_fused_generator_with_interleaved_profiles_and_frequency_response (tests/test_gpu_datagen.py) assert, with their bounds,
    at (seed, offset != 0) and per-frame SNRs: labels and H the same bits, tx <= 2e-6, x <= 1e-5, noise power <= 1e-6,
    x = y * inv + noise to 2e-7; the 4-sample prefix is a bitwise copy of the symbol's tail on both routes.  One frame alone in
    a block (n odd, n = 1), both frames of a block (n = 2), profiles of different lengths side by side (mix*)."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    ga, gb = gens(chan, nbits, 21, cp=cp)
    assert gb.CP == 4 and gb.n_sc == 68 and gb.T == 476
    snr = torch.linspace(-3.0, 27.0, n, device="cuda")
    ga.offset = gb.offset = 6
    assert FusedStaticGen.supported(gb) and gb.mixed == chan.startswith("mix")
    tx_a, bits_a = ga.transmit(n)
    x_a, npow_a, H_a = ga.channel(tx_a, snr, want_H=True)
    fg = FusedStaticGen(gb, n, 0.0, want_noise_power=True)
    assert not fg.has_doppler and fg.desc.CP == 4
    hshape = (n, gb.S, gb.K, 2) if gb.mixed else (n, gb.K, 2)
    x_b, bits_b, tx_b = torch.empty_like(x_a), torch.empty_like(bits_a), torch.empty_like(tx_a)
    H_b = torch.full(hshape, float("nan"), device="cuda")
    _, _, npow_b = fg.make_batch(x_b, bits_b, slot=1, tx_out=tx_b, out_H=H_b, snr=snr)
    torch.cuda.synchronize()
    assert gb.offset == 7
    assert torch.equal(bits_a, bits_b)
    for t in (tx_a, tx_b):                                          # the prefix: a copy of the symbol's tail, to the bit
        v = t.view(n, gb.S, 68, 2)
        assert torch.equal(v[:, :, :4], v[:, :, 64:])
    want_npow = float((fg.noise.double() ** 2).sum() / (n * gb.T))
    inv = np.float32(1.0) / np.sqrt(np.float32(float((fg.y.double() ** 2).sum()) / (n * gb.T)))
    want_x = fg.y.cpu().numpy() * inv + fg.noise.cpu().numpy()
    errs = dict(tx=float((tx_a - tx_b).abs().max()) / float(tx_a.abs().max()), x=float((x_a - x_b).abs().max()) / float(x_a.abs().max()),
                npow=abs(float(npow_a) - float(npow_b)) / float(npow_a), npow_own=abs(float(npow_b) - want_npow) / want_npow,
                x_formed=float(np.abs(x_b.cpu().numpy() - want_x).max() / np.abs(want_x).max()),
                H_bits=bool(torch.equal(torch.view_as_real(H_a).reshape(hshape), H_b)))
    print("fused vs launch-per-stage, CP = 4", chan, nbits, n, cp, errs)
    assert errs["H_bits"]
    assert errs["tx"] <= 2e-6
    assert errs["x"] <= 1e-5
    assert errs["npow"] <= 1e-6 and errs["npow_own"] <= 1e-6
    assert errs["x_formed"] <= 2e-7
    if gb.mixed:                             # neighbouring frames really run different channels
        Hc = torch.view_as_complex(H_b)[:, 0]
        assert float((Hc[0].abs() - Hc[1].abs()).abs().max()) > 1e-3


# ---- 3. Doppler frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chan,mix,nbits,n", [("mixRayleigh", True, 2, 7), ("mixRayleigh", True, 4, 27), ("ETU", False, 3, 2),
                                              ("Flat", False, 1, 1), ("ETU", False, 3, 1), ("ETU", False, 3, 3),
                                              ("mixRayleigh", True, 2, 3)])
def test_fused_generator_with_doppler_frames_matches_the_launch_per_stage_chain_at_the_short_prefix(chan, mix, nbits, n):
    """tests/test_gpu_datagen_mobile.py test_fused_generator_with_doppler_frames_matches_the_launch_per_stage_chain at CP = 4,
    its assertions and bounds (H <= 5e-5).  ETU: 9 taps of history against a 4-sample prefix -- the per-symbol FIR window reaches
    into the previous symbol's body; n = 27: every mixRayleigh profile appears as a Doppler frame; n = 1: a one-frame block (the
    second profile repeats the first); n = 3: a full block followed by a one-frame last block."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    ga, gb = gens(chan, nbits, 21, mobile=True, mix=mix)
    assert gb.CP == 4
    snr = torch.linspace(-3.0, 27.0, n, device="cuda")
    ga.offset = gb.offset = 6
    assert FusedStaticGen.supported(gb) and gb.mixed == chan.startswith("mix")
    dop = doppler_frames(gb, n)
    assert any(dop)
    if chan == "mixRayleigh" and n == 27:
        assert {pi for pi, d in gb.frame_plan(n) if d} == {0, 1, 2, 3}
    if chan == "ETU":
        assert gb.n_taps > gb.CP                      # the history is longer than the prefix
    tx_a, bits_a = ga.transmit(n)
    x_a, npow_a, H_a = ga.channel(tx_a, snr, want_H=True)
    fg = FusedStaticGen(gb, n, 0.0, want_noise_power=True)
    assert fg.has_doppler and fg.desc.doppler_period == (gb.period if gb.mixed else 1) and fg.desc.CP == 4
    hshape = (n, gb.S, gb.K, 2)
    x_b, bits_b, tx_b = torch.empty_like(x_a), torch.empty_like(bits_a), torch.empty_like(tx_a)
    H_b = torch.full(hshape, float("nan"), device="cuda")
    _, _, npow_b = fg.make_batch(x_b, bits_b, slot=1, tx_out=tx_b, out_H=H_b, snr=snr)
    torch.cuda.synchronize()
    assert gb.offset == 7
    assert torch.equal(bits_a, bits_b)
    H_a = torch.view_as_real(H_a).reshape(hshape)
    errs = dict(tx=float((tx_a - tx_b).abs().max()) / float(tx_a.abs().max()), x=float((x_a - x_b).abs().max()) / float(x_a.abs().max()),
                npow=abs(float(npow_a) - float(npow_b)) / float(npow_a),
                H=float(torch.view_as_complex(H_a - H_b).abs().max()) / max(float(torch.view_as_complex(H_a).abs().max()), 1.0))
    print("fused vs launch-per-stage, CP = 4, Doppler", chan, nbits, n, errs)
    assert errs["tx"] <= 2e-6
    assert errs["x"] <= 1e-5
    assert errs["npow"] <= 1e-6
    assert bool(torch.isfinite(H_b).all()) and errs["H"] <= 5e-5
    for f in range(n):
        if dop[f]:
            assert float((H_b[f, 0] - H_b[f, 6]).abs().max()) > 0.0, f      # a Doppler frame's response moves with the symbol
        else:
            assert torch.equal(H_b[f], H_a[f]) and torch.equal(H_b[f, 0], H_b[f, 6]), f


# ---- 4. static frames and their Doppler neighbours -----------------------------------------------------------------------------
def test_static_frames_do_not_notice_their_doppler_neighbours_at_the_short_prefix():
    """mixRayleigh at one (seed, offset) without and with ``mix`` (the static and the Doppler instantiation at CP = 4): every
    frame that is static in both plans has the same y, noise, H and labels; the static descriptor repeats itself bit for bit."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    n = 27
    runs = []
    for mix in (False, True, False):
        (g,) = gens("mixRayleigh", 2, 33, mobile=True, mix=mix, count=1)
        g.offset = 4
        fg = FusedStaticGen(g, n, 0.0, want_noise_power=True)
        assert fg.has_doppler == mix and fg.desc.doppler_period == (3 if mix else 0) and fg.desc.CP == 4
        x = torch.empty(n, g.S, g.n_sc, 2, device="cuda")
        bits = torch.empty(n, g.D, g.nbits, dtype=torch.int32, device="cuda")
        H = torch.full((n, g.S, g.K, 2), float("nan"), device="cuda")
        fg.make_batch(x, bits, slot=0, out_H=H, snr=torch.linspace(0.0, 20.0, n, device="cuda"))
        torch.cuda.synchronize()
        runs.append((fg, x, bits, H, doppler_frames(g, n)))
    (fa, xa, ba, Ha, da), (fb, xb, bb, Hb, db), (fc, xc, bc, Hc, _) = runs
    assert not any(da) and sum(db) == 9
    assert torch.equal(ba, bb)
    for f in range(n):
        if not db[f]:
            assert torch.equal(fa.y[f], fb.y[f]) and torch.equal(fa.noise[f], fb.noise[f]) and torch.equal(Ha[f], Hb[f]), f
        else:
            assert torch.equal(fa.noise[f], fb.noise[f]) and not torch.equal(fa.y[f], fb.y[f]), f
    for s, t in ((fa.y, fc.y), (fa.noise, fc.noise), (xa, xc), (Ha, Hc), (ba, bc), (fa.ppart, fc.ppart), (fa.npow, fc.npow)):
        assert torch.equal(s, t)


# ---- 5. refusals launch nothing -------------------------------------------------------------------------------------------------
def test_a_descriptor_at_a_prefix_without_an_instantiation_launches_nothing():
    """CP = 8 is neither instantiation: dccn_gen_static_frames and dccn_gen_static_apply return DCCN_ERR_INVALID_ARG, and y,
    noise, the partials, H, x and the labels keep the NaN / sentinel they were filled with."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    n = 8
    (g,) = gens("EPA", 2, 5, count=1)
    fg = FusedStaticGen(g, n, 10.0, want_noise_power=True)
    bits = torch.full((n, g.D, g.nbits), -7, dtype=torch.int32, device="cuda")
    H = torch.full((n, g.K, 2), float("nan"), device="cuda")
    d = fg.arm(bits, 0, None, H)
    lib, st = g.lib, g._stream()
    watched = [fg.y, fg.noise, fg.ppart, fg.npart, H]
    for t in watched:
        t.fill_(float("nan"))
    x = torch.full((n, g.S, g.n_sc, 2), float("nan"), device="cuda")
    torch.cuda.synchronize()
    assert d.CP == 4
    d.CP = 8
    assert int(lib.dccn_gen_static_supported(d.S, d.K, d.CP)) == 0
    rc = lib.dccn_gen_static_frames(C.byref(d), st)
    rc2 = lib.dccn_gen_static_apply(C.byref(d), x.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert rc == INVALID_ARG and rc2 == INVALID_ARG
    for t in watched + [x]:
        assert bool(torch.isnan(t).all())
    assert bool((bits == -7).all())


def test_a_short_prefix_descriptor_is_refused_by_a_long_prefix_engine_before_anything_runs():
    """dccn_rx_train_step with gen_next: the engine's rows hold 7 x 80 samples, the descriptor's frames 7 x 68 -- the plan refuses
    (DCCN_ERR_INVALID_ARG) and parameters, Adam slots, Adam state and x_norm are what they were."""
    from dl_ofdm_amd import ofdm, receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxEngine
    n = 36
    Fl = flags(longcp=True)
    eng = RxEngine(R.rx_dims(Fl, ofdm.ofdm_tx(Fl)), n, train=True, seed=1, want_prob=False, want_z=False)
    assert eng.shape.kin == 80
    (g,) = gens("EPA", 2, 3, count=1)
    fg = FusedStaticGen(g, n, 10.0)
    eng.x.copy_(torch.randn(eng.x.shape, generator=torch.Generator().manual_seed(1)))
    eng.prime()
    torch.cuda.synchronize()
    watched = (eng.params, eng.adam_m, eng.adam_v, eng.adam_state, eng._norm_bufs[0])
    before = [t.clone() for t in watched]
    d = fg.arm(eng.label_slot(1), 1)
    bufs = eng._pipe_buffers(0, False, 0, False, 1, 0, C.addressof(d), False)
    rc = eng.lib.dccn_rx_train_step(C.byref(eng.shape), C.byref(bufs), eng.hp, eng._stream())
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    for a, b in zip(before, watched):
        assert torch.equal(a, b)


# ---- 6. generated steps against pipelined steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [73, 301])
@pytest.mark.parametrize("mobile", [False, True])
def test_generated_steps_at_the_short_prefix_equal_pipelined_steps_on_the_materialised_batches(frames, mobile):
    """RxEngine.train_step_generated at kin = 68 (the step issues the CP = 4 generator launch -- static, or with every EPA frame
    a Doppler frame -- and reads (y, noise, power partials) as its virtual input) against train_step_pipelined on the batches the
    same generator materialises: the same bits in every parameter, Adam slot and metric after six steps."""
    from dl_ofdm_amd import receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxEngine
    gs = gens("EPA", 2, 21, mobile=mobile)
    dims = R.rx_dims(gs[0].FLAGS, gs[0].o)
    engs = [RxEngine(dims, frames, train=True, seed=5, want_prob=False, want_z=False) for _ in range(2)]
    assert engs[0].shape.kin == 68
    assert all(FusedStaticGen.supported(g, e) for g, e in zip(gs, engs))
    fgs = [FusedStaticGen(g, frames, 7.0, want_noise_power=True) for g in gs]
    assert fgs[0].has_doppler == mobile
    ea, eb = engs
    n = 6
    xs = []
    for i in range(n):
        ea.train_step_generated(fgs[0], slot=i & 1, last=(i + 1 == n), keep_x=True)
        xs.append(ea.x.clone())
    fgs[1].make_batch(eb.x, eb.label_slot(0), 0)
    eb.prime()
    for i in range(n):
        last = i + 1 == n
        if not last:
            fgs[1].make_batch(eb.x, eb.label_slot((i + 1) & 1), (i + 1) & 1)
            assert torch.equal(eb.x, xs[i]), i
        eb.train_step_pipelined(slot=i & 1, last=last)
    torch.cuda.synchronize()
    assert gs[0].offset == gs[1].offset == n
    for name in ("params", "adam_m", "adam_v", "adam_state"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name
    ma, mb = ea.metrics(), eb.metrics()
    assert ma["conf"] == mb["conf"] and ma["ce_mean"] == mb["ce_mean"] and ma["tx_power"] == mb["tx_power"]
    assert torch.equal(fgs[0].npow, fgs[1].npow)
    assert np.isfinite(ma["ce_mean"])


# ---- 7. the step under it ----------------------------------------------------------------------------------------------------------
def test_train_step_at_68_samples_per_symbol_matches_the_oracle():
    """the receiver step the generated steps run on, at kin = 68 (952 input columns: a multiple of 8, not of 16), against the
    float64 oracle stage by stage -- tests/test_gpu_engine.py has no such case"""
    from test_gpu_engine import make_case, staged_checks
    from dl_ofdm_amd.engine import RxEngine
    dims, cfg, x, bits, p = make_case(36, 2, kin=68)
    eng = RxEngine(dims, 36, params=p, train=True)
    eng.train_step(x, bits)
    torch.cuda.synchronize()
    staged_checks(eng, p, x, bits, cfg)
