"""Doppler frames in the fused generator launch (csrc/datagen.h gen_doppler_frames_kernel; include/dccn.h dccn_gen_static.
doppler_period): the mobile channels of rayleigh_chan_lte -- single-profile (every frame a Doppler frame) and the frame-
interleaved mixRayleigh / mixAll with ``mix`` (every 3rd / 4th frame; the reference driver's training channel) -- from ONE
launch, against the launch-per-stage device generator at the same (seed, offset).  That generator is held to the host substrate
by tests/test_gpu_datagen.py and the substrate to reference goldens by tests/test_golden_substrate.py (``-m gpu``)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)


def flags(**kw):
    from dl_ofdm_amd.receiver import Flags
    f = Flags(channel="EPA", nfilter=64, nbits=2, SNR=5.0)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def gens(chan, nbits, seed, mix, count=2):
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    F = flags(nbits=nbits, channel=chan)
    o = ofdm.ofdm_tx(F)
    return [DeviceDataGen(F, o, seed=seed, mobile=True, mix=mix) for _ in range(count)]


def doppler_frames(gen, n):
    """which frames of an n-frame batch are Doppler frames (DeviceDataGen.frame_plan; single-profile: gen.doppler)"""
    if gen.mixed:
        return [dop for _, dop in gen.frame_plan(n)]
    return [bool(gen.doppler)] * n


@pytest.mark.parametrize("chan,mix,nbits,n", [("mixRayleigh", True, 2, 1), ("mixRayleigh", True, 2, 3), ("mixRayleigh", True, 2, 7),
                                              ("mixRayleigh", True, 4, 27), ("mixRayleigh", True, 2, 73), ("mixAll", True, 1, 10),
                                              ("EPA", False, 2, 9), ("ETU", False, 3, 2), ("Flat", False, 1, 3)])
def test_fused_generator_with_doppler_frames_matches_the_launch_per_stage_chain(chan, mix, nbits, n):
    """dccn_gen_static_frames + dccn_gen_static_apply on a plan with Doppler frames against dccn_ofdm_tx_frames +
    dccn_channel_groups_awgn / dccn_channel_doppler_awgn: per-frame SNRs from a caller's tensor, a nonzero batch offset, the
    noise-power monitor.  mixRayleigh n = 1: a flat Doppler frame (L = 1) alone in its block; n = 3: a full block (Doppler + static)
    followed by a one-frame block, whose second profile repeats the first; n = 7: the last block holds a
    Doppler EVA frame alone, blocks (0, 1) and (2, 3) hold Doppler and static frames in both orders; n = 27: every profile
    appears as a Doppler frame; n = 73: the reference's batch; mixAll: the identity profile is never a Doppler frame; EPA / ETU /
    Flat: every frame a Doppler frame, both frames of a block.  Bounds: those tests/test_gpu_datagen.py holds the static launch
    and the launch-per-stage Doppler kernels to."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    ga, gb = gens(chan, nbits, 21, mix)
    snr = torch.linspace(-3.0, 27.0, n, device="cuda")
    ga.offset = gb.offset = 6
    assert FusedStaticGen.supported(gb) and gb.mixed == chan.startswith("mix")
    dop = doppler_frames(gb, n)
    assert any(dop)                                   # the plan really has Doppler frames
    if chan == "mixAll":
        assert not any(d for (pi, _), d in zip(gb.frame_plan(n), dop) if gb.profiles[pi]["identity"]) and not all(dop)
    if chan == "mixRayleigh" and n == 27:
        assert {pi for pi, d in gb.frame_plan(n) if d} == {0, 1, 2, 3}
    tx_a, bits_a = ga.transmit(n)
    x_a, npow_a, H_a = ga.channel(tx_a, snr, want_H=True)
    fg = FusedStaticGen(gb, n, 0.0, want_noise_power=True)
    assert fg.has_doppler and fg.desc.doppler_period == (gb.period if gb.mixed else 1)
    hshape = (n, gb.S, gb.K, 2)
    x_b, bits_b, tx_b = torch.empty_like(x_a), torch.empty_like(bits_a), torch.empty_like(tx_a)
    H_b = torch.full(hshape, float("nan"), device="cuda")
    with pytest.raises(ValueError):                   # one response per frame cannot hold a Doppler frame's S responses
        fg.arm(bits_b, 1, None, torch.empty(n, gb.K, 2, device="cuda"), snr)
    assert gb.offset == 6
    _, _, npow_b = fg.make_batch(x_b, bits_b, slot=1, tx_out=tx_b, out_H=H_b, snr=snr)
    torch.cuda.synchronize()
    assert gb.offset == 7
    assert torch.equal(bits_a, bits_b)
    H_a = torch.view_as_real(H_a).reshape(hshape)
    errs = dict(tx=float((tx_a - tx_b).abs().max()) / float(tx_a.abs().max()), x=float((x_a - x_b).abs().max()) / float(x_a.abs().max()),
                npow=abs(float(npow_a) - float(npow_b)) / float(npow_a),
                H=float(torch.view_as_complex(H_a - H_b).abs().max()) / max(float(torch.view_as_complex(H_a).abs().max()), 1.0),
                H_bits=bool(torch.equal(H_a, H_b)))
    print("fused vs launch-per-stage", chan, nbits, n, errs)
    assert errs["tx"] <= 2e-6
    assert errs["x"] <= 1e-5
    assert errs["npow"] <= 1e-6
    assert bool(torch.isfinite(H_b).all()) and errs["H"] <= 5e-5
    # the static frames of the plan: h_rep copies of ONE response, the bits of the launch-per-stage kernel (same draws and sums)
    for f in range(n):
        if dop[f]:
            assert float((H_b[f, 0] - H_b[f, 6]).abs().max()) > 0.0, f      # a Doppler frame's response moves with the symbol
        else:
            assert torch.equal(H_b[f], H_a[f]) and torch.equal(H_b[f, 0], H_b[f, 6]), f


def test_static_frames_do_not_notice_their_doppler_neighbours():
    """mixRayleigh at one (seed, offset) without and with ``mix``: the first plan is all static (the static instantiation), the
    second has a Doppler frame in every third slot (the Doppler instantiation).  Every frame that is static in both comes out
    with the same y, noise, H and labels; and the static-only descriptor repeats itself bit for bit."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    n = 27
    runs = []
    for mix in (False, True, False):
        (g,) = gens("mixRayleigh", 2, 33, mix, count=1)
        g.offset = 4
        fg = FusedStaticGen(g, n, 0.0, want_noise_power=True)
        assert fg.has_doppler == mix and fg.desc.doppler_period == (3 if mix else 0)
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


@pytest.mark.parametrize("case", ["one_response_per_frame", "no_symbol_time", "negative_symbol_time", "doppler_frequency_not_finite",
                                  "group_disagrees_on_the_period"])
def test_a_refused_doppler_descriptor_launches_nothing(case):
    """gen_static_ok holds the new fields: a Doppler plan with H_out needs h_rep == S, a nonzero period needs t_sym > 0 and a
    finite Fd, the chains of a group agree on the period -- DCCN_ERR_INVALID_ARG otherwise, and y, noise, the partials, H and
    the labels keep the NaN / sentinel they were filled with."""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.equalizer_group import _ptr_array
    n = 8
    (g,) = gens("EPA", 2, 5, False, count=1)
    fg = FusedStaticGen(g, n, 10.0, want_noise_power=True)
    bits = torch.full((n, g.D, g.nbits), -7, dtype=torch.int32, device="cuda")
    H = torch.full((n, g.S, g.K, 2), float("nan"), device="cuda")
    d = fg.arm(bits, 0, None, H)
    lib, st = g.lib, g._stream()
    assert d.doppler_period == 1 and d.h_rep == g.S and d.t_sym > 0
    watched = [fg.y, fg.noise, fg.ppart, fg.npart, H]
    for t in watched:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    if case == "one_response_per_frame":
        d.h_rep = 1
    elif case == "no_symbol_time":
        d.t_sym = 0.0
    elif case == "negative_symbol_time":
        d.t_sym = -d.t_sym
    elif case == "doppler_frequency_not_finite":
        d.Fd = float("inf")
    if case == "group_disagrees_on_the_period":
        other = _lib.GenStatic.from_buffer_copy(d)
        other.doppler_period = 3
        rc = lib.dccn_gen_static_frames_grouped(2, _ptr_array([d, other]), st)
    else:
        rc = lib.dccn_gen_static_frames(C.byref(d), st)
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    x = torch.full((n, g.S, g.n_sc, 2), float("nan"), device="cuda")
    if case != "group_disagrees_on_the_period":
        assert lib.dccn_gen_static_apply(C.byref(d), x.data_ptr(), None, st) == INVALID_ARG
        torch.cuda.synchronize()
    for t in watched + [x]:
        assert bool(torch.isnan(t).all())
    assert bool((bits == -7).all())


@pytest.mark.parametrize("frames", [73, 1170])
def test_generated_steps_on_a_mobile_channel_equal_pipelined_steps_on_the_materialised_batches(frames):
    """RxEngine.train_step_generated (dccn_rx_buffers.gen_next: the step issues the generator launch -- here the Doppler
    instantiation, every EPA frame a Doppler frame -- and reads (y, noise, power partials) as its virtual input) against
    train_step_pipelined on the batches the same generator materialises: the same bits in every parameter, Adam slot and
    metric after six steps, as tests/test_gpu_datagen.py holds for the static channels."""
    from dl_ofdm_amd import receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxEngine
    gs = gens("EPA", 2, 21, False)
    dims = R.rx_dims(gs[0].FLAGS, gs[0].o)
    engs = [RxEngine(dims, frames, train=True, seed=5, want_prob=False, want_z=False) for _ in range(2)]
    assert all(FusedStaticGen.supported(g, e) for g, e in zip(gs, engs))
    fgs = [FusedStaticGen(g, frames, 7.0, want_noise_power=True) for g in gs]
    assert fgs[0].has_doppler
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
