"""``dccn_gen_static_apply_sync`` (csrc/datagen.h gen_apply_sync_kernel): the launch that forms x = y / sqrt(mean |y|^2) + noise in
LDS, runs the cyclic-prefix estimator on it and writes the rotated frame once, ``-m gpu``.

The oracle is the project's own two-launch sequence on the SAME descriptor after ``dccn_gen_static_frames``:
``dccn_gen_static_apply`` then ``dccn_frame_sync`` (held to an fp64 restatement by tests/test_gpu_frame_sync.py).  x, offsets and
noise power must agree bit for bit -- ``torch.equal``, no tolerance, no frame left out.  The in-place rotation of the frequency
response is held to fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)
S, K = 7, 64


def make_gen(chan, longcp, n, snr_db, seed=21, offset=4):
    """(gen, fg) on the N = 64 grid, QPSK; mixRayleigh runs with ``mix`` (Doppler on every third frame: the Doppler launch)"""
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen, FusedStaticGen
    from dl_ofdm_amd.receiver import Flags
    F = Flags(channel=chan, nfilter=64, nbits=2, SNR=snr_db, longcp=longcp)
    mixed = chan.startswith("mix")
    gen = DeviceDataGen(F, ofdm.ofdm_tx(F), seed=seed, mobile=mixed, mix=mixed)
    assert (gen.S, gen.K, gen.CP) == (S, K, 16 if longcp else 4)
    gen.offset = offset
    fg = FusedStaticGen(gen, n, snr_db, want_noise_power=True)
    assert fg.has_doppler == mixed
    return gen, fg


def generate(gen, fg, per_symbol_H=True, tx_out=None):
    """one generator launch; (descriptor, labels, H as the generator wrote it)"""
    n = fg.n
    bits = torch.empty(n, gen.D, gen.nbits, dtype=torch.int32, device="cuda")
    H = torch.full((n, S, K, 2) if per_symbol_H else (n, K, 2), float("nan"), device="cuda")
    d = fg.arm(bits, 0, tx_out, H)
    st = gen._stream()
    assert gen.lib.dccn_gen_static_frames(C.byref(d), st) == 0
    return d, bits, H


def two_launch_oracle(gen, fg, d, W, out_kin):
    n = fg.n
    full = torch.empty(n, S, K + gen.CP, 2, device="cuda")
    x = torch.full((n, S, out_kin, 2), float("nan"), device="cuda")
    off = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    npow = torch.full((1,), float("nan"), device="cuda")
    st = gen._stream()
    assert gen.lib.dccn_gen_static_apply(C.byref(d), full.data_ptr(), npow.data_ptr(), st) == 0
    assert gen.lib.dccn_frame_sync(full.data_ptr(), n, S, K, gen.CP, W, out_kin, x.data_ptr(), off.data_ptr(), None, st) == 0
    return x, off, npow, full


def one_launch(gen, fg, d, W, out_kin, H=None, h_rep=0):
    n = fg.n
    x = torch.full((n, S, out_kin, 2), float("nan"), device="cuda")
    off = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    npow = torch.full((1,), float("nan"), device="cuda")
    st = gen.lib.dccn_gen_static_apply_sync(C.byref(d), W, out_kin, x.data_ptr(), off.data_ptr(),
                                            None if H is None else H.data_ptr(), h_rep, npow.data_ptr(), gen._stream())
    assert st == 0, st
    return x, off, npow


@pytest.mark.parametrize("n", [1, 5, 73])
@pytest.mark.parametrize("longcp", [True, False])
@pytest.mark.parametrize("chan", ["mixRayleigh", "EVA"])
def test_one_launch_equals_apply_then_frame_sync_bit_for_bit(chan, longcp, n):
    """frames 1 / 5 (a ragged last block of the four-frame blocks) / 73; CP 16 with W in {3, 16}, CP 4 with W in {3, 4}; the whole
    frames and the rows behind the prefix; mixRayleigh with ``mix`` and static EVA at 30 dB.  In the 73-frame mixRayleigh case
    at least two distinct offsets occur (the profiles alternate by frame: README's measured majority offsets 0 / -2 / -1 / 0)."""
    gen, fg = make_gen(chan, longcp, n, 30.0)
    d, _, _ = generate(gen, fg)
    CP = gen.CP
    for W in ((3, 16) if longcp else (3, 4)):
        for out_kin in (K + CP, K):
            xr, offr, npr, _ = two_launch_oracle(gen, fg, d, W, out_kin)
            xn, offn, npn = one_launch(gen, fg, d, W, out_kin)
            torch.cuda.synchronize()
            assert int(offr.min()) >= -W and int(offr.max()) <= W and bool(torch.isfinite(xr).all())
            assert torch.equal(offn, offr), (W, out_kin, offn.tolist(), offr.tolist())
            assert torch.equal(xn, xr), (W, out_kin, int((xn != xr).sum()))
            assert torch.equal(npn, npr) and float(npn) > 0.0
            if chan == "mixRayleigh" and n == 73:
                vals = torch.unique(offn).tolist()
                print("offsets", dict(CP=CP, W=W, out_kin=out_kin), vals)
                assert len(vals) >= 2


def ramp64(theta, reps):
    """exp(+2 pi i k theta / K) per frame in fp64, [n, 1 or nothing, K]"""
    k = np.arange(K)[None, :]
    m = (k * theta.astype(np.int64)[:, None]) % K
    r = np.exp(2j * np.pi * m / K)
    return r[:, None, :] if reps else r


@pytest.mark.parametrize("chan,longcp,per_symbol", [("EVA", True, False), ("EVA", True, True), ("mixRayleigh", True, True),
                                                    ("EVA", False, False), ("mixRayleigh", False, True)])
def test_H_inout_is_rotated_with_the_frame(chan, longcp, per_symbol):
    """H' = H exp(+2 pi i k offset / K) against fp64 with the launch's own offsets; every real component within
    8 * 2^-23 * |H[k]| (two products with a 1-ulp sine / cosine and one sum: under 4 ulp of |H[k]|; the bound leaves a factor of
    two).  h_rep = 1 (one row per frame) and h_rep = S; x and the offsets do not depend on whether H is given."""
    n, W = 73, 3
    gen, fg = make_gen(chan, longcp, n, 30.0)
    d, _, H = generate(gen, fg, per_symbol_H=per_symbol)
    torch.cuda.synchronize()
    H0 = torch.view_as_complex(H).cpu().numpy().astype(np.complex128)
    assert np.isfinite(H0).all()
    x0, off0, _ = one_launch(gen, fg, d, W, K + gen.CP)
    x1, off1, _ = one_launch(gen, fg, d, W, K + gen.CP, H=H, h_rep=S if per_symbol else 1)
    torch.cuda.synchronize()
    assert torch.equal(x0, x1) and torch.equal(off0, off1)
    theta = off1.cpu().numpy()
    assert (theta != 0).sum() >= 5
    want = H0 * ramp64(theta, per_symbol)
    got = torch.view_as_complex(H).cpu().numpy().astype(np.complex128)
    bound = 8.0 * 2.0 ** -23 * np.abs(H0)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    print("H rotation", chan, longcp, per_symbol, dict(worst=float((err / np.maximum(np.abs(H0), 1e-30)).max() / 2.0 ** -23),
                                                       rotated=int((theta != 0).sum())))
    assert (err <= bound).all()
    same = theta == 0                         # a frame that is not moved keeps its response to the bit
    assert np.array_equal(got[same], H0[same])


def test_rotation_sign_against_the_frames_themselves():
    """EVA at 60 dB: for the frames whose offset is not 0, the aligned frame's per-symbol FFT divided by the transmitted grid is
    closer in mean square to H' than to the unrotated H.  (H is ``fft(g)`` of the centred L-tap response, so both stand a fixed
    ramp of the (L - 1) // 2 samples' advance away from the measured response; the second assertion removes it: measured on the
    aligned frame over measured on the frame as generated is the ramp itself, and the opposite sign is further away.)"""
    n, W = 73, 3
    gen, fg = make_gen("EVA", True, n, 60.0)
    CP = gen.CP
    tx = torch.empty(n, S, K + CP, 2, device="cuda")
    d, _, H = generate(gen, fg, per_symbol_H=False, tx_out=tx)
    _, _, _, plain = two_launch_oracle(gen, fg, d, W, K + CP)
    torch.cuda.synchronize()
    H0 = torch.view_as_complex(H).cpu().numpy().astype(np.complex128)
    xa, off, _ = one_launch(gen, fg, d, W, K + CP, H=H, h_rep=1)
    torch.cuda.synchronize()
    H1 = torch.view_as_complex(H).cpu().numpy().astype(np.complex128)
    theta = off.cpu().numpy()
    sel = theta != 0
    assert sel.sum() >= 20                     # (EVA: the majority offset is -1)
    inv = 1.0 / np.sqrt(float((fg.y.double() ** 2).sum()) / (n * S * (K + CP)))
    cplx = lambda t: t.cpu().numpy().astype(np.float64).view(np.complex128)[..., 0]     # noqa: E731
    X = np.fft.fft(cplx(tx)[:, :, CP:], axis=-1) * inv
    used = np.abs(X) > 1e-6 * np.abs(X).max()
    Xs = np.where(used, X, 1.0)
    Ra = np.fft.fft(cplx(xa)[:, :, CP:], axis=-1) / Xs
    Rp = np.fft.fft(cplx(plain)[:, :, CP:], axis=-1) / Xs
    msq = lambda a, b: float((np.abs(a - b) ** 2 * used)[sel].sum() / used[sel].sum())      # noqa: E731
    to_rot, to_plain = msq(Ra, H1[:, None, :]), msq(Ra, H0[:, None, :])
    r = ramp64(theta, True)
    right, wrong = msq(Ra, Rp * r), msq(Ra, Rp * np.conj(r))
    print("sign", dict(to_rotated_H=to_rot, to_unrotated_H=to_plain, ratio_right=right, ratio_wrong=wrong, frames=int(sel.sum())))
    assert to_rot < to_plain
    assert right < 0.1 * wrong


def test_refusals_launch_nothing():
    """a bad W, a bad out_kin, a null offset, an x_out aliasing y or noise, a bad h_rep: DCCN_ERR_INVALID_ARG, and the
    sentinel-filled outputs are untouched"""
    n = 5
    gen, fg = make_gen("EVA", True, n, 30.0)
    d, _, H = generate(gen, fg)
    CP, lib, st = gen.CP, gen.lib, gen._stream()
    x = torch.full((n, S, K + CP, 2), -7.0, device="cuda")
    off = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    npow = torch.full((1,), -7.0, device="cuda")
    torch.cuda.synchronize()
    H_before, y_before, z_before = H.clone(), fg.y.clone(), fg.noise.clone()
    call = lambda W, kin, xo, of, Hp=None, rep=0: lib.dccn_gen_static_apply_sync(C.byref(d), W, kin, xo, of, Hp, rep, npow.data_ptr(), st)  # noqa: E731
    assert call(0, K + CP, x.data_ptr(), off.data_ptr()) == INVALID_ARG
    assert call(CP + 1, K + CP, x.data_ptr(), off.data_ptr()) == INVALID_ARG
    assert call(3, K + 1, x.data_ptr(), off.data_ptr()) == INVALID_ARG
    assert call(3, K + CP, x.data_ptr(), None) == INVALID_ARG
    assert call(3, K + CP, None, off.data_ptr()) == INVALID_ARG
    assert call(3, K + CP, x.data_ptr() + 4, off.data_ptr()) == INVALID_ARG
    assert call(3, K + CP, fg.y.data_ptr(), off.data_ptr()) == INVALID_ARG
    assert call(3, K, fg.y.data_ptr() + 16 * 64, off.data_ptr()) == INVALID_ARG
    assert call(3, K + CP, fg.noise.data_ptr(), off.data_ptr()) == INVALID_ARG
    assert call(3, K + CP, x.data_ptr(), off.data_ptr(), H.data_ptr(), 2) == INVALID_ARG
    assert lib.dccn_gen_static_apply_sync(None, 3, K + CP, x.data_ptr(), off.data_ptr(), None, 0, None, st) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((x == -7.0).all()) and bool((off == -99).all()) and float(npow) == -7.0
    assert torch.equal(H, H_before) and torch.equal(fg.y, y_before) and torch.equal(fg.noise, z_before)
    assert call(3, K + CP, x.data_ptr(), off.data_ptr()) == 0            # the same buffers, a legal call
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and int(off.abs().max()) <= 3


def test_two_calls_give_identical_bits():
    gen, fg = make_gen("mixRayleigh", False, 73, 30.0)
    d, _, H = generate(gen, fg)
    torch.cuda.synchronize()
    Ha, Hb = H.clone(), H.clone()
    a = one_launch(gen, fg, d, 4, K, H=Ha, h_rep=S)
    b = one_launch(gen, fg, d, 4, K, H=Hb, h_rep=S)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(Ha, Hb)


@pytest.mark.parametrize("window", [False, True])
def test_make_batch_sync_one_launch_and_three_launch_forms_agree(window):
    """FusedStaticGen.make_batch(sync=W): fused_sync=True and False give the same x, labels, offsets and noise power (bits) from
    the same (seed, offset); H agrees to the rounding of two different sines (1e-5 of its largest entry); without ``sync`` the
    call returns what it always did"""
    n, W = 9, 3
    out = []
    for fused in (True, False):
        gen, fg = make_gen("mixRayleigh", True, n, 30.0)
        x = torch.empty(n, S, K if window else K + gen.CP, 2, device="cuda")
        bits = torch.empty(n, gen.D, gen.nbits, dtype=torch.int32, device="cuda")
        H = torch.empty(n, S, K, 2, device="cuda")
        r = fg.make_batch(x, bits, slot=1, out_H=H, sync=W, fused_sync=fused)
        assert len(r) == 4 and r[3].dtype == torch.int32 and gen.offset == 5
        torch.cuda.synchronize()
        out.append((x, bits, r[2].clone(), r[3].clone(), H))
    (xa, ba, na, oa, Ha), (xb, bb, nb, ob, Hb) = out
    assert torch.equal(xa, xb) and torch.equal(ba, bb) and torch.equal(na, nb) and torch.equal(oa, ob)
    assert float((Ha - Hb).abs().max()) <= 1e-5 * float(Hb.abs().max())
    gen, fg = make_gen("mixRayleigh", True, n, 30.0)
    with pytest.raises(ValueError):
        fg.make_batch(xa, ba, sync=17)
    assert gen.offset == 4                       # refused before the descriptor was armed
    assert len(fg.make_batch(xa, ba)) == 3
