"""fp64 restatement of ONE carrier-frequency offset per capture, pooled over its frames (include/dccn.h
``dccn_capture_sync_pooled``), and the captures its tests share (tests/test_capture_pool_ref.py on the host,
tests/test_gpu_capture_pooled.py on the GPU).  Timing is tests/capture_sync_ref.py's, imported as ``C``; on top of it, per call:

    theta_f, Gamma_f(t) = C.reference's               (b_f = first + f stride, the capture indexed linearly)
    Gamma = sum_{f < frames} Gamma_f(theta_f)          (the plain sum: |Gamma_f| weights a frame by its prefix energy)
    eps   = 0 - atan2(Im Gamma, Re Gamma) / (2 pi)     (one value per call; +0 where Gamma = 0)
    out[f][n] = c[b_f + theta_f + n] exp(-2 pi i eps n / K),   n = 0 .. T-1

The order of the sum, as the header states it: 64 partial sums, partial l adding Gamma_l, Gamma_{l+64}, ... in ascending order onto
+0; then a butterfly over the partials, d = 1, 2, 4, 8, 16, 32: partial l becomes partial l + partial (l xor d), every l at once;
partial 0 is Gamma.  ``pooled_sum`` walks exactly that order (in the dtype it is given: fp64 for the reference, and in float32 it
is the kernel's arithmetic), so ``DEPTH(frames)`` -- the rounded additions a Gamma_f passes through -- is read off the same text.

Tolerance of the estimate (``pool_bound``, frame_cfo_ref.cfo_bound carried over the frames): each component of a Gamma_f is an
S CP-term fp32 sum, off by at most sqrt(2) METRIC_TOL max_t Phi_f; the pooled sum adds d = DEPTH(frames) roundings, each at most
2^-24 of a partial sum that is itself at most sum_f |Gamma_f|; the angle of Gamma moves by at most |dGamma| / |Gamma|; 1e-6 rad
covers atan2f and the division.  In turns:

    (sqrt(2) METRIC_TOL sum_f max_t Phi_f + d 2^-24 sum_f |Gamma_f|) / (2 pi |Gamma|) + 1e-6 / (2 pi)

It widens by itself where the frames' correlations cancel (small |Gamma|), so no frame and no case is left out.
"""
import numpy as np

import capture_sync_ref as C
import frame_sync_ref as R
from dl_ofdm_amd.radio import apply_cfo_stream

LANES = 64


def DEPTH(frames):
    """the largest number of rounded fp32 additions a Gamma_f passes through: the lane's chain (its first addition, onto +0,
    is exact), then the six butterfly steps"""
    return -(-int(frames) // LANES) - 1 + 6


def pooled_sum(gf):
    """sum of gf [frames] (complex, or a real array) in the stated order, in gf's own dtype"""
    gf = np.asarray(gf)
    part = np.zeros(LANES, dtype=gf.dtype)
    for f0 in range(0, gf.shape[0], LANES):             # lane l: frames l, l + 64, ... ascending
        chunk = gf[f0:f0 + LANES]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    d = 1
    while d < LANES:                                    # the butterfly: every lane adds its partner's value
        part = part + part[np.arange(LANES) ^ d]
        d <<= 1
    return part[0]


def cfo_of(gamma):
    """fp64, subcarrier spacings; 0 - a: +0 where the angle is 0 (numpy.arctan2(0, 0) = 0)"""
    return 0.0 - np.arctan2(np.imag(gamma), np.real(gamma)) / (2.0 * np.pi)


def pooled(gam, offset, W):
    """(Gamma_f(offset_f) complex128 [frames], Gamma, eps) from C.reference's Gamma table and ANY offsets (the reference's own,
    or the GPU's: then no frame is left out)"""
    gf = C.gamma_at(gam, offset, W)
    total = pooled_sum(gf)
    return gf, total, float(cfo_of(total))


def reference(cap, first, stride, frames, S, K, CP, W):
    """cap [n, 2] -> (offset, Lambda, Phi, Gamma table, Gamma_f(offset_f), Gamma, eps)"""
    off, lam, phi, gam = C.reference(cap, first, stride, frames, S, K, CP, W)
    gf, total, eps = pooled(gam, off, W)
    return off, lam, phi, gam, gf, total, eps


def derotated(cap, first, stride, offset, eps, S, K, CP):
    """fp64 [frames, S, K + CP, 2]: every frame cut at its own offset and derotated with the ONE eps"""
    return C.derotated(cap, first, stride, offset, np.full(len(offset), float(eps)), S, K, CP)


def pool_bound(phi, gf, total):
    """the bound on |eps32 - eps64| on the circle, in turns (module docstring); phi [frames, 2 W + 1], gf [frames], total = Gamma"""
    frames = gf.shape[0]
    num = np.sqrt(2.0) * R.METRIC_TOL * phi.max(axis=1).sum() + DEPTH(frames) * 2.0 ** -24 * np.abs(gf).sum()
    return num / (2.0 * np.pi * np.abs(total)) + 1e-6 / (2.0 * np.pi)


# ---- what the definition is NOT (the planted errors of the host test) ---------------------------------------------------
def mean_of_angles(gf):
    """the mean of the per-frame estimates"""
    return float(np.mean(cfo_of(gf)))


def unit_vector_sum(gf):
    """the angle of sum_f Gamma_f / |Gamma_f|: every frame weighted alike, faded or not"""
    return float(cfo_of(np.sum(gf / np.abs(gf))))


# ---- shared inputs: capture_sync_ref's captures under ONE common offset ----------------------------------------------------
EPS = (0.137, -0.31)
# (channel, snr, CP, W): the fading cases of the estimator claim, and the one where every estimator agrees
FADING = (("ETU", 5.0, 16, 3), ("EPA", 5.0, 16, 3), ("ETU", 5.0, 4, 4), ("EVA", 30.0, 4, 1))
_caps, _long, _refs = {}, {}, {}


def case_capture(channel, snr, CP, spare, eps):
    """(cap float32 [75 (T + spare), 2] read-only, stride): C.case_capture(..., cfo=False) with the phase of ONE offset running
    over the whole capture (radio.apply_cfo_stream)"""
    key = (channel, float(snr), CP, spare, float(eps))
    if key not in _caps:
        cap, stride = C.case_capture(channel, snr, CP, spare, cfo=False)
        out = apply_cfo_stream(cap, eps, R.K)
        assert out.dtype == np.float32 and out.shape == cap.shape
        out.setflags(write=False)
        _caps[key] = (out, stride)
    return _caps[key]


def long_capture(channel, snr, CP, eps, spare=0):
    """(cap, stride = T + spare): all R.MAX_FRAMES = 300 frames of the case under one offset (the 259-frame cases)"""
    key = (channel, float(snr), CP, float(eps), spare)
    if key not in _long:
        cap, stride = C.contiguous_capture(R.case_frames(channel, snr, CP), spare)
        out = apply_cfo_stream(cap, eps, R.K)
        out.setflags(write=False)
        _long[key] = (out, stride)
    return _long[key]


def case_reference(channel, snr, CP, W, spare, shift, eps, frames=C.FRAMES):
    """``reference`` of the case's leading ``frames`` frames from first = T + shift, computed once"""
    key = (channel, float(snr), CP, W, spare, shift, float(eps), frames)
    if key not in _refs:
        cap, stride = case_capture(channel, snr, CP, spare, eps)
        _refs[key] = reference(cap, C.case_first(CP, shift), stride, frames, R.S, R.K, CP, W)
    return _refs[key]
