"""fp64 restatement of the cyclic-prefix estimator on frames that sit inside ONE CONTIGUOUS CAPTURE (include/dccn.h
``dccn_capture_sync``) and the captures its tests share (tests/test_capture_sync_ref.py on the host,
tests/test_gpu_capture_sync.py on the GPU).

The definition: c = the capture, indexed linearly; frame f nominally starts at b_f = first + f stride; N = K + CP, T = S N:

    p[n] = c[n] conj(c[n + K])                    e[n] = (|c[n]|^2 + |c[n + K]|^2) / 2
    Gamma_f(t) = sum_{s < S} sum_{n < CP} p[b_f + s N + t + n]          Phi_f likewise over e          Lambda = |Gamma| - Phi
    offset_f = the smallest t in [-W, W] with the largest Lambda_f(t)
    cfo_f = -atan2(Im Gamma_f(offset_f), Re Gamma_f(offset_f)) / (2 pi)
    out_f[n] = c[b_f + offset_f + n] exp(-2 pi i cfo_f n / K),   n = 0 .. T-1

``reference`` states it with direct double loops over (s, n) on linear indices, vectorised over the frames only.

Tolerances: frame_sync_ref's and frame_cfo_ref's, unchanged -- the sums have the same S CP terms, bounded the same way; only the
places the terms are read from differ.
"""
import numpy as np

import frame_sync_ref as R


def complex_of(cap):
    cap = np.asarray(cap, dtype=np.float64)
    assert cap.ndim == 2 and cap.shape[1] == 2
    return cap[:, 0] + 1j * cap[:, 1]


def starts(first, stride, frames):
    return int(first) + int(stride) * np.arange(int(frames), dtype=np.int64)


def reference(cap, first, stride, frames, S, K, CP, W):
    """cap [n, 2] -> (offset int64 [frames], Lambda fp64 [frames, 2 W + 1], Phi likewise, Gamma complex128 [frames, 2 W + 1])"""
    c = complex_of(cap)
    N = K + CP
    T = S * N
    b = starts(first, stride, frames)
    assert 1 <= W <= CP and stride >= T and b[0] - W >= 0 and b[-1] + T + W <= c.shape[0]
    lam = np.zeros((frames, 2 * W + 1))
    phi = np.zeros((frames, 2 * W + 1))
    gam = np.zeros((frames, 2 * W + 1), dtype=np.complex128)
    for col, t in enumerate(range(-W, W + 1)):
        gamma = np.zeros(frames, dtype=np.complex128)
        energy = np.zeros(frames)
        for s in range(S):
            for n in range(CP):
                u = c[b + s * N + t + n]
                v = c[b + s * N + t + n + K]
                gamma += u * np.conj(v)
                energy += 0.5 * (u.real ** 2 + u.imag ** 2 + v.real ** 2 + v.imag ** 2)
        lam[:, col] = np.abs(gamma) - energy
        phi[:, col] = energy
        gam[:, col] = gamma
    offset = np.argmax(lam, axis=1) - W                 # (numpy.argmax: the first, i.e. smallest, lag on ties)
    return offset.astype(np.int64), lam, phi, gam


def gamma_at(gam, offset, W):
    """Gamma_f(offset_f), complex128 [frames]"""
    return gam[np.arange(gam.shape[0]), np.asarray(offset, dtype=np.int64) + W]


def cut(cap, first, stride, offset, S, K, CP):
    """out[f, n] = cap[b_f + offset_f + n] in cap's own dtype (a pure data movement): [frames, S, K + CP, 2]"""
    cap = np.asarray(cap)
    T = S * (K + CP)
    b = starts(first, stride, len(offset)) + np.asarray(offset, dtype=np.int64)
    return np.stack([cap[s:s + T] for s in b]).reshape(len(offset), S, K + CP, 2)


def derotated(cap, first, stride, offset, cfo, S, K, CP):
    """fp64 [frames, S, K + CP, 2]: out[n] = c[b_f + offset_f + n] exp(-2 pi i cfo_f n / K) from the given offsets / estimates"""
    x = cut(np.asarray(cap, dtype=np.float64), first, stride, offset, S, K, CP)
    T = S * (K + CP)
    y = (x[..., 0] + 1j * x[..., 1]).reshape(len(offset), T)
    out = y * np.exp(-2j * np.pi * np.asarray(cfo, dtype=np.float64)[:, None] * np.arange(T)[None, :] / float(K))
    return np.stack([out.real, out.imag], axis=-1).reshape(x.shape)


# ---- captures -----------------------------------------------------------------------------------------------------
def padded_capture(x, W):
    """Every frame of x [frames, S, N, 2] in a slot [its last W samples | the frame | its first W samples]: on this capture
    (first = W, stride = T + 2 W) the linear window of a frame holds exactly what the circular estimator reads.
    -> (cap [frames (T + 2 W), 2] in x's dtype, first, stride)"""
    x = np.asarray(x)
    frames = x.shape[0]
    y = x.reshape(frames, -1, 2)
    T = y.shape[1]
    cap = np.concatenate([y[:, T - W:], y, y[:, :W]], axis=1).reshape(frames * (T + 2 * W), 2)
    return np.ascontiguousarray(cap), W, T + 2 * W


def contiguous_capture(x, spare=0):
    """The frames of x [frames, S, N, 2] one after the other, ``spare`` zero samples behind each: (cap [frames (T + spare), 2],
    stride = T + spare)"""
    x = np.asarray(x)
    frames = x.shape[0]
    y = x.reshape(frames, -1, 2)
    T = y.shape[1]
    if spare:
        y = np.concatenate([y, np.zeros((frames, spare, 2), y.dtype)], axis=1)
    return np.ascontiguousarray(y.reshape(-1, 2)), T + spare


# ---- the contiguous cases of the GPU tests ------------------------------------------------------------------------------
FRAMES = 73                                     # frames 1 .. 73 of a 75-frame capture
CASES = ((16, 16, "AWGN", 30.0), (16, 3, "ETU", 5.0), (16, 3, "EVA", 30.0), (16, 1, "EPA", 5.0), (16, 16, "ETU", 30.0),
         (4, 4, "ETU", 5.0), (4, 1, "EVA", 30.0), (4, 4, "AWGN", 5.0))         # (CP, W, channel, snr), all of R.all_cases()
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))      # (spare samples between frames: stride = T + spare; first - T)
_caps, _refs = {}, {}


def case_capture(channel, snr, CP, spare, cfo=False):
    """(cap float32 [75 (T + spare), 2] read-only, stride) of the case's leading 75 frames (``cfo``: frame_cfo_ref's impaired
    frames, every frame with its own offset)"""
    key = (channel, float(snr), CP, spare, bool(cfo))
    if key not in _caps:
        if cfo:
            import frame_cfo_ref as F
            xs = F.case_frames(channel, snr, CP)
        else:
            xs = R.case_frames(channel, snr, CP)
        cap, stride = contiguous_capture(xs[:FRAMES + 2], spare)
        assert cap.dtype == np.float32
        cap.setflags(write=False)
        _caps[key] = (cap, stride)
    return _caps[key]


def case_first(CP, shift):
    """T + shift: one whole frame of the capture lies in front of the first window (with a spare sample between the frames,
    shift = 1 is frame 1's own start and shift = 0 one sample early; without, shift = 0 is its start and 1 one sample late)"""
    return R.S * (R.K + CP) + shift


def case_reference(channel, snr, CP, W, spare, shift, cfo=False):
    """(offset, Lambda, Phi, Gamma, decidable) of the case's 73 frames, computed once"""
    key = (channel, float(snr), CP, W, spare, shift, bool(cfo))
    if key not in _refs:
        cap, stride = case_capture(channel, snr, CP, spare, cfo)
        off, lam, phi, gam = reference(cap, case_first(CP, shift), stride, FRAMES, R.S, R.K, CP, W)
        _refs[key] = (off, lam, phi, gam, R.decidable(lam, phi))
    return _refs[key]
