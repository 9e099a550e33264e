"""fp64 restatement of the cyclic-prefix timing estimator (include/dccn.h ``dccn_frame_sync``) and the inputs the frame-sync
tests share (tests/test_frame_sync_ref.py on the host, tests/test_gpu_frame_sync.py on the GPU).

The definition, per frame of T = S (K + CP) complex samples taken as circular, N = K + CP:

    p[n] = y[n] conj(y[n + K])                    e[n] = (|y[n]|^2 + |y[n + K]|^2) / 2
    Gamma(t) = sum_{s < S} sum_{n < CP} p[s N + t + n]          Phi(t) likewise over e
    Lambda(t) = |Gamma(t)| - Phi(t)
    offset = the smallest t in [-W, W] with the largest Lambda(t)          aligned[n] = y[(n + offset) mod T]

``reference`` states it with direct double loops over (s, n) -- no sliding window, no running sums -- vectorised over the
frames only.

Tolerances (from the definition, not from the kernel): a sum of n = S CP products in fp32 is off by at most about
(n + 4) 2^-24 sum|terms|, and |p| <= e, so |Lambda32 - Lambda64| <= METRIC_TOL max_t Phi64(t) per frame (6.9e-6 in the worst
case at n = 112; 1e-5 is the project's bar).  A frame is *decidable* when its fp64 best lag leads every other by more than
MARGIN max_t Phi64(t) = twice the two-sided tolerance: there the fp32 argmax must equal the fp64 one exactly.  At most CAP of a
case's frames may be undecidable, which the host test asserts of the reference alone.
"""
import numpy as np

METRIC_TOL = 1e-5
MARGIN = 4e-5
CAP = 0.02

S, K = 7, 64
SHAPES = ((S, K, 16), (S, K, 4))                       # the two prefix lengths of the driver grid
WINDOWS = {16: (16, 1, 3), 4: (4, 1)}                  # W per CP: W = CP, W = 1, and W = 3 at CP = 16
FRAME_COUNTS = (1, 5, 73, 300)                         # one wave; a ragged last block of four; 73; many blocks
CHANNELS = ("AWGN", "EPA", "EVA", "ETU")
SNRS = (5.0, 30.0)
SEED = 3
MAX_FRAMES = max(FRAME_COUNTS)


def reference(x, K, CP, W):
    """x [frames, S, K + CP, 2] (any float type) -> (offset int [frames], Lambda fp64 [frames, 2 W + 1], Phi fp64 likewise)."""
    x = np.asarray(x, dtype=np.float64)
    frames, S_, N = x.shape[0], x.shape[1], x.shape[2]
    assert N == K + CP and 1 <= W <= CP
    T = S_ * N
    y = (x[..., 0] + 1j * x[..., 1]).reshape(frames, T)
    lam = np.zeros((frames, 2 * W + 1))
    phi = np.zeros((frames, 2 * W + 1))
    for c, t in enumerate(range(-W, W + 1)):
        gamma = np.zeros(frames, dtype=np.complex128)
        energy = np.zeros(frames)
        for s in range(S_):
            for n in range(CP):
                a = y[:, (s * N + t + n) % T]
                b = y[:, (s * N + t + n + K) % T]
                gamma += a * np.conj(b)
                energy += 0.5 * (a.real ** 2 + a.imag ** 2 + b.real ** 2 + b.imag ** 2)
        lam[:, c] = np.abs(gamma) - energy
        phi[:, c] = energy
    offset = np.argmax(lam, axis=1) - W                 # (numpy.argmax: the first, i.e. smallest, lag on ties)
    return offset.astype(np.int64), lam, phi


def decidable(lam, phi):
    """bool [frames]: the best lag leads every other by more than MARGIN max_t Phi(t)"""
    srt = np.sort(lam, axis=1)
    return (srt[:, -1] - srt[:, -2]) > MARGIN * phi.max(axis=1)


def roll_frames(x, d):
    """every frame delayed by d samples, circularly: out[f, n] = x[f, (n - d) mod T]"""
    x = np.asarray(x)
    frames = x.shape[0]
    return np.ascontiguousarray(np.roll(x.reshape(frames, -1, 2), d, axis=1).reshape(x.shape))


def aligned(x, offset):
    """aligned[f, n] = x[f, (n + offset[f]) mod T], in x's own dtype (a pure data movement)"""
    x = np.asarray(x)
    out = np.empty_like(x)
    for f in range(x.shape[0]):
        out[f] = np.roll(x[f].reshape(-1, 2), -int(offset[f]), axis=0).reshape(x.shape[1:])
    return out


# ---- shared inputs: the host substrate's frames (receiver_mp.make_batch), QPSK, one fixed seed per case ---------------
_frames, _refs = {}, {}


def _flags(channel, CP):
    from dl_ofdm_amd.receiver_mp import Flags
    return Flags(channel=channel, nbits=2, nfft=K, nsymbol=S, longcp=(CP == 16), nfilter=64)


def case_frames(channel, snr, CP):
    """float32 [MAX_FRAMES, S, K + CP, 2]; a case of fewer frames takes the leading ones"""
    key = (channel, float(snr), CP)
    if key not in _frames:
        from dl_ofdm_amd import ofdm
        from dl_ofdm_amd.receiver_mp import RayleighChanParallel, make_batch
        F = _flags(channel, CP)
        o = ofdm.ofdm_tx(F)
        assert (o.K, o.CP) == (K, CP)
        np.random.seed(SEED + 101 * CHANNELS.index(channel) + int(snr) + 7 * CP)
        fading = RayleighChanParallel(F, o.Fs)
        xs = make_batch(F, o, fading, MAX_FRAMES, float(snr))[0]
        assert xs.shape == (MAX_FRAMES, S, K + CP, 2) and xs.dtype == np.float32
        xs.setflags(write=False)
        _frames[key] = xs
    return _frames[key]


def case_reference(channel, snr, CP, W):
    """(offset, Lambda, Phi, decidable) of the case's MAX_FRAMES frames, computed once"""
    key = (channel, float(snr), CP, W)
    if key not in _refs:
        off, lam, phi = reference(case_frames(channel, snr, CP), K, CP, W)
        _refs[key] = (off, lam, phi, decidable(lam, phi))
    return _refs[key]


def all_cases():
    """(CP, W, channel, snr) of every GPU case"""
    return [(CP, W, ch, snr) for (_, _, CP) in SHAPES for W in WINDOWS[CP] for ch in CHANNELS for snr in SNRS]
