"""fp64 restatement of coarse acquisition inside a contiguous capture (include/dccn.h ``dccn_capture_acquire``) and the captures
its tests share (tests/test_capture_acquire_ref.py on the host, tests/test_gpu_capture_acquire.py on the GPU).

The definition: c = the capture, indexed linearly; N = K + CP, T = S N; lo the search origin, J the number of frames used;
p[n] = c[n] conj(c[n + K]), e[n] = (|c[n]|^2 + |c[n + K]|^2) / 2.

Stage A, for r in [0, N):
    Gamma(r) = sum_{u < J S} sum_{n < CP} p[lo + r + u N + n]       Phi(r) likewise over e       Lambda(r) = |Gamma(r)| - Phi(r)
    r^ = the smallest r with the largest Lambda(r)                  eps^ = -atan2(Im Gamma(r^), Re Gamma(r^)) / (2 pi)
Stage B, pilot symbols = the symbols with at least two pilot cells, k_0 < k_1 < ... the pilot carriers of pilot symbol s, q in [0, S):
    Y_{j,q,s}[k] = sum_{n < K} c[lo + r^ + (q + s) N + j T + CP + n] exp(-2 pi i (k + eps^) n / K)
    D(q) = sum_{j < J} sum_{pilot symbols s} | sum_i Y_{j,q,s}[k_i] conj(Y_{j,q,s}[k_{i+1}]) |
    q^ = the smallest q with the largest D(q)                       first = lo + r^ + q^ N

``stage_a`` and ``stage_b`` state it with direct loops (no sliding sums, no FFT), vectorised over the lags r / the pilot carriers
only.  The twiddle's turns are reduced exactly: (k n mod K) is an integer, so the fp64 phase is good to 1e-15.

Error bounds of an fp32 evaluation (u = 2^-24), from the definition's term counts, not from the kernel:

* Lambda.  The library documents the order of the J S CP-term sums: the J S symbols first, then the CP lags.  A term passes
  through at most (J S - 1) + (CP - 1) additions and its product carries up to 4 roundings: each component of Gamma, and Phi, is
  off by at most g_A sum|terms|, g_A = (J S + CP + 4) u.  |Re p| + |Im p| <= sqrt(2) |p| and |p| <= e, so |dGamma| <= sqrt(2) g_A Phi,
  dPhi <= g_A Phi, and with the square root and the subtraction (2 u)
      |Lambda32(r) - Lambda64(r)| <= LAMBDA_TOL max_r Phi(r),      LAMBDA_TOL = (1 + sqrt(2)) g_A + 2 u           (``lambda_tol``)
  r^ is *decidable* when the fp64 best lag leads every other by more than 2 LAMBDA_TOL max Phi (both may move, in opposite
  directions): there the fp32 argmax must be the fp64 one.
* eps^: frame_cfo_ref's bound with the components of Gamma off by g_A Phi; g_A <= frame_sync_ref.METRIC_TOL for every shape used
  here (asserted), so ``frame_cfo_ref.cfo_bound`` applies as it stands.
* D.  One window of K samples, A = sum_n |c_n| <= sqrt(K E), E the window's energy.  The twiddle: eps^ n (<= K / 2, one rounding),
  plus the integer (< 3 K / 2, one rounding), divided by K (one rounding): the turns are off by at most 3.5 u, the phase by 2 pi 3.5 u
  < 22 u; sincospif adds 4 u: |dw| <= 26 u.  The K-term complex sum: each component (K + 3) u sum|terms|, sum|terms| <= A.  So
      |dY[k]| <= g_Y A,   g_Y = (sqrt(2) (K + 3) + 26) u,   and |Y[k]| <= A.
  A product Y_i conj(Y_{i+1}) moves by at most (2 g_Y + g_Y^2) A^2; the (P - 1)-term complex sum of products adds
  sqrt(2) (P + 2) u per unit of sum|Y_i||Y_{i+1}| <= (P - 1) A^2; the modulus 2 u.  With A^2 <= K E:
      |d inner_{j,q,s}| <= (P_s - 1) K E_{j,q,s} (2 g_Y + g_Y^2 + (sqrt(2) (P_s + 2) + 2) u)
  and the sum over the J n_ps moduli adds (J n_ps) u D(q).  ``stage_b`` returns that bound per q.  q^ is decidable when the fp64 best
  leads every other q by more than the sum of the two bounds.

At most CAP of the GPU cases may be undecidable; the host test asserts that of the reference alone.
"""
import numpy as np

import frame_sync_ref as R

U = 2.0 ** -24
CAP = 0.02
S, K = R.S, R.K


def complex_of(cap):
    cap = np.asarray(cap, dtype=np.float64)
    assert cap.ndim == 2 and cap.shape[1] == 2
    return cap[:, 0] + 1j * cap[:, 1]


def lambda_tol(J, S_, CP):
    return (1.0 + np.sqrt(2.0)) * (J * S_ + CP + 4) * U + 2 * U


def stage_a(cap, lo, J, S_, K_, CP):
    """-> (r^, eps^ fp64, Lambda fp64 [N], Phi [N], Gamma complex128 [N])"""
    c = complex_of(cap)
    N = K_ + CP
    assert lo >= 0 and lo + (J + 2) * S_ * N <= c.shape[0]
    r = np.arange(N)
    gamma = np.zeros(N, dtype=np.complex128)
    phi = np.zeros(N)
    for u in range(J * S_):
        for n in range(CP):
            a = c[lo + r + u * N + n]
            b = c[lo + r + u * N + n + K_]
            gamma += a * np.conj(b)
            phi += 0.5 * (a.real ** 2 + a.imag ** 2 + b.real ** 2 + b.imag ** 2)
    lam = np.abs(gamma) - phi
    rhat = int(np.argmax(lam))                          # (numpy.argmax: the first, i.e. smallest, lag on ties)
    eps = float(-np.arctan2(gamma[rhat].imag, gamma[rhat].real) / (2.0 * np.pi))
    return rhat, eps, lam, phi, gamma


def a_decidable(lam, phi, J, S_, CP):
    srt = np.sort(lam)
    return bool(srt[-1] - srt[-2] > 2.0 * lambda_tol(J, S_, CP) * phi.max())


def pilot_symbols(pilot_sc, S_, K_):
    """[(s, carriers ascending)] of the symbols that hold at least two pilot cells"""
    sc = np.asarray(pilot_sc, dtype=np.int64)
    assert (np.diff(sc) > 0).all() and sc[0] >= 0 and sc[-1] < S_ * K_
    out = []
    for s in range(S_):
        ks = sc[sc // K_ == s] % K_
        if len(ks) >= 2:
            out.append((s, ks))
    return out


def stage_b(cap, lo, rhat, eps, J, S_, K_, CP, pilot_sc):
    """D fp64 [S] and its fp32 error bound [S], evaluated at the given r^ and eps^"""
    c = complex_of(cap)
    N = K_ + CP
    T = S_ * N
    ps = pilot_symbols(pilot_sc, S_, K_)
    D = np.zeros(S_)
    bound = np.zeros(S_)
    g_y = (np.sqrt(2.0) * (K_ + 3) + 26.0) * U
    for q in range(S_):
        for j in range(J):
            for s, ks in ps:
                at = lo + rhat + (q + s) * N + j * T + CP
                Y = np.zeros(len(ks), dtype=np.complex128)
                energy = 0.0
                for n in range(K_):
                    turns = (((ks * n) % K_) + eps * n) / float(K_)
                    Y += c[at + n] * np.exp(-2j * np.pi * turns)
                    energy += c[at + n].real ** 2 + c[at + n].imag ** 2
                inner = 0j
                for i in range(len(ks) - 1):
                    inner += Y[i] * np.conj(Y[i + 1])
                D[q] += abs(inner)
                P = len(ks)
                bound[q] += (P - 1) * K_ * energy * (2 * g_y + g_y ** 2 + (np.sqrt(2.0) * (P + 2) + 2) * U)
        bound[q] += J * len(ps) * U * D[q]
    return D, bound


def b_decidable(D, bound):
    top = int(np.argmax(D))
    rest = np.delete(np.arange(len(D)), top)
    return bool((D[top] - D[rest] > bound[top] + bound[rest]).all())


def tied_maxima(D, bound):
    """the q that an fp32 evaluation may return: those whose D is within the two bounds of the largest"""
    top = int(np.argmax(D))
    return [q for q in range(len(D)) if D[top] - D[q] <= bound[top] + bound[q]]


def reference(cap, lo, J, S_, K_, CP, pilot_sc):
    """the whole definition in fp64 -> dict(r, eps, lam, phi, gamma, D, bound, q, first, a_ok, b_ok)"""
    rhat, eps, lam, phi, gamma = stage_a(cap, lo, J, S_, K_, CP)
    D, bound = stage_b(cap, lo, rhat, eps, J, S_, K_, CP, pilot_sc)
    q = int(np.argmax(D))
    return dict(r=rhat, eps=eps, lam=lam, phi=phi, gamma=gamma, D=D, bound=bound, q=q, first=lo + rhat + q * (K_ + CP),
                a_ok=a_decidable(lam, phi, J, S_, CP), b_ok=b_decidable(D, bound))


# ---- captures: the host model's frames through run_stream, AWGN and apply_cfo_stream, begun inside frame 0 ----------------------
def flags(channel, CP, nbits):
    from dl_ofdm_amd.receiver_mp import Flags
    return Flags(channel=channel, nbits=nbits, nfft=K, nsymbol=S, longcp=(CP == 16), nfilter=64)


def pilot_sc_of(CP, nbits=2):
    from dl_ofdm_amd import ofdm
    return np.asarray(ofdm.ofdm_tx(flags("AWGN", CP, nbits)).pilotSc, dtype=np.int32)


def build_capture(channel, snr, CP, nbits, frames, cut, eps, seed):
    """``frames`` transmitted frames through ``channel`` (``"AWGN"``: the identity) at ``snr`` dB (``None``: no noise) with a
    carrier offset of ``eps`` subcarrier spacings, as one capture that begins ``cut`` samples into frame 0 (0 <= cut < T).
    -> (cap float32 [n, 2] read-only, start: the sample of the capture at which frame 1 starts -- frames start at start + m T)"""
    from dl_ofdm_amd import ofdm, util
    from dl_ofdm_amd.radio import apply_cfo_stream, rayleigh_chan_lte
    Fl = flags(channel, CP, nbits)
    o = ofdm.ofdm_tx(Fl)
    assert (o.K, o.CP) == (K, CP)
    T = S * (K + CP)
    assert 0 <= cut < T
    np.random.seed(seed)
    bits = util.bit_source(nbits, o.frame_size, frames)
    iq, _, _ = o.ofdm_tx_frame_np(bits)
    lead = 40
    cap, _ = rayleigh_chan_lte(Fl, o.Fs).run_stream(iq, lead)
    cap = cap.astype(np.complex128)
    body = cap[lead:lead + frames * T]
    cap = cap / np.sqrt(np.mean(np.abs(body) ** 2))                   # unit mean power over the frames, as AWGN_channel_np scales
    if snr is not None:
        std = np.sqrt(0.5) * 10.0 ** (-float(snr) / 20.0)
        cap = cap + std * (np.random.randn(cap.shape[0]) + 1j * np.random.randn(cap.shape[0]))
    cap = apply_cfo_stream(cap, eps, K)[lead + cut:]
    out = np.ascontiguousarray(np.stack([cap.real, cap.imag], axis=-1).astype(np.float32))
    out.setflags(write=False)
    return out, T - cut


def true_first(start, lo, T):
    """the frame start inside [lo, lo + T)"""
    return lo + (start - lo) % T


# ---- the cases of the GPU test -------------------------------------------------------------------------------------------------
CHANNELS = (("AWGN", 30.0), ("ETU", 5.0))
JS = (1, 2, 16)
LOS = (0, 37, 300, 555)                               # even and odd origins
SEEDS = (0, 1)
NBITS = 2                                             # QPSK, as the other sync cases; J = 1 with BPSK is a case of its own


def gpu_cases():
    """(CP, J, lo, channel, snr, seed): 2 x 3 x 4 x 2 x 2 = 96 captures"""
    return [(CP, J, lo, ch, snr, seed) for CP in (16, 4) for J in JS for lo in LOS for (ch, snr) in CHANNELS for seed in SEEDS]


_caps, _refs = {}, {}


def case_capture(CP, channel, snr, seed, nbits=NBITS):
    """one capture per (CP, channel, snr, seed): 21 frames, begun at a seed-dependent sample of frame 0; every J and lo reads it"""
    key = (CP, channel, float(snr), seed, nbits)
    if key not in _caps:
        T = S * (K + CP)
        rs = np.random.RandomState(900 + 31 * seed + CP + (7 if channel != "AWGN" else 0) + 1000 * nbits)
        cut = int(rs.randint(0, T))
        eps = float(rs.uniform(-0.45, 0.45))
        _caps[key] = build_capture(channel, snr, CP, nbits, 21, cut, eps, seed=4000 + seed + 13 * CP) + (eps,)
    return _caps[key]


def case_reference(CP, J, lo, channel, snr, seed, nbits=NBITS):
    key = (CP, J, lo, channel, float(snr), seed, nbits)
    if key not in _refs:
        cap, _, _ = case_capture(CP, channel, snr, seed, nbits)
        _refs[key] = reference(cap, lo, J, S, K, CP, pilot_sc_of(CP, nbits))
    return _refs[key]
