"""fp64 restatement of acquisition and the capture cut for carrier offsets beyond half a subcarrier spacing (include/dccn.h
``dccn_capture_acquire_wide``, ``dccn_capture_sync_wide``, ``dccn_capture_sync_pooled_wide``) and the captures its tests share
(tests/test_capture_wide_ref.py on the host, tests/test_gpu_capture_wide.py on the GPU).  Stage A, the captures and the narrow
stage B are tests/capture_acquire_ref.py's (``A``), the per-frame and pooled prefix estimates tests/capture_sync_ref.py's and
tests/capture_pool_ref.py's (``C``, ``P``).

Acquisition.  eps = m + f, m whole, |f| < 1/2: stage A gives r^ and eps^ = f; the pilots sit m bins up, so with Y of
capture_acquire_ref (twiddle turns ((k n mod K) + eps^ n) / K):

    D(q, m) = sum_{j < J} sum_{pilot symbols s} | sum_i Y_{j,q,s}[(k_i + m) mod K] conj(Y_{j,q,s}[(k_{i+1} + m) mod K]) |,  m in [-M, M]
    (q^, m^) = the first maximum of D in row-major order of [S, 2 M + 1]       first = lo + r^ + q^ N

``stage_b_wide`` states it with direct loops (no FFT): every bin of a symbol from its K samples, n ascending, then the shifted
products.  Its fp32 error bound per (q, m) is ``A.stage_b``'s per q, term for term: a bin is a K-term sum whichever bin it is,
|Y[k]| <= A for every k, and (q, m) sums the same J n_ps moduli of (P_s - 1)-term products.  (q^, m^) is *decidable* when the
fp64 best leads every other entry of D by more than the sum of the two bounds; at most CAP of the GPU cases may not be.

The cut.  The prefix gives a fraction eps_f (per frame, or pooled over the capture); with acquisition's pair (m^, eps^_acq):

    ref = m^ + eps^_acq        I = rint(ref - eps_f), kept inside [-K/2, K/2]        cfo_f = I + eps_f
    out_f[n] = c[b_f + theta_f + n] exp(-2 pi i cfo_f n / K)

``unwrap`` is that in fp64; it is *decidable* where ref - eps_f lies further than UNWRAP_MARGIN from a half-integer (ref and the
difference are one fp32 rounding each, at magnitudes below K / 2 + 1: 2 * 2^-24 * 33 < 4e-6 at K = 64).  The total is one more
rounded addition: |cfo32 - (I + eps_f)| <= U (|I| + 1/2).

The derotation against fp64 on the GPU's own offset, fraction and I.  The kernel forms the turns as ((I n mod K) + eps_f n) / K:
the integer is exact, eps_f n (< T / 2 = 280) is one rounding (<= 2^-17 * 2 = 1.5e-5 at that magnitude, half an ulp 7.6e-6), the
sum (< K + T / 2 = 344) one more (half an ulp 1.5e-5), the division by K and its result (< 5.4 turns) half an ulp 2.4e-7:
(7.6e-6 + 1.5e-5) / 64 + 2.4e-7 = 5.9e-7 turns = 3.7e-6 rad, under the 4.9e-6 rad frame_cfo_ref allows the narrow phase; sincospif
and the complex multiply as there.  So ``F.DEROT_TOL`` max|y| holds for any I: the integer part of the offset costs nothing.
"""
import numpy as np

import capture_acquire_ref as A
import capture_pool_ref as P
import capture_sync_ref as C
import frame_cfo_ref as F

U = A.U
CAP = 0.02
S, K = A.S, A.K
UNWRAP_MARGIN = 1e-5
DEROT_TOL = F.DEROT_TOL


def stage_b_wide(cap, lo, rhat, eps, J, S_, K_, CP, pilot_sc, M):
    """D fp64 [S, 2 M + 1] and its fp32 error bound, evaluated at the given r^ and eps^ (the fraction)"""
    c = A.complex_of(cap)
    N = K_ + CP
    T = S_ * N
    assert 0 <= M <= K_ // 2 - 1
    ps = A.pilot_symbols(pilot_sc, S_, K_)
    ms = np.arange(-M, M + 1)
    bins = np.arange(K_)
    D = np.zeros((S_, 2 * M + 1))
    bound = np.zeros((S_, 2 * M + 1))
    g_y = (np.sqrt(2.0) * (K_ + 3) + 26.0) * U
    for q in range(S_):
        for j in range(J):
            for s, ks in ps:
                at = lo + rhat + (q + s) * N + j * T + CP
                Y = np.zeros(K_, dtype=np.complex128)                  # every bin of the symbol
                energy = 0.0
                for n in range(K_):
                    turns = (((bins * n) % K_) + eps * n) / float(K_)
                    Y += c[at + n] * np.exp(-2j * np.pi * turns)
                    energy += c[at + n].real ** 2 + c[at + n].imag ** 2
                inner = np.zeros(2 * M + 1, dtype=np.complex128)
                for i in range(len(ks) - 1):
                    inner += Y[(ks[i] + ms) % K_] * np.conj(Y[(ks[i + 1] + ms) % K_])
                D[q] += np.abs(inner)
                Pn = len(ks)
                bound[q] += (Pn - 1) * K_ * energy * (2 * g_y + g_y ** 2 + (np.sqrt(2.0) * (Pn + 2) + 2) * U)
        bound[q] += J * len(ps) * U * D[q]
    return D, bound


def decide(D):
    """(q^, m^ index) of the first maximum in row-major order (numpy.argmax of the flattened array: the first on ties)"""
    e = int(np.argmax(D.reshape(-1)))
    return e // D.shape[1], e % D.shape[1]


def b_decidable(D, bound):
    d, b = D.reshape(-1), bound.reshape(-1)
    top = int(np.argmax(d))
    rest = np.delete(np.arange(len(d)), top)
    return bool((d[top] - d[rest] > b[top] + b[rest]).all())


def reference(cap, lo, J, S_, K_, CP, pilot_sc, M):
    """the whole definition in fp64 -> dict(r, eps, lam, phi, gamma, D, bound, q, m, first, a_ok, b_ok)"""
    rhat, eps, lam, phi, gamma = A.stage_a(cap, lo, J, S_, K_, CP)
    D, bound = stage_b_wide(cap, lo, rhat, eps, J, S_, K_, CP, pilot_sc, M)
    q, mi = decide(D)
    return dict(r=rhat, eps=eps, lam=lam, phi=phi, gamma=gamma, D=D, bound=bound, q=q, m=mi - M, first=lo + rhat + q * (K_ + CP),
                a_ok=A.a_decidable(lam, phi, J, S_, CP), b_ok=b_decidable(D, bound))


# ---- the cut ----------------------------------------------------------------------------------------------------------------
def unwrap(m_hat, eps_acq, frac, K_):
    """(I int64, decidable) per entry of ``frac``: the whole spacings that bring the prefix's fraction next to m^ + eps^_acq"""
    d = (float(m_hat) + float(eps_acq)) - np.asarray(frac, dtype=np.float64)
    lim = K_ // 2
    I = np.clip(np.rint(d), -lim, lim).astype(np.int64)
    ok = (np.abs(np.abs(d - np.floor(d)) - 0.5) > UNWRAP_MARGIN) & (np.abs(d) < lim)
    return I, ok


def total_bound(I):
    return U * (np.abs(I) + 0.5)


def derotated(cap, first, stride, offset, total, S_, K_, CP):
    """fp64 [frames, S, K + CP, 2]: every frame cut at its own offset and derotated with its TOTAL offset I + eps_f"""
    return C.derotated(cap, first, stride, offset, np.asarray(total, dtype=np.float64), S_, K_, CP)


# ---- what the definition is NOT (the planted errors of the host test) ----------------------------------------------------------
def stage_b_planted(kind, cap, lo, rhat, eps, J, S_, K_, CP, pilot_sc, M):
    """(q^, m^) of a wrong stage B: ``"sign"`` looks for the pilots at k_i - m; ``"clip"`` keeps a shifted bin inside [0, K) by
    clamping, not mod K; ``"uniform"`` takes the comb as uniform across DC (the first half's spacing continued)"""
    sc = np.asarray(pilot_sc, dtype=np.int64)
    if kind == "uniform":
        rows = []
        for s, ks in A.pilot_symbols(sc, S_, K_):
            step = int(ks[1] - ks[0])
            rows.append(s * K_ + ks[0] + step * np.arange(len(ks)))
        sc = np.concatenate(rows)
    if kind == "clip":
        c = A.complex_of(cap)
        N, T = K_ + CP, S_ * (K_ + CP)
        ms = np.arange(-M, M + 1)
        D = np.zeros((S_, 2 * M + 1))
        n = np.arange(K_)
        for q in range(S_):
            for j in range(J):
                for s, ks in A.pilot_symbols(sc, S_, K_):
                    at = lo + rhat + (q + s) * N + j * T + CP
                    w = np.exp(-2j * np.pi * (((np.arange(K_)[:, None] * n[None, :]) % K_) + eps * n[None, :]) / float(K_))
                    Y = w @ c[at:at + K_]
                    inner = np.zeros(2 * M + 1, dtype=np.complex128)
                    for i in range(len(ks) - 1):
                        inner += Y[np.clip(ks[i] + ms, 0, K_ - 1)] * np.conj(Y[np.clip(ks[i + 1] + ms, 0, K_ - 1)])
                    D[q] += np.abs(inner)
        q, mi = decide(D)
        return q, mi - M
    D, _ = stage_b_wide(cap, lo, rhat, eps, J, S_, K_, CP, sc, M)
    q, mi = decide(D)
    return (q, -(mi - M)) if kind == "sign" else (q, mi - M)


# ---- the cases of the GPU test: <= 64 captures ------------------------------------------------------------------------------------
SPANS = (0, 1, 7, 31)
JS = A.JS
EXTRA = ((2.49, 7), (-3.51, 7), (0.2, 0), (0.2, 1), (0.2, 7), (0.2, 31))        # (eps, the span it is searched with)
LOS = {16: (0, 37), 4: (300, 555)}                                              # an even and an odd origin per prefix


def case_list():
    """(CP, channel, snr, eps, M): eps = +-(M + 0.45) at every span, and EXTRA.  44 captures (0.2 is one capture, four spans)"""
    out = []
    for CP in (16, 4):
        for ch, snr in A.CHANNELS:
            for M in SPANS:
                out += [(CP, ch, snr, M + 0.45, M), (CP, ch, snr, -(M + 0.45), M)]
            out += [(CP, ch, snr, eps, M) for eps, M in EXTRA]
    return out


def gpu_cases():
    """(CP, J, lo, channel, snr, eps, M): every case at every J, the origin's parity alternating from case to case"""
    return [(CP, J, LOS[CP][(i + J) % 2], ch, snr, eps, M) for i, (CP, ch, snr, eps, M) in enumerate(case_list()) for J in JS]


_caps, _refs = {}, {}


def case_capture(CP, channel, snr, eps):
    """(cap, start, eps): 21 QPSK frames under ONE offset, begun at a sample of frame 0 that depends on the case"""
    key = (CP, channel, float(snr), float(eps))
    if key not in _caps:
        T = S * (K + CP)
        rs = np.random.RandomState(77 + CP + (5 if channel != "AWGN" else 0) + int(round(100 * abs(eps))) + (3 if eps < 0 else 0))
        cut = int(rs.randint(0, T))
        _caps[key] = A.build_capture(channel, snr, CP, A.NBITS, 21, cut, float(eps), seed=6000 + int(rs.randint(0, 1000))) + (eps,)
    return _caps[key]


def n_captures():
    return len({(c[0], c[1], c[2], c[3]) for c in case_list()})


def case_stage_a(CP, J, lo, channel, snr, eps):
    """stage A alone (what the GPU test holds Lambda and r^ to; its stage B is evaluated at the GPU's own r^ and eps^)"""
    key = ("a", CP, J, lo, channel, float(snr), float(eps))
    if key not in _refs:
        cap, _, _ = case_capture(CP, channel, snr, eps)
        rhat, e, lam, phi, gamma = A.stage_a(cap, lo, J, S, K, CP)
        _refs[key] = dict(r=rhat, eps=e, lam=lam, phi=phi, gamma=gamma, a_ok=A.a_decidable(lam, phi, J, S, CP))
    return _refs[key]


def case_reference(CP, J, lo, channel, snr, eps, M):
    key = (CP, J, lo, channel, float(snr), float(eps), M)
    if key not in _refs:
        cap, _, _ = case_capture(CP, channel, snr, eps)
        _refs[key] = reference(cap, lo, J, S, K, CP, A.pilot_sc_of(CP), M)
    return _refs[key]


# ---- a synthetic frame whose shifted bins wrap mod K: K = 16, CP = 4, S = 3, two pilot symbols of three pilots, M = 7 ---------------
SYN = dict(S=3, K=16, CP=4, M=7, pilots={0: (1, 6, 14), 2: (2, 9, 13)})


def synthetic_pilot_sc():
    return np.asarray(sorted(s * SYN["K"] + k for s, ks in SYN["pilots"].items() for k in ks), dtype=np.int32)


def synthetic_capture(frames, cut, eps, seed, snr=30.0):
    """``frames`` frames of the synthetic grid (boosted 3+3j pilots, unit QPSK data on every other carrier but DC) under ONE offset,
    from ``cut`` samples into frame 0 on -> (cap float32 [n, 2] read-only, start of frame 1)"""
    from dl_ofdm_amd.radio import apply_cfo_stream
    S_, K_, CP = SYN["S"], SYN["K"], SYN["CP"]
    rs = np.random.RandomState(seed)
    sym = []
    for _ in range(frames):
        for s in range(S_):
            X = (rs.choice([-1.0, 1.0], K_) + 1j * rs.choice([-1.0, 1.0], K_)) / np.sqrt(2.0)
            X[0] = 0.0
            for k in SYN["pilots"].get(s, ()):
                X[k] = 3.0 + 3.0j
            x = np.fft.ifft(X) * np.sqrt(K_)
            sym.append(np.concatenate([x[-CP:], x]))
    cap = np.concatenate(sym)
    cap = cap / np.sqrt(np.mean(np.abs(cap) ** 2))
    cap = cap + np.sqrt(0.5) * 10.0 ** (-snr / 20.0) * (rs.randn(cap.shape[0]) + 1j * rs.randn(cap.shape[0]))
    cap = apply_cfo_stream(cap, eps, K_)[cut:]
    out = np.ascontiguousarray(np.stack([cap.real, cap.imag], axis=-1).astype(np.float32))
    out.setflags(write=False)
    return out, S_ * (K_ + CP) - cut
