"""The four device stages of the classical pilot-aided receivers (csrc/classical.h, include/dccn.h "classical pilot-aided
receivers"), each called through the C ABI on synthetic inputs and held to oracle/classical_oracle.py in float64 on the
same float32 inputs (``-m gpu``).

tests/test_gpu_benchmark.py sees these kernels only through hard decisions at one geometry; BPSK / QPSK decisions do not
move under any positive scaling of G, so the noise term c, the gain scalar and small errors of any kind are invisible
there.  Here every stage's numbers are compared: pilot LS, the four gain sums, the five estimate modes and the detector,
at sizes that run every stride of the launch geometry (more frames than the 512 block partials, P and K beyond one pass
of a 256-thread block, S at its limit of 32, K below one wave, more cells than 512 blocks of 256).

Tolerances: RTOL / assert_close of test_gpu_ops.py (1e-5 max-norm) for every float output; the gain sums per component
within 1e-6 of the L1 norm of their terms (a term carries at most four fp32 roundings, about 2.4e-7, before the double
accumulation); detected bits and the error count exact -- the inputs keep every cell at least 0.25 dmin away from a tie,
which the test asserts on the reference first.  Outputs lie between NaN guard bands of 64 floats that must stay untouched.
Each comparison prints its measured error (``pytest -s``) before it asserts.
"""
import numpy as np
import pytest
import torch

from oracle import classical_oracle as CO
from test_gpu_gemm_operands import Guarded
from test_gpu_ops import RTOL, assert_close, relerr

pytestmark = pytest.mark.gpu

INVALID_ARG, ERR_WORKSPACE = -1, -2     # DCCN_ERR_INVALID_ARG, DCCN_ERR_WORKSPACE (include/dccn.h)
PV = [3 + 3j, 0.6 - 1.7j]               # the product's pilot value; an asymmetric one (conjugation / plane order cannot hide)
A0 = 0.8 - 0.6j                         # gain of the synthetic frames: complex, not real


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def check(status, what):
    from dl_ofdm_amd import _lib
    _lib.check(status, what)


def fresh_workspace(lib, short=0):
    """dccn_classical_workspace_size() bytes (less `short`), every byte 0xFF: a partial left unwritten reads as NaN"""
    nws = int(lib.dccn_classical_workspace_size()) - short
    return torch.full((nws,), 255, dtype=torch.uint8, device="cuda"), nws


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def cplx(rng, *shape):
    return rng.randn(*shape) + 1j * rng.randn(*shape)


def c2f(z):
    """complex [...] -> float32 [..., 2]: the device's interleaved layout, and the rounding of the inputs"""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], -1).astype(np.float32)


def f2c(a):
    a = np.asarray(a, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


def pv32(pv):
    """the pilot value as the float arguments of the ABI carry it"""
    return complex(np.float32(pv.real), np.float32(pv.imag))


def held(got, ref, what):
    print("measured %-58s rel err %.3e" % (what, relerr(got, ref)))
    assert_close(got, ref, what, tol=RTOL)


def cells(rng, SK, count):
    """`count` distinct flat cell indices in [0, SK), not sorted"""
    idx = rng.permutation(SK)[:count].astype(np.int32)
    if count > 1 and (np.diff(idx) > 0).all():
        idx = idx[::-1].copy()
    return idx


def planes_of(z):
    """complex [...] -> float64 [..., 2], the layout assert_close compares in"""
    return np.stack([z.real, z.imag], -1)


# ---- pilot LS -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pv", PV)
@pytest.mark.parametrize("n,SK,P", [(1, 12, 3), (37, 448, 16), (3, 900, 300)])
def test_pilot_ls(lib, n, SK, P, pv):
    rng = np.random.RandomState(n + SK + P)
    Y = c2f(cplx(rng, n, SK))
    pil = cells(rng, SK, P)
    dY, dpil, gp = dev(Y, np.float32), dev(pil, np.int32), Guarded(2 * n * P)
    check(lib.dccn_classical_pilot_ls(dY.data_ptr(), dpil.data_ptr(), gp.ptr, n, SK, P, pv.real, pv.imag, None),
          "dccn_classical_pilot_ls")
    torch.cuda.synchronize()
    got = gp.get("gp").reshape(2, n, P)
    ref = CO.pilot_ls(f2c(Y), pil, pv32(pv))
    assert ref.shape == (2, n, P)
    held(got, ref, "pilot_ls %s pv %s" % ((n, SK, P), pv))
    # the [2][n][P] plane layout, plane by plane: real parts first, then imaginary parts, of Y[pilot] / pv
    q = f2c(Y)[:, pil] / pv32(pv)
    held(got[0], q.real, "pilot_ls %s pv %s, plane 0 = Re" % ((n, SK, P), pv))
    held(got[1], q.imag, "pilot_ls %s pv %s, plane 1 = Im" % ((n, SK, P), pv))


# ---- gain sums ------------------------------------------------------------------------------------------------------
def frames_case(rng, n, S, K, P, pv):
    """A static channel H0 [n, K] with |H0| in [0.8, 1.25], 5 % variation over the S symbols; G_ls = A0 H + noise at 10 dB;
    Y = A0 H pv + small noise (the sums over the pilots are coherent).  Everything rounded to float32 first."""
    SK = S * K
    H0 = rng.uniform(0.8, 1.25, (n, 1, K)) * np.exp(2j * np.pi * rng.uniform(size=(n, 1, K)))
    H = c2f((H0 * (1.0 + 0.05 * cplx(rng, n, S, K))).reshape(n, SK))
    Gz = A0 * f2c(H) + np.sqrt(0.05) * abs(A0) * cplx(rng, n, SK)
    Gls = np.stack([Gz.real, Gz.imag], 0).astype(np.float32)                  # planes [2, n, SK]
    Y = c2f(A0 * f2c(H) * pv32(pv) + 0.05 * cplx(rng, n, SK))
    return dict(n=n, S=S, K=K, SK=SK, P=P, pv=pv, H=H, Gls=Gls, Y=Y, pil=cells(rng, SK, P))


def run_gain(lib, c, d, ws, nws, with_H=True, sums=None):
    check(lib.dccn_classical_gain(d["Y"].data_ptr(), d["H"].data_ptr() if with_H else None, d["Gls"].data_ptr(),
                                  d["pil"].data_ptr(), c["n"], c["SK"], c["P"], c["pv"].real, c["pv"].imag,
                                  None if sums is None else sums.ptr, ws.data_ptr(), nws, None), "dccn_classical_gain")


def on_device(c):
    return dict(Y=dev(c["Y"], np.float32), H=dev(c["H"], np.float32), Gls=dev(c["Gls"], np.float32), pil=dev(c["pil"], np.int32))


def read_sums(g):
    return g.get("sums4").view(np.float64).copy()


@pytest.mark.parametrize("n,SK,P", [(1, 448, 16), (3, 448, 16), (513, 64, 8), (700, 448, 16), (2, 900, 300)])
def test_gain(lib, n, SK, P):
    """n = 513, 700: more frames than the 512 block partials (frames per block, and two partials per thread of the final
    sum); P = 300: more pilots than one pass of the block; SK = 900: the same for the cells."""
    c = frames_case(np.random.RandomState(7 * n + SK + P), n, 1, SK, P, PV[1])
    d = on_device(c)
    ref, scale = CO.gain_sums(f2c(c["Y"]), f2c(c["H"]), c["Gls"], c["pil"], pv32(c["pv"]))
    a = CO.gain_scalar(ref)
    assert abs(a.imag) > 0.3 * abs(a) and abs(a.real) > 0.3 * abs(a)          # coherent, neither part a cancellation
    ws, nws = fresh_workspace(lib)
    sums = Guarded(8)
    run_gain(lib, c, d, ws, nws, True, sums)
    torch.cuda.synchronize()
    got = read_sums(sums)
    for k in range(4):
        print("measured gain %-24s sums4[%d] |got - ref| / sum|term| %.3e" % ((n, SK, P), k, abs(got[k] - ref[k]) / scale[k]))
    for k in range(4):
        assert abs(got[k] - ref[k]) <= 1e-6 * scale[k], (k, got[k], ref[k], scale[k])
    # H = NULL: the three pilot sums are exactly 0, the fourth as before
    ws, nws = fresh_workspace(lib)
    sums = Guarded(8)
    run_gain(lib, c, d, ws, nws, False, sums)
    torch.cuda.synchronize()
    got = read_sums(sums)
    ref0, scale0 = CO.gain_sums(f2c(c["Y"]), None, c["Gls"], c["pil"], pv32(c["pv"]))
    assert (got[:3] == 0.0).all() and not np.signbit(got[:3]).any(), got
    assert abs(got[3] - ref0[3]) <= 1e-6 * scale0[3]


# ---- estimate -------------------------------------------------------------------------------------------------------
ESTIMATE_SHAPES = [(1, 1, 1), (3, 7, 64), (5, 32, 20), (2, 3, 300), (700, 2, 16)]


@pytest.fixture(scope="module")
def estimate_case():
    cache = {}

    def make(n, S, K):
        if (n, S, K) not in cache:
            c = frames_case(np.random.RandomState(100 * n + 10 * S + K), n, S, K, min(S * K, 16), PV[0])
            H64 = f2c(c["H"]).reshape(n, S, K)
            planes = c["Gls"].astype(np.float64).reshape(2, n, S, K)
            sums, _ = CO.gain_sums(f2c(c["Y"]), f2c(c["H"]), c["Gls"], c["pil"], pv32(c["pv"]))
            a = CO.gain_scalar(sums)
            # c so that the weights sit around 1/2: the geometric middle of the energies it is added to, as a float
            e1 = (np.abs(H64 * a) ** 2).sum(-1)
            e2 = (np.abs(CO.from_planes(planes).mean(axis=1)) ** 2).sum(-1) / S
            cv = {CO.LMMSE: float(np.float32(np.sqrt(e1.min() * e1.max()))),
                  CO.ALMMSE: float(np.float32(np.sqrt(e2.min() * e2.max())))}
            w1, w2 = CO.lmmse_weights(H64, cv[CO.LMMSE], a), CO.almmse_weights(planes, cv[CO.ALMMSE])
            # conditions on the reference, not measurements: the noise term matters in every frame ...
            assert 0.3 <= w1.min() and w1.max() <= 0.7 and 0.3 <= w2.min() and w2.max() <= 0.7, (w1, w2)
            # ... and the projection's fp32 reduction is not a cancellation, so RTOL is the honest bound
            h, g = H64 * a, CO.from_planes(planes)
            assert (np.abs((np.conj(h) * g).sum(-1)) >= 0.5 * (np.abs(h) * np.abs(g)).sum(-1)).all()
            c.update(H64=H64, planes=planes, a=a, cv=cv)
            cache[(n, S, K)] = c
        return cache[(n, S, K)]
    return make


@pytest.mark.parametrize("mode", [CO.LS, CO.LMMSE, CO.ALMMSE, CO.PERFECT, CO.FRAME_MEAN])
@pytest.mark.parametrize("n,S,K", ESTIMATE_SHAPES)
def test_estimate(lib, estimate_case, n, S, K, mode):
    """(1, 1, 1): the smallest call; (5, 32, 20): S at its limit, K below one wave; (2, 3, 300): K beyond one pass of the
    block; (700, 2, 16): more frames than block partials, so modes 1 and 3 add two partials per thread."""
    c = estimate_case(n, S, K)
    d = on_device(c)
    need_gain = mode in (CO.LMMSE, CO.PERFECT)
    cvar = c["cv"].get(mode, 0.25)
    ws, nws = fresh_workspace(lib)
    if need_gain:                               # the order contract: same n, workspace and stream; sums4 = NULL
        run_gain(lib, c, d, ws, nws, True, None)
    G = Guarded(n * (K if mode == CO.FRAME_MEAN else S * K) * 2)
    check(lib.dccn_classical_estimate(d["Gls"].data_ptr(), d["H"].data_ptr() if need_gain else None, G.ptr, n, S, K, mode,
                                      cvar, ws.data_ptr(), nws, None), "dccn_classical_estimate")
    torch.cuda.synchronize()
    got32 = G.get("G mode %d" % mode)           # mode 4: exactly n K 2 floats, or the guard band says so
    ref = CO.estimate(c["planes"], c["H64"] if need_gain else None, mode, cvar, c["a"])
    assert ref.shape == ((n, K) if mode == CO.FRAME_MEAN else (n, S * K))
    held(got32.reshape(ref.shape + (2,)), planes_of(ref), "estimate mode %d %s" % (mode, (n, S, K)))
    if mode == CO.LS:                           # bitwise the interleaving of the planes
        assert np.array_equal(got32.reshape(n, S * K, 2), np.stack([c["Gls"][0], c["Gls"][1]], -1))
    if mode == CO.ALMMSE:                       # one row per frame, written S times
        rows = got32.reshape(n, S, K, 2)
        assert np.array_equal(rows, np.broadcast_to(rows[:, :1], rows.shape))


def test_estimate_refusals(lib, estimate_case):
    n, S, K = 3, 7, 64
    c = estimate_case(n, S, K)
    d = on_device(c)
    ws, nws = fresh_workspace(lib)
    short, nshort = fresh_workspace(lib, short=8)
    big = dev(np.zeros((2, n, 33 * K)), np.float32)                  # what S = 33 would read, were it launched
    bigH = dev(np.zeros((n, 33 * K, 2)), np.float32)
    G = Guarded(n * 33 * K * 2)
    gl, H, w = d["Gls"].data_ptr(), d["H"].data_ptr(), ws.data_ptr()
    calls = [("S = 33", (big.data_ptr(), bigH.data_ptr(), G.ptr, n, 33, K, 0, 0.25, w, nws, None), INVALID_ARG),
             ("S = 0", (gl, H, G.ptr, n, 0, K, 0, 0.25, w, nws, None), INVALID_ARG),
             ("mode 5", (gl, H, G.ptr, n, S, K, 5, 0.25, w, nws, None), INVALID_ARG),
             ("mode -1", (gl, H, G.ptr, n, S, K, -1, 0.25, w, nws, None), INVALID_ARG),
             ("mode 1, H = NULL", (gl, None, G.ptr, n, S, K, 1, 0.25, w, nws, None), INVALID_ARG),
             ("mode 3, H = NULL", (gl, None, G.ptr, n, S, K, 3, 0.25, w, nws, None), INVALID_ARG),
             ("short workspace", (gl, H, G.ptr, n, S, K, 0, 0.25, short.data_ptr(), nshort, None), ERR_WORKSPACE),
             ("no workspace", (gl, H, G.ptr, n, S, K, 0, 0.25, None, nws, None), ERR_WORKSPACE)]
    for what, args, code in calls:
        assert lib.dccn_classical_estimate(*args) == code, what
    torch.cuda.synchronize()
    assert np.isnan(G.get("refused estimate")).all()
    # the other two workspace users refuse a short one the same way
    sums = Guarded(8)
    assert lib.dccn_classical_gain(d["Y"].data_ptr(), H, gl, d["pil"].data_ptr(), n, S * K, c["P"], 3.0, 3.0, sums.ptr,
                                   short.data_ptr(), nshort, None) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert np.isnan(sums.get("refused gain")).all()


# ---- detect ---------------------------------------------------------------------------------------------------------
def msb_first_labels(m, nbits):
    return ((np.arange(m)[:, None] >> np.arange(nbits - 1, -1, -1)[None, :]) & 1).astype(np.int32)


def constellation(nbits):
    """(table [m] complex, as float32 values; labels [m, nbits]; dmin).  nbits 1 ... 4: the product's tables; 8: a 16 x 16
    grid on the odd integers (the ABI allows nbits up to 8)."""
    if nbits == 8:
        lv = np.arange(-15.0, 16.0, 2.0)
        table = (lv[None, :] + 1j * lv[::-1, None]).reshape(-1)
    else:
        from dl_ofdm_amd import ofdm
        table = ofdm.const_map(nbits).astype(np.complex128)
    m = table.shape[0]
    assert m == 1 << nbits
    assert np.array_equal(np.sort_complex(table), np.sort_complex(-table)) and \
        np.array_equal(np.sort_complex(table), np.sort_complex(np.conj(table)))             # sign-symmetric: exact ties at x = 0
    dist = np.abs(table[:, None] - table[None, :]) + 1e9 * np.eye(m)
    return table, msb_first_labels(m, nbits), float(dist.min())


DETECT_GEOMETRY = {(1, 1): (2, 3), (3, 320): (7, 64), (7, 333): (3, 150), (700, 200): (4, 64)}      # (n, D) -> (S, K)


def detect_case(rng, n, D, S, K, nbits, one_row=False):
    """x = table[q] + delta, |Re delta|, |Im delta| <= 0.25 dmin / sqrt 2; |G| in [0.5, 2], any phase; Y = fl32(x G); the
    transmitted bits are labels[q] with about 10 % flipped.  one_row: G is one row [K] per frame."""
    table, labels, dmin = constellation(nbits)
    SK = S * K
    dat = cells(rng, SK, D)
    Gs = c2f(rng.uniform(0.5, 2.0, (n, K if one_row else SK)) * np.exp(2j * np.pi * rng.uniform(size=(n, K if one_row else SK))))
    Gfull = np.tile(Gs, (1, S, 1)) if one_row else Gs                                       # [n, SK, 2]
    q = rng.randint(0, table.shape[0], (n, SK))
    lim = 0.25 * dmin / np.sqrt(2.0)
    x = table[q] + rng.uniform(-lim, lim, (n, SK)) + 1j * rng.uniform(-lim, lim, (n, SK))
    Y = c2f(x * f2c(Gfull))
    bits = labels[q[:, dat]] ^ (rng.uniform(size=(n, D, nbits)) < 0.1).astype(np.int32)
    return dict(n=n, D=D, SK=SK, K=K, nbits=nbits, table=table, labels=labels, dmin=dmin, dat=dat, G=Gs, Gfull=Gfull, Y=Y,
                bits=bits.astype(np.int32), q=q)


def run_detect(lib, c, Y, G, g_row, g_mod, want_det=True):
    """-> (det [n, D, nbits] or None, errors)"""
    n, D, nbits = c["n"], c["D"], c["nbits"]
    t = [dev(Y, np.float32), dev(G, np.float32), dev(c["dat"], np.int32), dev(c2f(c["table"]), np.float32),
         dev(c["labels"], np.int32), dev(c["bits"], np.int32)]
    det = Guarded(n * D * nbits) if want_det else None
    err = Guarded(2)
    ws, nws = fresh_workspace(lib)
    check(lib.dccn_classical_detect(*[a.data_ptr() for a in t], det.ptr if want_det else None, err.ptr, n, c["SK"], D,
                                    c["table"].shape[0], nbits, g_row, g_mod, ws.data_ptr(), nws, None), "dccn_classical_detect")
    torch.cuda.synchronize()
    errors = int(err.get("errors").view(np.int64)[0])
    return (det.get("det").view(np.int32).reshape(n, D, nbits).copy() if want_det else None), errors


@pytest.mark.parametrize("nbits", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n,D", sorted(DETECT_GEOMETRY))
def test_detect(lib, n, D, nbits):
    """Every cell counts: the decisions and the error count are the oracle's exactly.  (700, 200) is 140 000 cells, more than
    512 blocks of 256: the grid-stride path."""
    S, K = DETECT_GEOMETRY[(n, D)]
    c = detect_case(np.random.RandomState(1000 * nbits + n + D), n, D, S, K, nbits)
    Y64, G64 = f2c(c["Y"]), f2c(c["G"])
    idx, margin = CO.nearest(Y64, G64, c["dat"], c["table"], c["SK"], 0)
    print("measured detect nbits %d %-12s min margin / dmin %.3f" % (nbits, (n, D), margin.min() / c["dmin"]))
    assert margin.min() >= 0.25 * c["dmin"]
    assert np.array_equal(idx, c["q"][:, c["dat"]])                              # the construction decides what was sent
    ref = c["labels"][idx]                                                       # what CO.detect returns, from the idx at hand
    ref_err = int(np.count_nonzero(ref != c["bits"]))
    if n * D <= 1000:
        assert CO.detect(Y64, G64, c["dat"], c["table"], c["labels"], c["bits"], c["SK"], 0)[1] == ref_err
    assert n * D * nbits < 20 or 0.05 * ref.size < ref_err < 0.15 * ref.size    # a count that is not trivial
    det, errors = run_detect(lib, c, c["Y"], c["G"], c["SK"], 0)
    assert np.array_equal(det, ref), "%d of %d detected bits differ" % (np.count_nonzero(det != ref), ref.size)
    assert errors == ref_err
    none, errors = run_detect(lib, c, c["Y"], c["G"], c["SK"], 0, want_det=False)
    assert none is None and errors == ref_err                                    # det = NULL: the same count


@pytest.mark.parametrize("nbits", [1, 2, 3, 4, 8])
def test_detect_one_row_per_frame(lib, nbits):
    """g_row = K, g_mod = K with G [n, K] is the full-grid call on that row tiled over the symbols"""
    n, D = 7, 333
    S, K = DETECT_GEOMETRY[(n, D)]
    c = detect_case(np.random.RandomState(50 + nbits), n, D, S, K, nbits, one_row=True)
    Y64 = f2c(c["Y"])
    assert CO.decision_margin(Y64, f2c(c["Gfull"]), c["dat"], c["table"], c["SK"], 0).min() >= 0.25 * c["dmin"]
    ref, ref_err = CO.detect(Y64, f2c(c["G"]), c["dat"], c["table"], c["labels"], c["bits"], K, K)
    ref_full = CO.detect(Y64, f2c(c["Gfull"]), c["dat"], c["table"], c["labels"], c["bits"], c["SK"], 0)
    assert np.array_equal(ref, ref_full[0]) and ref_err == ref_full[1]
    det1, err1 = run_detect(lib, c, c["Y"], c["G"], K, K)
    detf, errf = run_detect(lib, c, c["Y"], c["Gfull"], c["SK"], 0)
    assert np.array_equal(det1, detf) and err1 == errf
    assert np.array_equal(det1, ref) and err1 == ref_err


@pytest.mark.parametrize("nbits", [1, 2, 3, 4, 8])
def test_detect_ties_take_the_first_minimum(lib, nbits):
    """Y = 0: x = 0 is equally far from the innermost points, exactly in fp32 and fp64 (the tables are sign-symmetric); the
    decision is the first of them, like np.argmin."""
    n, D = 3, 320
    S, K = DETECT_GEOMETRY[(n, D)]
    c = detect_case(np.random.RandomState(70 + nbits), n, D, S, K, nbits)
    Y = np.zeros_like(c["Y"])
    d2 = np.abs(c["table"]) ** 2
    tied = np.flatnonzero(d2 == d2.min())
    assert len(tied) >= 2 and tied[0] < tied[-1]
    ref, ref_err = CO.detect(f2c(Y), f2c(c["G"]), c["dat"], c["table"], c["labels"], c["bits"], c["SK"], 0)
    assert np.array_equal(ref, np.broadcast_to(c["labels"][tied[0]], ref.shape))
    det, errors = run_detect(lib, c, Y, c["G"], c["SK"], 0)
    assert np.array_equal(det, ref) and errors == ref_err
