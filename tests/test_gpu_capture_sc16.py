"""16-bit integer I/Q captures on the GPU (``-m gpu``): ``dccn_capture_sync_sc16``, ``dccn_capture_sync_pooled_sc16`` and
``dccn_capture_acquire_sc16`` held BIT FOR BIT to the float32 entries on the converted capture ``radio.sc16_to_float(q, scale)``
-- there is no tolerance anywhere in this file -- then ``receive_capture`` of the receiver and of the chain on an int16 capture
held the same way, and the refusals (C: the status, and poisoned outputs left as they were; Python: ``DccnError``).

Shapes: S = 7, K = 64, CP in {16, 4}, W = 3; 1 and 9 frames (three blocks, one live wave in the last); J in {1, 4}.  Captures: the
existing builders', quantised with scale = max|component| / 16384 and with the non-power-of-two fp32(1 / 3000), then a handful of
samples inside the windows overwritten with -32768, 32767, -1 and 0, in I and in Q separately (sign extension of both halves, the
extremes); fewer than 1 % of the samples may be zero.  A window start takes every residue mod 4 (first - W = 0 .. 3 crossed with
stride = T .. T + 3; the comparison is between two readings of the same numbers, so the frames need not sit at that stride), and
every capture of the cut tests ends on its last window's last sample, so n_samples mod 4 takes every value too."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A
import capture_sync_ref as CR
import frame_sync_ref as R
from dl_ofdm_amd.radio import apply_cfo_stream, quantize_sc16, sc16_to_float
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K, W = R.S, R.K, 3
GUARD = 64
SENT_X, SENT_OFF, SENT_C, SENT_M, SENT_W, SENT_F = 777.0, -99, 333.0, 555.0, 0x5A, -12345
DEV = "cuda"
INVALID, WORKSPACE = -1, -2
FRAME_COUNTS = (1, 9)
EXTREMES = (-32768, 32767, -1, 0)
THIRD = np.float32(1.0 / 3000.0)


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def scales_of(cap):
    return (np.float32(np.abs(cap).max() / 16384.0), THIRD)


def quantised(cap, scale, plant=()):
    """(q int16 [n, 2], its value float32 [n, 2]): ``cap`` quantised, then EXTREMES planted at the samples ``plant`` -- entry i
    goes to I (i even) or Q (i odd), every value once in each -- and the zero share of the input checked"""
    q = quantize_sc16(cap, scale)
    assert len(plant) == 0 or len(plant) >= 8
    for i, at in enumerate(plant):
        q[at, i % 2] = EXTREMES[(i // 2) % 4]
    assert (q == 0).mean() < 0.01
    return q, sc16_to_float(q, scale)


class Out:
    """guarded, sentinel-filled outputs (and pooled workspace) of one cut"""

    def __init__(self, lib, n, out_kin, n_cfo):
        self.n, self.out_kin, self.n_cfo = n, out_kin, n_cfo
        self.n_out, self.n_met = n * S * out_kin * 2, n * (2 * W + 1)
        self.n_ws = int(lib.dccn_capture_sync_pooled_workspace_size(n))
        self.out_buf = torch.full((self.n_out + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.off_buf = torch.full((n + GUARD,), SENT_OFF, dtype=torch.int32, device=DEV)
        self.cfo_buf = torch.full((n_cfo + GUARD,), SENT_C, dtype=torch.float32, device=DEV)
        self.met_buf = torch.full((self.n_met + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        self.ws_buf = torch.full((self.n_ws + GUARD,), SENT_W, dtype=torch.uint8, device=DEV)
        self.status = None

    def guards_intact(self):
        return (bool((self.out_buf[self.n_out:] == SENT_X).all()) and bool((self.off_buf[self.n:] == SENT_OFF).all())
                and bool((self.cfo_buf[self.n_cfo:] == SENT_C).all()) and bool((self.met_buf[self.n_met:] == SENT_M).all())
                and bool((self.ws_buf[self.n_ws:] == SENT_W).all()))

    def untouched(self):
        return (bool((self.out_buf == SENT_X).all()) and bool((self.off_buf == SENT_OFF).all())
                and bool((self.cfo_buf == SENT_C).all()) and bool((self.met_buf == SENT_M).all())
                and bool((self.ws_buf == SENT_W).all()))

    def same_as(self, other):
        """every buffer, guards and unwritten parts included (the Gamma_f workspace too: the same sums)"""
        return all(same_bits(getattr(self, b), getattr(other, b)) for b in ("out_buf", "off_buf", "cfo_buf", "met_buf", "ws_buf"))


def cut(lib, cap, scale, first, stride, n, CP, crop=False, cfo=False, metric=True, first_dev=None, lo=0, x_out=True):
    """one per-frame cut: the float32 entries (``scale`` None: dccn_capture_sync, or dccn_capture_sync_at with ``first_dev``) or
    dccn_capture_sync_sc16"""
    o = Out(lib, n, K if crop else K + CP, n)
    tail = (stride, n, S, K, CP, W, o.out_kin, ptr(o.out_buf) if x_out else None, ptr(o.off_buf), ptr(o.cfo_buf) if cfo else None,
            ptr(o.met_buf) if metric else None, stream())
    ns = int(cap.shape[0])
    if scale is not None:
        o.status = lib.dccn_capture_sync_sc16(ptr(cap), ns, float(scale), 0 if first_dev is not None else first, ptr(first_dev),
                                              lo if first_dev is not None else 0, *tail)
    elif first_dev is not None:
        o.status = lib.dccn_capture_sync_at(ptr(cap), ns, ptr(first_dev), lo, *tail)
    else:
        o.status = lib.dccn_capture_sync(ptr(cap), ns, first, *tail)
    torch.cuda.synchronize()
    return o


def pooled(lib, cap, scale, first, stride, n, CP, crop=False, metric=True, first_dev=None, lo=0, ws_bytes=None):
    o = Out(lib, n, K if crop else K + CP, 1)
    head = (0 if first_dev is not None else first, ptr(first_dev), lo if first_dev is not None else 0, stride, n, S, K, CP, W,
            o.out_kin, ptr(o.out_buf), ptr(o.off_buf), ptr(o.cfo_buf), ptr(o.met_buf) if metric else None, ptr(o.ws_buf),
            o.n_ws if ws_bytes is None else ws_bytes, stream())
    if scale is not None:
        o.status = lib.dccn_capture_sync_pooled_sc16(ptr(cap), int(cap.shape[0]), float(scale), *head)
    else:
        o.status = lib.dccn_capture_sync_pooled(ptr(cap), int(cap.shape[0]), *head)
    torch.cuda.synchronize()
    return o


def first_of(T, r):
    """frame 0's nominal start with (first - W) = r mod 4 (T is a multiple of 4 at both prefixes), a frame into the capture"""
    assert T % 4 == 0
    return T + W + r


def layout(T, r, n, a):
    """(first, stride, n_samples: the last window ends on the capture's last sample, the samples to plant extremes at)"""
    first, stride = first_of(T, r), T + a
    ns = first + (n - 1) * stride + T + W
    last = first + (n - 1) * stride
    plant = [first - W, ns - 1, first - W + 1, ns - 2, first + 7, last + T // 2, last + T // 2 + 1, first + T - 9,
             first - W + 2, ns - 3, first - W + 3, ns - 4]
    return first, stride, ns, plant


def test_the_layouts_reach_every_residue():
    for T in (S * (K + 16), S * (K + 4)):
        ends = set()
        for r in range(4):
            for a in range(4):
                first, stride, ns, plant = layout(T, r, 9, a)
                assert (first - W) % 4 == r and max(plant) < ns and min(plant) >= first - W
                ends.add(ns % 4)
                if a % 2:
                    assert {(first - W + f * stride) % 4 for f in range(9)} == {0, 1, 2, 3}
            assert layout(T, r, 1, 0)[2] % 4 == (r + 2) % 4
        assert ends == {0, 1, 2, 3}


# ---- 1. the cut ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("CP", (16, 4))
def test_cut_equals_the_float32_cut_on_the_converted_capture(lib, CP, r, which):
    T = S * (K + CP)
    base, _ = CR.case_capture("ETU", 5.0, CP, 0, cfo=True)
    scale = scales_of(base)[which]
    for n in FRAME_COUNTS:
        for a in (range(4) if n > 1 else (0,)):
            first, stride, ns, plant = layout(T, r, n, a)
            q, f = quantised(base[:ns], scale, plant)
            assert set(EXTREMES) <= set(q[plant].reshape(-1).tolist())
            qd, fd = dev(q), dev(f)
            for cfo in (False, True):
                for crop in (False, True):
                    for metric in (True, False):
                        want = cut(lib, fd, None, first, stride, n, CP, crop, cfo, metric)
                        got = cut(lib, qd, scale, first, stride, n, CP, crop, cfo, metric)
                        what = (n, a, cfo, crop, metric)
                        assert want.status == 0 and got.status == 0, what
                        assert got.same_as(want) and got.guards_intact(), what
                        assert not bool((got.out_buf[:got.n_out] == SENT_X).any()) and bool((got.off_buf[:n].abs() <= W).all())
            again = cut(lib, qd, scale, first, stride, n, CP, cfo=True)
            assert again.same_as(cut(lib, qd, scale, first, stride, n, CP, cfo=True))           # a second run: the same bits
            only = cut(lib, qd, scale, first, stride, n, CP, cfo=True, x_out=False)            # the offsets alone
            assert only.status == 0 and bool((only.out_buf == SENT_X).all())
            assert same_bits(only.off_buf, again.off_buf) and same_bits(only.cfo_buf, again.cfo_buf)


@pytest.mark.parametrize("CP", (16, 4))
def test_cut_with_the_start_on_the_device(lib, CP):
    T, n = S * (K + CP), 9
    base, _ = CR.case_capture("EVA", 30.0, CP, 0, cfo=True)
    scale = scales_of(base)[1]
    for r in range(4):
        lo, stride = T - 8 + r, T + 1
        ns = lo + T - 1 + (n - 1) * stride + T + W              # exactly enough for every start the kernel can clamp to
        q, f = quantised(base[:ns], scale, [lo - W, ns - 1, lo + 1, ns - 2, lo + 9, lo + T, lo + 2 * T + 1, ns - 3])
        qd, fd = dev(q), dev(f)
        for value in (lo + 11, lo, lo + T - 1, lo + T, -5, -(1 << 62), (1 << 62), lo - 1):       # good, the ends, wild
            fdev = torch.tensor([value], dtype=torch.int64, device=DEV)
            for cfo in (False, True):
                want = cut(lib, fd, None, 0, stride, n, CP, cfo=cfo, first_dev=fdev, lo=lo)
                got = cut(lib, qd, scale, 0, stride, n, CP, cfo=cfo, first_dev=fdev, lo=lo)
                assert want.status == 0 and got.status == 0 and got.same_as(want) and got.guards_intact(), (r, value, cfo)
                assert int(fdev[0]) == value
        host = cut(lib, qd, scale, lo + 11, stride, n, CP, cfo=True)                             # the same start from the host
        fdev = torch.tensor([lo + 11], dtype=torch.int64, device=DEV)
        assert host.same_as(cut(lib, qd, scale, 0, stride, n, CP, cfo=True, first_dev=fdev, lo=lo))


# ---- 2. one carrier offset per capture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel,snr", (("ETU", 5.0), ("EVA", 30.0)))
@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("CP", (16, 4))
def test_pooled_equals_the_float32_call(lib, CP, r, channel, snr):
    T = S * (K + CP)
    base, _ = CR.case_capture(channel, snr, CP, 0, cfo=True)
    seen = set()
    for which, scale in enumerate(scales_of(base)):
        for n in FRAME_COUNTS:
            a = (r + which + n) % 4
            first, stride, ns, plant = layout(T, r, n, a)
            q, f = quantised(base[:ns], scale, plant)
            qd, fd = dev(q), dev(f)
            for crop in (False, True):
                for metric in (True, False):
                    want = pooled(lib, fd, None, first, stride, n, CP, crop, metric)
                    got = pooled(lib, qd, scale, first, stride, n, CP, crop, metric)
                    assert want.status == 0 and got.status == 0, (n, crop, metric)
                    assert got.same_as(want) and got.guards_intact(), (n, crop, metric)
            seen |= {int(v) for v in (first + stride * torch.arange(n, device=DEV) + got.off_buf[:n]).cpu() % 4}
            assert got.same_as(pooled(lib, qd, scale, first, stride, n, CP, True, False))      # a second run: the same bits
            # a device start whose range [lo, lo + T - 1] does not fit this capture (it ends on the last window): refused
            fdev = torch.tensor([first], dtype=torch.int64, device=DEV)
            at = pooled(lib, qd, scale, 0, stride, n, CP, True, False, first_dev=fdev, lo=first - 2)
            assert at.status == INVALID and at.untouched()
    assert len(seen) >= 3                                                   # the cut's own window starts: first + f stride + theta_f


def test_pooled_start_on_the_device(lib):
    CP, n = 16, 9
    T = S * (K + CP)
    base, _ = CR.case_capture("ETU", 5.0, CP, 0, cfo=True)
    scale = scales_of(base)[0]
    lo, stride = T - 2, T
    ns = lo + T - 1 + (n - 1) * stride + T + W
    q, f = quantised(base[:ns], scale, [lo - W, ns - 1, lo + 1, ns - 2, lo + 9, lo + T, lo + 2 * T + 1, ns - 3])
    qd, fd = dev(q), dev(f)
    for value in (T, lo - 100, 1 << 60):
        fdev = torch.tensor([value], dtype=torch.int64, device=DEV)
        want = pooled(lib, fd, None, 0, stride, n, CP, first_dev=fdev, lo=lo)
        got = pooled(lib, qd, scale, 0, stride, n, CP, first_dev=fdev, lo=lo)
        assert want.status == 0 and got.status == 0 and got.same_as(want) and got.guards_intact(), value
    assert got.same_as(pooled(lib, qd, scale, lo + T - 1, stride, n, CP))


# ---- 3. acquisition ------------------------------------------------------------------------------------------------------------------
class AcqOut:
    def __init__(self, lib, CP, J):
        self.N = K + CP
        self.n_ws = int(lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J))
        self.first_buf = torch.full((1 + GUARD,), SENT_F, dtype=torch.int64, device=DEV)
        self.cfo_buf = torch.full((1 + GUARD,), SENT_C, dtype=torch.float32, device=DEV)
        self.sym_buf = torch.full((self.N + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        self.phase_buf = torch.full((S + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.ws_buf = torch.full((self.n_ws + GUARD,), SENT_W, dtype=torch.uint8, device=DEV)
        self.status = None

    def same_as(self, other):
        return all(same_bits(getattr(self, b), getattr(other, b)) for b in ("first_buf", "cfo_buf", "sym_buf", "phase_buf"))

    def guards_intact(self):
        return (bool((self.first_buf[1:] == SENT_F).all()) and bool((self.cfo_buf[1:] == SENT_C).all())
                and bool((self.sym_buf[self.N:] == SENT_M).all()) and bool((self.phase_buf[S:] == SENT_X).all())
                and bool((self.ws_buf[self.n_ws:] == SENT_W).all()))

    def untouched(self):
        return (bool((self.first_buf == SENT_F).all()) and bool((self.cfo_buf == SENT_C).all()) and bool((self.sym_buf == SENT_M).all())
                and bool((self.phase_buf == SENT_X).all()) and bool((self.ws_buf == SENT_W).all()))


def acquire(lib, cap, scale, lo, J, CP, sc, metrics=True, ws_bytes=None, n_samples=None):
    o = AcqOut(lib, CP, J)
    ns = int(cap.shape[0]) if n_samples is None else n_samples
    tail = (lo, J, S, K, CP, ptr(sc), int(sc.numel()), ptr(o.first_buf), ptr(o.cfo_buf), ptr(o.sym_buf) if metrics else None,
            ptr(o.phase_buf) if metrics else None, ptr(o.ws_buf), o.n_ws if ws_bytes is None else ws_bytes, stream())
    if scale is not None:
        o.status = lib.dccn_capture_acquire_sc16(ptr(cap), ns, float(scale), *tail)
    else:
        o.status = lib.dccn_capture_acquire(ptr(cap), ns, *tail)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("channel,snr", A.CHANNELS)
@pytest.mark.parametrize("J", (1, 4))
@pytest.mark.parametrize("CP", (16, 4))
def test_acquisition_equals_the_float32_call(lib, CP, J, channel, snr):
    T = S * (K + CP)
    base, _, _ = A.case_capture(CP, channel, snr, 0)
    sc = dev(A.pilot_sc_of(CP))
    los = (0, 37, 302, 555)
    assert {lo % 4 for lo in los} == {0, 1, 2, 3}
    for scale in scales_of(base):
        q, f = quantised(base, scale, [3, 40, 303, 556, 700, 701, 1500, 2001, 5, 38])
        qd, fd = dev(q), dev(f)
        for lo in los:
            want = acquire(lib, fd, None, lo, J, CP, sc)
            got = acquire(lib, qd, scale, lo, J, CP, sc)
            assert want.status == 0 and got.status == 0 and got.same_as(want) and got.guards_intact(), lo
            assert lo <= int(got.first_buf[0]) < lo + T
        bare = acquire(lib, qd, scale, 37, J, CP, sc, metrics=False)
        assert bare.status == 0 and bool((bare.sym_buf == SENT_M).all()) and bool((bare.phase_buf == SENT_X).all())
        ref = acquire(lib, qd, scale, 37, J, CP, sc)
        assert same_bits(bare.first_buf, ref.first_buf) and same_bits(bare.cfo_buf, ref.cfo_buf)
        assert ref.same_as(acquire(lib, qd, scale, 37, J, CP, sc))                               # a second run: the same bits


# ---- 4. refusals at the C level: the status, and nothing written ---------------------------------------------------------------------
BAD_SCALES = (0.0, -2.0 ** -15, float("inf"), float("nan"))


def test_refused_calls_write_nothing(lib):
    CP, n, J = 16, 9, 4
    T = S * (K + CP)
    base, _ = CR.case_capture("ETU", 5.0, CP, 0, cfo=True)
    scale = scales_of(base)[0]
    first, stride, ns, plant = layout(T, 1, n, 0)
    q, _ = quantised(base[:ns + 1], scale, plant)
    qd = dev(q)[:ns]
    off4 = dev(q)[1:]                                                       # a base off by 4 bytes
    calls = []
    for bad in BAD_SCALES:
        calls.append(cut(lib, qd, bad, first, stride, n, CP, cfo=True))
        calls.append(pooled(lib, qd, bad, first, stride, n, CP))
    calls.append(cut(lib, off4, scale, first, stride, n, CP))
    calls.append(pooled(lib, off4, scale, first, stride, n, CP))
    calls.append(cut(lib, qd, scale, first + 1, stride, n, CP))             # the last window one sample past the end
    calls.append(pooled(lib, qd, scale, first + 1, stride, n, CP))
    calls.append(cut(lib, qd[:ns - 1], scale, first, stride, n, CP))
    fdev = torch.tensor([first], dtype=torch.int64, device=DEV)
    calls.append(cut(lib, qd, scale, 0, stride, n, CP, first_dev=fdev, lo=first))         # the range's last start would not fit
    for o in calls:
        assert o.status == INVALID and o.untouched()
    o = Out(lib, n, K + CP, n)                                              # null cap
    o.status = lib.dccn_capture_sync_sc16(None, ns, float(scale), first, None, 0, stride, n, S, K, CP, W, K + CP, ptr(o.out_buf),
                                          ptr(o.off_buf), None, None, stream())
    torch.cuda.synchronize()
    assert o.status == INVALID and o.untouched()
    short = pooled(lib, qd, scale, first, stride, n, CP, ws_bytes=int(lib.dccn_capture_sync_pooled_workspace_size(n)) - 1)
    assert short.status == WORKSPACE and short.untouched()

    abase, _, _ = A.case_capture(CP, "AWGN", 30.0, 0)
    aq, _ = quantised(abase, scale, [3, 40, 303, 556, 700, 701, 1500, 2001])
    ad, sc = dev(aq), dev(A.pilot_sc_of(CP))
    refused = [acquire(lib, ad, bad, 5, J, CP, sc) for bad in BAD_SCALES]
    refused.append(acquire(lib, ad[1:], scale, 5, J, CP, sc))
    refused.append(acquire(lib, ad, scale, 5, J, CP, sc, n_samples=5 + (J + 2) * T - 1))
    for o in refused:
        assert o.status == INVALID and o.untouched()
    short = acquire(lib, ad, scale, 5, J, CP, sc, ws_bytes=int(lib.dccn_capture_acquire_workspace_size(S, K, CP, 16, J)) - 1)
    assert short.status == WORKSPACE and short.untouched()


def test_output_overlap_is_judged_on_four_bytes_per_sample(lib):
    """x_out inside the capture's 4 n_samples bytes is refused; x_out that starts right behind them is accepted (a check that still
    took a sample for 8 bytes would refuse it) and holds what any other destination holds"""
    CP, n = 16, 1
    T = S * (K + CP)
    base, _ = CR.case_capture("ETU", 5.0, CP, 0, cfo=True)
    scale = scales_of(base)[0]
    first = first_of(T, 1)
    ns = (first + T + W + 3) // 4 * 4                                       # 4 ns bytes: a multiple of 16, x_out may start there
    q, _ = quantised(base[:ns], scale, layout(T, 1, n, 0)[3])
    out_bytes = n * T * 8
    buf = torch.full((4 * ns + out_bytes + 256,), SENT_W, dtype=torch.uint8, device=DEV)
    buf[:4 * ns] = dev(q).view(torch.uint8).reshape(-1)
    assert buf.data_ptr() % 16 == 0
    off = torch.full((n,), SENT_OFF, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.dccn_capture_sync_pooled_workspace_size(n)), dtype=torch.uint8, device=DEV)
    cfo = torch.zeros(1, dtype=torch.float32, device=DEV)

    def per_frame(x_out):
        st = lib.dccn_capture_sync_sc16(buf.data_ptr(), ns, float(scale), first, None, 0, T, n, S, K, CP, W, K + CP, x_out,
                                        ptr(off), None, None, stream())
        torch.cuda.synchronize()
        return st

    def pooled_at(x_out):
        st = lib.dccn_capture_sync_pooled_sc16(buf.data_ptr(), ns, float(scale), first, None, 0, T, n, S, K, CP, W, K + CP, x_out,
                                               ptr(off), ptr(cfo), None, ptr(ws), int(ws.numel()), stream())
        torch.cuda.synchronize()
        return st

    for call in (per_frame, pooled_at):
        assert call(buf.data_ptr() + 4 * ns - 16) == INVALID and call(buf.data_ptr() + 16) == INVALID
        assert bool((buf[4 * ns:] == SENT_W).all()) and bool((off == SENT_OFF).all())
    assert per_frame(buf.data_ptr() + 4 * ns) == 0
    ref = cut(lib, dev(q), scale, first, T, n, CP)
    got = buf[4 * ns:4 * ns + out_bytes].view(torch.float32)
    assert ref.status == 0 and same_bits(got, ref.out_buf[:ref.n_out]) and bool((buf[4 * ns + out_bytes:] == SENT_W).all())
    assert torch.equal(buf[:4 * ns], dev(q).view(torch.uint8).reshape(-1))
    buf[4 * ns:] = SENT_W
    assert pooled_at(buf.data_ptr() + 4 * ns) == 0
    assert not bool((buf[4 * ns:4 * ns + out_bytes] == SENT_W).all()) and bool((buf[4 * ns + out_bytes:] == SENT_W).all())


# ---- 5. the Python classes -----------------------------------------------------------------------------------------------------------
def test_capture_classes_serve_both_dtypes_and_refuse(lib):
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureSync, CaptureSyncGroup
    CP, n = 16, 9
    T = S * (K + CP)
    base, _ = CR.case_capture("ETU", 5.0, CP, 0, cfo=True)
    first, stride, ns, plant = layout(T, 2, n, 1)
    q0, f0 = quantised(0.2 * base[:ns], 2.0 ** -15, plant)                  # the default scale
    q1, f1 = quantised(base[:ns], THIRD, plant)
    for scope in ("frame", "capture"):
        cs = CaptureSync(S, K, CP, W, n, DEV, cfo=True, cfo_scope=scope)
        for q, f, scale in ((q0, f0, None), (q1, f1, THIRD), (q1, f1, float(THIRD))):
            out, off = cs.run(dev(f), first, stride)
            torch.cuda.synchronize()
            want = [t.clone() for t in (out, off, cs.cfo, cs.metric)]
            cs.out.fill_(SENT_X)
            out, off = cs.run(dev(q), first, stride, scale=scale)               # the same resident object, call by call
            torch.cuda.synchronize()
            assert all(same_bits(a, b) for a, b in zip(want, (out, off, cs.cfo, cs.metric))), (scope, scale)
            if scope == "frame":
                cs.offset.fill_(SENT_OFF)
                assert same_bits(cs.offsets(dev(q), first, stride, scale=scale), want[1])
        with pytest.raises(DccnError, match="scale"):
            cs.run(dev(f1), first, stride, scale=2.0 ** -15)                    # scale with a float32 capture
        for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60, "x"):
            with pytest.raises(DccnError, match="scale"):
                cs.run(dev(q1), first, stride, scale=bad)
        with pytest.raises(DccnError):
            cs.run(dev(q1).to(torch.int32), first, stride)
    abase, _, _ = A.case_capture(CP, "AWGN", 30.0, 0)
    aq, af = quantised(abase, THIRD, [3, 40, 303, 556, 700, 701, 1500, 2001])
    acq = CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), 4, DEV)
    want = [t.clone() for t in (acq.run(dev(af), 37), acq.cfo, acq.sym_metric, acq.phase_metric)]
    got = (acq.run(dev(aq), 37, scale=THIRD), acq.cfo, acq.sym_metric, acq.phase_metric)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(want, got))
    with pytest.raises(DccnError, match="scale"):
        acq.run(dev(af), 37, scale=THIRD)
    with pytest.raises(DccnError, match="scale"):
        acq.run(dev(aq), 37, scale=0.0)
    # int16 and cfo_span > 0: the wide entries are float32-only
    both = r"(?s)(?=.*int16)(?=.*cfo_span)"
    wide = CaptureSync(S, K, CP, W, n, DEV, cfo=True, cfo_span=7)
    pair = (torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.float32, device=DEV))
    fdev = torch.tensor([first], dtype=torch.int64, device=DEV)
    with pytest.raises(DccnError, match=both):
        wide.run(dev(q1), fdev, stride, lo=first - 2, acquired=pair)
    with pytest.raises(DccnError, match=both):
        CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), 4, DEV, cfo_span=7).run(dev(aq), 37)
    with pytest.raises(DccnError, match="float32"):                             # the group classes stay float32-only
        CaptureSyncGroup(S, K, CP, W, n, 2, DEV).run([dev(q1), dev(q1)], [first, first], stride)


# ---- 6. end to end: receive_capture of the receiver and of the chain ---------------------------------------------------------------
class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer():
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    Fl = _Flags()
    Fl.opt, Fl.init_learning = 0, 1e-3
    tx = ofdm_tx(Fl)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size, pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=2)
    tr = EqualizerTrainer(Fl, tx, O.init_params(rcfg, seed=24), seed=3)
    tr.load_params(E.init_params(ecfg, seed=23, bias_scale=0.05))
    return tr


def _fields(res):
    return [None if t is None else t.clone() for t in (res.packed, res.llr, res.offset, res.cfo, res.first, res.acquired_cfo)]


def _same_fields(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and same_bits(x, y)) for x, y in zip(a, b))


def test_receive_capture_end_to_end():
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    CP, nbits, batch, lo = 16, 2, 9, 5
    T = S * (K + CP)
    cap_np, start = A.build_capture("AWGN", None, CP, 2, 16, 211, 0.0, seed=77)
    cap_np = apply_cfo_stream(cap_np, 0.11, K)
    true = A.true_first(start, lo, T)
    plant = [true - W, true + 1, true + T, true + T + 1, true + 2 * T + 5, true + 3 * T, true + 4 * T + 2, true + 5 * T + 7]
    captures = ((quantised(0.2 * cap_np, 2.0 ** -15, plant), None), (quantised(cap_np, THIRD, plant), THIRD))
    dims = RxDims(S=S, kin=K + CP, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=K + CP, F=64, D=320, nbits=nbits), seed=13)
    rcv = RxReceiver(dims, batch, p, want_llr=True, CP=CP, pilot_sc=A.pilot_sc_of(CP))
    tr = _trainer()
    calls = (lambda cap, **kw: rcv.receive_capture(cap, sync=W, **kw),
             lambda cap, **kw: tr.receive_capture(cap, sync=W, want_llr=True, frames=batch, **kw))
    starts = (dict(first=true), dict(acquire=4, lo=lo))
    offsets = (dict(), dict(cfo=True), dict(cfo=True, cfo_scope="capture"))
    for (q, f), scale in captures:
        qd, fd = dev(q), dev(f)
        for call in calls:
            for st in starts:
                for cf in offsets:
                    want = call(fd, **st, **cf)
                    torch.cuda.synchronize()
                    want = _fields(want)
                    got = call(qd, scale=scale, **st, **cf)
                    torch.cuda.synchronize()
                    got = _fields(got)
                    assert _same_fields(got, want), (scale, st, cf)
                    assert got[1] is not None and got[2] is not None and (got[3] is None) == (not cf)
                    if "acquire" in st:
                        assert lo <= int(got[4][0]) < lo + T and got[5] is not None
            with pytest.raises(DccnError, match="scale"):
                call(fd, first=true, scale=THIRD)
            with pytest.raises(DccnError, match="scale"):
                call(qd, first=true, scale=-1.0)
            with pytest.raises(DccnError, match=r"(?s)(?=.*int16)(?=.*cfo_span)"):
                call(qd, acquire=4, lo=lo, cfo=True, cfo_span=7)
