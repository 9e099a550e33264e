"""``dccn_classical_receive`` / ``ClassicalRxReceiver`` on the GPU (``-m gpu``), held to tests/classical_receive_ref.py on the
GPU's own inputs (the tables are read back from the engine): ``y_freq``, ``chest``, ``noise`` and ``llr`` inside their derived
bounds, ``packed`` exact on every decidable cell (at most 1 % are not); then the statements that have no tolerance -- run to
run, frame by frame against a one-frame call, the decision against ``dccn_classical_detect`` on the kernel's own Y and G, the
LLR sign, the three front ends against their stand-alone launches -- the noise-free loopback, a ragged row between guard bands,
and refusals that leave poisoned outputs alone.

Worst share of each bound on the MI355X (printed per case; a share above 1 fails): see profiles/classical_receive.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A
import classical_receive_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 24
# geometry -> (nfft, longcp); the window positions each prefix allows: advance 0, 3, 4 = win even, odd, even (CP 4: win 4, 1, 0)
GEOM = {"64/16": (64, True), "64/4": (64, False), "128/32": (128, True)}
CASES = [("64/16", 2, "ALMMSE", 0, "EPA", 10.0, False), ("64/16", 4, "LS-Spline", 3, "ETU", 30.0, True),
         ("64/16", 1, "LS-Linear", 4, "AWGN", 5.0, False), ("64/16", 3, "ALMMSE", 3, "ETU", 30.0, True),
         ("64/4", 2, "ALMMSE", 3, "EPA", 10.0, False), ("64/4", 3, "LS-Spline", 4, "ETU", 30.0, True),
         ("64/4", 4, "LS-Spline", 0, "AWGN", 5.0, False), ("128/32", 2, "ALMMSE", 3, "EPA", 10.0, False)]


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def engine(c, batch, noise_var=None, **kw):
    from dl_ofdm_amd.classical_receive import ClassicalRxReceiver
    rx = ClassicalRxReceiver(c["F"], batch, method=c["method"], advance=c["advance"], noise_var=noise_var, want_llr=True, **kw)
    rx.want_y_freq()
    return rx


def outputs(rx):
    torch.cuda.synchronize()
    return {k: getattr(rx, k).clone() for k in ("packed", "llr", "chest", "y_freq", "noise")}


def host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def device_case(c, rx):
    """the case with the tables the engine really hands the kernel"""
    d = dict(c)
    d.update(dft=rx.dft.cpu().numpy(), w=rx.w.cpu().numpy(), pil=rx.pil.cpu().numpy(), dat=rx.dat.cpu().numpy(),
             empty=rx.empty.cpu().numpy(), table=rx.table.cpu().numpy(), labels=rx.labels.cpu().numpy(),
             pv=(np.float32(rx.args.pv_re), np.float32(rx.args.pv_im)), win=int(rx.args.win), mode=int(rx.args.mode))
    return d


_cases = {}


def case_of(geom, nbits, method, adv, channel, snr):
    key = (geom, nbits, method, adv, channel, snr)
    if key not in _cases:
        nfft, longcp = GEOM[geom]
        _cases[key] = R.make_case(nbits, channel, snr, n=N, seed=5 + nbits, nfft=nfft, longcp=longcp, method=method, advance=adv)
    return _cases[key]


@pytest.mark.parametrize("geom,nbits,method,adv,channel,snr,known", CASES)
def test_outputs_inside_their_bounds_at_1_3_and_24_frames(geom, nbits, method, adv, channel, snr, known):
    c = case_of(geom, nbits, method, adv, channel, snr)
    nv = c["known_noise"] if known else None
    rx = engine(c, N, nv)
    res = rx.receive(c["x"])
    assert res.prob is None and res.packed is rx.packed and res.llr is rx.llr and res.offset is None
    full = outputs(rx)
    ref = R.restate_case(device_case(c, rx), nv or 0.0)
    fig = R.compare(ref, host(full), c["D"], nbits)
    print("%s nbits=%d %s adv=%d %s %gdB %s: %s" % (geom, nbits, method, adv, channel, snr, "given" if known else "estimated",
                                                   {k: (round(v, 4) if isinstance(v, float) else v) for k, v in fig.items()}))
    assert R.failures(fig) == [], fig
    # a second run gives the same bits
    rx.receive(c["x"])
    again = outputs(rx)
    assert all(same_bits(full[k], again[k]) for k in full)
    # a ragged last tile: 3 frames = one tile of two frames and one of one
    r3 = engine(c, 3, nv)
    r3.receive(c["x"][5:8])
    o3 = outputs(r3)
    assert all(same_bits(o3[k], full[k][5:8]) for k in full)
    # frame f of the 24-frame call is the one-frame call on that frame, in every output
    r1 = engine(c, 1, nv)
    for f in (0, 1, 13, N - 1):
        r1.receive(c["x"][f:f + 1])
        o1 = outputs(r1)
        assert all(same_bits(o1[k], full[k][f:f + 1]) for k in full), f


@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_packed_is_exact_on_decidable_cells_for_both_modes_and_both_noise_sources(lib, nbits):
    from dl_ofdm_amd.receive import unpack_bits
    for method in ("LS-Spline", "ALMMSE"):
        c = case_of("64/16", nbits, method, 0, "EPA", 10.0)
        for nv in (None, c["known_noise"]):
            rx = engine(c, N, nv)
            rx.receive(c["x"])
            got = outputs(rx)
            ref = R.restate_case(device_case(c, rx), nv or 0.0)
            fig = R.compare(ref, host(got), c["D"], nbits)
            assert R.failures(fig) == [], (method, nv, fig)
            # the decision stage is dccn_classical_detect's arithmetic: that entry, fed the kernel's own Y and G, decides alike
            ws = torch.empty(int(lib.dccn_classical_workspace_size()), dtype=torch.uint8, device=DEV)
            det = torch.full((N, c["D"], nbits), -1, dtype=torch.int32, device=DEV)
            err = torch.zeros(1, dtype=torch.int64, device=DEV)
            zeros = torch.zeros(N, c["D"], nbits, dtype=torch.int32, device=DEV)
            st = lib.dccn_classical_detect(got["y_freq"].data_ptr(), got["chest"].data_ptr(), rx.dat.data_ptr(), rx.table.data_ptr(),
                                           rx.labels.data_ptr(), zeros.data_ptr(), det.data_ptr(), err.data_ptr(), N, c["S"] * c["K"],
                                           c["D"], 1 << nbits, nbits, c["S"] * c["K"], 0, ws.data_ptr(), ws.numel(),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert st == 0
            torch.cuda.synchronize()
            assert np.array_equal(unpack_bits(got["packed"].cpu().numpy(), c["D"], nbits), det.cpu().numpy().astype(np.uint8))


@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
def test_noise_free_loopback(nbits):
    from dl_ofdm_amd.receive import pack_bits
    c = R.make_case(nbits, "AWGN", 0.0, n=N, seed=3, method="LS-Spline", noise_free=True)
    rx = engine(c, N)
    res = rx.receive(c["x"])
    torch.cuda.synchronize()
    assert np.array_equal(res.packed.cpu().numpy(), pack_bits(c["bits"]))
    assert np.array_equal(res.bits().cpu().numpy(), c["bits"].astype(np.uint8))
    llr = res.llr.cpu().numpy()
    assert np.all(np.isfinite(llr))
    assert np.all((llr > 0) == (c["bits"] == 1)) and np.all(llr != 0)
    assert np.all(rx.noise.cpu().numpy() >= np.float32(1e-20))


def test_front_ends_equal_their_stand_alone_launches():
    from dl_ofdm_amd.radio import quantize_sc16, sc16_to_float
    from dl_ofdm_amd.sync import CaptureSync, FrameSync
    CP, nbits, batch, lo, W = 16, 2, 9, 5, 3
    S, K = A.S, A.K
    T = S * (K + CP)
    c = case_of("64/16", nbits, "ALMMSE", 0, "EPA", 10.0)
    rx, plain = engine(c, batch), engine(c, batch)

    def fields(res):
        torch.cuda.synchronize()
        return [None if t is None else t.clone() for t in (res.packed, res.llr, res.offset, res.cfo, res.first, res.acquired_cfo)]

    def same(a, b):
        return all((x is None and y is None) or (x is not None and y is not None and same_bits(x, y)) for x, y in zip(a, b))

    # receive(x, sync=3, cfo=True) = FrameSync.run, then receive(aligned)
    x = dev(np.roll(c["x"][:batch].reshape(batch, -1, 2), 2, axis=1).reshape(batch, S, K + CP, 2))
    got = fields(rx.receive(x, sync=W, cfo=True))
    fs = FrameSync(S, K, CP, W, batch, DEV, want_metric=False, cfo=True)
    aligned, off = fs.run(x)
    want = fields(plain.receive(aligned))
    assert same(got[:2], want[:2]) and same_bits(got[2], off) and same_bits(got[3], fs.cfo)
    # receive_capture(cap, first) = CaptureSync.run, then receive -- float32 and int16 captures
    cap_np, start = A.build_capture("AWGN", 30.0, CP, nbits, 16, 211, 0.11, seed=77)
    cap_np = (0.2 * cap_np).astype(np.float32)                                  # (room for the 16-bit range at 2**-15)
    true = A.true_first(start, lo, T)
    q = quantize_sc16(cap_np, 2.0 ** -15)
    for cap, scale in ((dev(cap_np), None), (dev(q), None), (dev(q), np.float32(1.0 / 3000.0))):
        for kw in (dict(), dict(cfo=True), dict(cfo=True, cfo_scope="capture")):
            got = fields(rx.receive_capture(cap, first=true, sync=W, scale=scale, **kw))
            cs = CaptureSync(S, K, CP, W, batch, DEV, want_metric=False, **kw)
            frames, off = cs.run(cap, true, scale=scale)
            want = fields(plain.receive(frames))
            assert same(got[:2], want[:2]) and same_bits(got[2], off), (scale, kw)
            assert (got[3] is None) == (not kw) and (not kw or same_bits(got[3], cs.cfo))
            # receive_capture(first=None, acquire=4) = receive_capture(first = the true start)
            acq = fields(rx.receive_capture(cap, acquire=4, lo=lo, sync=W, scale=scale, **kw))
            assert int(acq[4][0]) == true and acq[5] is not None
            assert same(acq[:4], got[:4]), (scale, kw)
    # an int16 capture decides like its float32 value
    a = fields(rx.receive_capture(dev(q), first=true, sync=W, cfo=True))
    b = fields(rx.receive_capture(dev(sc16_to_float(q, 2.0 ** -15)), first=true, sync=W, cfo=True))
    assert same(a, b)
    # the refusals are RxReceiver's
    from dl_ofdm_amd._lib import DccnError
    with pytest.raises(DccnError, match="sync"):
        rx.receive(x, cfo=True)
    with pytest.raises(DccnError, match="acquire"):
        rx.receive_capture(dev(cap_np), sync=W)
    with pytest.raises(DccnError, match="not both"):
        rx.receive_capture(dev(cap_np), first=true, acquire=4, sync=W)


GUARD, POISON = 64, 0xA5


class CallBuffers:
    """a call through the C entry with every output between poisoned guard bands, ``packed`` at an odd address"""

    def __init__(self, c, rx, n, D, nbits):
        from dl_ofdm_amd import _lib
        from dl_ofdm_amd.receive import row_bytes
        self.n, self.D, self.nbits, self.RB = n, D, nbits, row_bytes(D, nbits)
        SK = c["S"] * c["K"]
        self.sizes = dict(packed=n * self.RB, llr=4 * n * D * nbits, chest=8 * n * SK, y_freq=8 * n * SK, noise=4 * n)
        self.lead = dict(packed=GUARD + 1, llr=GUARD, chest=GUARD, y_freq=GUARD, noise=GUARD)
        self.buf = {k: torch.full((self.lead[k] + v + GUARD,), POISON, dtype=torch.uint8, device=DEV) for k, v in self.sizes.items()}
        self.x = dev(c["x"][:n])
        self.args = _lib.ClassicalReceiveArgs.from_buffer_copy(rx.args)
        self.args.frames, self.args.D, self.args.nbits, self.args.m = n, D, nbits, 1 << nbits
        self.args.x = self.x.data_ptr()
        for k in self.sizes:
            setattr(self.args, k, self.buf[k].data_ptr() + self.lead[k])

    def call(self, lib):
        st = lib.dccn_classical_receive(C.byref(self.args), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return st

    def body(self, k):
        return self.buf[k][self.lead[k]:self.lead[k] + self.sizes[k]]

    def guards_intact(self):
        return all(bool((b[:self.lead[k]] == POISON).all()) and bool((b[self.lead[k] + self.sizes[k]:] == POISON).all())
                   for k, b in self.buf.items())

    def untouched(self):
        return all(bool((b == POISON).all()) for b in self.buf.values())


def test_a_ragged_row_between_guard_bands(lib):
    from dl_ofdm_amd.receive import unpack_bits
    c = case_of("64/16", 3, "ALMMSE", 3, "ETU", 30.0)
    rx = engine(c, N)
    D = 317
    o = CallBuffers(c, rx, 5, D, 3)
    assert o.RB == 119 and o.RB * 8 - D * 3 == 1 and (o.args.packed % 2) == 1
    assert o.call(lib) == 0
    assert o.guards_intact()
    packed = o.body("packed").view(5, o.RB).cpu().numpy()
    assert np.all(packed[:, -1] & 1 == 0)                                     # the padding bit
    d = device_case(c, rx)
    d["dat"], d["x"] = d["dat"][:D], c["x"][:5]
    ref = R.restate_case(d, 0.0)
    got = dict(packed=packed, llr=o.body("llr").view(torch.float32).view(5, D, 3).cpu().numpy(),
               chest=o.body("chest").view(torch.float32).view(5, -1, 2).cpu().numpy(),
               y_freq=o.body("y_freq").view(torch.float32).view(5, -1, 2).cpu().numpy(),
               noise=o.body("noise").view(torch.float32).cpu().numpy())
    fig = R.compare(ref, got, D, 3)
    assert R.failures(fig) == [], fig
    # the first 317 cells decide as they do in the full row
    rx.receive(c["x"])
    torch.cuda.synchronize()
    assert np.array_equal(unpack_bits(packed, D, 3), unpack_bits(rx.packed.cpu().numpy(), c["D"], 3)[:5, :D])


REFUSED = [("frames", 0), ("S", 17), ("K", 60), ("CP", 15), ("P", 0), ("D", 0), ("E", 0), ("nbits", 5), ("m", 4), ("win", -1), ("win", 17),
           ("mode", 1), ("mode", 3), ("noise_var", -1.0), ("noise_var", float("nan")), ("pv_re", float("inf")), ("dft", None),
           ("w", None), ("pil", None), ("dat", None), ("empty", None), ("table", None), ("labels", None), ("x", None),
           ("packed", None), ("x", "+8"), ("chest", "+4"), ("y_freq", "+4"), ("llr", "+2"), ("noise", "+1")]


def test_every_refusal_leaves_poisoned_outputs_untouched(lib):
    c = case_of("64/16", 3, "ALMMSE", 3, "ETU", 30.0)
    rx = engine(c, N)
    for field, value in REFUSED:
        o = CallBuffers(c, rx, 5, c["D"], 3)
        if isinstance(value, str):
            value = getattr(o.args, field) + int(value)
        setattr(o.args, field, value)
        assert o.call(lib) == -1, (field, value)
        assert o.untouched(), (field, value)
    o = CallBuffers(c, rx, 5, c["D"], 3)
    o.args.pv_re = o.args.pv_im = 0.0
    assert o.call(lib) == -1 and o.untouched()
