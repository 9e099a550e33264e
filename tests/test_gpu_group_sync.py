"""The receive front end for several links per launch on the GPU (``-m gpu``; include/dccn.h dccn_frame_sync_grouped,
dccn_capture_sync_grouped, dccn_capture_acquire_grouped).  The bar is bitwise: link i of a grouped call gets what the solo entry
writes for link i's arguments (the solo entries are held to fp64 by test_gpu_frame_sync / _frame_cfo / _capture_sync /
_capture_acquire), a refused call writes nothing for any link, and two runs give the same bits.

Every link has its own seed (its own capture, frame start, offsets and carrier offset); links 0 and 1 share one capture where the
test says so.  Outputs are pre-filled with sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

import capture_acquire_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0
INVALID, WORKSPACE = -1, -2
SHAPES = [(7, 64, 16, 3), (7, 64, 4, 4), (3, 12, 4, 2)]                  # (S, K, CP, W)
FRAMES = (1, 5, 9)                                                       # dead waves in a block of four
CAP_FRAMES = 21


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_host, _devcaps = {}, {}


def host_capture(shape, i):
    """link i's capture of 21 frames for the shape: (float32 [n, 2], a sample at which a frame starts).  S = 7, K = 64: the
    captures of tests/capture_acquire_ref.py with seed i (AWGN and ETU alternate); the small shape has no transmitter in the
    package: random symbols with their cyclic prefixes, a carrier offset, noise and a seed-dependent cut, built here."""
    S, K, CP, _ = shape
    key = (S, K, CP, i)
    if key not in _host:
        if (S, K) == (A.S, A.K):
            ch, snr = A.CHANNELS[i % 2]
            cap, start, _ = A.case_capture(CP, ch, snr, i)
        else:
            rs = np.random.RandomState(5000 + 13 * i + CP)
            T = S * (K + CP)
            sym = rs.standard_normal((CAP_FRAMES * S, K)) + 1j * rs.standard_normal((CAP_FRAMES * S, K))
            iq = np.concatenate([sym[:, K - CP:], sym], axis=1).reshape(-1)
            iq = iq * np.exp(2j * np.pi * rs.uniform(-0.4, 0.4) * np.arange(iq.shape[0]) / K)
            iq = iq + 0.05 * (rs.standard_normal(iq.shape[0]) + 1j * rs.standard_normal(iq.shape[0]))
            cut = int(rs.randint(0, T))
            iq = iq[cut:]
            cap, start = np.ascontiguousarray(np.stack([iq.real, iq.imag], axis=-1).astype(np.float32)), T - cut
        _host[key] = (cap, int(start))
    return _host[key]


def dev_capture(shape, i):
    key = shape[:3] + (i,)
    if key not in _devcaps:
        _devcaps[key] = torch.from_numpy(np.array(host_capture(shape, i)[0])).to(DEV)
    return _devcaps[key]


class Outs:
    """sentinel-filled outputs of one link of a sync / cut call"""

    def __init__(self, shape, frames, out_kin):
        S, _, _, W = shape
        self.out = torch.full((frames, S, out_kin, 2), SENT, dtype=torch.float32, device=DEV)
        self.offset = torch.full((frames,), -99, dtype=torch.int32, device=DEV)
        self.cfo = torch.full((frames,), SENT, dtype=torch.float32, device=DEV)
        self.metric = torch.full((frames, 2 * W + 1), SENT, dtype=torch.float32, device=DEV)

    def same(self, o):
        return (same_bits(self.out, o.out) and torch.equal(self.offset, o.offset) and same_bits(self.cfo, o.cfo)
                and same_bits(self.metric, o.metric))

    def untouched(self):
        return (bool((self.out == SENT).all()) and bool((self.offset == -99).all()) and bool((self.cfo == SENT).all())
                and bool((self.metric == SENT).all()))

    def ptrs(self, cfo, metric, x_out=True):
        return (self.out.data_ptr() if x_out else None, self.offset.data_ptr(), self.cfo.data_ptr() if cfo else None,
                self.metric.data_ptr() if metric else None)


class CutLink:
    """one link of a cut: its capture, where its frames nominally start, and the two ways to ask for them"""

    def __init__(self, cap, n_samples, first, stride, first_dev=None, lo=0):
        self.cap, self.ns, self.first, self.stride, self.first_dev, self.lo = cap, int(n_samples), int(first), int(stride), first_dev, int(lo)

    def entry(self, o, cfo, metric, x_out=True):
        from dl_ofdm_amd import _lib
        xo, off, cf, me = o.ptrs(cfo, metric, x_out)
        return _lib.CaptureLink(self.cap.data_ptr(), self.ns, 0 if self.first_dev is not None else self.first,
                                None if self.first_dev is None else self.first_dev.data_ptr(), self.lo, self.stride, xo, off, cf, me)

    def solo(self, lib, shape, frames, out_kin, o, cfo, metric):
        xo, off, cf, me = o.ptrs(cfo, metric)
        if self.first_dev is None:
            return lib.dccn_capture_sync(self.cap.data_ptr(), self.ns, self.first, self.stride, frames, *shape, out_kin, xo, off, cf, me,
                                         stream())
        return lib.dccn_capture_sync_at(self.cap.data_ptr(), self.ns, self.first_dev.data_ptr(), self.lo, self.stride, frames, *shape,
                                        out_kin, xo, off, cf, me, stream())


def table(entries, n=None):
    t = (type(entries[0]) * (len(entries) if n is None else n))()
    for i, e in enumerate(entries):
        t[i] = e
    return t


def cut_links(shape, n_links, frames, share=True):
    """link i: its own capture (link 1 reads link 0's when share), a start near a true frame start whose window begins on an even
    sample for even i and on an odd one for odd i, stride T for even i and T + 1 for odd i, its own n_samples"""
    S, K, CP, W = shape
    T = S * (K + CP)
    links = []
    for i in range(n_links):
        src = 0 if (share and i == 1) else i
        cap = dev_capture(shape, src)
        start = host_capture(shape, src)[1]
        first = A.true_first(start, W + 1 + i, T) + (T if i == 1 else 0) + (i % (2 * W)) - W
        first += ((first - W) & 1) ^ (i & 1)                                # the window's parity: i's
        if first < W:
            first += T
        stride = T + (i & 1)
        ns = int(cap.shape[0]) - 3 * i
        assert first + (frames - 1) * stride + T + W <= ns
        links.append(CutLink(cap, ns, first, stride))
    return links


def run_cut_group(lib, shape, frames, out_kin, links, cfo, metric):
    outs = [Outs(shape, frames, out_kin) for _ in links]
    t = table([l.entry(o, cfo, metric) for l, o in zip(links, outs)])
    st = lib.dccn_capture_sync_grouped(len(links), t, frames, *shape, out_kin, stream())
    torch.cuda.synchronize()
    return st, outs


def check_cut_group(lib, shape, frames, out_kin, links, cfo, metric):
    st, outs = run_cut_group(lib, shape, frames, out_kin, links, cfo, metric)
    assert st == 0
    for i, (l, o) in enumerate(zip(links, outs)):
        ref = Outs(shape, frames, out_kin)
        assert l.solo(lib, shape, frames, out_kin, ref, cfo, metric) == 0
        torch.cuda.synchronize()
        assert o.same(ref), (shape, frames, out_kin, len(links), i, cfo, metric)
        assert bool((o.offset != -99).all()) and bool((o.out != SENT).any())
        assert bool((o.cfo != SENT).all()) == cfo and bool((o.metric != SENT).all()) == metric
    return outs


# ---- the cut -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_links", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_cut_gives_the_solo_cuts_bits(lib, shape, n_links):
    S, K, CP, W = shape
    assert lib.dccn_capture_sync_supported(*shape) == 1
    seen = set()
    for frames in FRAMES:
        links = cut_links(shape, n_links, frames)
        if n_links > 1:
            assert {(l.first - W) & 1 for l in links} == {0, 1} and {l.stride for l in links} == {S * (K + CP), S * (K + CP) + 1}
            assert links[0].cap is links[1].cap and len({l.ns for l in links}) > 1
        for out_kin in (K + CP, K):
            for cfo in (False, True):
                for metric in (False, True):
                    outs = check_cut_group(lib, shape, frames, out_kin, links, cfo, metric)
                    seen.update(tuple(o.offset.tolist()) for o in outs)
    assert n_links == 1 or len(seen) > 1                                   # (the links really differ)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_starts_on_the_device_mix_with_known_starts(lib, shape):
    """links 0 and 4: `first`; the others `first_dev`: the true start, one below the range (clamped to lo) and one beyond it
    (clamped to lo + T - 1), as test_sync_at_gives_capture_syncs_bits uses; against dccn_capture_sync / _at per link"""
    S, K, CP, W = shape
    T, frames = S * (K + CP), 5
    links, values = [], []
    for i in range(5):
        cap = dev_capture(shape, i)
        lo = (W, W + 1, 300, 301, 37)[i]
        true = A.true_first(host_capture(shape, i)[1], lo, T)
        value = (None, true, lo - 7, lo + 3 * T, None)[i]
        fd = None if value is None else torch.tensor([value], dtype=torch.int64, device=DEV)
        links.append(CutLink(cap, int(cap.shape[0]), true, T, fd, lo))
        values.append(value)
    for out_kin in (K + CP, K):
        for cfo in (False, True):
            outs = check_cut_group(lib, shape, frames, out_kin, links, cfo, True)
    for l, v in zip(links, values):
        assert v is None or int(l.first_dev[0]) == v                        # (read, never written)
    # the clamped links got what the clamped value gives as a known start
    for i, clamped in ((2, links[2].lo), (3, links[3].lo + T - 1)):
        ref = Outs(shape, frames, K)
        known = CutLink(links[i].cap, links[i].ns, clamped, T)
        assert known.solo(lib, shape, frames, K, ref, True, True) == 0
        torch.cuda.synchronize()
        assert outs[i].same(ref), i


SMALL = (2, 8, 4, 2)                                                     # T = 24: every load loop has a ragged end


@pytest.mark.parametrize("parity", [0, 1])
def test_known_start_device_start_and_group_links_agree(lib, parity):
    """dccn_capture_sync(first = F), dccn_capture_sync_at(first_dev -> F) and each link of a grouped call that holds a known-start
    link and a device-start link side by side: the same frames, offsets, cfo and metric, bit for bit.  F even and odd (the
    half-pair loads at the window's ends), 5 frames (a dead wave in the last block), full and cropped rows, with and without cfo."""
    S, K, CP, W = SMALL
    T, frames = S * (K + CP), 5
    assert lib.dccn_capture_sync_supported(*SMALL) == 1
    cap = dev_capture(SMALL, 0)
    F = A.true_first(host_capture(SMALL, 0)[1], W + 4, T)
    F += (F & 1) ^ parity
    lo = F - 3
    assert F & 1 == parity and W <= lo <= F <= lo + T - 1
    first_dev = torch.tensor([F], dtype=torch.int64, device=DEV)
    known = CutLink(cap, int(cap.shape[0]), F, T)
    on_device = CutLink(cap, int(cap.shape[0]), F, T, first_dev, lo)
    for out_kin in (K + CP, K):
        for cfo in (False, True):
            want, at = Outs(SMALL, frames, out_kin), Outs(SMALL, frames, out_kin)
            assert known.solo(lib, SMALL, frames, out_kin, want, cfo, True) == 0
            assert on_device.solo(lib, SMALL, frames, out_kin, at, cfo, True) == 0
            torch.cuda.synchronize()
            assert at.same(want), (out_kin, cfo)
            assert bool((want.offset != -99).all()) and bool((want.out != SENT).all()) and bool((want.metric != SENT).all())
            assert bool((want.cfo != SENT).all()) == cfo
            for links in ([known, on_device], [on_device, known]):
                st, outs = run_cut_group(lib, SMALL, frames, out_kin, links, cfo, True)
                assert st == 0
                assert all(o.same(want) for o in outs), (out_kin, cfo)
    assert int(first_dev[0]) == F                                           # (read, never written)


# ---- frames already cut ------------------------------------------------------------------------------------------------------------
def frame_links_of(shape, n_links, frames):
    """link i's frames: cut back to back from its capture at a start up to W samples off a true one"""
    S, K, CP, W = shape
    T = S * (K + CP)
    xs = []
    for i in range(n_links):
        cap, start = host_capture(shape, i)
        first = A.true_first(start, W, T) + (i % (2 * W + 1)) - W
        xs.append(torch.from_numpy(np.array(cap[first:first + frames * T]).reshape(frames, S, K + CP, 2)).to(DEV))
    return xs


def run_frame_group(lib, shape, frames, out_kin, xs, cfo, metric, outs=None):
    from dl_ofdm_amd import _lib
    outs = outs or [Outs(shape, frames, out_kin) for _ in xs]
    entries = []
    for x, o in zip(xs, outs):
        xo, off, cf, me = o.ptrs(cfo, metric)
        entries.append(_lib.FrameLink(x.data_ptr(), xo, off, cf, me))
    st = lib.dccn_frame_sync_grouped(len(xs), table(entries), frames, *shape, out_kin, stream())
    torch.cuda.synchronize()
    return st, outs


@pytest.mark.parametrize("n_links", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_frame_sync_gives_the_solo_bits(lib, shape, n_links):
    S, K, CP, W = shape
    for frames in FRAMES:
        xs = frame_links_of(shape, n_links, frames)
        for out_kin in (K + CP, K):
            for cfo in (False, True):
                for metric in (False, True):
                    st, outs = run_frame_group(lib, shape, frames, out_kin, xs, cfo, metric)
                    assert st == 0
                    for i, (x, o) in enumerate(zip(xs, outs)):
                        ref = Outs(shape, frames, out_kin)
                        xo, off, cf, me = ref.ptrs(cfo, metric)
                        if cfo:
                            sr = lib.dccn_frame_sync_cfo(x.data_ptr(), frames, *shape, out_kin, xo, off, cf, me, stream())
                        else:
                            sr = lib.dccn_frame_sync(x.data_ptr(), frames, *shape, out_kin, xo, off, me, stream())
                        torch.cuda.synchronize()
                        assert sr == 0 and o.same(ref), (shape, frames, out_kin, n_links, i, cfo, metric)
                        assert bool((o.offset != -99).all()) and bool((o.cfo != SENT).all()) == cfo


# ---- acquisition -------------------------------------------------------------------------------------------------------------------
class AcqOuts:
    def __init__(self, lib, CP, J, n_pilot, short=0):
        self.first = torch.full((1,), -99, dtype=torch.int64, device=DEV)
        self.cfo = torch.full((1,), SENT, dtype=torch.float32, device=DEV)
        self.sym = torch.full((A.K + CP,), SENT, dtype=torch.float32, device=DEV)
        self.phase = torch.full((A.S,), SENT, dtype=torch.float32, device=DEV)
        self.nws = int(lib.dccn_capture_acquire_workspace_size(A.S, A.K, CP, n_pilot, J)) - short
        self.ws = torch.zeros(self.nws + short, dtype=torch.uint8, device=DEV)

    def same(self, o):
        return (torch.equal(self.first, o.first) and same_bits(self.cfo, o.cfo) and same_bits(self.sym, o.sym)
                and same_bits(self.phase, o.phase))

    def untouched(self):
        return (int(self.first[0]) == -99 and bool((self.cfo == SENT).all()) and bool((self.sym == SENT).all())
                and bool((self.phase == SENT).all()) and bool((self.ws == 0).all()))

    def entry(self, cap, ns, lo, sc, metrics=True):
        from dl_ofdm_amd import _lib
        return _lib.AcquireLink(cap.data_ptr(), int(ns), int(lo), sc.data_ptr(), self.first.data_ptr(), self.cfo.data_ptr(),
                                self.sym.data_ptr() if metrics else None, self.phase.data_ptr() if metrics else None,
                                self.ws.data_ptr(), self.nws)

    def solo(self, lib, cap, ns, lo, J, CP, sc):
        return lib.dccn_capture_acquire(cap.data_ptr(), int(ns), int(lo), J, A.S, A.K, CP, sc.data_ptr(), int(sc.numel()),
                                        self.first.data_ptr(), self.cfo.data_ptr(), self.sym.data_ptr(), self.phase.data_ptr(),
                                        self.ws.data_ptr(), self.nws, stream())


def run_acq_group(lib, CP, J, caps, los, sc, ns=None):
    outs = [AcqOuts(lib, CP, J, int(sc.numel())) for _ in caps]
    ns = ns or [int(c.shape[0]) for c in caps]
    t = table([o.entry(c, n, lo, sc) for o, c, n, lo in zip(outs, caps, ns, los)])
    st = lib.dccn_capture_acquire_grouped(len(caps), t, J, A.S, A.K, CP, int(sc.numel()), stream())
    torch.cuda.synchronize()
    return st, outs


@pytest.mark.parametrize("n_links", [1, 3, 8])
@pytest.mark.parametrize("J", [1, 4])
@pytest.mark.parametrize("CP", [16, 4])
def test_grouped_acquisition_gives_the_solo_bits(lib, CP, J, n_links):
    shape = (A.S, A.K, CP, 3 if CP == 16 else 4)
    sc = torch.from_numpy(np.array(A.pilot_sc_of(CP))).to(DEV)
    caps = [dev_capture(shape, i) for i in range(n_links)]
    los = [A.LOS[(i + J) % len(A.LOS)] for i in range(n_links)]              # even and odd origins, differing per link
    st, outs = run_acq_group(lib, CP, J, caps, los, sc)
    assert st == 0
    for i, (cap, lo, o) in enumerate(zip(caps, los, outs)):
        ref = AcqOuts(lib, CP, J, int(sc.numel()))
        assert ref.solo(lib, cap, cap.shape[0], lo, J, CP, sc) == 0
        torch.cuda.synchronize()
        assert o.same(ref), (CP, J, n_links, i)
        assert lo <= int(o.first[0]) < lo + A.S * (A.K + CP) and bool((o.sym != SENT).all()) and bool((o.phase != SENT).all())
    assert n_links == 1 or len({int(o.first[0]) - lo for o, lo in zip(outs, los)}) > 1


@pytest.mark.parametrize("CP", [16, 4])
def test_acquire_then_cut_as_four_launches(lib, CP):
    """grouped acquisition, then the grouped cut reading every link's start on the device, against the solo sequence per link"""
    W = 3 if CP == 16 else 4
    shape, J, frames, n_links = (A.S, A.K, CP, W), 4, 5, 8
    T = A.S * (A.K + CP)
    sc = torch.from_numpy(np.array(A.pilot_sc_of(CP))).to(DEV)
    caps = [dev_capture(shape, i) for i in range(n_links)]
    los = [A.LOS[1 + i % 3] for i in range(n_links)]                         # 37, 300, 555: every lo >= W
    st, acq = run_acq_group(lib, CP, J, caps, los, sc)
    assert st == 0
    links = [CutLink(c, c.shape[0], 0, T, a.first, lo) for c, a, lo in zip(caps, acq, los)]
    for cfo in (False, True):
        st, outs = run_cut_group(lib, shape, frames, A.K + CP, links, cfo, True)
        assert st == 0
        for i, (cap, lo, o) in enumerate(zip(caps, los, outs)):
            sa = AcqOuts(lib, CP, J, int(sc.numel()))
            assert sa.solo(lib, cap, cap.shape[0], lo, J, CP, sc) == 0
            ref = Outs(shape, frames, A.K + CP)
            assert CutLink(cap, cap.shape[0], 0, T, sa.first, lo).solo(lib, shape, frames, A.K + CP, ref, cfo, True) == 0
            torch.cuda.synchronize()
            assert o.same(ref) and torch.equal(sa.first, acq[i].first), (CP, i, cfo)


# ---- tight captures ----------------------------------------------------------------------------------------------------------------
def tight(cap, need, pad=6):
    """the first `need` samples of cap inside a NaN-filled buffer (pad samples either side; an even pad keeps 16-byte alignment)"""
    buf = torch.full((pad + need + pad, 2), float("nan"), dtype=torch.float32, device=DEV)
    buf[pad:pad + need] = cap[:need]
    return buf, buf[pad:]


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_tight_captures(lib, shape):
    S, K, CP, W = shape
    T, frames, n_links, J = S * (K + CP), 5, 4, 4
    roomy = cut_links(shape, n_links, frames, share=False)
    need = [l.first + (frames - 1) * l.stride + T + W for l in roomy]
    keep = [tight(l.cap, n) for l, n in zip(roomy, need)]
    links = [CutLink(k[1], n, l.first, l.stride) for k, n, l in zip(keep, need, roomy)]
    _, want = run_cut_group(lib, shape, frames, K + CP, roomy, True, True)
    st, got = run_cut_group(lib, shape, frames, K + CP, links, True, True)
    assert st == 0
    for g, w in zip(got, want):
        assert g.same(w) and bool(torch.isfinite(g.out).all()) and bool(torch.isfinite(g.metric).all()) and bool(torch.isfinite(g.cfo).all())
    # one sample less on ONE link: the whole call is refused, nothing is written for any link
    for victim in (0, n_links - 1):
        short = [CutLink(l.cap, l.ns - (i == victim), l.first, l.stride) for i, l in enumerate(links)]
        st, outs = run_cut_group(lib, shape, frames, K + CP, short, True, True)
        assert st == INVALID and all(o.untouched() for o in outs), victim
    # acquisition: lo + (J + 2) T samples per link
    sc = torch.from_numpy(np.array(A.pilot_sc_of(CP))).to(DEV)
    caps = [dev_capture(shape, i) for i in range(n_links)]
    los = [A.LOS[i % len(A.LOS)] for i in range(n_links)]
    need = [lo + (J + 2) * T for lo in los]
    keep = [tight(c, n) for c, n in zip(caps, need)]
    _, want = run_acq_group(lib, CP, J, caps, los, sc)
    st, got = run_acq_group(lib, CP, J, [k[1] for k in keep], los, sc, ns=need)
    assert st == 0
    for g, w in zip(got, want):
        assert g.same(w) and bool(torch.isfinite(g.sym).all()) and bool(torch.isfinite(g.phase).all()) and bool(torch.isfinite(g.cfo).all())
    st, outs = run_acq_group(lib, CP, J, [k[1] for k in keep], los, sc, ns=[n - (i == 2) for i, n in enumerate(need)])
    assert st == INVALID and all(o.untouched() for o in outs)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_for_any_link(lib):
    from dl_ofdm_amd import _lib
    shape = SHAPES[0]
    S, K, CP, W = shape
    T, frames, n = S * (K + CP), 5, 3
    links = cut_links(shape, n, frames)
    outs = [Outs(shape, frames, K + CP) for _ in links]

    def cut(entries, n_links=n, null=False):
        t = table(entries, 9)
        st = lib.dccn_capture_sync_grouped(n_links, None if null else t, frames, *shape, K + CP, stream())
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)
        return st

    good = lambda: [l.entry(o, True, True) for l, o in zip(links, outs)]      # noqa: E731
    assert cut(good() * 3, 0) == INVALID and cut(good() * 3, 9) == INVALID and cut(good(), null=True) == INVALID
    e = good()
    e[1].cfo = None                                                          # cfo for some links only
    assert cut(e) == INVALID
    e = good()
    e[2].metric = None
    assert cut(e) == INVALID
    e = good()
    e[2].x_out = links[0].cap.data_ptr() + 16 * T                            # inside ANOTHER link's capture
    assert cut(e) == INVALID
    e = good()
    e[0].x_out = outs[2].out.data_ptr() + 16                                 # inside another link's x_out
    assert cut(e) == INVALID
    e = good()
    e[1].x_out += 8                                                          # one misaligned pointer
    assert cut(e) == INVALID
    e = good()
    e[1].offset = outs[0].offset.data_ptr()                                  # two links, one offset array
    assert cut(e) == INVALID
    # frames already cut
    xs = frame_links_of(shape, n, frames)

    def fr(entries, n_links=n):
        st = lib.dccn_frame_sync_grouped(n_links, table(entries, 9), frames, *shape, K + CP, stream())
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)
        return st

    fgood = lambda: [_lib.FrameLink(x.data_ptr(), *o.ptrs(True, True)) for x, o in zip(xs, outs)]      # noqa: E731
    assert fr(fgood() * 3, 0) == INVALID and fr(fgood() * 3, 9) == INVALID
    e = fgood()
    e[0].cfo = None
    assert fr(e) == INVALID
    e = fgood()
    e[1].x_out = xs[2].data_ptr()                                            # onto another link's frames
    assert fr(e) == INVALID
    e = fgood()
    e[2].x += 8
    assert fr(e) == INVALID
    # acquisition
    J = 4
    sc = torch.from_numpy(np.array(A.pilot_sc_of(CP))).to(DEV)
    caps = [dev_capture(shape, i) for i in range(n)]
    aouts = [AcqOuts(lib, CP, J, int(sc.numel()), short=(i == 1)) for i in range(n)]

    def acq(entries, n_links=n):
        st = lib.dccn_capture_acquire_grouped(n_links, table(entries, 9), J, S, K, CP, int(sc.numel()), stream())
        torch.cuda.synchronize()
        assert all(o.untouched() for o in aouts)
        return st

    agood = lambda: [o.entry(c, c.shape[0], 37, sc) for o, c in zip(aouts, caps)]      # noqa: E731
    assert acq(agood()) == WORKSPACE                                         # link 1's workspace is a byte short
    e = agood()
    e[1].workspace_bytes += 1
    e[2].phase_metric = None                                                 # a metric for some links only
    assert acq(e) == INVALID
    e = agood()
    e[1].workspace_bytes += 1
    e[2].first_out = aouts[0].first.data_ptr()
    assert acq(e) == INVALID
    e = agood()
    e[1].workspace_bytes += 1
    assert acq(e, 0) == INVALID and acq(e * 3, 9) == INVALID
    # ... and the unbroken tables are accepted
    e = agood()
    e[1].workspace_bytes += 1
    assert lib.dccn_capture_acquire_grouped(n, table(e), J, S, K, CP, int(sc.numel()), stream()) == 0
    assert lib.dccn_capture_sync_grouped(n, table(good()), frames, *shape, K + CP, stream()) == 0
    assert lib.dccn_frame_sync_grouped(n, table(fgood()), frames, *shape, K + CP, stream()) == 0
    torch.cuda.synchronize()


# ---- reproducibility and the classes -----------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(lib):
    shape = SHAPES[1]
    S, K, CP, W = shape
    frames, n = 9, 8
    links = cut_links(shape, n, frames)
    a, b = (run_cut_group(lib, shape, frames, K, links, True, True)[1] for _ in range(2))
    assert all(x.same(y) for x, y in zip(a, b))
    xs = frame_links_of(shape, n, frames)
    a, b = (run_frame_group(lib, shape, frames, K + CP, xs, True, True)[1] for _ in range(2))
    assert all(x.same(y) for x, y in zip(a, b))
    sc = torch.from_numpy(np.array(A.pilot_sc_of(CP))).to(DEV)
    caps = [dev_capture(shape, i) for i in range(n)]
    a, b = (run_acq_group(lib, CP, 4, caps, [37 + i for i in range(n)], sc)[1] for _ in range(2))
    assert all(x.same(y) for x, y in zip(a, b))


def test_group_classes():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import (CaptureAcquire, CaptureAcquireGroup, CaptureSync, CaptureSyncGroup, FrameSync, FrameSyncGroup)
    shape = SHAPES[0]
    S, K, CP, W = shape
    T, frames, n, J = S * (K + CP), 5, 3, 4
    caps = [dev_capture(shape, i) for i in range(n)]
    los = [37, 300, 555]
    acq = CaptureAcquireGroup(S, K, CP, A.pilot_sc_of(CP), J, n, DEV)
    firsts = acq.run(caps, los)
    assert firsts is acq.first and len(firsts) == n and firsts[0].dtype == torch.int64
    cs = CaptureSyncGroup(S, K, CP, W, frames, n, DEV, cfo=True)
    mixed = [firsts[0], int(A.true_first(host_capture(shape, 1)[1], W, T)), firsts[2]]
    outs, offs = cs.run(caps, mixed, los=los)
    torch.cuda.synchronize()
    for i in range(n):
        one = CaptureSync(S, K, CP, W, frames, DEV, cfo=True)
        if isinstance(mixed[i], torch.Tensor):
            sa = CaptureAcquire(S, K, CP, A.pilot_sc_of(CP), J, DEV)
            o, f = one.run(caps[i], sa.run(caps[i], los[i]), lo=los[i])
            assert torch.equal(sa.first, firsts[i]) and same_bits(sa.cfo, acq.cfo[i]) and same_bits(sa.sym_metric, acq.sym_metric[i])
        else:
            o, f = one.run(caps[i], mixed[i])
        torch.cuda.synchronize()
        assert same_bits(o, outs[i]) and torch.equal(f, offs[i]) and same_bits(one.cfo, cs.cfo[i]) and same_bits(one.metric, cs.metric[i])
    assert all(torch.equal(a, b) for a, b in zip(cs.offsets(caps, mixed, los=los), offs))
    xs = frame_links_of(shape, n, frames)
    fs = FrameSyncGroup(S, K, CP, W, frames, n, DEV, out_kin=K)
    outs, offs = fs.run(xs)
    torch.cuda.synchronize()
    for i in range(n):
        o, f = FrameSync(S, K, CP, W, frames, DEV, out_kin=K).run(xs[i])
        torch.cuda.synchronize()
        assert same_bits(o, outs[i]) and torch.equal(f, offs[i])
    with pytest.raises(ValueError):
        fs.run(xs[:2])
    with pytest.raises(_lib.DccnError):
        fs.run([x.cpu() for x in xs])
    with pytest.raises(_lib.DccnError):
        cs.run(caps, [firsts[0], 5, 5])                                      # a device first needs los
    with pytest.raises(_lib.DccnError):
        cs.run(caps, mixed, los=[W - 1, W, W])
    with pytest.raises(ValueError):
        cs.run(caps, mixed[:2], los=los)
    with pytest.raises(_lib.DccnError):
        acq.run([c.cpu() for c in caps], los)
    with pytest.raises(ValueError):
        CaptureAcquireGroup(S, K, CP, A.pilot_sc_of(CP), J, 9, DEV)
