"""``dccn_classical_receive_grouped`` / ``ClassicalReceiveGroup`` on the GPU (``-m gpu``): several links' classical detectors in
ONE launch.  The bar is bitwise -- link i gets the bytes ``ClassicalRxReceiver`` / ``dccn_classical_receive`` write for link i
alone, in all five outputs, for any mix of modulations, methods, window positions and noise sources -- and, independently of the
solo kernel, the fp64 restatement of tests/classical_receive_ref.py (a switch that dispatched a link to the wrong modulation's
body would still agree with nothing there).  Then rows that end off a byte boundary packed back to back, links that share their
frames, refusals that leave poisoned outputs alone, and the grouped front ends against the solo ones.

Cases: ``classical_receive_ref.make_case(nbits, "EPA", 10.0, n=24, seed=5 + nbits, ...)``, the inputs of
tests/test_gpu_classical_receive.py (at most 0.64 % of their cells are undecidable in fp64; ``failures`` allows 1 %)."""
import ctypes as C

import numpy as np
import pytest
import torch

import classical_receive_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 24
OUT = ("packed", "llr", "chest", "y_freq", "noise")
GEOM = {"64/16": (64, True), "64/4": (64, False), "128/32": (128, True)}
# nbits, method, advance (3: win = 13, odd -- the 8-byte head and tail of the window), noise variance known
MIXED = [(1, "ALMMSE", 0, False), (2, "LS-Spline", 3, False), (3, "LS-Linear", 0, True), (4, "ALMMSE", 3, False)]
POISON = 0xA5


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_cases = {}


def case_of(geom, nbits, method, adv):
    key = (geom, nbits, method, adv)
    if key not in _cases:
        nfft, longcp = GEOM[geom]
        _cases[key] = R.make_case(nbits, "EPA", 10.0, n=N, seed=5 + nbits, nfft=nfft, longcp=longcp, method=method, advance=adv)
    return _cases[key]


def links_of(geom, spec):
    """[(case, known noise variance or None)] for a list of (nbits, method, advance, known)"""
    out = []
    for nbits, method, adv, known in spec:
        c = case_of(geom, nbits, method, adv)
        out.append((c, c["known_noise"] if known else None))
    return out


def group_of(links, batch):
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    grp = ClassicalReceiveGroup([c["F"] for c, _ in links], batch, methods=[c["method"] for c, _ in links],
                                advances=[c["advance"] for c, _ in links], noise_vars=[nv for _, nv in links], want_llr=True)
    grp.want_y_freq()
    return grp


def solo_of(c, nv, batch):
    from dl_ofdm_amd.classical_receive import ClassicalRxReceiver
    rx = ClassicalRxReceiver(c["F"], batch, method=c["method"], advance=c["advance"], noise_var=nv, want_llr=True)
    rx.want_y_freq()
    return rx


def outputs(rx):
    torch.cuda.synchronize()
    return {k: getattr(rx, k).clone() for k in OUT}


def poison(rx):
    for k in OUT:
        getattr(rx, k).view(torch.uint8).fill_(POISON)


def untouched(rx) -> bool:
    torch.cuda.synchronize()
    return all(bool((getattr(rx, k).view(torch.uint8) == POISON).all()) for k in OUT)


def check_group_equals_solo(links, frames, lo=0):
    """one grouped call on frames [lo, lo + frames) of every link's case against the solo calls into buffers of their own; a
    second grouped run gives the same bytes.  -> (group, the links' outputs)"""
    grp = group_of(links, frames)
    xs = [c["x"][lo:lo + frames] for c, _ in links]
    for l in grp.links:
        poison(l)
    res = grp.receive(xs)
    assert len(res) == len(links)
    for r, l in zip(res, grp.links):
        assert r.prob is None and r.packed is l.packed and r.llr is l.llr and r.offset is None and r.cfo is None and r.first is None
        assert (r.D, r.nbits) == (l.D, l.nbits)
    got = [outputs(l) for l in grp.links]
    for i, (c, nv) in enumerate(links):
        solo = solo_of(c, nv, frames)
        poison(solo)
        solo.receive(xs[i])
        want = outputs(solo)
        for k in OUT:
            assert same_bits(got[i][k], want[k]), (frames, i, c["nbits"], c["method"], k)
    grp.receive(xs)
    again = [outputs(l) for l in grp.links]
    assert all(same_bits(a[k], b[k]) for a, b in zip(got, again) for k in OUT)
    return grp, got


_mixed24 = {}


def mixed24():
    """the 24-frame grouped call of the four mixed links, run once: (links, group, outputs)"""
    if not _mixed24:
        links = links_of("64/16", MIXED)
        grp, got = check_group_equals_solo(links, N)
        _mixed24.update(links=links, grp=grp, got=got)
    return _mixed24["links"], _mixed24["grp"], _mixed24["got"]


def test_mixed_links_equal_solo_at_24_frames():
    links, grp, got = mixed24()
    assert [l.nbits for l in grp.links] == [1, 2, 3, 4]
    assert [int(l.args.win) for l in grp.links] == [16, 13, 16, 13] and [int(l.args.mode) for l in grp.links] == [2, 0, 0, 2]
    assert [float(l.args.noise_var) > 0 for l in grp.links] == [False, False, True, False]
    assert [g["packed"].shape[1] for g in got] == [40, 80, 120, 160]


@pytest.mark.parametrize("frames,lo", [(3, 5), (1, 13)])
def test_mixed_links_equal_solo_on_a_ragged_tile_and_on_one_frame(frames, lo):
    # 3 frames: one tile of two frames and one of one, per link
    _, got = check_group_equals_solo(links_of("64/16", MIXED), frames, lo)
    # ... and a frame's outputs do not depend on how many frames or links the call carries
    _, _, full = mixed24()
    assert all(same_bits(g[k], f[k][lo:lo + frames]) for g, f in zip(got, full) for k in OUT)


def device_case(c, rx):
    """the case with the tables the engine really hands the kernel"""
    d = dict(c)
    d.update(dft=rx.dft.cpu().numpy(), w=rx.w.cpu().numpy(), pil=rx.pil.cpu().numpy(), dat=rx.dat.cpu().numpy(),
             empty=rx.empty.cpu().numpy(), table=rx.table.cpu().numpy(), labels=rx.labels.cpu().numpy(),
             pv=(np.float32(rx.args.pv_re), np.float32(rx.args.pv_im)), win=int(rx.args.win), mode=int(rx.args.mode))
    return d


@pytest.mark.parametrize("i", range(len(MIXED)))
def test_mixed_links_inside_the_fp64_bounds(i):
    links, grp, got = mixed24()
    c, nv = links[i]
    ref = R.restate_case(device_case(c, grp.links[i]), nv or 0.0)
    fig = R.compare(ref, {k: v.cpu().numpy() for k, v in got[i].items()}, c["D"], c["nbits"])
    print("link %d nbits=%d %s adv=%d: %s" % (i, c["nbits"], c["method"], c["advance"],
                                              {k: (round(v, 4) if isinstance(v, float) else v) for k, v in fig.items()}))
    assert R.failures(fig) == [], fig


def test_eight_links_and_one_link():
    spec = [(1 + i % 4, ("ALMMSE", "LS-Spline", "LS-Linear")[i % 3], (0, 3)[i % 2], i in (2, 5)) for i in range(8)]
    check_group_equals_solo(links_of("64/16", spec), 3, lo=7)
    check_group_equals_solo(links_of("64/16", [(3, "ALMMSE", 3, False)]), 3, lo=7)        # n_links == 1 is the solo call


@pytest.mark.parametrize("geom,spec", [("64/4", [(2, "ALMMSE", 3, False), (4, "LS-Spline", 0, True)]),
                                       ("128/32", [(3, "LS-Spline", 3, False), (2, "ALMMSE", 0, False)])])
def test_other_geometries(geom, spec):
    check_group_equals_solo(links_of(geom, spec), 3, lo=2)


# ---- through the C entry: rows that do not end on a boundary, back to back ------------------------------------------------------
GUARD = 64


def link_struct(rx, **over):
    from dl_ofdm_amd import _lib
    a = rx.args
    l = _lib.ClassicalLink(a.nbits, a.m, a.mode, a.win, a.noise_var, a.pv_re, a.pv_im, a.dft, a.w, a.pil, a.dat, a.empty, a.table,
                           a.labels, a.x, a.packed, a.llr, a.chest, a.y_freq, a.noise)
    for k, v in over.items():
        setattr(l, k, v)
    return l


def call_grouped(lib, links, frames, rx, D=None):
    from dl_ofdm_amd import _lib
    t = (_lib.ClassicalLink * len(links))(*links)
    st = lib.dccn_classical_receive_grouped(len(links), t, frames, rx.S, rx.K, rx.CP, rx.P, rx.D if D is None else D, rx.E,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def test_ragged_rows_back_to_back_between_guard_bytes(lib):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import row_bytes
    n, D = 5, 317
    cs = [case_of("64/16", 3, "ALMMSE", 3), case_of("64/16", 4, "ALMMSE", 3)]
    rxs = [solo_of(c, None, N) for c in cs]
    for rx, c in zip(rxs, cs):
        rx.x[:n].copy_(dev(c["x"][:n]))
    SK = rxs[0].S * rxs[0].K
    RB = [row_bytes(D, 3), row_bytes(D, 4)]
    assert RB == [119, 159] and RB[0] * 8 - D * 3 == 1 and RB[1] * 8 - D * 4 == 4
    size = dict(packed=[n * RB[0], n * RB[1]], llr=[4 * n * D * 3, 4 * n * D * 4], chest=[8 * n * SK] * 2, y_freq=[8 * n * SK] * 2,
                noise=[4 * n] * 2)
    # packed: guard + 1 (an odd address), link 0's rows, link 1's rows right behind them, guard.  The others: guard, link 0,
    # a gap of at least a guard up to the next 64-byte boundary, link 1, guard.
    at = {"packed": [GUARD + 1, GUARD + 1 + size["packed"][0]]}
    for k in OUT[1:]:
        at[k] = [GUARD, (GUARD + size[k][0] + GUARD + 63) // 64 * 64]
    buf = {k: torch.full((at[k][1] + size[k][1] + GUARD,), POISON, dtype=torch.uint8, device=DEV) for k in OUT}
    assert all(b.data_ptr() % 64 == 0 for b in buf.values()) and (buf["packed"].data_ptr() + at["packed"][0]) % 2 == 1
    links = [link_struct(rx, **{k: buf[k].data_ptr() + at[k][i] for k in OUT}) for i, rx in enumerate(rxs)]
    assert call_grouped(lib, links, n, rxs[0], D) == 0
    for i, rx in enumerate(rxs):
        # the solo entry on the same arguments, into buffers of its own
        own = {k: torch.full((GUARD + 1 + size[k][i] + GUARD,), POISON, dtype=torch.uint8, device=DEV) for k in OUT}
        lead = {k: GUARD + (1 if k == "packed" else 0) for k in OUT}
        a = _lib.ClassicalReceiveArgs.from_buffer_copy(rx.args)
        a.frames, a.D = n, D
        for k in OUT:
            setattr(a, k, own[k].data_ptr() + lead[k])
        assert lib.dccn_classical_receive(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        torch.cuda.synchronize()
        for k in OUT:
            assert torch.equal(buf[k][at[k][i]:at[k][i] + size[k][i]], own[k][lead[k]:lead[k] + size[k][i]]), (i, k)
        packed = buf["packed"][at["packed"][i]:at["packed"][i] + size["packed"][i]].view(n, RB[i]).cpu().numpy()
        pad = RB[i] * 8 - D * rx.nbits
        assert np.all(packed[:, -1] & ((1 << pad) - 1) == 0)                     # the padding bits
    # every byte that belongs to no link keeps the pattern
    for k in OUT:
        keep = torch.ones_like(buf[k], dtype=torch.bool)
        for i in range(2):
            keep[at[k][i]:at[k][i] + size[k][i]] = False
        assert bool((buf[k][keep] == POISON).all()), k
        assert int(keep.sum()) >= 2 * GUARD


def test_two_links_share_their_frames():
    c_ls, c_mm = case_of("64/16", 2, "LS-Spline", 0), case_of("64/16", 2, "ALMMSE", 0)
    assert np.array_equal(c_ls["x"], c_mm["x"])
    links = [(c_ls, None), (c_mm, None)]
    grp = group_of(links, N)
    grp.links[1].args.x = grp.links[0].args.x                                    # both links read link 0's resident frames
    grp.links[1].x.fill_(float("nan"))
    grp.receive([c_ls["x"], None])
    got = [outputs(l) for l in grp.links]
    for i, (c, nv) in enumerate(links):
        solo = solo_of(c, nv, N)
        solo.receive(c["x"])
        want = outputs(solo)
        assert all(same_bits(got[i][k], want[k]) for k in OUT), i
    assert not same_bits(got[0]["chest"], got[1]["chest"])


def test_refusals_leave_every_links_outputs_alone(lib):
    from dl_ofdm_amd._lib import DccnError
    links = links_of("64/16", MIXED)
    grp = group_of(links, 3)
    xs = [c["x"][:3] for c, _ in links]

    def refused(field, value, link):
        keep = getattr(grp.links[link].args, field)
        setattr(grp.links[link].args, field, value)
        for l in grp.links:
            poison(l)
        with pytest.raises(DccnError, match="dccn_classical_receive_grouped"):
            grp.receive(xs)
        assert all(untouched(l) for l in grp.links), (field, link)
        setattr(grp.links[link].args, field, keep)

    refused("mode", 1, 2)                                                        # one bad link among good ones (the third)
    refused("win", 17, 3)
    refused("llr", None, 1)                                                      # an output for some links only
    refused("packed", grp.links[1].chest.data_ptr() + 16, 0)                     # link 0's rows inside link 1's chest
    refused("packed", grp.links[1].x.data_ptr(), 0)                              # ... and on link 1's frames
    rx = grp.links[0]
    for l in grp.links:
        poison(l)
    assert call_grouped(lib, [link_struct(l) for l in grp.links], 0, rx) == -1   # frames == 0
    assert call_grouped(lib, [link_struct(grp.links[i % 4]) for i in range(9)], 3, rx) == -1
    assert all(untouched(l) for l in grp.links)
    # the group is whole again
    grp.receive(xs)
    assert not any(untouched(l) for l in grp.links)


# ---- front ends ----------------------------------------------------------------------------------------------------------------
W, LEAD, B = 3, 64, 5


def stream_capture(nbits, seed, eps):
    """8 frames through a static EPA channel as ONE contiguous capture (radio.rayleigh_chan_lte.run_stream: the frames' full
    convolutions overlap-added), 20 dB, one carrier offset over the capture -> (flags, float32 [n, 2]); frame f starts at
    LEAD + f T"""
    from dl_ofdm_amd import ofdm, util
    from dl_ofdm_amd.radio import apply_cfo_stream, rayleigh_chan_lte
    from dl_ofdm_amd.receiver import Flags
    F = Flags(nbits=nbits, channel="EPA")
    o = ofdm.ofdm_tx(F)
    T = o.nSymbol * (o.K + o.CP)
    st = np.random.get_state()
    np.random.seed(seed)
    try:
        bits = util.bit_source(nbits, o.frame_size, 8)
        iq, _, _ = o.ofdm_tx_frame_np(bits)
        c, _ = rayleigh_chan_lte(F, o.Fs).run_stream(iq, LEAD)
        c = c.astype(np.complex128)
        c /= np.sqrt(np.mean(np.abs(c[LEAD:LEAD + 8 * T]) ** 2))
        c = c + np.sqrt(0.5) * 10.0 ** (-20.0 / 20.0) * (np.random.randn(c.shape[0]) + 1j * np.random.randn(c.shape[0]))
    finally:
        np.random.set_state(st)
    cap = apply_cfo_stream(np.stack([c.real, c.imag], axis=-1).astype(np.float32), eps, int(o.K))
    return F, np.ascontiguousarray(cap, dtype=np.float32), T


def fields(res):
    torch.cuda.synchronize()
    return [None if t is None else t.clone() for t in (res.packed, res.llr, res.offset, res.cfo, res.first, res.acquired_cfo)]


def same_fields(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and same_bits(x, y)) for x, y in zip(a, b))


def test_front_ends_equal_the_solo_front_ends():
    from dl_ofdm_amd._lib import DccnError
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    from dl_ofdm_amd.radio import quantize_sc16
    (F2, cap2, T), (F4, cap4, _) = stream_capture(2, 31, 0.11), stream_capture(4, 32, -0.07)
    caps = [dev(cap2), dev(cap4)]
    grp = ClassicalReceiveGroup([F2, F4], B, methods=["ALMMSE", "LS-Spline"], advances=[0, 3], want_llr=True)
    S, K, CP = grp.links[0].S, grp.links[0].K, grp.links[0].CP
    assert T == S * (K + CP)
    los = [W, 37]

    def check(group_call, solo_call, what, present):
        for l in grp.links:
            poison_front(l)
        got = [fields(r) for r in group_call()]
        for i, l in enumerate(grp.links):
            poison_front(l)
            want = fields(solo_call(i, l))
            assert same_fields(got[i], want), (what, i)
            assert [g is not None for g in got[i]] == (present(i) if callable(present) else present), (what, i)

    def poison_front(l):
        l.packed.fill_(POISON)
        l.llr.view(torch.uint8).fill_(POISON)
        l.x.view(torch.uint8).fill_(POISON)

    # frames cut two samples late: one alignment launch for both links, then the one classical launch
    xs = [c[LEAD + 2:LEAD + 2 + B * T].reshape(B, S, K + CP, 2).clone() for c in caps]
    check(lambda: grp.receive(xs, sync=W, cfo=True), lambda i, l: l.receive(xs[i], sync=W, cfo=True), "sync cfo",
          [True, True, True, True, False, False])
    check(lambda: grp.receive(xs), lambda i, l: l.receive(xs[i]), "copies", [True, True, False, False, False, False])
    # acquisition for both links (three launches), the cut (one), the classical launch
    for kw in (dict(), dict(cfo=True), dict(cfo=True, cfo_scope="capture")):
        check(lambda: grp.receive_capture(caps, acquire=4, los=los, sync=W, **kw),
              lambda i, l: l.receive_capture(caps[i], acquire=4, lo=los[i], sync=W, **kw), "acquire %r" % kw,
              [True, True, True, bool(kw), True, True])
    # a start known on the host and one left on the device, in one call
    firsts = [LEAD, torch.tensor([LEAD], dtype=torch.int64, device=DEV)]
    check(lambda: grp.receive_capture(caps, firsts=firsts, los=los, sync=W, cfo=True),
          lambda i, l: l.receive_capture(caps[i], first=firsts[i], lo=los[i], sync=W, cfo=True), "firsts",
          lambda i: [True, True, True, True, i == 1, False])             # (a start on the device comes back as result.first)
    res = grp.receive_capture(caps, firsts=firsts, los=los, sync=W, cfo=True)
    assert res[0].first is None and res[1].first is firsts[1]
    # what the grouped front end does not offer names itself, before anything is launched
    for l in grp.links:
        poison_front(l)
    with pytest.raises(DccnError, match="cfo_span"):
        grp.receive_capture(caps, acquire=4, los=los, sync=W, cfo=True, cfo_span=1)
    with pytest.raises(DccnError, match="int16"):
        grp.receive_capture([caps[0], dev(quantize_sc16(0.2 * cap4, 2.0 ** -15))], firsts=[LEAD, LEAD], sync=W)
    with pytest.raises(DccnError, match="not both"):
        grp.receive_capture(caps, firsts=[LEAD, LEAD], acquire=4, sync=W)
    with pytest.raises(DccnError, match="sync"):
        grp.receive(xs, cfo=True)
    with pytest.raises(ValueError):
        grp.receive(xs[:1])
    torch.cuda.synchronize()
    assert all(bool((l.packed == POISON).all()) and bool((l.x.view(torch.uint8) == POISON).all()) for l in grp.links)
