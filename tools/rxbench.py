"""Receive path against what a user had to do before it existed, timed in ONE process, alternating:

    (a) eval_step(want_prob=True) + the device-side argmax + pack a user writes in torch (labels are dummies)
    (b) eval_step(want_prob=False)                (the metrics-only evaluation step: a subset of (a)'s launches)
    (c) receive, bits only
    (d) receive, bits + LLRs

    python tools/rxbench.py [--iters 200] [--repeats 7]            -> one JSON line (all shapes)
    python tools/rxbench.py --one 1170,2 --only c --iters 50        -> one shape, one variant (kernel-trace runs)
    python tools/rxbench.py --chains 2 4 8 [--mods 1 2 3 4] [--frames 73] [--out FILE]
        several links, each with its own (equaliser -> frozen receiver) chain: (a) G solo receive calls back to back on one
        stream against (b) ONE grouped call (dccn_eq_receive_step_grouped), per group size G; same alternation and repeats
    python tools/rxbench.py --chains 2 4 8 [--sync 3] [--cfo] [--capture] [--acquire] [--out FILE]
        the front end of a multi-link round: (a) FrameSync / CaptureSync / CaptureAcquire issued per link in front of ONE grouped
        step against (b) the grouped front end (dccn_frame_sync_grouped, dccn_capture_sync_grouped,
        dccn_capture_acquire_grouped) in front of the same step, and the front-end launches alone; same alternation and repeats
    python tools/rxbench.py --sync 3 [--out FILE]
        the same receive call on full frames resident on the device: (copy) receive(x), whose first launch copies the frames
        into the receiver, against (sync) receive(x, sync=W), where the alignment launch (dccn_frame_sync) takes the copy's
        place, and (step) receive() with neither; same shapes, alternation and repeats
    python tools/rxbench.py --sync 3 --cfo [--out FILE]
        the same, plus (cfo) receive(x, sync=W, cfo=True): the launch that also estimates and removes the carrier-frequency
        offset (dccn_frame_sync_cfo) in the alignment launch's place, and that launch alone
    python tools/rxbench.py --capture [--sync 3] [--out FILE]
        receive_capture(cap, first, sync=W[, cfo=True]) on one contiguous capture (dccn_capture_sync) against receive(x, sync=W[,
        cfo=True]) on the same frames cut in advance, and each launch alone; 1170 and 20 000 frames QPSK, same alternation
    python tools/rxbench.py --capture --cfo --cfo_scope capture [--chains 2 4 8] [--out FILE]
        the same with receive_capture(..., cfo=True, cfo_scope="capture") added: one carrier offset per capture, pooled over its
        frames (dccn_capture_sync_pooled: three launches in place of the one), at 73, 1170 and 20 000 frames; with --chains the
        grouped round with the pooled cut against the per-frame one
    python tools/rxbench.py --acquire [--sync 3] [--cfo_span 7 31] [--out FILE]
        receive_capture(cap, first=None, acquire=J, lo=...) (dccn_capture_acquire + dccn_capture_sync_at + the step) against
        receive_capture(cap, first) with the start known, J = 4 and 16, and the acquisition launches alone; 73 and 1170 frames
        QPSK, same alternation.  --cfo_span M ...: also dccn_capture_acquire_wide alone at every M against dccn_capture_acquire of
        the same build, and receive_capture(..., cfo=True, acquire=16, cfo_span=M) against cfo_span=0, per frame and pooled
    python tools/rxbench.py --sc16 [--sync 3] [--out FILE]
        receive_capture on a 16-bit integer I/Q capture (dccn_capture_sync_sc16, dccn_capture_sync_pooled_sc16,
        dccn_capture_acquire_sc16) against (f32) the same call on the same values as float32 and (conv) cap.to(float32) * scale
        followed by (f32), what a caller without the sc16 entries does; cfo=True under both cfo_scopes and acquire=16; 73, 1170 and
        20 000 frames QPSK on run_stream captures quantised with radio.quantize_sc16, same alternation

Shapes: 1170 frames QPSK and 16-QAM, and one 20 000-frame QPSK sweep batch (N = 64).  Every shape runs in a child process of
its own under a time limit; the parent never opens the GPU and stops at the first child that fails.  Times are medians over
the repeats of the per-step mean of `iters` back-to-back steps (inputs resident on the device); `spread` is (max - min) /
median over the repeats.  `bytes` is what each variant reads and writes beyond the receiver's own activations, from shapes.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1170, 2), (1170, 4), (20000, 2)]
S, KIN, F, D = 7, 80, 64, 320


def io_bytes(frames, nbits):
    cells = frames * D
    labels, prob, llr = cells * nbits * 4, cells * nbits * 2 * 4, cells * nbits * 4
    packed = frames * ((D * nbits + 7) // 8)
    return {"a": {"in": labels, "out": prob + packed, "reread": prob}, "b": {"in": labels, "out": 64},
            "c": {"in": 0, "out": packed}, "d": {"in": 0, "out": packed + llr}}


def run_one(frames, nbits, iters, repeats, only):
    import numpy as np
    import torch
    from dl_ofdm_amd.engine import RxDims, RxEngine, glorot_init
    from dl_ofdm_amd.receive import RxReceiver
    dims = RxDims(S, KIN, F, D, nbits)
    p = glorot_init(dims, 1)
    rng = np.random.RandomState(0)
    x = torch.as_tensor(rng.randn(frames, S, KIN, 2).astype(np.float32), device="cuda")
    variants = {}
    if only in (None, "a"):
        ea = RxEngine(dims, frames, train=False, params=p, want_prob=True, want_z=False)
        ea.x.copy_(x)
        sh = torch.arange(7, -1, -1, dtype=torch.int32, device="cuda")
        n = D * nbits
        pad = (-n) % 8

        def va():
            ea.eval_step()
            h = (ea.prob[..., 1] > ea.prob[..., 0]).reshape(frames, n).to(torch.int32)
            if pad:
                h = torch.nn.functional.pad(h, (0, pad))
            return (h.reshape(frames, -1, 8) << sh).sum(-1).to(torch.uint8)
        variants["a"] = va
    if only in (None, "b"):
        eb = RxEngine(dims, frames, train=False, params=p, want_prob=False, want_z=False)
        eb.x.copy_(x)
        variants["b"] = eb.eval_step
    if only in (None, "c"):
        rc = RxReceiver(dims, frames, p)
        rc.x.copy_(x)
        variants["c"] = rc.receive
    if only in (None, "d"):
        rd = RxReceiver(dims, frames, p, want_llr=True)
        rd.x.copy_(x)
        variants["d"] = rd.receive
    if only is None:                       # (a) and (c) must agree before anything is timed
        assert torch.equal(variants["a"](), variants["c"]().packed)
    for f in variants.values():            # warm-up: first-launch costs, clocks
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for k, f in variants.items():      # alternating: every repeat visits every variant
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    out = {"frames": frames, "nbits": nbits, "iters": iters, "repeats": repeats, "bytes": io_bytes(frames, nbits), "us": {}, "spread": {}}
    for k, v in t.items():
        v = sorted(v)
        med = v[len(v) // 2]
        out["us"][k] = round(med, 2)
        out["spread"][k] = round((v[-1] - v[0]) / med, 4)
    return out


def timed(variants, iters, repeats):
    """warm up, then `repeats` rounds that visit every variant in turn: (median us per call, (max - min) / median) per variant"""
    import torch
    for f in variants.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for k, f in variants.items():
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    us, spread = {}, {}
    for k, v in t.items():
        v = sorted(v)
        med = v[len(v) // 2]
        us[k], spread[k] = round(med, 2), round((v[-1] - v[0]) / med, 4)
    return us, spread


def run_sync(frames, nbits, W, iters, repeats, cfo=False):
    """receive(x) (copy + step) against receive(x, sync=W) (alignment launch + step) and receive() (the step alone), on full
    frames [frames, S, K + CP, 2] resident on the device; the first two must agree where every offset is 0 before anything is timed.
    ``cfo``: also receive(x, sync=W, cfo=True), which must agree too (an exact prefix has no offset of either kind)"""
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims, glorot_init
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import FrameSync
    CP = KIN - F
    dims = RxDims(S, KIN, F, D, nbits)
    rc = RxReceiver(dims, frames, glorot_init(dims, 1), CP=CP)
    rng = np.random.RandomState(0)
    # frames with a true cyclic prefix (so the estimate is 0 and both calls must return the same bits)
    body = rng.randn(frames, S, F, 2).astype(np.float32)
    x = torch.as_tensor(np.concatenate([body[:, :, F - CP:], body], axis=2), device="cuda")
    a, b = rc.receive(x).packed.clone(), rc.receive(x, sync=W)
    assert int(b.offset.abs().max()) == 0 and torch.equal(a, b.packed)
    fs = FrameSync(S, F, CP, W, frames, "cuda", want_metric=False)
    variants = {"copy": lambda: rc.receive(x), "sync": lambda: rc.receive(x, sync=W), "step": rc.receive,
                "sync_alone": lambda: fs.run(x), "copy_alone": lambda: rc.x.copy_(x)}
    if cfo:
        c = rc.receive(x, sync=W, cfo=True)
        assert int(c.offset.abs().max()) == 0 and float(c.cfo.abs().max()) == 0.0 and torch.equal(a, c.packed)
        fc = FrameSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=True)
        variants["cfo"] = lambda: rc.receive(x, sync=W, cfo=True)
        variants["cfo_alone"] = lambda: fc.run(x)
    us, spread = timed(variants, iters, repeats)
    moved = 2 * frames * S * KIN * 2 * 4
    return {"frames": frames, "nbits": nbits, "W": W, "iters": iters, "repeats": repeats, "us": us, "spread": spread,
            "bytes_moved_by_copy_or_sync": moved, "build_id": _lib.load().dccn_build_id().decode()}


def run_capture(frames, nbits, W, iters, repeats, pooled=False):
    """receive_capture(cap, first, sync=W[, cfo=True]) on a contiguous capture against the path it replaces: receive(x, sync=W[,
    cfo=True]) on the same frames cut in advance (both resident on the device), and each launch alone.  The frames carry a true
    cyclic prefix, so every estimate is 0 and all four calls must return the same bits before anything is timed.
    ``pooled``: also receive_capture(..., cfo=True, cfo_scope="capture") -- one offset per capture, three launches in place of the
    one -- and those launches alone; it must return the same bits too."""
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims, glorot_init
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import CaptureSync, FrameSync
    CP = KIN - F
    T = S * KIN
    dims = RxDims(S, KIN, F, D, nbits)
    rc = RxReceiver(dims, frames, glorot_init(dims, 1), CP=CP)
    rng = np.random.RandomState(0)
    body = rng.randn(frames + 2, S, F, 2).astype(np.float32)
    full = np.concatenate([body[:, :, F - CP:], body], axis=2)            # one frame in front of the cut ones and one behind
    cap = torch.as_tensor(full.reshape(-1, 2), device="cuda")
    x = torch.as_tensor(full[1:-1], device="cuda")
    a = rc.receive(x).packed.clone()
    for call in (lambda: rc.receive(x, sync=W), lambda: rc.receive(x, sync=W, cfo=True), lambda: rc.receive_capture(cap, T, sync=W),
                 lambda: rc.receive_capture(cap, T, sync=W, cfo=True)):
        r = call()
        assert int(r.offset.abs().max()) == 0 and torch.equal(a, r.packed) and (r.cfo is None or float(r.cfo.abs().max()) == 0.0)
    fs, fc = (FrameSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=c) for c in (False, True))
    cs, cc = (CaptureSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=c) for c in (False, True))
    variants = {"sync": lambda: rc.receive(x, sync=W), "capture": lambda: rc.receive_capture(cap, T, sync=W),
                "cfo": lambda: rc.receive(x, sync=W, cfo=True), "capture_cfo": lambda: rc.receive_capture(cap, T, sync=W, cfo=True),
                "sync_alone": lambda: fs.run(x), "capture_alone": lambda: cs.run(cap, T),
                "cfo_alone": lambda: fc.run(x), "capture_cfo_alone": lambda: cc.run(cap, T)}
    if pooled:
        r = rc.receive_capture(cap, T, sync=W, cfo=True, cfo_scope="capture")
        assert int(r.offset.abs().max()) == 0 and torch.equal(a, r.packed) and float(r.cfo.abs().max()) == 0.0 and r.cfo.numel() == 1
        cp = CaptureSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=True, cfo_scope="capture")
        variants["capture_cfo_pooled"] = lambda: rc.receive_capture(cap, T, sync=W, cfo=True, cfo_scope="capture")
        variants["capture_cfo_pooled_alone"] = lambda: cp.run(cap, T)
    us, spread = timed(variants, iters, repeats)
    return {"frames": frames, "nbits": nbits, "W": W, "iters": iters, "repeats": repeats, "us": us, "spread": spread,
            "bytes_read_per_frame": {"sync": T * 8, "capture": (T + 2 * W) * 8, "capture_cfo_pooled": (2 * T + 2 * W) * 8},
            "bytes_written_per_frame": T * 8,
            "build_id": _lib.load().dccn_build_id().decode()}


def main_capture(a):
    """one child process per shape (1170 and 20 000 frames, QPSK; 73 as well with --cfo_scope capture), under a time limit; the
    parent never opens the GPU"""
    res, W = [], a.sync or 3
    pooled = a.cfo_scope == "capture"
    for fr, nb in (((73, 2),) if pooled else ()) + ((1170, 2), (20000, 2)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--capture", "--one", "%d,%d" % (fr, nb),
               "--sync", str(W), "--iters", str(a.iters if fr < 10000 else max(a.iters // 5, 10)), "--repeats", str(a.repeats)]
        cmd += ["--cfo", "--cfo_scope", "capture"] if pooled else []
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:               # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench.capture", "failed": [fr, nb], "rc": r.returncode, "shapes": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"bench": "rxbench.capture",
           "variants": {"sync": "receive(x, sync=W) on frames cut in advance", "capture": "receive_capture(cap, first, sync=W)",
                        "cfo": "receive(x, sync=W, cfo=True)", "capture_cfo": "receive_capture(cap, first, sync=W, cfo=True)",
                        "sync_alone": "FrameSync.run(x)", "capture_alone": "CaptureSync.run(cap, first)",
                        "cfo_alone": "FrameSync(cfo=True).run(x)", "capture_cfo_alone": "CaptureSync(cfo=True).run(cap, first)",
                        "capture_cfo_pooled": "receive_capture(cap, first, sync=W, cfo=True, cfo_scope='capture') (--cfo_scope capture)",
                        "capture_cfo_pooled_alone": "CaptureSync(cfo=True, cfo_scope='capture').run(cap, first) (--cfo_scope capture)"},
           "unit": "us per call (median over repeats of the mean of `iters` back-to-back calls); spread = (max - min) / median",
           "shapes": res}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def run_acquire(frames, nbits, W, iters, repeats, spans=()):
    """receive_capture(cap, first=None, acquire=J, lo=...) (acquisition + cut + step) against receive_capture(cap, first) with the
    start known on the host, on one clean transmitted capture that begins inside frame 0; and the acquisition launches alone at
    J = 4 and J = 16.  Both calls must find the same start and return the same bits before anything is timed.
    ``spans`` (--cfo_span M ...): also the wide acquisition launches alone at every M (dccn_capture_acquire_wide against
    dccn_capture_acquire of the same build), and receive_capture(..., cfo=True, acquire=16, cfo_span=M) against cfo_span=0, per
    frame and pooled; the capture carries no offset, so every call must find m^ = 0."""
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib, ofdm, util
    from dl_ofdm_amd.engine import RxDims, glorot_init
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.receiver_mp import Flags
    from dl_ofdm_amd.sync import CaptureAcquire
    CP = KIN - F
    T = S * KIN
    Fl = Flags(channel="AWGN", nbits=nbits, nfft=F, nsymbol=S, longcp=True, nfilter=64)
    o = ofdm.ofdm_tx(Fl)
    np.random.seed(0)
    _, iq, _ = o.ofdm_tx_frame_np(util.bit_source(nbits, o.frame_size, frames + 3))
    cut, lo = 211, 5
    cap = torch.as_tensor(np.ascontiguousarray(iq.reshape(-1, 2)[cut:]), device="cuda")
    true = lo + (T - cut - lo) % T
    dims = RxDims(S, KIN, F, D, nbits)
    rc = RxReceiver(dims, frames, glorot_init(dims, 1), CP=CP, pilot_sc=o.pilotSc)
    a = rc.receive_capture(cap, true, sync=W).packed.clone()
    for J in (4, 16):
        r = rc.receive_capture(cap, sync=W, acquire=J, lo=lo)
        assert int(r.first[0]) == true and torch.equal(a, r.packed)
    a4, a16 = (CaptureAcquire(S, F, CP, o.pilotSc, J, "cuda") for J in (4, 16))
    variants = {"known": lambda: rc.receive_capture(cap, true, sync=W),
                "acquire4": lambda: rc.receive_capture(cap, sync=W, acquire=4, lo=lo),
                "acquire16": lambda: rc.receive_capture(cap, sync=W, acquire=16, lo=lo),
                "acquire4_alone": lambda: a4.run(cap, lo), "acquire16_alone": lambda: a16.run(cap, lo)}
    if spans:
        for scope, tag in (("frame", ""), ("capture", "_pooled")):
            variants["acquire16_cfo" + tag] = lambda sc=scope: rc.receive_capture(cap, sync=W, cfo=True, acquire=16, lo=lo, cfo_scope=sc)
    for M in spans:
        for J in (4, 16):
            wide = CaptureAcquire(S, F, CP, o.pilotSc, J, "cuda", cfo_span=M)
            assert int(wide.run(cap, lo)[0]) == true and int(wide.cfo_int[0]) == 0
            variants["acquire%d_span%d_alone" % (J, M)] = lambda w=wide: w.run(cap, lo)
        for scope, tag in (("frame", ""), ("capture", "_pooled")):
            call = lambda sc=scope, M=M: rc.receive_capture(cap, sync=W, cfo=True, acquire=16, lo=lo, cfo_scope=sc, cfo_span=M)  # noqa: E731
            r = call()
            assert int(r.first[0]) == true and int(r.acquired_cfo_int[0]) == 0 and float(r.cfo.abs().max()) < 1e-3
            variants["acquire16_cfo%s_span%d" % (tag, M)] = call
    us, spread = timed(variants, iters, repeats)
    return {"frames": frames, "nbits": nbits, "W": W, "iters": iters, "repeats": repeats, "spans": list(spans), "us": us,
            "spread": spread, "build_id": _lib.load().dccn_build_id().decode()}


def main_acquire(a):
    """one child process per shape (73 and 1170 frames, QPSK), under a time limit; the parent never opens the GPU"""
    res, W = [], a.sync or 3
    for fr, nb in ((73, 2), (1170, 2)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--acquire", "--one", "%d,%d" % (fr, nb),
               "--sync", str(W), "--iters", str(a.iters), "--repeats", str(a.repeats)]
        cmd += ["--cfo_span"] + [str(M) for M in a.cfo_span] if a.cfo_span else []
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:               # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench.acquire", "failed": [fr, nb], "rc": r.returncode, "shapes": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"bench": "rxbench.acquire",
           "variants": {"known": "receive_capture(cap, first, sync=W), first an integer",
                        "acquire4": "receive_capture(cap, first=None, sync=W, acquire=4, lo=5)",
                        "acquire16": "receive_capture(cap, first=None, sync=W, acquire=16, lo=5)",
                        "acquire4_alone": "CaptureAcquire(J=4).run(cap, lo): the three acquisition launches",
                        "acquire16_alone": "CaptureAcquire(J=16).run(cap, lo)",
                        "acquireJ_spanM_alone": "CaptureAcquire(J, cfo_span=M).run(cap, lo): dccn_capture_acquire_wide (--cfo_span)",
                        "acquire16_cfo[_pooled]": "receive_capture(cap, first=None, sync=W, cfo=True, acquire=16, lo=5[, "
                                                  "cfo_scope='capture']) (--cfo_span)",
                        "acquire16_cfo[_pooled]_spanM": "the same with cfo_span=M (--cfo_span)"},
           "unit": "us per call (median over repeats of the mean of `iters` back-to-back calls); spread = (max - min) / median",
           "shapes": res}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def run_sc16(frames, nbits, W, iters, repeats):
    """receive_capture(int16 capture, scale) against (f32) receive_capture on sc16_to_float of the same capture and (conv) the
    conversion a caller writes in torch, cap.to(float32) * scale, followed by (f32) -- on one run_stream capture (ETU, static),
    quantised with scale = max|component| / 16384.  Three settings: cfo=True per frame, cfo=True pooled over the capture, and
    acquire=16 (the start unknown).  sc16 and f32 must return the same bits, offsets and estimates before anything is timed; the
    cut launches alone as well."""
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib, ofdm, util
    from dl_ofdm_amd.engine import RxDims, glorot_init
    from dl_ofdm_amd.radio import quantize_sc16, rayleigh_chan_lte, sc16_to_float
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.receiver_mp import Flags
    from dl_ofdm_amd.sync import CaptureSync
    CP = KIN - F
    T = S * KIN
    Fl = Flags(channel="ETU", nbits=nbits, nfft=F, nsymbol=S, longcp=True, nfilter=64)
    o = ofdm.ofdm_tx(Fl)
    np.random.seed(0)
    iq, _, _ = o.ofdm_tx_frame_np(util.bit_source(nbits, o.frame_size, frames + 3))
    lead, cut, lo = 40, 211, 5
    stream, _ = rayleigh_chan_lte(Fl, o.Fs).run_stream(iq, lead)
    stream = stream[lead + cut:]                                          # the capture begins inside frame 0
    pairs = np.stack([stream.real, stream.imag], axis=-1).astype(np.float32)
    scale = float(np.float32(np.abs(pairs).max() / 16384.0))
    q_np = quantize_sc16(pairs, scale)
    q = torch.as_tensor(q_np, device="cuda")
    f = torch.as_tensor(sc16_to_float(q_np, scale), device="cuda")
    true = lo + (T - cut - lo) % T
    dims = RxDims(S, KIN, F, D, nbits)
    rc = RxReceiver(dims, frames, glorot_init(dims, 1), CP=CP, pilot_sc=o.pilotSc)
    settings = {"cfo": dict(first=true, cfo=True), "cfo_pooled": dict(first=true, cfo=True, cfo_scope="capture"),
                "acquire16": dict(acquire=16, lo=lo)}
    variants = {}
    for name, kw in settings.items():
        want = rc.receive_capture(f, sync=W, **kw)
        want = [None if t is None else t.clone() for t in (want.packed, want.offset, want.cfo, want.first, want.acquired_cfo)]
        got = rc.receive_capture(q, sync=W, scale=scale, **kw)
        got = (got.packed, got.offset, got.cfo, got.first, got.acquired_cfo)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(want, got)), name
        assert torch.equal(q.to(torch.float32) * scale, f)
        variants[name + "_sc16"] = lambda kw=kw: rc.receive_capture(q, sync=W, scale=scale, **kw)
        variants[name + "_f32"] = lambda kw=kw: rc.receive_capture(f, sync=W, **kw)
        variants[name + "_conv"] = lambda kw=kw: rc.receive_capture(q.to(torch.float32) * scale, sync=W, **kw)
    for name, kw in (("cfo", {}), ("cfo_pooled", dict(cfo_scope="capture"))):
        cs = CaptureSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=True, **kw)
        variants[name + "_cut_sc16"] = lambda cs=cs: cs.run(q, true, scale=scale)
        variants[name + "_cut_f32"] = lambda cs=cs: cs.run(f, true)
    variants["conv_alone"] = lambda: q.to(torch.float32) * scale
    us, spread = timed(variants, iters, repeats)
    n = int(q.shape[0])
    return {"frames": frames, "nbits": nbits, "W": W, "iters": iters, "repeats": repeats, "us": us, "spread": spread,
            "capture_samples": n, "capture_bytes": {"sc16": 4 * n, "f32": 8 * n}, "frames_bytes_written": frames * T * 8,
            "scale": scale, "build_id": _lib.load().dccn_build_id().decode()}


def main_sc16(a):
    """one child process per shape (73, 1170 and 20 000 frames, QPSK), under a time limit; the parent never opens the GPU"""
    res, W = [], a.sync or 3
    for fr, nb in ((73, 2), (1170, 2), (20000, 2)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--sc16", "--one", "%d,%d" % (fr, nb),
               "--sync", str(W), "--iters", str(a.iters if fr < 10000 else max(a.iters // 5, 10)), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:               # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench.sc16", "failed": [fr, nb], "rc": r.returncode, "shapes": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"bench": "rxbench.sc16",
           "variants": {"*_sc16": "receive_capture(int16 capture, scale=...)", "*_f32": "receive_capture(the same values as float32)",
                        "*_conv": "receive_capture(cap.to(float32) * scale): the conversion launches, then the float32 call",
                        "cfo": "first known, cfo=True (per frame)", "cfo_pooled": "first known, cfo=True, cfo_scope='capture'",
                        "acquire16": "first=None, acquire=16, lo=5", "*_cut_*": "the CaptureSync launches alone",
                        "conv_alone": "cap.to(float32) * scale alone"},
           "unit": "us per call (median over repeats of the mean of `iters` back-to-back calls); spread = (max - min) / median",
           "shapes": res}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def run_chains(mods, frames, iters, repeats):
    """G (equaliser -> frozen receiver) chains, one per link, `frames` frames each: (a) G solo receive calls back to back on one
    stream, (b) one grouped call -- same parameters, same frames, inputs resident; the two must agree before anything is timed"""
    import numpy as np
    import torch
    from dl_ofdm_amd import ofdm, receiver as R, receiver_mp as H
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    fl = [H.Flags(nbits=nb, nfilter=F, seed=10 + i) for i, nb in enumerate(mods)]
    rx = [glorot_init(R.rx_dims(f, ofdm.ofdm_tx(f)), 3 + i) for i, f in enumerate(fl)]
    solo = [EqualizerTrainer(f, ofdm.ofdm_tx(f), r, seed=f.seed) for f, r in zip(fl, rx)]
    grp = ChainReceiveGroup(fl, rx, frames)
    rng = np.random.RandomState(0)
    plans = []
    for tr, ch in zip(solo, grp.chains):
        ch.tr.load_params(tr.get_params())
        pl = tr.resident(frames)
        pl.x.copy_(torch.as_tensor((rng.standard_normal(tuple(pl.x.shape)) * 2).astype(np.float32)))
        ch.pl.x.copy_(pl.x)
        plans.append(pl)
    none = [None] * len(mods)

    def va():
        return [pl.receive()[0] for pl in plans]

    def vb():
        return [r.packed for r in grp.receive(none)]
    variants = {"a": va, "b": vb}
    assert all(torch.equal(p, q) for p, q in zip(va(), vb()))
    for f in variants.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for k, f in variants.items():
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    out = {"chains": len(mods), "mods": list(mods), "frames": frames, "iters": iters, "repeats": repeats, "us": {}, "spread": {}}
    for k, v in t.items():
        v = sorted(v)
        med = v[len(v) // 2]
        out["us"][k] = round(med, 2)
        out["spread"][k] = round((v[-1] - v[0]) / med, 4)
    return out


def main_chains(a):
    """one child process per group size, under a time limit; the parent never opens the GPU and stops at the first failure"""
    res = []
    for G in a.chains:
        mods = [a.mods[i % len(a.mods)] for i in range(G)]
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one-chains", ",".join(map(str, mods)),
               "--frames", str(a.frames), "--iters", str(a.iters), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench.chains", "failed": G, "rc": r.returncode, "groups": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"bench": "rxbench.chains", "variants": {"a": "G solo receive calls back to back, one stream", "b": "one grouped receive call"},
           "unit": "us per round of G links (median over repeats of the mean of `iters` back-to-back rounds); spread = (max - min) / median",
           "groups": res}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def run_group_front(mods, frames, W, cfo, want_sync, want_capture, want_acquire, iters, repeats, solo_only=False, pooled=False):
    """G links, each with its own chain and its own clean transmitted capture: a round of the front end + ONE grouped step, with
    (a) the front end issued per link -- FrameSync.run / CaptureSync.run(out=chain.pl.x) / CaptureAcquire.run + CaptureSync.run,
        what a caller of the solo stages does in front of the grouped step -- against
    (b) the grouped front end (group.receive(xs, sync=W) / group.receive_capture(...)): one alignment or cut launch, three
        acquisition launches, for all links;
    and the front-end launches alone (`*_front`).  (a) and (b) must return the same bits before anything is timed.
    ``solo_only``: the (a) variants alone -- they use nothing an older build of the library lacks, so with DCCN_LIB_PATH naming
    the parent's build (tools/build_rev.sh, DCCN_LIB_ALLOW_MISSING=1) this times (a) on the parent's kernels.
    ``pooled`` (with ``cfo`` and ``want_capture``): also the cut with one carrier offset per capture (cfo_scope="capture": three
    launches per link in (a), three for all links in (b)), as ``*_cut_pooled``."""
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib, ofdm, receiver as R, receiver_mp as H, util
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    from dl_ofdm_amd.sync import CaptureAcquire, CaptureAcquireGroup, CaptureSync, CaptureSyncGroup, FrameSync, FrameSyncGroup
    both = not solo_only
    G = len(mods)
    fl = [H.Flags(nbits=nb, nfilter=F, seed=10 + i) for i, nb in enumerate(mods)]
    tx = [ofdm.ofdm_tx(f) for f in fl]
    rx = [glorot_init(R.rx_dims(f, o), 3 + i) for i, (f, o) in enumerate(zip(fl, tx))]
    grp = ChainReceiveGroup(fl, rx, frames)
    CP = KIN - F
    T = S * KIN
    lo, cut = 5, 211
    caps, xs, true = [], [], []
    for i, (nb, o) in enumerate(zip(mods, tx)):
        assert (o.K, o.CP) == (F, CP)
        np.random.seed(100 + i)
        _, iq, _ = o.ofdm_tx_frame_np(util.bit_source(nb, o.frame_size, frames + 3))
        c = cut + 37 * i                                                  # every link's capture begins somewhere else in its frame 0
        cap = torch.as_tensor(np.ascontiguousarray(iq.reshape(-1, 2)[c:]), device="cuda")
        first = lo + (T - c - lo) % T
        caps.append(cap)
        true.append(first)
        xs.append(cap[first:first + frames * T].reshape(frames, S, KIN, 2).clone())
    outs = [ch.pl.x for ch in grp.chains]
    none = [None] * G
    step = lambda: grp.receive(none)                                     # noqa: E731
    packed = lambda res: [r.packed.clone() for r in res]                 # noqa: E731
    variants = {"step": step}

    def agree(a, b):
        pa = packed(a())
        assert all(torch.equal(p, q) for p, q in zip(pa, packed(b())))

    if want_sync:
        fs = [FrameSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=cfo) for _ in range(G)]
        fg = FrameSyncGroup(S, F, CP, W, frames, G, "cuda", want_metric=False, cfo=cfo) if both else None

        def a_sync_front():
            for s, x, o in zip(fs, xs, outs):
                s.run(x, out=o)
        variants.update(a_sync=lambda: (a_sync_front(), step())[1], a_sync_front=a_sync_front)
        if both:
            variants.update(b_sync=lambda: grp.receive(xs, sync=W, cfo=cfo), b_sync_front=lambda: fg.run(xs, outs=outs))
            agree(variants["a_sync"], variants["b_sync"])
    if want_capture:
        cs = [CaptureSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=cfo) for _ in range(G)]
        cg = CaptureSyncGroup(S, F, CP, W, frames, G, "cuda", want_metric=False, cfo=cfo) if both else None

        def a_cut_front():
            for s, c, f, o in zip(cs, caps, true, outs):
                s.run(c, f, out=o)
        variants.update(a_cut=lambda: (a_cut_front(), step())[1], a_cut_front=a_cut_front)
        if both:
            variants.update(b_cut=lambda: grp.receive_capture(caps, firsts=true, sync=W, cfo=cfo),
                            b_cut_front=lambda: cg.run(caps, true, outs=outs))
            agree(variants["a_cut"], variants["b_cut"])
        if pooled and cfo and both:
            ps = [CaptureSync(S, F, CP, W, frames, "cuda", want_metric=False, cfo=True, cfo_scope="capture") for _ in range(G)]
            pg = CaptureSyncGroup(S, F, CP, W, frames, G, "cuda", want_metric=False, cfo=True, cfo_scope="capture")

            def a_pooled_front():
                for s, c, f, o in zip(ps, caps, true, outs):
                    s.run(c, f, out=o)
            variants.update(a_cut_pooled=lambda: (a_pooled_front(), step())[1], a_cut_pooled_front=a_pooled_front,
                            b_cut_pooled=lambda: grp.receive_capture(caps, firsts=true, sync=W, cfo=True, cfo_scope="capture"),
                            b_cut_pooled_front=lambda: pg.run(caps, true, outs=outs))
            agree(variants["a_cut_pooled"], variants["b_cut_pooled"])
        for J in (want_acquire or ()):
            acq = [CaptureAcquire(S, F, CP, o.pilotSc, J, "cuda") for o in tx]
            ag = CaptureAcquireGroup(S, F, CP, [np.asarray(o.pilotSc) for o in tx], J, G, "cuda") if both else None

            def a_front(acq=acq):
                for q, s, c, o in zip(acq, cs, caps, outs):
                    s.run(c, q.run(c, lo), out=o, lo=lo)

            def b_front(ag=ag):
                cg.run(caps, ag.run(caps, lo), outs=outs, los=lo)
            variants.update({"a_acquire%d" % J: lambda f=a_front: (f(), step())[1], "a_acquire%d_front" % J: a_front})
            if both:
                variants.update({"b_acquire%d" % J: lambda J=J: grp.receive_capture(caps, acquire=J, los=lo, sync=W, cfo=cfo),
                                 "b_acquire%d_front" % J: b_front})
                agree(variants["a_acquire%d" % J], variants["b_acquire%d" % J])
                b_front()
                assert [int(t[0]) for t in ag.first] == [int(q.first[0]) for q in acq]
    us, spread = timed(variants, iters, repeats)
    return {"chains": G, "mods": list(mods), "frames": frames, "W": W, "cfo": bool(cfo), "iters": iters, "repeats": repeats, "us": us,
            "spread": spread, "solo_only": bool(solo_only), "build_id": _lib.load().dccn_build_id().decode()}


def main_group_front(a):
    """--chains with --sync / --capture / --acquire: one child process per group size, under a time limit"""
    res, W = [], a.sync or 3
    for G in a.chains:
        mods = [a.mods[i % len(a.mods)] for i in range(G)]
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one-chains", ",".join(map(str, mods)),
               "--frames", str(a.frames), "--iters", str(a.iters), "--repeats", str(a.repeats), "--sync", str(W)]
        cmd += (["--cfo"] if a.cfo else []) + (["--capture"] if a.capture or a.acquire else []) + (["--acquire"] if a.acquire else [])
        cmd += (["--front-sync"] if a.sync else []) + (["--front-solo-only"] if a.front_solo_only else [])
        cmd += ["--cfo_scope", a.cfo_scope] if a.cfo_scope != "frame" else []
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:               # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench.group_front", "failed": G, "rc": r.returncode, "groups": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    doc = {"bench": "rxbench.group_front",
           "variants": {"step": "the grouped receive step alone (frames resident)",
                        "a_*": "the front end issued per link (FrameSync / CaptureSync / CaptureAcquire + CaptureSync, out=chain.pl.x), "
                               "then ONE grouped step",
                        "b_*": "the grouped front end (one alignment or cut launch, three acquisition launches) + the same grouped step",
                        "*_front": "the front-end launches alone",
                        "sync": "frames cut in advance, alignment", "cut": "captures, starts known", "acquireJ": "captures, starts acquired from J frames",
                        "cut_pooled": "captures, starts known, one carrier offset per capture (--cfo --cfo_scope capture)"},
           "unit": "us per round of G links (median over repeats of the mean of `iters` back-to-back rounds); spread = (max - min) / median",
           "groups": res}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--one", default=None, help="frames,nbits: measure this shape in this process")
    ap.add_argument("--only", default=None, choices=["a", "b", "c", "d"])
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--chains", type=int, nargs="+", default=None, help="group sizes: G solo chain receive calls against one grouped call")
    ap.add_argument("--mods", type=int, nargs="+", default=[1, 2, 3, 4], help="--chains: bits per cell of the links, cycled")
    ap.add_argument("--frames", type=int, default=73, help="--chains: frames per link and call")
    ap.add_argument("--one-chains", default=None, help="nbits,nbits,...: measure this group in this process")
    ap.add_argument("--out", default=None, help="--chains / --sync: also write the result document to this file")
    ap.add_argument("--sync", type=int, default=0, help="W: time receive(x) against receive(x, sync=W) on every shape")
    ap.add_argument("--cfo", action="store_true", help="with --sync: also time receive(x, sync=W, cfo=True)")
    ap.add_argument("--cfo_scope", "--cfo-scope", default="frame", choices=["frame", "capture"],
                    help="with --capture --cfo: capture also times the offset pooled over the capture (cfo_scope='capture')")
    ap.add_argument("--capture", action="store_true",
                    help="time receive_capture against receive(x, sync=W[, cfo=True]) on the same frames cut in advance (W: --sync, default 3)")
    ap.add_argument("--acquire", action="store_true",
                    help="time receive_capture(first=None, acquire=J) against receive_capture(first=int), and the acquisition launches alone")
    ap.add_argument("--cfo_span", "--cfo-span", type=int, nargs="+", default=[],
                    help="with --acquire: also time the wide acquisition (dccn_capture_acquire_wide) at these spans M, and "
                         "receive_capture(..., cfo=True, cfo_span=M) against cfo_span=0")
    ap.add_argument("--sc16", action="store_true",
                    help="time receive_capture on an int16 capture against the float32 call and against convert-then-call")
    ap.add_argument("--front-sync", action="store_true", help="(internal, with --one-chains: time the alignment of frames cut in advance)")
    ap.add_argument("--front-solo-only", action="store_true",
                    help="--chains with a front end: only the per-link variants (for DCCN_LIB_PATH = the parent's build)")
    ap.add_argument("--acquire-frames", type=int, nargs="+", default=[4, 16], help="--chains --acquire: the J to time")
    a = ap.parse_args()
    if a.cfo_scope == "capture" and not (a.cfo and a.capture):
        ap.error("--cfo_scope capture needs --capture --cfo")
    if a.sc16:
        if a.one:
            fr, nb = (int(v) for v in a.one.split(","))
            print(json.dumps(run_sc16(fr, nb, a.sync or 3, a.iters, a.repeats)))
            return 0
        return main_sc16(a)
    if a.one_chains and (a.front_sync or a.capture or a.acquire):
        print(json.dumps(run_group_front([int(v) for v in a.one_chains.split(",")], a.frames, a.sync or 3, a.cfo, a.front_sync,
                                         a.capture or a.acquire, a.acquire_frames if a.acquire else None, a.iters, a.repeats,
                                         a.front_solo_only, a.cfo_scope == "capture")))
        return 0
    if a.chains and (a.sync or a.capture or a.acquire):
        return main_group_front(a)
    if a.acquire:
        if a.one:
            fr, nb = (int(v) for v in a.one.split(","))
            print(json.dumps(run_acquire(fr, nb, a.sync or 3, a.iters, a.repeats, a.cfo_span)))
            return 0
        return main_acquire(a)
    if a.capture:
        if a.one:
            fr, nb = (int(v) for v in a.one.split(","))
            print(json.dumps(run_capture(fr, nb, a.sync or 3, a.iters, a.repeats, a.cfo_scope == "capture")))
            return 0
        return main_capture(a)
    if a.one_chains:
        print(json.dumps(run_chains([int(v) for v in a.one_chains.split(",")], a.frames, a.iters, a.repeats)))
        return 0
    if a.chains:
        return main_chains(a)
    if a.cfo and not a.sync:
        ap.error("--cfo needs --sync W")
    if a.one:
        fr, nb = (int(v) for v in a.one.split(","))
        print(json.dumps(run_sync(fr, nb, a.sync, a.iters, a.repeats, a.cfo) if a.sync else run_one(fr, nb, a.iters, a.repeats, a.only)))
        return 0
    res = []
    for fr, nb in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", "%d,%d" % (fr, nb),
               "--iters", str(a.iters if fr < 10000 else max(a.iters // 5, 10)), "--repeats", str(a.repeats)]
        if a.only:
            cmd += ["--only", a.only]
        if a.sync:
            cmd += ["--sync", str(a.sync)] + (["--cfo"] if a.cfo else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:               # nothing more is started on the GPU after a failure
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"bench": "rxbench", "failed": [fr, nb], "rc": r.returncode, "shapes": res}))
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
    if a.sync:
        doc = {"bench": "rxbench.sync", "variants": {"copy": "receive(x): copy + step", "sync": "receive(x, sync=W): alignment launch + step",
                                                     "step": "receive(): the step alone", "sync_alone": "FrameSync.run(x)",
                                                     "copy_alone": "x.copy_ alone",
                                                     "cfo": "receive(x, sync=W, cfo=True): alignment + CFO launch + step (--cfo)",
                                                     "cfo_alone": "FrameSync(cfo=True).run(x) (--cfo)"},
               "unit": "us per call (median over repeats of the mean of `iters` back-to-back calls); spread = (max - min) / median",
               "shapes": res}
        print(json.dumps(doc))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return 0
    print(json.dumps({"bench": "rxbench", "variants": {"a": "eval_step(want_prob) + torch argmax/pack", "b": "eval_step(no prob)",
                                                       "c": "receive bits", "d": "receive bits+llr"}, "shapes": res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
