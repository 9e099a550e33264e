"""checksums of what the receive front end's entry points leave behind on seeded captures -- to compare two builds of the library bit
for bit (DCCN_LIB_PATH=<other build> python tools/synchash.py): every dccn_frame_sync*, dccn_capture_sync* and dccn_capture_acquire*
entry, solo and grouped, with the start on the host and on the device, float32 and sc16 captures, full and cropped rows, with and
without the metric -- at the workload's shape (S 7, K 64, CP 16, W 3, 73 frames) and at S 2, K 8, CP 4, W 2 with 5 frames from an
odd and from an even start (the half-pair loads and a ragged last block).  One line per call: its outputs' checksums."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_ofdm_amd import _lib      # noqa: E402

DEV = "cuda"
SCALE = 2.0 ** -12
lib = _lib.load()


def h(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def make_capture(S, K, CP, n_frames, seed):
    """n_frames back-to-back frames of random symbols with their cyclic prefixes, a carrier offset and noise, behind a seeded
    number of lead samples: (float32 [n, 2], int16 [n, 2], a sample at which a frame starts)"""
    rs = np.random.RandomState(seed)
    T = S * (K + CP)
    sym = rs.standard_normal((n_frames * S, K)) + 1j * rs.standard_normal((n_frames * S, K))
    iq = np.concatenate([sym[:, K - CP:], sym], axis=1).reshape(-1)
    iq = iq * np.exp(2j * np.pi * rs.uniform(-0.4, 0.4) * np.arange(iq.shape[0]) / K)
    iq = iq + 0.05 * (rs.standard_normal(iq.shape[0]) + 1j * rs.standard_normal(iq.shape[0]))
    cut = int(rs.randint(0, T))
    iq = iq[cut:]
    f32 = np.ascontiguousarray(np.stack([iq.real, iq.imag], axis=-1).astype(np.float32))
    i16 = np.clip(np.rint(f32 / SCALE), -32767, 32767).astype(np.int16)
    return torch.from_numpy(f32).to(DEV), torch.from_numpy(i16).to(DEV), T - cut


class Outs:
    def __init__(self, frames, S, out_kin, W, metric, pooled=False, x_out=True):
        self.out = torch.full((frames, S, out_kin, 2), 777.0, device=DEV) if x_out else None
        self.offset = torch.full((frames,), -99, dtype=torch.int32, device=DEV)
        self.cfo = torch.full((1 if pooled else frames,), 777.0, device=DEV)
        self.metric = torch.full((frames, 2 * W + 1), 777.0, device=DEV) if metric else None

    def sums(self, cfo=True):
        torch.cuda.synchronize()
        return " ".join("%s %s" % (n, h(t)) for n, t in (("out", self.out), ("offset", self.offset), ("cfo", self.cfo if cfo else None),
                                                         ("metric", self.metric)) if t is not None)


def show(tag, st, text):
    assert st == 0, (tag, st)
    print(tag, text)


def front_end(name, S, K, CP, W, frames, parity):
    T = S * (K + CP)
    shape = (S, K, CP, W)
    caps = [make_capture(S, K, CP, frames + 6, 100 * S + 7 * i + (parity or 0)) for i in range(3)]
    pool_ws = lib.dccn_capture_sync_pooled_workspace_size(frames)
    wide_ws = lib.dccn_capture_sync_pooled_wide_workspace_size(frames)
    wide_in = (torch.tensor([2], dtype=torch.int32, device=DEV), torch.tensor([0.13], dtype=torch.float32, device=DEV))

    def start_of(i):
        """link i's start: W + 4 or more, up to W off a true start; `parity` (where given) is link 0's"""
        first = W + 4 + (caps[i][2] - (W + 4)) % T + (i % (2 * W + 1)) - W + 2
        if parity is not None:
            first += (first & 1) ^ ((parity + i) & 1)
        return first

    starts = [start_of(i) for i in range(3)]
    on_dev = [torch.tensor([f], dtype=torch.int64, device=DEV) for f in starts]
    los = [f - 2 - i for i, f in enumerate(starts)]

    def start_args(i, where):
        """(first, first_dev, lo) of link i"""
        return (starts[i], None, 0) if where == "host" else (0, ptr(on_dev[i]), los[i])

    for out_kin, rows in ((K + CP, "full"), (K, "crop")):
        for metric in (0, 1):
            tag = "%s %s metric %d" % (name, rows, metric)

            def outs(**kw):
                return Outs(frames, S, out_kin, W, metric, **kw)

            # frames given on their own: cut at the links' starts
            xs = [c[0][f:f + frames * T].reshape(frames, S, K + CP, 2).clone() for c, f in zip(caps, starts)]
            o = outs()
            show(tag + " frame_sync", lib.dccn_frame_sync(ptr(xs[0]), frames, *shape, out_kin, ptr(o.out), ptr(o.offset), ptr(o.metric),
                                                          stream()), o.sums(cfo=False))
            o = outs()
            show(tag + " frame_sync_cfo", lib.dccn_frame_sync_cfo(ptr(xs[0]), frames, *shape, out_kin, ptr(o.out), ptr(o.offset),
                                                                  ptr(o.cfo), ptr(o.metric), stream()), o.sums())
            for cfo in (0, 1):
                os_ = [outs() for _ in xs]
                t = (_lib.FrameLink * 3)(*[_lib.FrameLink(ptr(x), ptr(q.out), ptr(q.offset), ptr(q.cfo) if cfo else None, ptr(q.metric))
                                           for x, q in zip(xs, os_)])
                st = lib.dccn_frame_sync_grouped(3, t, frames, *shape, out_kin, stream())
                for i, q in enumerate(os_):
                    show(tag + " frame_sync_grouped cfo %d link %d" % (cfo, i), st, q.sums(cfo=bool(cfo)))

            # the per-frame cut
            for where in ("host", "device"):
                first, fd, lo = start_args(0, where)
                for cfo in (0, 1):
                    o = outs()
                    if where == "host":
                        st = lib.dccn_capture_sync(ptr(caps[0][0]), caps[0][0].shape[0], first, T, frames, *shape, out_kin, ptr(o.out),
                                                   ptr(o.offset), ptr(o.cfo) if cfo else None, ptr(o.metric), stream())
                    else:
                        st = lib.dccn_capture_sync_at(ptr(caps[0][0]), caps[0][0].shape[0], fd, lo, T, frames, *shape, out_kin, ptr(o.out),
                                                      ptr(o.offset), ptr(o.cfo) if cfo else None, ptr(o.metric), stream())
                    show(tag + " capture_sync%s float32 cfo %d" % ("" if where == "host" else "_at", cfo), st, o.sums(cfo=bool(cfo)))
                    o = outs()
                    st = lib.dccn_capture_sync_sc16(ptr(caps[0][1]), caps[0][1].shape[0], SCALE, first, fd, lo, T, frames, *shape, out_kin,
                                                    ptr(o.out), ptr(o.offset), ptr(o.cfo) if cfo else None, ptr(o.metric), stream())
                    show(tag + " capture_sync_sc16 start %s cfo %d" % (where, cfo), st, o.sums(cfo=bool(cfo)))
                # one offset per capture
                o = outs(pooled=True)
                ws = torch.zeros(pool_ws, dtype=torch.uint8, device=DEV)
                st = lib.dccn_capture_sync_pooled(ptr(caps[0][0]), caps[0][0].shape[0], first, fd, lo, T, frames, *shape, out_kin, ptr(o.out),
                                                  ptr(o.offset), ptr(o.cfo), ptr(o.metric), ptr(ws), pool_ws, stream())
                show(tag + " capture_sync_pooled float32 start %s" % where, st, o.sums() + " gamma " + h(ws))
                o = outs(pooled=True)
                ws = torch.zeros(pool_ws, dtype=torch.uint8, device=DEV)
                st = lib.dccn_capture_sync_pooled_sc16(ptr(caps[0][1]), caps[0][1].shape[0], SCALE, first, fd, lo, T, frames, *shape, out_kin,
                                                       ptr(o.out), ptr(o.offset), ptr(o.cfo), ptr(o.metric), ptr(ws), pool_ws, stream())
                show(tag + " capture_sync_pooled_sc16 start %s" % where, st, o.sums() + " gamma " + h(ws))
                # the whole offset taken out
                o = outs(pooled=True)
                ws = torch.zeros(wide_ws, dtype=torch.uint8, device=DEV)
                st = lib.dccn_capture_sync_pooled_wide(ptr(caps[0][0]), caps[0][0].shape[0], first, fd, lo, T, frames, *shape, out_kin,
                                                       ptr(o.out), ptr(o.offset), ptr(o.cfo), ptr(o.metric), ptr(wide_in[0]), ptr(wide_in[1]),
                                                       ptr(ws), wide_ws, stream())
                show(tag + " capture_sync_pooled_wide start %s" % where, st, o.sums() + " workspace " + h(ws))
            o = outs()
            _, fd, lo = start_args(0, "device")
            st = lib.dccn_capture_sync_wide(ptr(caps[0][0]), caps[0][0].shape[0], fd, lo, T, frames, *shape, out_kin, ptr(o.out),
                                            ptr(o.offset), ptr(o.cfo), ptr(o.metric), ptr(wide_in[0]), ptr(wide_in[1]), stream())
            show(tag + " capture_sync_wide", st, o.sums())

            # several links per launch: link 1 starts on the device, link 2 has a stride of its own
            where = ("host", "device", "host")
            strides = (T, T, T + 1)
            for cfo in (0, 1):
                os_ = [outs() for _ in caps]
                t = (_lib.CaptureLink * 3)(*[_lib.CaptureLink(ptr(c[0]), c[0].shape[0], *start_args(i, where[i]), strides[i], ptr(q.out),
                                                              ptr(q.offset), ptr(q.cfo) if cfo else None, ptr(q.metric))
                                             for i, (c, q) in enumerate(zip(caps, os_))])
                st = lib.dccn_capture_sync_grouped(3, t, frames, *shape, out_kin, stream())
                for i, q in enumerate(os_):
                    show(tag + " capture_sync_grouped cfo %d link %d" % (cfo, i), st, q.sums(cfo=bool(cfo)))
            os_ = [outs(pooled=True) for _ in caps]
            wss = [torch.zeros(pool_ws, dtype=torch.uint8, device=DEV) for _ in caps]
            t = (_lib.PooledLink * 3)(*[_lib.PooledLink(ptr(c[0]), c[0].shape[0], *start_args(i, where[i]), strides[i], ptr(q.out),
                                                        ptr(q.offset), ptr(q.cfo), ptr(q.metric), ptr(w), pool_ws)
                                        for i, (c, q, w) in enumerate(zip(caps, os_, wss))])
            st = lib.dccn_capture_sync_pooled_grouped(3, t, frames, *shape, out_kin, stream())
            for i, (q, w) in enumerate(zip(os_, wss)):
                show(tag + " capture_sync_pooled_grouped link %d" % i, st, q.sums() + " gamma " + h(w))

    # acquisition: J = 2, every fourth carrier of every symbol a pilot; with and without the two metrics
    J, M = 2, 2
    sc = torch.from_numpy(np.array([s * K + k for s in range(S) for k in range(0, K, 4)], dtype=np.int32)).to(DEV)
    n_pilot = int(sc.shape[0])

    class Acq:
        def __init__(self, metric, wide=False):
            self.first = torch.full((1,), -99, dtype=torch.int64, device=DEV)
            self.cfo = torch.full((1,), 777.0, device=DEV)
            self.cfo_int = torch.full((1,), -99, dtype=torch.int32, device=DEV)
            self.sym = torch.full((K + CP,), 777.0, device=DEV) if metric else None
            self.phase = torch.full((S, 2 * M + 1) if wide else (S,), 777.0, device=DEV) if metric else None
            size = lib.dccn_capture_acquire_wide_workspace_size(S, K, CP, n_pilot, J, M) if wide else \
                lib.dccn_capture_acquire_workspace_size(S, K, CP, n_pilot, J)
            self.ws = torch.zeros(size, dtype=torch.uint8, device=DEV)

        def sums(self, wide=False):
            torch.cuda.synchronize()
            return " ".join("%s %s" % (n, h(t)) for n, t in (("first", self.first), ("cfo", self.cfo), ("cfo_int", self.cfo_int if wide else None),
                                                             ("sym", self.sym), ("phase", self.phase)) if t is not None)

    for metric in (0, 1):
        tag = "%s metric %d" % (name, metric)
        f32, i16, _ = caps[0]
        a = Acq(metric)
        st = lib.dccn_capture_acquire(ptr(f32), f32.shape[0], los[0], J, S, K, CP, ptr(sc), n_pilot, ptr(a.first), ptr(a.cfo), ptr(a.sym),
                                      ptr(a.phase), ptr(a.ws), a.ws.shape[0], stream())
        show(tag + " capture_acquire float32", st, a.sums())
        a = Acq(metric)
        st = lib.dccn_capture_acquire_sc16(ptr(i16), i16.shape[0], SCALE, los[0], J, S, K, CP, ptr(sc), n_pilot, ptr(a.first), ptr(a.cfo),
                                           ptr(a.sym), ptr(a.phase), ptr(a.ws), a.ws.shape[0], stream())
        show(tag + " capture_acquire_sc16", st, a.sums())
        a = Acq(metric, wide=True)
        st = lib.dccn_capture_acquire_wide(ptr(f32), f32.shape[0], los[0], J, S, K, CP, ptr(sc), n_pilot, M, ptr(a.first), ptr(a.cfo),
                                           ptr(a.cfo_int), ptr(a.sym), ptr(a.phase), ptr(a.ws), a.ws.shape[0], stream())
        show(tag + " capture_acquire_wide", st, a.sums(wide=True))
        acqs = [Acq(metric) for _ in caps]
        t = (_lib.AcquireLink * 3)(*[_lib.AcquireLink(ptr(c[0]), c[0].shape[0], los[i], ptr(sc), ptr(q.first), ptr(q.cfo), ptr(q.sym),
                                                      ptr(q.phase), ptr(q.ws), q.ws.shape[0])
                                     for i, (c, q) in enumerate(zip(caps, acqs))])
        st = lib.dccn_capture_acquire_grouped(3, t, J, S, K, CP, n_pilot, stream())
        for i, q in enumerate(acqs):
            show(tag + " capture_acquire_grouped link %d" % i, st, q.sums())


front_end("S7 K64 CP16 W3 x73", 7, 64, 16, 3, 73, None)
front_end("S2 K8 CP4 W2 x5 odd", 2, 8, 4, 2, 5, 1)
front_end("S2 K8 CP4 W2 x5 even", 2, 8, 4, 2, 5, 0)
