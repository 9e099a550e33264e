"""The label-free receive path: raw IQ frames -> packed bits (and LLRs for a channel decoder behind it).

What ``sess.run(outputs, {x: frames})`` is in the reference (dev/py/test_v1/test_ofdm_cdnn_awgn.py:113-118; ``output:0``
depends on ``tx_ofdm:0`` alone) plus the argmax of dev/py/ofdmreceiver_np.py:166, as one launch sequence of the library
(``dccn_rx_receive_step``: R0 -> C-Conv forward -> dense forward with the decision stage in its epilogue): no label tensor,
no cross entropy, no confusion counts, no metrics record.

Row layout of ``packed`` ``uint8 [frames, ceil(D * nbits / 8)]``: row ``f`` is ``numpy.packbits(hard[f].reshape(-1))`` with
``hard [frames, D, nbits]`` laid out like ``bits_in`` (data cell, then bit, most significant bit of the symbol first); the
most significant bit of a byte comes first and the padding bits of a row's last byte are 0.

The hard decision is the evaluation step's, bit for bit (argmax over the pair of ``output:0``, first index on ties).  One
consequence: where ``llr = u1 - u0`` is positive but so small that ``exp(-llr)`` rounds to 1, ``p1 == p0`` and the bit is 0
although ``llr > 0``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import RxReceiveBuffers, RxShape, check, ptr, stream_ptr
from .engine import PARAM_NAMES, RxDims, glorot_init, param_layout
from .sync import (CaptureAcquire, CaptureAcquireGroup, CaptureSync, CaptureSyncGroup, FrameSync, FrameSyncGroup, _per_link,
                   capture_format, check_cfo_scope, resident_stage)


def row_bytes(D: int, nbits: int) -> int:
    return (int(D) * int(nbits) + 7) // 8


def pack_bits(hard) -> np.ndarray:
    """``hard [frames, D, nbits]`` (0 / 1) -> ``uint8 [frames, ceil(D * nbits / 8)]`` in the row layout above (NumPy, host)."""
    h = np.asarray(hard)
    if h.ndim != 3:
        raise ValueError("hard must be [frames, D, nbits]")
    frames = h.shape[0]
    flat = (h.reshape(frames, -1) != 0).astype(np.uint8)
    nb = row_bytes(h.shape[1], h.shape[2])
    out = np.zeros((frames, nb), np.uint8)
    pad = nb * 8 - flat.shape[1]
    if pad:
        flat = np.concatenate([flat, np.zeros((frames, pad), np.uint8)], axis=1)
    w = (1 << np.arange(7, -1, -1)).astype(np.uint16)
    out[:] = (flat.reshape(frames, nb, 8).astype(np.uint16) * w).sum(axis=2).astype(np.uint8)
    return out


def unpack_bits(packed, D: int, nbits: int) -> np.ndarray:
    """Inverse of :func:`pack_bits`: ``uint8 [frames, ceil(D * nbits / 8)]`` -> ``uint8 [frames, D, nbits]`` (NumPy, host)."""
    p = np.ascontiguousarray(np.asarray(packed, dtype=np.uint8))
    nb = row_bytes(D, nbits)
    if p.ndim != 2 or p.shape[1] != nb:
        raise ValueError("packed must be [frames, %d] for D=%d, nbits=%d" % (nb, D, nbits))
    sh = np.arange(7, -1, -1).astype(np.uint8)
    bits = (p[:, :, None] >> sh) & 1
    return np.ascontiguousarray(bits.reshape(p.shape[0], nb * 8)[:, :D * nbits].reshape(p.shape[0], D, nbits))


class ReceiveResult:
    """Device tensors of one receive call (they are the receiver's resident buffers: the next call overwrites them)."""

    def __init__(self, packed: torch.Tensor, llr: Optional[torch.Tensor], prob: Optional[torch.Tensor], D: int, nbits: int,
                 offset: Optional[torch.Tensor] = None, cfo: Optional[torch.Tensor] = None,
                 first: Optional[torch.Tensor] = None, acquired_cfo: Optional[torch.Tensor] = None,
                 acquired_cfo_int: Optional[torch.Tensor] = None):
        self.packed, self.llr, self.prob, self.D, self.nbits = packed, llr, prob, int(D), int(nbits)
        self.offset = offset        # int32 [frames]: the timing offsets of a call with sync > 0 (None otherwise)
        self.cfo = cfo              # float32 [frames]: the carrier-frequency offsets of a call with cfo=True (None otherwise);
                                    # float32 [1] from receive_capture(cfo_scope="capture"): the capture's one offset
        self.first = first          # int64 [1]: frame 0's start as receive_capture(first=None) acquired it (None otherwise)
        self.acquired_cfo = acquired_cfo    # float32 [1]: the carrier-frequency offset acquisition estimated on the way
        # int32 [1]: the whole subcarrier spacings acquisition found (receive_capture(cfo_span=M > 0); None otherwise).  The
        # acquired offset is acquired_cfo_int + acquired_cfo, and `cfo` then holds totals.
        self.acquired_cfo_int = acquired_cfo_int

    def bits(self) -> torch.Tensor:
        """``uint8 [frames, D, nbits]``, unpacked on the device."""
        p = self.packed.to(torch.int32)
        sh = torch.arange(7, -1, -1, dtype=torch.int32, device=p.device)
        b = (p.unsqueeze(-1) >> sh) & 1
        n = self.D * self.nbits
        return b.reshape(p.shape[0], -1)[:, :n].reshape(p.shape[0], self.D, self.nbits).to(torch.uint8)


# ---- what every receive call refuses before anything is sized or launched (`what`: the call the user made) ---------------------------
def _checked_alignment(what: str, sync, cfo) -> None:
    if cfo and not sync:
        raise _lib.DccnError("%s(cfo=True) needs sync = W > 0: the offset is read off the timing correlation" % what)


def _checked_capture_call(what: str, cap, first, sync, cfo, acquire, cfo_scope, cfo_span, scale):
    """``(W, M)`` of a solo ``receive_capture``.  Acquisition runs ahead of the cut, which would otherwise be the first to look:
    so the cut's refusals of the scope, of an int16 capture or a ``scale`` (:func:`~dl_ofdm_amd.sync.capture_format`) and of the
    window are made here.  ``cfo_span = M > 0`` needs acquisition and the carrier offset taken out: the integer is only known
    through acquisition."""
    check_cfo_scope(cfo, cfo_scope)
    M = int(cfo_span)
    if scale is not None or (isinstance(cap, torch.Tensor) and cap.dtype == torch.int16):
        capture_format(cap, scale, what, M)
    if M < 0:
        raise _lib.DccnError("%s: cfo_span must not be negative" % what)
    if M and (first is not None or not acquire or not cfo):
        raise _lib.DccnError("%s(cfo_span=M > 0) needs first=None, acquire=J and cfo=True: the whole subcarrier spacings of the "
                             "offset are only known through acquisition" % what)
    return _checked_window(what, sync), M


def _checked_window(what: str, sync) -> int:
    if int(sync) <= 0:
        raise _lib.DccnError("%s needs sync = W > 0" % what)
    return int(sync)


def _acquisition_frames(what: str, first, acquire, s: str = "") -> int:
    """``J > 0``: acquisition over ``J`` frames finds the start; 0: the caller gave it"""
    if first is not None:
        if acquire:
            raise _lib.DccnError("%s: give `first%s` or `acquire`, not both" % (what, s))
        return 0
    if int(acquire) <= 0:
        raise _lib.DccnError("%s(first%s=None) needs acquire = J > 0, the number of frames acquisition may use" % (what, s))
    return int(acquire)


def _pilot_cells(pilot_sc) -> tuple:
    """pilot cells as a stage's cache key takes them"""
    return tuple(int(v) for v in np.asarray(pilot_sc).reshape(-1))


class _FrontEnd:
    """The stages in front of a solo detector, each writing the detector's resident ``x`` (``[batch, S, kin, 2]``): the copy, the
    alignment launch (``sync=W``), and the capture cut with acquisition.  Every solo engine owns one -- :class:`RxReceiver`,
    :class:`~dl_ofdm_amd.classical_receive.ClassicalRxReceiver`, and each resident plan of an ``EqualizerTrainer`` (whose plans
    share their acquisition stages: ``acquires``).  ``kin``: samples per symbol the detector takes (``K + CP``: whole symbols;
    ``K``: a ``cp=False`` receiver).  ``prefix``: what stands in front of ``receive`` / ``receive_capture`` in a refusal."""

    def __init__(self, owner: str, device, x: torch.Tensor, CP=None, K=None, pilot_sc=None, acquires=None, prefix: str = ""):
        self.owner, self.device, self.x, self.CP, self.K, self.prefix = owner, device, x, CP, K, prefix
        self.batch, self.S, self.kin = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        self.pilots = None if pilot_sc is None else _pilot_cells(pilot_sc)
        self.stages = {}                                       # resident: sync.resident_stage
        self.acquires = self.stages if acquires is None else acquires

    def frames(self, x, sync: int, cfo: bool):
        """``receive``'s front end: ``x`` into ``self.x`` by the copy or the alignment launch -> ``(offset, cfo estimates)``"""
        what, kin = self.prefix + "receive", self.kin
        _checked_alignment(what, sync, cfo)
        if not sync:
            if x is not None:
                self.x.copy_(torch.as_tensor(x, dtype=torch.float32).reshape(self.x.shape), non_blocking=True)
            return None, None
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise _lib.DccnError("%s(sync=W) takes a device tensor [batch, S, K + CP, 2]" % what)
        n_sc = int(x.shape[2])
        if self.CP is not None:
            CP = self.CP
        elif n_sc > kin:
            CP = n_sc - kin
        else:
            raise _lib.DccnError("%s(sync=W) of a receiver that takes whole symbols needs %s(..., CP=...)" % (what, self.owner))
        K = n_sc - CP
        if kin not in (n_sc, K):
            raise _lib.DccnError("%s(sync=W): frames of %d samples per symbol (CP = %d) do not fit kin = %d" % (what, n_sc, CP, kin))
        fs = resident_stage(self.stages, FrameSync, self.S, K, CP, int(sync), self.batch, self.device, kin, False, bool(cfo))
        _, offset = fs.run(x, out=self.x)
        return offset, fs.cfo

    def capture(self, cap, first, stride, sync, cfo, acquire, lo, cfo_scope, cfo_span, scale):
        """``receive_capture``'s front end: the refusals, then :meth:`cut`"""
        what = self.prefix + "receive_capture"
        W, M = _checked_capture_call(what, cap, first, sync, cfo, acquire, cfo_scope, cfo_span, scale)
        return self.cut(what, cap, first, stride, W, cfo, acquire, lo, cfo_scope, M, scale)

    def cut(self, what, cap, first, stride, W, cfo, acquire, lo, cfo_scope, M, scale):
        """acquisition (``first=None``) and the cut, writing ``self.x`` -> ``(offset, cfo estimates, first, acquired_cfo,
        acquired_cfo_int)`` as :class:`ReceiveResult` takes them"""
        if self.CP is None:
            raise _lib.DccnError("%s needs %s(..., CP=...)" % (what, self.owner))
        kin = self.kin
        K = kin - self.CP if self.K is None else self.K
        if K < 1 or kin not in (K + self.CP, K):
            raise _lib.DccnError("%s: K = %d, CP = %d do not fit kin = %d" % (what, K, self.CP, kin))
        cs = resident_stage(self.stages, CaptureSync, self.S, K, self.CP, W, self.batch, self.device, kin, False, bool(cfo),
                            cfo_scope, M)
        est0 = est_int = None
        J = _acquisition_frames(what, first, acquire)
        if J:
            if self.pilots is None:
                raise _lib.DccnError("%s(first=None) needs the frame's pilot cells (%s(..., pilot_sc=...))" % (what, self.owner))
            acq = resident_stage(self.acquires, CaptureAcquire, self.S, K, self.CP, self.pilots, J, self.device, M)
            first, est0, est_int = acq.run(cap, lo, scale=scale), acq.cfo, (acq.cfo_int if M else None)
        _, offset = cs.run(cap, first, stride, out=self.x, lo=lo,             # (lo matters to a device `first` only)
                           acquired=(est_int, est0) if M else None, scale=scale)
        return offset, cs.cfo, (first if isinstance(first, torch.Tensor) else None), est0, est_int


def _refuse_group_span(engine, cfo_span) -> None:
    """what a group's ``receive_capture`` begins with (it needs nothing of the engine but its class)"""
    if int(cfo_span) != 0:
        raise _lib.DccnError("%s.receive_capture: cfo_span > 0 is not offered for groups (the grouped entries have no wide "
                             "variant); use %s(..., cfo_span=M) per link" % (type(engine).__name__, engine._solo_call))


class _GroupFrontEnd:
    """The stages in front of a grouped detector (:class:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup`,
    :class:`~dl_ofdm_amd.classical_receive.ClassicalReceiveGroup`), each ONE launch sequence for all links (sync.py: the
    ``*Group`` classes), writing every link's resident ``x`` (``xs[i]``: ``[batch, S, K + CP, 2]``).  The engine that owns it
    provides ``device`` and ``_solo_call`` (a class attribute: the call that serves one link, for the refusals).  What the ``*Group``
    stage behind a call checks anyway is left to it."""

    def __init__(self, engine, K: int, CP: int, xs: list, pilots: list):
        self.owner, self.solo, self.device, self.xs = type(engine).__name__, engine._solo_call, engine.device, xs
        self.shape = (int(xs[0].shape[1]), int(K), int(CP))    # (S, K, CP) of every link
        self.batch = int(xs[0].shape[0])
        self.pilots = tuple(_pilot_cells(sc) for sc in pilots)
        self.stages = {}                                       # resident: sync.resident_stage

    def _stage(self, cls, W: int, cfo: bool, *scope):
        """FrameSyncGroup / CaptureSyncGroup writing the links' ``x`` (``scope``: the latter's ``cfo_scope``); no ``out_kin``, no
        metric"""
        return resident_stage(self.stages, cls, *self.shape, int(W), self.batch, len(self.xs), self.device, None, False,
                              bool(cfo), *scope)

    def frames(self, xs, sync: int, cfo: bool):
        """``receive``'s front end for every link: the per-link copies, or (``sync = W > 0``) one alignment launch ->
        ``(offsets, cfo estimates)``, one entry per link (``None`` where the call has none)"""
        _checked_alignment("receive", sync, cfo)
        offsets = ests = [None] * len(self.xs)
        if sync:
            fs = self._stage(FrameSyncGroup, sync, cfo)
            _, offsets = fs.run(xs, outs=self.xs)
            ests = fs.cfo if cfo else ests
        else:
            for dst, x in zip(self.xs, xs):
                if x is not None:
                    dst.copy_(torch.as_tensor(x, dtype=torch.float32).reshape(dst.shape), non_blocking=True)
        return offsets, ests

    def capture(self, caps, firsts, strides, sync, cfo, acquire, los, cfo_scope):
        """``receive_capture``'s front end for every link: acquisition (``firsts=None``: three launches) and the cut (one launch,
        three when pooled) -> ``(offsets, cfo estimates, firsts, acquired cfo)``, one entry per link as
        :class:`ReceiveResult` takes them"""
        what, n = self.owner + ".receive_capture", len(self.xs)
        check_cfo_scope(cfo, cfo_scope)
        W = _checked_window("receive_capture", sync)
        if any(isinstance(c, torch.Tensor) and c.dtype == torch.int16 for c in caps):
            raise _lib.DccnError("%s: int16 captures are not offered for groups (the grouped entries read float32 captures only); "
                                 "use %s per link, or radio.sc16_to_float" % (what, self.solo))
        strides = _per_link(strides, n, "receive_capture(strides)")     # (ahead of acquisition, which takes none)
        J = _acquisition_frames("receive_capture", firsts, acquire, "s")
        if not J and (not isinstance(firsts, (list, tuple)) or len(firsts) != n):
            raise ValueError("receive_capture(firsts): one entry per link (%d)" % n)
        cs = self._stage(CaptureSyncGroup, W, cfo, cfo_scope)
        acq_cfo = [None] * n
        if J:
            acq = resident_stage(self.stages, CaptureAcquireGroup, *self.shape, self.pilots, J, n, self.device)
            firsts, acq_cfo = acq.run(caps, los), acq.cfo
        _, offsets = cs.run(caps, firsts, strides, outs=self.xs, los=los)
        return (offsets, [cs.cfo[i] if cfo else None for i in range(n)],
                [f if isinstance(f, torch.Tensor) else None for f in firsts], acq_cfo)


class RxReceiver:
    """Fixed-shape receive engine of the basic receiver on one GPU: ``receive(x)`` -> :class:`ReceiveResult`.

    ``x``: host array or device tensor ``[batch, S, kin, 2]`` (as ``RxEngine.set_batch`` takes it).  ``x_norm`` (``input:0``)
    and ``fft_out`` hold what the evaluation step writes for the same frames.
    """

    def __init__(self, dims: RxDims, batch: int, params: Optional[Dict[str, np.ndarray]] = None, device="cuda",
                 want_llr: bool = False, want_prob: bool = False, seed: int = 1, CP: Optional[int] = None,
                 K: Optional[int] = None, pilot_sc=None):
        """``CP``: the frames' cyclic-prefix length, for ``receive(x, sync=W)`` of a receiver that takes whole symbols
        (``dims.kin == K + CP``: K cannot be read off the shape).  A ``cp=False`` receiver (``dims.kin == K``) finds it from
        the frames it is given.  ``receive_capture`` has no frame shape to look at: it needs ``CP``, and takes ``K`` as
        ``dims.kin - CP`` (whole symbols) unless ``K`` says otherwise (``K=dims.kin``: a ``cp=False`` receiver).
        ``pilot_sc``: the frame's pilot cells (``ofdm_tx.pilotSc``), for ``receive_capture(first=None, acquire=J)``."""
        self.lib = _lib.load()
        self.CP = None if CP is None else int(CP)
        self.K = None if K is None else int(K)
        self.pilot_sc = None if pilot_sc is None else np.asarray(pilot_sc, dtype=np.int32).reshape(-1)
        self.dims, self.batch = dims, int(batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DccnError("RxReceiver needs a CUDA (ROCm) device; there is no CPU fallback")
        self.shape = RxShape(self.batch, dims.S, dims.kin, dims.F, dims.D, dims.nbits)
        self.layout, total = param_layout(dims)
        f32 = dict(dtype=torch.float32, device=self.device)
        B, d = self.batch, dims
        self.params = torch.zeros(total, **f32)
        self.x = torch.zeros(B, d.S, d.kin, 2, **f32)
        self.x_norm = torch.empty(B, d.S, d.kin, 2, **f32)
        self.fft_out = torch.empty(B, d.S, d.F, 2, **f32)
        # the dense output exists in memory only where the decision does not run inside the dense launch
        self.fused = bool(self.lib.dccn_rx_receive_fused(C.byref(self.shape)))
        self.z = None if self.fused else torch.empty(B, 2 * d.D, **f32)
        self.packed = torch.zeros(B, row_bytes(d.D, d.nbits), dtype=torch.uint8, device=self.device)
        self.llr = torch.empty(B, d.D, d.nbits, **f32) if want_llr else None
        self.prob = torch.empty(B, d.D, d.nbits, 2, **f32) if want_prob else None
        nws = self.lib.dccn_rx_receive_workspace_size(C.byref(self.shape))
        if nws == 0:
            raise _lib.DccnError("dccn_rx_receive_workspace_size refused the shape %r" % (dims,))
        self.ws = torch.empty(nws, dtype=torch.uint8, device=self.device)
        self.buffers = RxReceiveBuffers(*map(ptr, (self.x, self.params, self.x_norm, self.fft_out, self.z, self.packed, self.llr,
                                                   self.prob, self.ws)), nws, None)
        self._front = _FrontEnd(type(self).__name__, self.device, self.x, self.CP, self.K, self.pilot_sc)
        self.load_params(params if params is not None else glorot_init(dims, seed))

    def view(self, name: str) -> torch.Tensor:
        o, shp = self.layout[name]
        return self.params[o:o + int(np.prod(shp))].view(*shp)

    def load_params(self, params: Dict[str, np.ndarray]):
        for n in PARAM_NAMES:
            self.view(n).copy_(torch.as_tensor(np.asarray(params[n], dtype=np.float32)).reshape(self.layout[n][1]))

    def close_graph(self):
        """(nothing captured: lets a :class:`~dl_ofdm_amd.session.Session` keep receivers next to its engines)"""

    def _stream(self):
        return stream_ptr(self.device)

    def _detect(self, offset=None, est=None, first=None, est0=None, est_int=None) -> ReceiveResult:
        check(self.lib.dccn_rx_receive_step(C.byref(self.shape), C.byref(self.buffers), self._stream()), "dccn_rx_receive_step")
        return ReceiveResult(self.packed, self.llr, self.prob, self.dims.D, self.dims.nbits, offset, est, first, est0, est_int)

    def receive(self, x=None, sync: int = 0, cfo: bool = False) -> ReceiveResult:
        """Stage ``x`` (``None``: whatever ``self.x`` holds) and run one receive step on the current stream.

        ``sync = W > 0``: ``x`` is a device tensor of FULL frames ``[batch, S, K + CP, 2]`` that may sit up to ``W`` samples off
        the FFT window.  The alignment launch (:class:`~dl_ofdm_amd.sync.FrameSync`) takes the place of the copy: it writes
        each frame, rotated by its own estimated offset, straight into ``self.x`` (only the K samples behind each prefix when
        ``dims.kin == K``); the receive step behind it is unchanged.  ``result.offset`` holds the offsets.

        ``cfo=True`` (needs ``sync > 0``): the same launch also estimates each frame's carrier-frequency offset from its prefix
        and writes the frames with it taken out (``FrameSync(..., cfo=True)``); ``result.cfo`` holds the estimates, in
        subcarrier spacings."""
        return self._detect(*self._front.frames(x, sync, cfo))

    def receive_capture(self, cap, first=None, stride: Optional[int] = None, sync: int = 3, cfo: bool = False, acquire: int = 0,
                        lo: int = 0, cfo_scope: str = "frame", cfo_span: int = 0, scale: Optional[float] = None) -> ReceiveResult:
        """One receive step on ``batch`` frames that still sit inside one contiguous capture ``cap`` (device tensor ``float32
        [n, 2]``, or ``int16 [n, 2]`` as a front end delivers it -- see ``scale`` below): frame ``f`` nominally starts at sample ``first + f * stride`` (``None``: frames back to back) and may sit up to
        ``sync = W > 0`` samples off.  One launch (:class:`~dl_ofdm_amd.sync.CaptureSync`) stands where ``receive(x, sync=W)``
        has its alignment launch: it cuts each frame at its own estimated start -- linearly, the samples it brings in are the
        capture's, not the frame's other end -- and writes it straight into ``self.x`` (only the K samples behind each prefix
        when ``dims.kin == K``).  ``cfo=True`` takes each frame's carrier-frequency offset out on the way.  Needs
        ``RxReceiver(..., CP=...)``, and ``K=dims.kin`` as well for a ``cp=False`` receiver: a capture has no shape to read them
        off.  ``result.offset`` / ``result.cfo``.  ``cfo=True, cfo_scope="capture"``: ONE offset for the whole capture, pooled
        over its frames (``CaptureSync(..., cfo_scope="capture")``: three launches in place of the one), ``result.cfo`` a
        one-element tensor; with any ``first``, acquisition included.

        ``first=None, acquire=J, lo=...``: nobody knows where frame 0 starts.  Acquisition (:class:`~dl_ofdm_amd.sync.
        CaptureAcquire`, ``J`` frames, needs ``RxReceiver(..., pilot_sc=...)``) finds the frame start inside ``[lo, lo + T)`` and
        leaves it on the device, the cut reads it there (``dccn_capture_sync_at``), and the receive step follows: one launch
        sequence, no host round trip.  ``lo >= sync``, and the capture must hold the ``batch`` frames from ``lo + T - 1`` on.
        ``first`` may also be such a device ``int64`` tensor of one element itself (with ``lo``).  ``result.first`` /
        ``result.acquired_cfo``.

        ``cfo_span = M > 0`` (needs ``first=None, acquire=J, cfo=True``): nobody knows the oscillator either -- the carrier
        offset may be up to ``M + 1/2`` subcarrier spacings.  Acquisition decides the frame start and the whole spacings
        together (``CaptureAcquire(..., cfo_span=M)``), the cut unwraps the prefix's fraction against that and takes the whole
        offset out (``CaptureSync(..., cfo_span=M)``, either ``cfo_scope``): the same number of launches, no host round trip.
        ``result.cfo`` holds totals, ``result.acquired_cfo_int`` the acquired integer.

        ``cap`` of dtype ``int16`` (interleaved 16-bit I/Q): sample ``n`` is ``(float(I) * scale, float(Q) * scale)``
        (``scale=None``: ``2**-15``), converted inside the acquisition and cut launches -- no conversion launch, no float copy --
        and every result is bit for bit that of the float32 capture ``radio.sc16_to_float(cap, scale)``.  Every combination
        above at ``cfo_span=0``; ``cfo_span > 0`` with an int16 capture, and ``scale`` with a float32 one, raise."""
        return self._detect(*self._front.capture(cap, first, stride, sync, cfo, acquire, lo, cfo_scope, cfo_span, scale))


def _chain_front(tr, pl) -> _FrontEnd:
    """the front end of a trainer's resident plan, writing the plan's ``x``; the trainer's plans share their acquisition stages"""
    if pl.front is None:
        o = tr.ofdmobj
        pl.front = _FrontEnd("EqualizerTrainer", tr.device, pl.x, int(o.CP), int(o.K), o.pilotSc, acquires=tr.acquire_stages,
                             prefix="chain_")
    return pl.front


def _chain_result(tr, pl, want_llr, want_prob, *front) -> ReceiveResult:
    packed, llr, prob = pl.receive(want_llr, want_prob)
    return ReceiveResult(packed, llr, prob, int(tr.ofdmobj.frame_size), int(tr.FLAGS.nbits), *front)


def chain_receive(tr, x, want_llr: bool = False, want_prob: bool = False, sync: int = 0, cfo: bool = False) -> ReceiveResult:
    """Equaliser + frozen receiver chain (``EqualizerTrainer.receive``): ``dccn_eq_receive_step`` on the trainer's resident
    plan of this batch size.  ``out_eq`` / ``chest`` of the plan hold what ``eval_step`` writes for the same frames.

    ``sync = W > 0``: as :meth:`RxReceiver.receive` -- ``x`` is a device tensor ``[batch, S, K + CP, 2]``, and the alignment
    launch writes the rotated frames into the plan's ``x`` in place of the copy; ``result.offset`` holds the offsets.
    ``cfo=True`` (needs ``sync > 0``): that launch also takes each frame's carrier-frequency offset out; ``result.cfo``."""
    if not tr.fused_ok:
        raise _lib.DccnError("the chain's receive path needs the fused equaliser step")
    _checked_alignment("chain_receive", sync, cfo)             # (ahead of the plan, which this call may be the first to build)
    pl = tr.resident(int(x.shape[0]) if isinstance(x, torch.Tensor) else int(np.shape(x)[0]))
    return _chain_result(tr, pl, want_llr, want_prob, *_chain_front(tr, pl).frames(x, sync, cfo))


def chain_receive_capture(tr, cap, first=None, stride: Optional[int] = None, sync: int = 3, cfo: bool = False,
                          want_llr: bool = False, want_prob: bool = False, frames: Optional[int] = None, acquire: int = 0,
                          lo: int = 0, cfo_scope: str = "frame", cfo_span: int = 0, scale: Optional[float] = None) -> ReceiveResult:
    """:func:`chain_receive` on frames that still sit inside one contiguous capture ``cap`` (device tensor ``float32 [n, 2]``, or
    ``int16 [n, 2]`` with ``scale`` as :meth:`RxReceiver.receive_capture` takes it;
    ``EqualizerTrainer.receive_capture``): as :meth:`RxReceiver.receive_capture`, one :class:`~dl_ofdm_amd.sync.CaptureSync`
    launch cuts every frame at its estimated start -- linearly, up to ``sync = W > 0`` samples off ``first + f * stride`` -- and
    writes it into the plan's ``x`` where ``chain_receive(x, sync=W)`` has its alignment launch.  ``frames`` (``None``: every
    frame whose window ``[start - W, start + T + W)`` lies inside the capture) selects the resident plan.

    ``first=None, acquire=J, lo=...``: as :meth:`RxReceiver.receive_capture` -- acquisition over ``J`` frames (the pilot cells are
    ``tr.ofdmobj.pilotSc``) leaves the frame start inside ``[lo, lo + T)`` on the device and the cut reads it there.  The host
    then does not know the start: ``frames=None`` counts the frames that fit from the LAST start of that range on, and with a
    device tensor ``first`` (and ``lo``) ``frames`` must be given.

    ``cfo=True, cfo_scope="capture"``: one carrier offset for the whole capture, as :meth:`RxReceiver.receive_capture`.
    ``cfo_span = M > 0``: offsets beyond half a subcarrier spacing, as there."""
    what = "chain_receive_capture"
    W, M = _checked_capture_call(what, cap, first, sync, cfo, acquire, cfo_scope, cfo_span, scale)
    if not tr.fused_ok:
        raise _lib.DccnError("the chain's receive path needs the fused equaliser step")
    if not isinstance(cap, torch.Tensor) or cap.dim() != 2:
        raise _lib.DccnError("chain_receive_capture takes a device tensor [n, 2]")
    if frames is None:
        if isinstance(first, torch.Tensor):
            raise _lib.DccnError("chain_receive_capture: a device tensor `first` needs frames=...")
        o = tr.ofdmobj
        T = int(tr.FLAGS.nsymbol) * (int(o.K) + int(o.CP))
        step = T if stride is None else int(stride)
        latest = int(lo) + T - 1 if first is None else int(first)   # (acquisition: the LAST start of the range)
        room = int(cap.shape[0]) - latest - T - W
        if room < 0 or step < T:
            raise _lib.DccnError("chain_receive_capture: no frame at first = %d fits a capture of %d samples (stride %d)"
                                 % (latest, int(cap.shape[0]), step))
        frames = room // step + 1
    pl = tr.resident(int(frames))
    front = _chain_front(tr, pl).cut(what, cap, first, stride, W, cfo, acquire, lo, cfo_scope, M, scale)
    return _chain_result(tr, pl, want_llr, want_prob, *front)


def group_receive(group, xs, sync: int = 0, cfo: bool = False) -> list:
    """Several links' chains in ONE launch sequence (``dccn_eq_receive_step_grouped``): ``group`` is a
    :class:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup`, ``xs`` one ``[batch, S, K + CP, 2]`` batch of frames per chain.
    One :class:`ReceiveResult` per chain, bit for bit what :func:`chain_receive` returns for that chain alone.

    ``sync = W > 0`` (and ``cfo=True``) as :func:`chain_receive`: ``xs`` are device tensors, and one alignment launch for all
    links (``dccn_frame_sync_grouped``, :class:`~dl_ofdm_amd.sync.FrameSyncGroup`) writes every chain's frames in place of the
    per-chain copies; ``result.offset`` / ``result.cfo`` per chain."""
    return group.receive(xs, sync=sync, cfo=cfo)


def group_receive_capture(group, caps, firsts=None, strides=None, sync: int = 3, cfo: bool = False, acquire: int = 0, los=0,
                          cfo_scope: str = "frame", cfo_span: int = 0) -> list:
    """:func:`chain_receive_capture` for every chain of a :class:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup` at once
    (``frames`` is the group's batch): one capture per chain, acquisition (``firsts=None, acquire=J``: three launches for all
    links) and the cut (one launch for all links) in front of the grouped step.  ``ChainReceiveGroup.receive_capture`` says the
    rest; one :class:`ReceiveResult` per chain, bit for bit what :func:`chain_receive_capture` returns for that chain alone."""
    return group.receive_capture(caps, firsts, strides, sync=sync, cfo=cfo, acquire=acquire, los=los, cfo_scope=cfo_scope,
                                 cfo_span=cfo_span)


def __getattr__(name):
    # the classical engines live in classical_receive.py (which imports this module): exported here on first use
    if name in ("ClassicalRxReceiver", "ClassicalReceiveGroup"):
        from . import classical_receive
        return getattr(classical_receive, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
