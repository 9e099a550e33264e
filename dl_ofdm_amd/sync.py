"""Per-frame timing alignment from the cyclic prefix (``dccn_frame_sync``; include/dccn.h).

The receive path takes frames that sit on the FFT window.  The centred L-tap response of the LTE profiles makes a frame arrive
``(L - 1) // 2`` samples early (datagen.py), and ``align_window`` undoes that on the generator side with the KNOWN advance.
:class:`FrameSync` is the receiver-side stage: every frame's prefix samples repeat K samples later, and the lag in ``[-W, W]`` at
which they correlate best is the frame's own timing -- per frame, so it also serves channels whose advance differs from frame to
frame (``mixRayleigh``).  The frame is taken as circular, exactly as ``align_window``'s ``torch.roll`` treats it:
``aligned[f] = torch.roll(x[f].view(T, 2), -offset[f], 0)``.

``FrameSync(..., cfo=True)`` is the same launch with the carrier-frequency offset taken out as well (``dccn_frame_sync_cfo``): a
frame ``s[n] exp(+2 pi i eps n / K)`` turns the prefix correlation by ``exp(-2 pi i eps)``, so the angle of the correlation at the
chosen lag estimates ``eps`` (in subcarrier spacings, unambiguous for ``|eps| < 1/2``), and sample ``n`` of the aligned frame
leaves multiplied by ``exp(-2 pi i cfo n / K)``.  The frame is circular here too: the ``|offset|`` samples that wrap carry a phase
step of ``2 pi eps T / K`` against their neighbours.

:class:`CaptureSync` (``dccn_capture_sync``) lifts that limit where the frames still sit inside one contiguous capture: the same
estimator over a window that extends ``W`` samples beyond the nominal frame on both sides, indexed linearly, and the frame cut at
its estimated start -- the samples the alignment brings in are the frame's neighbours in the air.  :class:`CaptureAcquire`
(``dccn_capture_acquire``) finds the ``first`` that stage needs -- anywhere in a frame period, not within ``W`` -- and leaves it on
the device, where ``CaptureSync.run(cap, first_tensor, lo=...)`` reads it.  ``cfo_span=M`` on both lifts the half-spacing limit
of the carrier offset: acquisition decides the whole number of spacings together with the frame start
(``dccn_capture_acquire_wide``), and the cut unwraps the prefix's fraction against it and takes the whole offset out
(``dccn_capture_sync_wide``, ``dccn_capture_sync_pooled_wide``).

:class:`FrameSyncGroup`, :class:`CaptureSyncGroup` and :class:`CaptureAcquireGroup` run the same stages for several links at once
(``dccn_frame_sync_grouped``, ``dccn_capture_sync_grouped``, ``dccn_capture_acquire_grouped``: one launch each, acquisition three), the
front end of :class:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup`; link i's results are bit for bit the solo class's.

:class:`CaptureSync` and :class:`CaptureAcquire` also take the capture as a front end delivers it, ``int16 [n, 2]`` ("sc16":
interleaved 16-bit integer I/Q) with a ``scale`` (``dccn_capture_sync_sc16``, ``dccn_capture_sync_pooled_sc16``,
``dccn_capture_acquire_sc16``): sample ``n`` is ``(float(I) * scale, float(Q) * scale)``, converted inside the launches, and every
output is bit for bit what the float32 call writes for ``radio.sc16_to_float(cap, scale)``.  ``cfo_span > 0`` and the group
classes stay float32-only.

There is no CPU or PyTorch fallback: an unsupported shape or a tensor that is not on the GPU raises :class:`DccnError`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import DccnError, check


def rotate_response_(H: torch.Tensor, offset: torch.Tensor) -> torch.Tensor:
    """The frequency response of frames aligned by ``offset``, in place: ``aligned[n] = x[n + offset]`` has the response
    ``H[k] * exp(+2 pi i k offset / K)`` (column ``k`` = DFT bin ``k``, the generator's numbering).  ``H``: float32
    ``[frames, K, 2]`` or ``[frames, S, K, 2]``; ``offset``: int32 ``[frames]``.  The torch statement of what
    ``dccn_gen_static_apply_sync`` does to ``H_inout`` (the integer ``k * offset`` reduced mod K first)."""
    K = H.shape[-2]
    k = torch.arange(K, device=H.device, dtype=torch.int64)
    m = torch.remainder(k[None, :] * offset.to(torch.int64)[:, None], K)
    ang = m.to(torch.float32) * (2.0 / K)
    ramp = torch.complex(torch.cos(ang * torch.pi), torch.sin(ang * torch.pi))
    Hc = torch.view_as_complex(H)
    Hc.mul_(ramp[:, None, :] if Hc.dim() == 3 else ramp)
    return H


CFO_SCOPES = ("frame", "capture")
SC16_DEFAULT_SCALE = 2.0 ** -15     # full scale onto [-1, 1)


def capture_format(cap, scale, what: str, cfo_span: int = 0):
    """``(is_sc16, scale)`` of a capture handed to ``what``: a contiguous device tensor ``float32 [n, 2]`` (``scale`` must be
    ``None``) or ``int16 [n, 2]`` (``scale=None``: ``2**-15``; otherwise finite and positive).  :class:`DccnError` for anything
    else, and for an int16 capture where ``cfo_span > 0``: the wide entries are float32-only."""
    if not isinstance(cap, torch.Tensor) or cap.device.type != "cuda":
        raise DccnError("%s takes a device tensor; there is no CPU fallback" % what)
    if cap.dtype not in (torch.float32, torch.int16) or cap.dim() != 2 or cap.shape[1] != 2 or not cap.is_contiguous():
        raise DccnError("%s: cap must be a contiguous float32 [n, 2] or int16 [n, 2] tensor, got %s %r"
                        % (what, cap.dtype, tuple(cap.shape)))
    if cap.dtype == torch.float32:
        if scale is not None:
            raise DccnError("%s: `scale` belongs to an int16 capture; a float32 capture is taken as it is" % what)
        return False, None
    if cfo_span:
        raise DccnError("%s: an int16 capture cannot be combined with cfo_span > 0 (the wide entries are float32-only)" % what)
    try:
        value = SC16_DEFAULT_SCALE if scale is None else float(scale)
    except (TypeError, ValueError):
        raise DccnError("%s: scale must be a finite, positive number, got %r" % (what, scale))
    # the library takes an fp32: judge the value it will see
    value = C.c_float(value).value
    if not (value > 0.0) or value == float("inf"):
        raise DccnError("%s: scale must be a finite, positive fp32 number, got %r" % (what, scale))
    return True, value


def check_cfo_scope(cfo, cfo_scope) -> bool:
    """``True`` where the carrier offset is pooled over the capture (``cfo_scope="capture"``).  ``ValueError``, before anything is
    launched, for an unknown scope and for ``"capture"`` without ``cfo``: there is no offset to pool."""
    if cfo_scope not in CFO_SCOPES:
        raise ValueError("cfo_scope must be one of %r, got %r" % (CFO_SCOPES, cfo_scope))
    if cfo_scope == "capture" and not cfo:
        raise ValueError('cfo_scope="capture" needs cfo=True: there is no carrier offset to pool without it')
    return cfo_scope == "capture"


class FrameSync:
    """Fixed-shape alignment stage on one GPU: ``run(x) -> (aligned, offset)``.

    ``x``: device tensor ``float32 [frames, S, K + CP, 2]``.  ``out_kin``: ``K + CP`` (default: the aligned frames) or ``K`` (the
    ``K`` samples behind each symbol's prefix, the input of a receiver built with ``cp=False``).  ``offset`` (``int32
    [frames]``), ``metric`` (``float32 [frames, 2 W + 1]``: the estimator's value at the lags ``-W .. W``) and the output
    buffer are resident: the next ``run`` overwrites them.  ``cfo=True``: ``run`` and ``offsets`` also estimate every frame's
    carrier-frequency offset into ``self.cfo`` (``float32 [frames]``, subcarrier spacings, resident) and ``run`` writes the
    frames with it taken out; ``run`` keeps returning ``(aligned, offset)``.
    """

    def __init__(self, S: int, K: int, CP: int, W: int, frames: int, device="cuda", out_kin: Optional[int] = None,
                 want_metric: bool = True, cfo: bool = False):
        self.lib = _lib.load()
        self.S, self.K, self.CP, self.W, self.frames = int(S), int(K), int(CP), int(W), int(frames)
        self.out_kin = self.K + self.CP if out_kin is None else int(out_kin)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DccnError("FrameSync needs a CUDA (ROCm) device; there is no CPU fallback")
        if not self.lib.dccn_frame_sync_supported(self.S, self.K, self.CP, self.W):
            raise DccnError("dccn_frame_sync_supported refused S=%d K=%d CP=%d W=%d (needs 1 <= W <= CP, 2 W + CP <= 64, an even "
                            "frame length)" % (self.S, self.K, self.CP, self.W))
        if self.out_kin not in (self.K + self.CP, self.K) or self.frames <= 0:
            raise DccnError("FrameSync: out_kin must be K + CP or K and frames positive (got out_kin=%d, frames=%d)"
                            % (self.out_kin, self.frames))
        self.offset = torch.zeros(self.frames, dtype=torch.int32, device=self.device)
        self.metric = (torch.zeros(self.frames, 2 * self.W + 1, dtype=torch.float32, device=self.device) if want_metric else None)
        self.cfo = torch.zeros(self.frames, dtype=torch.float32, device=self.device) if cfo else None
        self.out = None         # allocated by the first run() that is not given a destination

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _device_frames(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise DccnError("FrameSync.run takes a device tensor; there is no CPU fallback")
        want = (self.frames, self.S, self.K + self.CP, 2)
        if x.dtype != torch.float32 or tuple(x.shape) != want or not x.is_contiguous():
            raise DccnError("FrameSync.run: x must be a contiguous float32 %r tensor, got %s %r" % (want, x.dtype, tuple(x.shape)))
        return x

    def _launch(self, x: torch.Tensor, out: Optional[torch.Tensor]) -> None:
        """the one launch: ``dccn_frame_sync``, or ``dccn_frame_sync_cfo`` of a stage built with ``cfo=True``"""
        head = (x.data_ptr(), self.frames, self.S, self.K, self.CP, self.W, self.out_kin, None if out is None else out.data_ptr(),
                self.offset.data_ptr())
        tail = (None if self.metric is None else self.metric.data_ptr(), self._stream())
        if self.cfo is None:
            check(self.lib.dccn_frame_sync(*head, *tail), "dccn_frame_sync")
        else:
            check(self.lib.dccn_frame_sync_cfo(*head, self.cfo.data_ptr(), *tail), "dccn_frame_sync_cfo")

    def run(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Estimate every frame's offset and write the aligned frames to ``out`` (``None``: this object's own buffer), on the
        current stream.  ``out`` must not overlap ``x``."""
        x = self._device_frames(x)
        want = (self.frames, self.S, self.out_kin, 2)
        if out is None:
            if self.out is None:
                self.out = torch.empty(*want, dtype=torch.float32, device=self.device)
            out = self.out
        elif (not isinstance(out, torch.Tensor) or out.device != x.device or out.dtype != torch.float32
              or tuple(out.shape) != want or not out.is_contiguous()):
            raise DccnError("FrameSync.run: out must be a contiguous float32 %r tensor on %s" % (want, x.device))
        self._launch(x, out)
        return out, self.offset

    def offsets(self, x: torch.Tensor) -> torch.Tensor:
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(self._device_frames(x), None)
        return self.offset


class CaptureSync:
    """Frames cut from ONE CONTIGUOUS CAPTURE at their estimated starts (``dccn_capture_sync``): ``run(cap, first) -> (frames_out,
    offset)``.

    ``cap``: contiguous device tensor ``float32 [n, 2]``, or ``int16 [n, 2]`` with ``scale`` -- what a front end hands over
    (``dccn_capture_sync_sc16`` / ``dccn_capture_sync_pooled_sc16``: converted inside the launch, the results bit for bit those of
    the float32 capture ``radio.sc16_to_float(cap, scale)``; one object serves both dtypes call by call).  Frame ``f`` nominally starts at sample
    ``first + f * stride`` (``stride=None``: ``T = S (K + CP)``, frames back to back).  The estimator is :class:`FrameSync`'s over
    the window ``[start - W, start + T + W)``, indexed linearly: nothing wraps, so the samples the alignment brings in are the
    frame's neighbours in the air, and with ``cfo=True`` they carry no phase step.  The caller leaves ``W`` samples of the capture
    in front of the first frame and behind the last.  ``offset``, ``metric``, ``cfo`` and the output buffer are resident, as
    :class:`FrameSync`'s are; ``out_kin`` as there.

    ``cfo=True, cfo_scope="capture"`` (``dccn_capture_sync_pooled``): a capture comes from one front end with one oscillator, so
    ONE carrier offset is estimated for the whole call -- from the sum over the frames of each frame's prefix correlation at its own
    lag -- and every frame is derotated with it; timing stays per frame.  ``self.cfo`` is then ``float32 [1]``.  Three launches
    (estimate, sum, cut) instead of one, no host round trip; ``offsets`` is not offered.  The default ``"frame"`` is the
    per-frame estimate above.

    ``cfo=True, cfo_span=M > 0`` (``dccn_capture_sync_wide``, ``dccn_capture_sync_pooled_wide``; either scope): the offset may
    exceed half a subcarrier spacing.  ``run(..., acquired=(cfo_int, cfo_frac))`` takes the pair that
    ``CaptureAcquire(..., cfo_span=M)`` left on the device (``.cfo_int``, ``.cfo``); the prefix's fraction is unwrapped against it,
    the whole offset is taken out and ``self.cfo`` holds totals.  The integer is only known through acquisition, so with
    ``cfo_scope="frame"`` the start is a device tensor too.  ``cfo_span=0``, the default, is the calls above.  float32 captures
    only: an int16 capture raises :class:`DccnError`.
    """

    def __init__(self, S: int, K: int, CP: int, W: int, frames: int, device="cuda", out_kin: Optional[int] = None,
                 want_metric: bool = True, cfo: bool = False, cfo_scope: str = "frame", cfo_span: int = 0):
        self.pooled = check_cfo_scope(cfo, cfo_scope)
        self.lib = _lib.load()
        self.S, self.K, self.CP, self.W, self.frames = int(S), int(K), int(CP), int(W), int(frames)
        self.cfo_span = int(cfo_span)
        if self.cfo_span and not cfo:
            raise DccnError("CaptureSync(cfo_span=M > 0) needs cfo=True: there is no carrier offset to unwrap without it")
        if not (0 <= self.cfo_span <= max(self.K // 2 - 1, 0)):
            raise DccnError("CaptureSync: cfo_span must lie in [0, K / 2 - 1], got %d at K=%d" % (self.cfo_span, self.K))
        self.T = self.S * (self.K + self.CP)
        self.out_kin = self.K + self.CP if out_kin is None else int(out_kin)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DccnError("CaptureSync needs a CUDA (ROCm) device; there is no CPU fallback")
        if not self.lib.dccn_capture_sync_supported(self.S, self.K, self.CP, self.W):
            raise DccnError("dccn_capture_sync_supported refused S=%d K=%d CP=%d W=%d (needs 1 <= W <= CP, 2 W + CP <= 64, an "
                            "even frame length, four windows of T + 2 W samples within 64 KB)" % (self.S, self.K, self.CP, self.W))
        if self.out_kin not in (self.K + self.CP, self.K) or self.frames <= 0:
            raise DccnError("CaptureSync: out_kin must be K + CP or K and frames positive (got out_kin=%d, frames=%d)"
                            % (self.out_kin, self.frames))
        self.offset = torch.zeros(self.frames, dtype=torch.int32, device=self.device)
        self.metric = (torch.zeros(self.frames, 2 * self.W + 1, dtype=torch.float32, device=self.device) if want_metric else None)
        self.cfo = torch.zeros(1 if self.pooled else self.frames, dtype=torch.float32, device=self.device) if cfo else None
        self.ws = None
        if self.pooled:
            size = (self.lib.dccn_capture_sync_pooled_wide_workspace_size if self.cfo_span
                    else self.lib.dccn_capture_sync_pooled_workspace_size)
            self.ws = torch.empty(int(size(self.frames)), dtype=torch.uint8, device=self.device)
        self.out = None         # allocated by the first run() that is not given a destination

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _acquired_pair(self, acquired, cap) -> tuple:
        """the pointers of ``(cfo_int, cfo_frac)``: ``()`` for a stage built with ``cfo_span=0``, which takes none"""
        if not self.cfo_span:
            if acquired is not None:
                raise DccnError("CaptureSync: `acquired` belongs to a stage built with cfo_span = M > 0")
            return ()
        ok = isinstance(acquired, (tuple, list)) and len(acquired) == 2 and all(
            isinstance(t, torch.Tensor) and t.device == cap.device and t.numel() == 1 and t.is_contiguous() for t in acquired)
        if not ok or acquired[0].dtype != torch.int32 or acquired[1].dtype != torch.float32:
            raise DccnError("CaptureSync(cfo_span=M > 0) needs acquired=(cfo_int, cfo_frac): an int32 and a float32 tensor of one "
                            "element on the capture's device, what CaptureAcquire(cfo_span=M) left there")
        return (acquired[0].data_ptr(), acquired[1].data_ptr())

    def _launch(self, cap, first, stride, out: Optional[torch.Tensor], lo: Optional[int] = None, acquired=None, scale=None) -> None:
        sc16, scale = capture_format(cap, scale, "CaptureSync", self.cfo_span)
        stride = self.T if stride is None else int(stride)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        pair = self._acquired_pair(acquired, cap)
        if self.pooled:
            return self._launch_pooled(cap, first, stride, out, lo, pair, scale if sc16 else None)
        if pair and not isinstance(first, torch.Tensor):
            raise DccnError("CaptureSync(cfo_span=M > 0): the per-frame cut reads the start where acquisition left it, a device "
                            "tensor `first` with lo=...")
        tail = (stride, self.frames, self.S, self.K, self.CP, self.W, self.out_kin, p(out), self.offset.data_ptr(), p(self.cfo),
                p(self.metric), *pair, self._stream())
        on_dev = isinstance(first, torch.Tensor)
        if on_dev:
            # the start is on the device (CaptureAcquire left it there): nothing is read back
            if lo is None:
                raise DccnError("CaptureSync: a device tensor `first` needs lo=..., the origin of the range [lo, lo + T) it lies in")
            if first.device != cap.device or first.dtype != torch.int64 or first.numel() != 1 or not first.is_contiguous():
                raise DccnError("CaptureSync: a device `first` must be an int64 tensor of one element on the capture's device")
        if sc16:
            check(self.lib.dccn_capture_sync_sc16(cap.data_ptr(), int(cap.shape[0]), scale, 0 if on_dev else int(first),
                                                  first.data_ptr() if on_dev else None, int(lo) if on_dev else 0, *tail),
                  "dccn_capture_sync_sc16")
        elif on_dev:
            entry = "dccn_capture_sync_wide" if pair else "dccn_capture_sync_at"
            check(getattr(self.lib, entry)(cap.data_ptr(), int(cap.shape[0]), first.data_ptr(), int(lo), *tail), entry)
        else:
            check(self.lib.dccn_capture_sync(cap.data_ptr(), int(cap.shape[0]), int(first), *tail), "dccn_capture_sync")

    def _launch_pooled(self, cap, first, stride: int, out: Optional[torch.Tensor], lo: Optional[int], pair: tuple = (),
                       scale: Optional[float] = None) -> None:
        """``dccn_capture_sync_pooled`` (``pair``: ``dccn_capture_sync_pooled_wide``; ``scale``: ``dccn_capture_sync_pooled_sc16``
        on an int16 capture): estimate, sum and cut, three launches on the current stream"""
        if out is None:
            raise DccnError('CaptureSync(cfo_scope="capture") has no offsets-only call: the pooled entry writes the frames')
        on_dev = isinstance(first, torch.Tensor)
        if on_dev:
            if lo is None:
                raise DccnError("CaptureSync: a device tensor `first` needs lo=..., the origin of the range [lo, lo + T) it lies in")
            if first.device != cap.device or first.dtype != torch.int64 or first.numel() != 1 or not first.is_contiguous():
                raise DccnError("CaptureSync: a device `first` must be an int64 tensor of one element on the capture's device")
        entry = "dccn_capture_sync_pooled_wide" if pair else "dccn_capture_sync_pooled"
        if scale is not None:
            entry = "dccn_capture_sync_pooled_sc16"
        fmt = () if scale is None else (scale,)
        check(getattr(self.lib, entry)(cap.data_ptr(), int(cap.shape[0]), *fmt, 0 if on_dev else int(first),
                                       first.data_ptr() if on_dev else None, int(lo) if on_dev else 0, stride,
                                       self.frames, self.S, self.K, self.CP, self.W, self.out_kin, out.data_ptr(),
                                       self.offset.data_ptr(), self.cfo.data_ptr(),
                                       None if self.metric is None else self.metric.data_ptr(), *pair, self.ws.data_ptr(),
                                       int(self.ws.numel()), self._stream()), entry)

    def run(self, cap: torch.Tensor, first, stride: Optional[int] = None, out: Optional[torch.Tensor] = None,
            lo: Optional[int] = None, acquired=None, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Estimate every frame's offset and write the frames, cut at their estimated starts (and with ``cfo=True`` derotated),
        to ``out`` (``None``: this object's own buffer), on the current stream.  ``out`` must not overlap ``cap``.

        ``first``: an integer, or a device ``int64`` tensor of one element together with ``lo`` (``dccn_capture_sync_at``: the
        launch reads the start from device memory and keeps it inside ``[lo, lo + T - 1]``; every window must lie inside the
        capture for every start in that range).  ``acquired``: the pair of a stage built with ``cfo_span = M > 0``.
        ``scale``: the value of one count of an ``int16`` capture (``None``: ``2**-15``); not given with a float32 capture."""
        want = (self.frames, self.S, self.out_kin, 2)
        if out is None:
            if self.out is None:
                self.out = torch.empty(*want, dtype=torch.float32, device=self.device)
            out = self.out
        elif (not isinstance(out, torch.Tensor) or out.device.type != "cuda" or out.dtype != torch.float32
              or tuple(out.shape) != want or not out.is_contiguous()):
            raise DccnError("CaptureSync.run: out must be a contiguous float32 %r device tensor" % (want,))
        self._launch(cap, first, stride, out, lo, acquired, scale)
        return out, self.offset

    def offsets(self, cap: torch.Tensor, first, stride: Optional[int] = None, lo: Optional[int] = None, acquired=None,
                scale: Optional[float] = None) -> torch.Tensor:
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``.  ``first`` / ``lo`` / ``acquired`` /
        ``scale`` as :meth:`run`."""
        self._launch(cap, first, stride, None, lo, acquired, scale)
        return self.offset


class CaptureAcquire:
    """Coarse acquisition inside a contiguous capture (``dccn_capture_acquire``): ``run(cap, lo) -> first``, the sample in
    ``[lo, lo + T)`` at which a frame starts, as a device ``int64`` tensor of one element -- what :meth:`CaptureSync.run` takes
    as ``first`` together with the same ``lo``.  Nothing is read back and nothing synchronises.

    Stage A finds the symbol timing (any lag of a symbol period) and the carrier offset from the cyclic prefixes of ``J * S``
    symbols; stage B finds which of the ``S`` symbol positions is the frame's first from the pilot symbols (``pilot_sc``:
    ``ofdm_tx.pilotSc``, the pilot cells as sorted flat ``symbol * K + carrier`` indices).  The ``J`` frames are assumed back to
    back (stride ``T``), and ``lo + (J + 2) T`` samples of the capture must exist.  ``first``, ``cfo`` (``float32 [1]``,
    subcarrier spacings), ``sym_metric`` (``float32 [K + CP]``) and ``phase_metric`` (``float32 [S]``) are resident: the next
    ``run`` overwrites them.  ``J = 1`` with BPSK data can tie exactly; a batch's worth of frames (``J = 16``) is the intended
    setting (README).

    ``cfo_span = M > 0`` (``dccn_capture_acquire_wide``): the carrier offset may exceed half a subcarrier spacing.  Stage B then
    decides the symbol position and the whole number of spacings ``m`` in ``[-M, M]`` together, from the pilots' bins shifted by
    ``m``; ``cfo`` stays the fraction, ``cfo_int`` (``int32 [1]``, resident) is ``m``, the offset is their sum, and
    ``phase_metric`` is ``float32 [S, 2 M + 1]``.  ``M <= K / 2 - 1``; the shift is circular in ``K``, so on the reference grid
    ``M <= 7`` is the span a real channel filter supports.  ``cfo_span=0``, the default, is the narrow call (``cfo_int`` stays 0).

    ``cap`` may be ``int16 [n, 2]`` with ``scale`` (``dccn_capture_acquire_sc16``; as :class:`CaptureSync`, bit for bit the float32
    call on the converted capture, one object for both dtypes); not with ``cfo_span > 0``."""

    def __init__(self, S: int, K: int, CP: int, pilot_sc, J: int, device="cuda", cfo_span: int = 0):
        self.lib = _lib.load()
        self.S, self.K, self.CP, self.J = int(S), int(K), int(CP), int(J)
        self.cfo_span = int(cfo_span)
        self.T = self.S * (self.K + self.CP)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DccnError("CaptureAcquire needs a CUDA (ROCm) device; there is no CPU fallback")
        sc = torch.as_tensor(pilot_sc).reshape(-1).to(torch.int32)
        self.n_pilot = int(sc.numel())
        if not self.lib.dccn_capture_acquire_supported(self.S, self.K, self.CP, self.n_pilot, self.J):
            raise DccnError("dccn_capture_acquire_supported refused S=%d K=%d CP=%d n_pilot=%d J=%d (needs S <= 64, CP <= K, "
                            "K + CP <= 1024, 2 <= n_pilot <= 256, 1 <= J <= 256)" % (self.S, self.K, self.CP, self.n_pilot, self.J))
        self.pilot_sc = sc.to(self.device).contiguous()
        self.first = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.cfo = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.sym_metric = torch.zeros(self.K + self.CP, dtype=torch.float32, device=self.device)
        self.phase_metric = torch.zeros(self.S, dtype=torch.float32, device=self.device)
        self.cfo_int = torch.zeros(1, dtype=torch.int32, device=self.device)
        M = self.cfo_span
        if M:
            if not self.lib.dccn_capture_acquire_wide_supported(self.S, self.K, self.CP, self.n_pilot, self.J, M):
                raise DccnError("dccn_capture_acquire_wide_supported refused cfo_span=%d at K=%d (needs 0 <= cfo_span <= K / 2 - 1)"
                                % (M, self.K))
            self.phase_metric = torch.zeros(self.S, 2 * M + 1, dtype=torch.float32, device=self.device)
            nws = int(self.lib.dccn_capture_acquire_wide_workspace_size(self.S, self.K, self.CP, self.n_pilot, self.J, M))
        else:
            nws = int(self.lib.dccn_capture_acquire_workspace_size(self.S, self.K, self.CP, self.n_pilot, self.J))
        self.ws = torch.empty(nws, dtype=torch.uint8, device=self.device)

    def run(self, cap: torch.Tensor, lo: int = 0, scale: Optional[float] = None) -> torch.Tensor:
        """Three launches on the current stream; returns ``self.first``.  ``scale``: the value of one count of an ``int16``
        capture (``None``: ``2**-15``); not given with a float32 capture."""
        sc16, scale = capture_format(cap, scale, "CaptureAcquire", self.cfo_span)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if sc16:
            check(self.lib.dccn_capture_acquire_sc16(cap.data_ptr(), int(cap.shape[0]), scale, int(lo), self.J, self.S, self.K,
                                                     self.CP, self.pilot_sc.data_ptr(), self.n_pilot, self.first.data_ptr(),
                                                     self.cfo.data_ptr(), self.sym_metric.data_ptr(), self.phase_metric.data_ptr(),
                                                     self.ws.data_ptr(), int(self.ws.numel()), stream), "dccn_capture_acquire_sc16")
            return self.first
        if self.cfo_span:
            check(self.lib.dccn_capture_acquire_wide(cap.data_ptr(), int(cap.shape[0]), int(lo), self.J, self.S, self.K, self.CP,
                                                     self.pilot_sc.data_ptr(), self.n_pilot, self.cfo_span, self.first.data_ptr(),
                                                     self.cfo.data_ptr(), self.cfo_int.data_ptr(), self.sym_metric.data_ptr(),
                                                     self.phase_metric.data_ptr(), self.ws.data_ptr(), int(self.ws.numel()),
                                                     stream), "dccn_capture_acquire_wide")
            return self.first
        check(self.lib.dccn_capture_acquire(cap.data_ptr(), int(cap.shape[0]), int(lo), self.J, self.S, self.K, self.CP,
                                            self.pilot_sc.data_ptr(), self.n_pilot, self.first.data_ptr(), self.cfo.data_ptr(),
                                            self.sym_metric.data_ptr(), self.phase_metric.data_ptr(), self.ws.data_ptr(),
                                            int(self.ws.numel()), stream), "dccn_capture_acquire")
        return self.first


# ---- the same stages for several links per launch (include/dccn.h "the receive front end for several links") -------------------
def _group_size(lib, n_links: int, what: str) -> int:
    gmax = int(lib.dccn_chain_group_max())
    if not (1 <= int(n_links) <= gmax):
        raise ValueError("%s: 1..%d links per group" % (what, gmax))
    return int(n_links)


def _per_link(v, n: int, what: str) -> list:
    """one entry per link: a scalar (or ``None``) serves every link, a list or tuple must have ``n`` entries"""
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError("%s: one entry per link (%d), got %d" % (what, n, len(v)))
        return list(v)
    return [v] * n


def _device_capture(cap, what: str) -> torch.Tensor:
    if not isinstance(cap, torch.Tensor) or cap.device.type != "cuda":
        raise DccnError("%s takes device tensors; there is no CPU fallback" % what)
    if cap.dtype != torch.float32 or cap.dim() != 2 or cap.shape[1] != 2 or not cap.is_contiguous():
        raise DccnError("%s: a capture must be a contiguous float32 [n, 2] tensor, got %s %r" % (what, cap.dtype, tuple(cap.shape)))
    return cap


class _SyncGroupBase:
    """what :class:`FrameSyncGroup` and :class:`CaptureSyncGroup` share: the shape, per-link resident ``offset`` / ``cfo`` /
    ``metric`` (lists of tensors, entry i as the solo class keeps it for link i) and the output buffers"""

    def __init__(self, supported, S, K, CP, W, frames, n_links, device, out_kin, want_metric, cfo, cfo_len=None):
        self.lib = _lib.load()
        name = type(self).__name__
        self.n_links = _group_size(self.lib, n_links, name)
        self.S, self.K, self.CP, self.W, self.frames = int(S), int(K), int(CP), int(W), int(frames)
        self.T = self.S * (self.K + self.CP)
        self.out_kin = self.K + self.CP if out_kin is None else int(out_kin)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DccnError("%s needs a CUDA (ROCm) device; there is no CPU fallback" % name)
        if not getattr(self.lib, supported)(self.S, self.K, self.CP, self.W):
            raise DccnError("%s refused S=%d K=%d CP=%d W=%d" % (supported, self.S, self.K, self.CP, self.W))
        if self.out_kin not in (self.K + self.CP, self.K) or self.frames <= 0:
            raise DccnError("%s: out_kin must be K + CP or K and frames positive (got out_kin=%d, frames=%d)"
                            % (name, self.out_kin, self.frames))
        n, dev = self.n_links, self.device
        self.offset = [torch.zeros(self.frames, dtype=torch.int32, device=dev) for _ in range(n)]
        self.metric = ([torch.zeros(self.frames, 2 * self.W + 1, dtype=torch.float32, device=dev) for _ in range(n)]
                       if want_metric else None)
        ncfo = self.frames if cfo_len is None else int(cfo_len)
        self.cfo = [torch.zeros(ncfo, dtype=torch.float32, device=dev) for _ in range(n)] if cfo else None
        self.out = None         # allocated by the first run() that is not given destinations

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _outs(self, outs) -> list:
        want = (self.frames, self.S, self.out_kin, 2)
        if outs is None:
            if self.out is None:
                self.out = [torch.empty(*want, dtype=torch.float32, device=self.device) for _ in range(self.n_links)]
            return self.out
        outs = _per_link(list(outs), self.n_links, type(self).__name__ + ".run(outs)")
        for o in outs:
            if (not isinstance(o, torch.Tensor) or o.device.type != "cuda" or o.dtype != torch.float32 or tuple(o.shape) != want
                    or not o.is_contiguous()):
                raise DccnError("%s.run: every out must be a contiguous float32 %r device tensor" % (type(self).__name__, want))
        return outs

    def _opt(self, tensors, i):
        return None if tensors is None else tensors[i].data_ptr()


class FrameSyncGroup(_SyncGroupBase):
    """:class:`FrameSync` for up to ``dccn_chain_group_max()`` links in ONE launch (``dccn_frame_sync_grouped``):
    ``run(xs) -> (aligned, offsets)``, lists with one entry per link, entry i bit for bit what ``FrameSync.run(xs[i])`` gives.
    ``offset``, ``metric``, ``cfo`` and the output buffers are resident per link (lists of tensors)."""

    def __init__(self, S: int, K: int, CP: int, W: int, frames: int, n_links: int, device="cuda", out_kin: Optional[int] = None,
                 want_metric: bool = True, cfo: bool = False):
        super().__init__("dccn_frame_sync_supported", S, K, CP, W, frames, n_links, device, out_kin, want_metric, cfo)
        self._table = (_lib.FrameLink * self.n_links)()

    def _launch(self, xs, outs) -> None:
        xs = _per_link(list(xs), self.n_links, "FrameSyncGroup.run(xs)")
        want = (self.frames, self.S, self.K + self.CP, 2)
        for x in xs:
            if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
                raise DccnError("FrameSyncGroup.run takes device tensors; there is no CPU fallback")
            if x.dtype != torch.float32 or tuple(x.shape) != want or not x.is_contiguous():
                raise DccnError("FrameSyncGroup.run: every x must be a contiguous float32 %r tensor, got %s %r"
                                % (want, x.dtype, tuple(x.shape)))
        for i, x in enumerate(xs):
            self._table[i] = _lib.FrameLink(x.data_ptr(), None if outs is None else outs[i].data_ptr(), self.offset[i].data_ptr(),
                                            self._opt(self.cfo, i), self._opt(self.metric, i))
        check(self.lib.dccn_frame_sync_grouped(self.n_links, self._table, self.frames, self.S, self.K, self.CP, self.W,
                                               self.out_kin, self._stream()), "dccn_frame_sync_grouped")

    def run(self, xs, outs=None):
        """One launch on the current stream.  ``outs``: one destination per link (``None``: this object's own buffers); no
        destination may overlap another link's frames or outputs."""
        outs = self._outs(outs)
        self._launch(xs, outs)
        return outs, self.offset

    def offsets(self, xs):
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(xs, None)
        return self.offset


class CaptureSyncGroup(_SyncGroupBase):
    """:class:`CaptureSync` for up to ``dccn_chain_group_max()`` links in ONE launch (``dccn_capture_sync_grouped``):
    ``run(caps, firsts) -> (frames_out, offsets)``, lists with one entry per link.  ``caps[i]``: link i's capture (two links may
    share one); ``firsts[i]``: an integer, or a device ``int64`` tensor of one element together with ``los[i]`` (what
    :class:`CaptureAcquireGroup` left there) -- known and acquired starts mix in one call; ``strides[i]``: ``None`` = ``T``.
    Entry i of every result is bit for bit what ``CaptureSync.run(caps[i], firsts[i], strides[i], lo=los[i])`` gives.

    ``cfo=True, cfo_scope="capture"`` (``dccn_capture_sync_pooled_grouped``): one carrier offset per link's capture, as
    :class:`CaptureSync` describes it -- three launches for all links, ``cfo[i]`` is ``float32 [1]``, ``offsets`` is not offered."""

    def __init__(self, S: int, K: int, CP: int, W: int, frames: int, n_links: int, device="cuda", out_kin: Optional[int] = None,
                 want_metric: bool = True, cfo: bool = False, cfo_scope: str = "frame"):
        self.pooled = check_cfo_scope(cfo, cfo_scope)
        super().__init__("dccn_capture_sync_supported", S, K, CP, W, frames, n_links, device, out_kin, want_metric, cfo,
                         cfo_len=1 if self.pooled else None)
        self._table = ((_lib.PooledLink if self.pooled else _lib.CaptureLink) * self.n_links)()
        self.ws = None
        if self.pooled:
            nws = int(self.lib.dccn_capture_sync_pooled_workspace_size(self.frames))
            self.ws = [torch.empty(nws, dtype=torch.uint8, device=self.device) for _ in range(self.n_links)]

    def _launch(self, caps, firsts, strides, outs, los) -> None:
        n = self.n_links
        caps = [_device_capture(c, "CaptureSyncGroup") for c in _per_link(list(caps), n, "CaptureSyncGroup.run(caps)")]
        firsts = _per_link(list(firsts), n, "CaptureSyncGroup.run(firsts)")
        strides = _per_link(strides, n, "CaptureSyncGroup.run(strides)")
        los = _per_link(los, n, "CaptureSyncGroup.run(los)")
        for i, (cap, first) in enumerate(zip(caps, firsts)):
            if isinstance(first, torch.Tensor):
                if los[i] is None:
                    raise DccnError("CaptureSyncGroup: a device tensor `first` needs los[i], the origin of the range [lo, lo + T) "
                                    "it lies in")
                if first.device != cap.device or first.dtype != torch.int64 or first.numel() != 1 or not first.is_contiguous():
                    raise DccnError("CaptureSyncGroup: a device `first` must be an int64 tensor of one element on the capture's device")
        if self.pooled and outs is None:
            raise DccnError('CaptureSyncGroup(cfo_scope="capture") has no offsets-only call: the pooled entry writes the frames')
        for i, (cap, first) in enumerate(zip(caps, firsts)):
            on_dev = isinstance(first, torch.Tensor)
            link = (cap.data_ptr(), int(cap.shape[0]), 0 if on_dev else int(first),
                    first.data_ptr() if on_dev else None, int(los[i]) if on_dev else 0,
                    self.T if strides[i] is None else int(strides[i]),
                    None if outs is None else outs[i].data_ptr(), self.offset[i].data_ptr(),
                    self._opt(self.cfo, i), self._opt(self.metric, i))
            if self.pooled:
                self._table[i] = _lib.PooledLink(*link, self.ws[i].data_ptr(), int(self.ws[i].numel()))
            else:
                self._table[i] = _lib.CaptureLink(*link)
        if self.pooled:
            check(self.lib.dccn_capture_sync_pooled_grouped(n, self._table, self.frames, self.S, self.K, self.CP, self.W,
                                                            self.out_kin, self._stream()), "dccn_capture_sync_pooled_grouped")
            return
        check(self.lib.dccn_capture_sync_grouped(n, self._table, self.frames, self.S, self.K, self.CP, self.W, self.out_kin,
                                                 self._stream()), "dccn_capture_sync_grouped")

    def run(self, caps, firsts, strides=None, outs=None, los=None):
        """One launch on the current stream.  ``strides`` / ``los``: one value for every link or one per link."""
        outs = self._outs(outs)
        self._launch(caps, firsts, strides, outs, los)
        return outs, self.offset

    def offsets(self, caps, firsts, strides=None, los=None):
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(caps, firsts, strides, None, los)
        return self.offset


class CaptureAcquireGroup:
    """:class:`CaptureAcquire` for up to ``dccn_chain_group_max()`` links in THREE launches (``dccn_capture_acquire_grouped``):
    ``run(caps, los) -> firsts``, one device ``int64`` tensor of one element per link -- what :meth:`CaptureSyncGroup.run` takes
    as ``firsts`` together with the same ``los``.  ``pilot_sc``: the pilot cells of every link, or a list of one array per link
    (of one length).  ``first``, ``cfo``, ``sym_metric``, ``phase_metric`` and the workspaces are resident per link (lists)."""

    def __init__(self, S: int, K: int, CP: int, pilot_sc, J: int, n_links: int, device="cuda"):
        self.lib = _lib.load()
        self.n_links = n = _group_size(self.lib, n_links, "CaptureAcquireGroup")
        self.S, self.K, self.CP, self.J = int(S), int(K), int(CP), int(J)
        self.T = self.S * (self.K + self.CP)
        self.device = dev = torch.device(device)
        if dev.type != "cuda":
            raise DccnError("CaptureAcquireGroup needs a CUDA (ROCm) device; there is no CPU fallback")
        per_link = isinstance(pilot_sc, (list, tuple)) and len(pilot_sc) > 0 and hasattr(pilot_sc[0], "__len__")
        scs = [torch.as_tensor(sc).reshape(-1).to(torch.int32) for sc in (_per_link(list(pilot_sc), n, "pilot_sc") if per_link
                                                                          else [pilot_sc])]
        self.n_pilot = int(scs[0].numel())
        if any(int(sc.numel()) != self.n_pilot for sc in scs):
            raise DccnError("CaptureAcquireGroup: the links' pilot cells must be of one length (n_pilot is the call's)")
        if not self.lib.dccn_capture_acquire_supported(self.S, self.K, self.CP, self.n_pilot, self.J):
            raise DccnError("dccn_capture_acquire_supported refused S=%d K=%d CP=%d n_pilot=%d J=%d"
                            % (self.S, self.K, self.CP, self.n_pilot, self.J))
        scs = [sc.to(dev).contiguous() for sc in scs]
        self.pilot_sc = scs if per_link else scs * n
        self.first = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(n)]
        self.cfo = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(n)]
        self.sym_metric = [torch.zeros(self.K + self.CP, dtype=torch.float32, device=dev) for _ in range(n)]
        self.phase_metric = [torch.zeros(self.S, dtype=torch.float32, device=dev) for _ in range(n)]
        nws = int(self.lib.dccn_capture_acquire_workspace_size(self.S, self.K, self.CP, self.n_pilot, self.J))
        self.ws = [torch.empty(nws, dtype=torch.uint8, device=dev) for _ in range(n)]
        self._table = (_lib.AcquireLink * n)()

    def run(self, caps, los=0):
        """Three launches on the current stream; returns ``self.first``."""
        n = self.n_links
        caps = [_device_capture(c, "CaptureAcquireGroup") for c in _per_link(list(caps), n, "CaptureAcquireGroup.run(caps)")]
        los = _per_link(los, n, "CaptureAcquireGroup.run(los)")
        for i, cap in enumerate(caps):
            self._table[i] = _lib.AcquireLink(cap.data_ptr(), int(cap.shape[0]), int(los[i]), self.pilot_sc[i].data_ptr(),
                                              self.first[i].data_ptr(), self.cfo[i].data_ptr(), self.sym_metric[i].data_ptr(),
                                              self.phase_metric[i].data_ptr(), self.ws[i].data_ptr(), int(self.ws[i].numel()))
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        check(self.lib.dccn_capture_acquire_grouped(n, self._table, self.J, self.S, self.K, self.CP, self.n_pilot, stream),
              "dccn_capture_acquire_grouped")
        return self.first
