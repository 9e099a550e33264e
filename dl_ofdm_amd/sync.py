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
from ._lib import DccnError, check, ptr, stream_ptr


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
    return _checked_capture(cap, scale, what, cfo_span)


def _on_device(t) -> bool:
    return isinstance(t, torch.Tensor) and t.device.type == "cuda"


def _checked_capture(cap, scale, what: str, cfo_span: int = 0, float32_only: bool = False):
    """:func:`capture_format`, the one statement of what a capture is; ``float32_only``: for the group classes, whose entries
    read no int16"""
    if not _on_device(cap):
        raise DccnError("%s takes a device tensor; there is no CPU fallback" % what)
    dtypes = (torch.float32,) if float32_only else (torch.float32, torch.int16)
    if cap.dtype not in dtypes or cap.dim() != 2 or cap.shape[1] != 2 or not cap.is_contiguous():
        raise DccnError("%s: cap must be a contiguous float32 [n, 2]%s tensor, got %s %r"
                        % (what, "" if float32_only else " or int16 [n, 2]", cap.dtype, tuple(cap.shape)))
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


def resident_stage(cache: dict, cls, *args):
    """The stage ``cls(*args)``, built on first use and kept in ``cache`` from then on: the key is the class and the constructor
    arguments themselves (hashable ones: pilot cells as tuples).  Positional only: every receive call comes through here, and a
    lookup is then one small tuple and one dictionary access."""
    key = (cls, args)
    stage = cache.get(key)
    if stage is None:
        stage = cache[key] = cls(*args)
    return stage


def group_size(lib, n_links: int, what: str) -> int:
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


def _checked_frames(x, want: tuple, what: str) -> torch.Tensor:
    if not _on_device(x):
        raise DccnError("%s takes a device tensor; there is no CPU fallback" % what)
    if x.dtype != torch.float32 or tuple(x.shape) != want or not x.is_contiguous():
        raise DccnError("%s: x must be a contiguous float32 %r tensor, got %s %r" % (what, want, x.dtype, tuple(x.shape)))
    return x


def _start(first, lo, cap: torch.Tensor, what: str) -> tuple:
    """The start of a cut as every call and link table states it, ``(first, first_dev, lo)``: an integer ``first``, or a device
    tensor (where :class:`CaptureAcquire` left it: nothing is read back) with the origin of the range it lies in."""
    if not isinstance(first, torch.Tensor):
        return int(first), None, 0
    if lo is None:
        raise DccnError("%s: a device tensor `first` needs its lo, the origin of the range [lo, lo + T) it lies in" % what)
    if first.device != cap.device or first.dtype != torch.int64 or first.numel() != 1 or not first.is_contiguous():
        raise DccnError("%s: a device `first` must be an int64 tensor of one element on the capture's device" % what)
    return 0, first.data_ptr(), int(lo)


class _Stage:
    """What every stage of this module is built on, stated once: the library handle, the device refusal, the frame shape, the
    ``*_supported`` refusal and the resident tensors.  A group (``n_links`` given) keeps a list with one tensor per link where a
    solo stage keeps the tensor."""

    def __init__(self, S, K, CP, device, n_links=None):
        self.lib = _lib.load()
        name = type(self).__name__
        if n_links is not None:
            self.n_links = group_size(self.lib, n_links, name)
        self._solo = n_links is None
        self.S, self.K, self.CP = int(S), int(K), int(CP)
        self.T = self.S * (self.K + self.CP)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DccnError("%s needs a CUDA (ROCm) device; there is no CPU fallback" % name)

    def _require(self, query: str, needs: str, **shape) -> None:
        if not getattr(self.lib, query)(*shape.values()):
            raise DccnError("%s refused %s (needs %s)" % (query, " ".join("%s=%d" % kv for kv in shape.items()), needs))

    def _resident(self, *shape, dtype=torch.float32, make=torch.zeros):
        if self._solo:
            return make(*shape, dtype=dtype, device=self.device)
        return [make(*shape, dtype=dtype, device=self.device) for _ in range(self.n_links)]

    def _stream(self):
        return stream_ptr(self.device)


def _link_ptr(tensors, i: int):
    """link i's pointer of a per-link list the stage may have been built without"""
    return None if tensors is None else tensors[i].data_ptr()


ALIGN_NEEDS = "1 <= W <= CP, 2 W + CP <= 64, an even frame length"
CUT_NEEDS = ALIGN_NEEDS + ", four windows of T + 2 W samples within 64 KB"


class _SyncStage(_Stage):
    """the alignment and cut stages: the window, the frame count, resident ``offset`` / ``metric`` / ``cfo`` and the checked
    destination"""

    def __init__(self, query, needs, S, K, CP, W, frames, device, out_kin, want_metric, cfo, n_links=None, cfo_len=None):
        super().__init__(S, K, CP, device, n_links)
        self.W, self.frames = int(W), int(frames)
        self.out_kin = self.K + self.CP if out_kin is None else int(out_kin)
        self._require(query, needs, S=self.S, K=self.K, CP=self.CP, W=self.W)
        if self.out_kin not in (self.K + self.CP, self.K) or self.frames <= 0:
            raise DccnError("%s: out_kin must be K + CP or K and frames positive (got out_kin=%d, frames=%d)"
                            % (type(self).__name__, self.out_kin, self.frames))
        self.offset = self._resident(self.frames, dtype=torch.int32)
        self.metric = self._resident(self.frames, 2 * self.W + 1) if want_metric else None
        self.cfo = self._resident(self.frames if cfo_len is None else cfo_len) if cfo else None
        self.out = None         # allocated by the first run() that is not given a destination

    def _dest(self, out, device, what: str):
        """where ``run`` writes: this stage's own buffer(s), allocated on first use, or the caller's ``out``, checked -- per link
        in a group.  ``device``: the input's."""
        want = (self.frames, self.S, self.out_kin, 2)
        if out is None:
            if self.out is None:
                self.out = self._resident(*want, make=torch.empty)
            return self.out
        outs = [out] if self._solo else _per_link(list(out), self.n_links, what + "(outs)")
        for o in outs:
            if not _on_device(o) or o.device != device or o.dtype != torch.float32 or tuple(o.shape) != want or not o.is_contiguous():
                raise DccnError("%s: out must be a contiguous float32 %r tensor on %s" % (what, want, device))
        return out if self._solo else outs


class FrameSync(_SyncStage):
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
        super().__init__("dccn_frame_sync_supported", ALIGN_NEEDS, S, K, CP, W, frames, device, out_kin, want_metric, cfo)

    def _launch(self, x, out, write: bool):
        """the one launch: ``dccn_frame_sync``, or ``dccn_frame_sync_cfo`` of a stage built with ``cfo=True``"""
        x = _checked_frames(x, (self.frames, self.S, self.K + self.CP, 2), "FrameSync.run")
        out = self._dest(out, x.device, "FrameSync.run") if write else None
        entry = "dccn_frame_sync" if self.cfo is None else "dccn_frame_sync_cfo"
        check(getattr(self.lib, entry)(x.data_ptr(), self.frames, self.S, self.K, self.CP, self.W, self.out_kin, ptr(out),
                                       self.offset.data_ptr(), *(() if self.cfo is None else (self.cfo.data_ptr(),)),
                                       ptr(self.metric), self._stream()), entry)
        return out

    def run(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Estimate every frame's offset and write the aligned frames to ``out`` (``None``: this object's own buffer), on the
        current stream.  ``out`` must not overlap ``x``."""
        return self._launch(x, out, True), self.offset

    def offsets(self, x: torch.Tensor) -> torch.Tensor:
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(x, None, False)
        return self.offset


# (pooled, cfo_span > 0, int16 capture, start on the device; None: either) -> the entry, and which of the start fields
# (first, first_dev, lo) it takes.  Every argument list is regular (include/dccn.h):
#   cap, n_samples, [scale], start, stride, frames, S, K, CP, W, out_kin, x_out, offset, cfo, metric, [cfo_int_dev, cfo_frac_dev],
#   [workspace, workspace_bytes], stream
_CUT_ROWS = (
    (False, False, False, False, "dccn_capture_sync", slice(0, 1)),
    (False, False, False, True, "dccn_capture_sync_at", slice(1, 3)),
    (False, True, False, True, "dccn_capture_sync_wide", slice(1, 3)),      # (the integer is only known through acquisition)
    (False, False, True, None, "dccn_capture_sync_sc16", slice(0, 3)),
    (True, False, False, None, "dccn_capture_sync_pooled", slice(0, 3)),
    (True, True, False, None, "dccn_capture_sync_pooled_wide", slice(0, 3)),
    (True, False, True, None, "dccn_capture_sync_pooled_sc16", slice(0, 3)),
)
CUT_ENTRIES = {(pooled, wide, sc16, on_dev): (entry, fields) for pooled, wide, sc16, either, entry, fields in _CUT_ROWS
               for on_dev in ((False, True) if either is None else (either,))}


class CaptureSync(_SyncStage):
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
        self.cfo_span = int(cfo_span)
        if self.cfo_span and not cfo:
            raise DccnError("CaptureSync(cfo_span=M > 0) needs cfo=True: there is no carrier offset to unwrap without it")
        if not (0 <= self.cfo_span <= max(int(K) // 2 - 1, 0)):
            raise DccnError("CaptureSync: cfo_span must lie in [0, K / 2 - 1], got %d at K=%d" % (self.cfo_span, int(K)))
        super().__init__("dccn_capture_sync_supported", CUT_NEEDS, S, K, CP, W, frames, device, out_kin, want_metric, cfo,
                         cfo_len=1 if self.pooled else None)
        self.ws = None
        if self.pooled:
            size = (self.lib.dccn_capture_sync_pooled_wide_workspace_size if self.cfo_span
                    else self.lib.dccn_capture_sync_pooled_workspace_size)
            self.ws = self._resident(int(size(self.frames)), dtype=torch.uint8, make=torch.empty)

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

    def _launch(self, cap, first, stride, out, write: bool, lo, acquired, scale):
        """the one call: the entry of :data:`CUT_ENTRIES` (one launch; the pooled ones estimate, sum and cut: three)"""
        sc16, scale = _checked_capture(cap, scale, "CaptureSync", self.cfo_span)
        pair = self._acquired_pair(acquired, cap)
        start = _start(first, lo, cap, "CaptureSync")
        if self.pooled and not write:
            raise DccnError('CaptureSync(cfo_scope="capture") has no offsets-only call: the pooled entry writes the frames')
        row = CUT_ENTRIES.get((self.pooled, bool(pair), sc16, start[1] is not None))
        if row is None:
            raise DccnError("CaptureSync(cfo_span=M > 0): the per-frame cut reads the start where acquisition left it, a device "
                            "tensor `first` with lo=...")
        out = self._dest(out, cap.device, "CaptureSync.run") if write else None
        entry, fields = row
        check(getattr(self.lib, entry)(cap.data_ptr(), int(cap.shape[0]), *((scale,) if sc16 else ()), *start[fields],
                                       self.T if stride is None else int(stride), self.frames, self.S, self.K, self.CP, self.W,
                                       self.out_kin, ptr(out), self.offset.data_ptr(), ptr(self.cfo), ptr(self.metric), *pair,
                                       *(() if self.ws is None else (self.ws.data_ptr(), int(self.ws.numel()))), self._stream()),
              entry)
        return out

    def run(self, cap: torch.Tensor, first, stride: Optional[int] = None, out: Optional[torch.Tensor] = None,
            lo: Optional[int] = None, acquired=None, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Estimate every frame's offset and write the frames, cut at their estimated starts (and with ``cfo=True`` derotated),
        to ``out`` (``None``: this object's own buffer), on the current stream.  ``out`` must not overlap ``cap``.

        ``first``: an integer, or a device ``int64`` tensor of one element together with ``lo`` (``dccn_capture_sync_at``: the
        launch reads the start from device memory and keeps it inside ``[lo, lo + T - 1]``; every window must lie inside the
        capture for every start in that range).  ``acquired``: the pair of a stage built with ``cfo_span = M > 0``.
        ``scale``: the value of one count of an ``int16`` capture (``None``: ``2**-15``); not given with a float32 capture."""
        return self._launch(cap, first, stride, out, True, lo, acquired, scale), self.offset

    def offsets(self, cap: torch.Tensor, first, stride: Optional[int] = None, lo: Optional[int] = None, acquired=None,
                scale: Optional[float] = None) -> torch.Tensor:
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``.  ``first`` / ``lo`` / ``acquired`` /
        ``scale`` as :meth:`run`."""
        self._launch(cap, first, stride, None, False, lo, acquired, scale)
        return self.offset


class _AcquireStage(_Stage):
    """the acquisition stages: the pilot cells (per link in a group, of one length), the ``*_supported`` refusals, resident
    ``first`` / ``cfo`` / ``sym_metric`` / ``phase_metric`` and the workspace"""

    def __init__(self, S, K, CP, pilot_sc, J, device, n_links=None, cfo_span=0):
        super().__init__(S, K, CP, device, n_links)
        self.J, self.cfo_span = int(J), int(cfo_span)
        per_link = (not self._solo and isinstance(pilot_sc, (list, tuple)) and len(pilot_sc) > 0
                    and hasattr(pilot_sc[0], "__len__"))
        scs = [torch.as_tensor(sc).reshape(-1).to(torch.int32)
               for sc in (_per_link(list(pilot_sc), self.n_links, "pilot_sc") if per_link else [pilot_sc])]
        self.n_pilot = int(scs[0].numel())
        if any(int(sc.numel()) != self.n_pilot for sc in scs):
            raise DccnError("%s: the links' pilot cells must be of one length (n_pilot is the call's)" % type(self).__name__)
        shape, M = dict(S=self.S, K=self.K, CP=self.CP, n_pilot=self.n_pilot, J=self.J), self.cfo_span
        self._require("dccn_capture_acquire_supported", "S <= 64, CP <= K, K + CP <= 1024, 2 <= n_pilot <= 256, 1 <= J <= 256",
                      **shape)
        if M:
            self._require("dccn_capture_acquire_wide_supported", "0 <= cfo_span <= K / 2 - 1", **shape, cfo_span=M)
        scs = [sc.to(self.device).contiguous() for sc in scs]
        self.pilot_sc = scs[0] if self._solo else (scs if per_link else scs * self.n_links)
        self.first = self._resident(1, dtype=torch.int64)
        self.cfo = self._resident(1)
        self.sym_metric = self._resident(self.K + self.CP)
        self.phase_metric = self._resident(self.S, 2 * M + 1) if M else self._resident(self.S)
        size = self.lib.dccn_capture_acquire_wide_workspace_size if M else self.lib.dccn_capture_acquire_workspace_size
        self.ws = self._resident(int(size(*shape.values(), *((M,) if M else ()))), dtype=torch.uint8, make=torch.empty)


class CaptureAcquire(_AcquireStage):
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
        super().__init__(S, K, CP, pilot_sc, J, device, cfo_span=cfo_span)
        self.cfo_int = self._resident(1, dtype=torch.int32)

    def run(self, cap: torch.Tensor, lo: int = 0, scale: Optional[float] = None) -> torch.Tensor:
        """Three launches on the current stream; returns ``self.first``.  ``scale``: the value of one count of an ``int16``
        capture (``None``: ``2**-15``); not given with a float32 capture."""
        sc16, scale = _checked_capture(cap, scale, "CaptureAcquire", self.cfo_span)
        M = self.cfo_span
        entry = "dccn_capture_acquire" + ("_sc16" if sc16 else "_wide" if M else "")
        check(getattr(self.lib, entry)(cap.data_ptr(), int(cap.shape[0]), *((scale,) if sc16 else ()), int(lo), self.J, self.S,
                                       self.K, self.CP, self.pilot_sc.data_ptr(), self.n_pilot, *((M,) if M else ()),
                                       self.first.data_ptr(), self.cfo.data_ptr(), *((self.cfo_int.data_ptr(),) if M else ()),
                                       self.sym_metric.data_ptr(), self.phase_metric.data_ptr(), self.ws.data_ptr(),
                                       int(self.ws.numel()), self._stream()), entry)
        return self.first


# ---- the same stages for several links per launch (include/dccn.h "the receive front end for several links") -------------------
class FrameSyncGroup(_SyncStage):
    """:class:`FrameSync` for up to ``dccn_chain_group_max()`` links in ONE launch (``dccn_frame_sync_grouped``):
    ``run(xs) -> (aligned, offsets)``, lists with one entry per link, entry i bit for bit what ``FrameSync.run(xs[i])`` gives.
    ``offset``, ``metric``, ``cfo`` and the output buffers are resident per link (lists of tensors)."""

    def __init__(self, S: int, K: int, CP: int, W: int, frames: int, n_links: int, device="cuda", out_kin: Optional[int] = None,
                 want_metric: bool = True, cfo: bool = False):
        super().__init__("dccn_frame_sync_supported", ALIGN_NEEDS, S, K, CP, W, frames, device, out_kin, want_metric, cfo, n_links)
        self._table = (_lib.FrameLink * self.n_links)()

    def _launch(self, xs, outs, write: bool):
        what, want = "FrameSyncGroup.run", (self.frames, self.S, self.K + self.CP, 2)
        xs = [_checked_frames(x, want, what) for x in _per_link(list(xs), self.n_links, what + "(xs)")]
        outs = self._dest(outs, xs[0].device, what) if write else None
        for i, x in enumerate(xs):
            self._table[i] = _lib.FrameLink(x.data_ptr(), _link_ptr(outs, i), self.offset[i].data_ptr(), _link_ptr(self.cfo, i),
                                            _link_ptr(self.metric, i))
        check(self.lib.dccn_frame_sync_grouped(self.n_links, self._table, self.frames, self.S, self.K, self.CP, self.W,
                                               self.out_kin, self._stream()), "dccn_frame_sync_grouped")
        return outs

    def run(self, xs, outs=None):
        """One launch on the current stream.  ``outs``: one destination per link (``None``: this object's own buffers); no
        destination may overlap another link's frames or outputs."""
        return self._launch(xs, outs, True), self.offset

    def offsets(self, xs):
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(xs, None, False)
        return self.offset


class CaptureSyncGroup(_SyncStage):
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
        super().__init__("dccn_capture_sync_supported", CUT_NEEDS, S, K, CP, W, frames, device, out_kin, want_metric, cfo, n_links,
                         cfo_len=1 if self.pooled else None)
        self._table = ((_lib.PooledLink if self.pooled else _lib.CaptureLink) * self.n_links)()
        self.ws = None
        if self.pooled:
            self.ws = self._resident(int(self.lib.dccn_capture_sync_pooled_workspace_size(self.frames)), dtype=torch.uint8,
                                     make=torch.empty)

    def _launch(self, caps, firsts, strides, outs, write: bool, los):
        n, what = self.n_links, "CaptureSyncGroup"
        caps = _link_captures(caps, n, what)
        firsts = _per_link(list(firsts), n, what + ".run(firsts)")
        strides = _per_link(strides, n, what + ".run(strides)")
        los = _per_link(los, n, what + ".run(los)")
        starts = [_start(first, lo, cap, what) for first, lo, cap in zip(firsts, los, caps)]
        if self.pooled and not write:
            raise DccnError('CaptureSyncGroup(cfo_scope="capture") has no offsets-only call: the pooled entry writes the frames')
        outs = self._dest(outs, caps[0].device, what + ".run") if write else None
        for i, cap in enumerate(caps):
            link = (cap.data_ptr(), int(cap.shape[0]), *starts[i], self.T if strides[i] is None else int(strides[i]),
                    _link_ptr(outs, i), self.offset[i].data_ptr(), _link_ptr(self.cfo, i), _link_ptr(self.metric, i))
            if self.pooled:
                self._table[i] = _lib.PooledLink(*link, self.ws[i].data_ptr(), int(self.ws[i].numel()))
            else:
                self._table[i] = _lib.CaptureLink(*link)
        entry = "dccn_capture_sync_pooled_grouped" if self.pooled else "dccn_capture_sync_grouped"
        check(getattr(self.lib, entry)(n, self._table, self.frames, self.S, self.K, self.CP, self.W, self.out_kin, self._stream()),
              entry)
        return outs

    def run(self, caps, firsts, strides=None, outs=None, los=None):
        """One launch on the current stream.  ``strides`` / ``los``: one value for every link or one per link."""
        return self._launch(caps, firsts, strides, outs, True, los), self.offset

    def offsets(self, caps, firsts, strides=None, los=None):
        """The offsets alone (no frame is written); with ``cfo=True`` also ``self.cfo``."""
        self._launch(caps, firsts, strides, None, False, los)
        return self.offset


def _link_captures(caps, n: int, what: str) -> list:
    """one float32 capture per link (two links may share one)"""
    caps = _per_link(list(caps), n, what + ".run(caps)")
    for cap in caps:
        _checked_capture(cap, None, what, float32_only=True)
    return caps


class CaptureAcquireGroup(_AcquireStage):
    """:class:`CaptureAcquire` for up to ``dccn_chain_group_max()`` links in THREE launches (``dccn_capture_acquire_grouped``):
    ``run(caps, los) -> firsts``, one device ``int64`` tensor of one element per link -- what :meth:`CaptureSyncGroup.run` takes
    as ``firsts`` together with the same ``los``.  ``pilot_sc``: the pilot cells of every link, or a list of one array per link
    (of one length).  ``first``, ``cfo``, ``sym_metric``, ``phase_metric`` and the workspaces are resident per link (lists)."""

    def __init__(self, S: int, K: int, CP: int, pilot_sc, J: int, n_links: int, device="cuda"):
        super().__init__(S, K, CP, pilot_sc, J, device, n_links)
        self._table = (_lib.AcquireLink * self.n_links)()

    def run(self, caps, los=0):
        """Three launches on the current stream; returns ``self.first``."""
        n = self.n_links
        caps = _link_captures(caps, n, "CaptureAcquireGroup")
        los = _per_link(los, n, "CaptureAcquireGroup.run(los)")
        for i, cap in enumerate(caps):
            self._table[i] = _lib.AcquireLink(cap.data_ptr(), int(cap.shape[0]), int(los[i]), self.pilot_sc[i].data_ptr(),
                                              self.first[i].data_ptr(), self.cfo[i].data_ptr(), self.sym_metric[i].data_ptr(),
                                              self.phase_metric[i].data_ptr(), self.ws[i].data_ptr(), int(self.ws[i].numel()))
        check(self.lib.dccn_capture_acquire_grouped(n, self._table, self.J, self.S, self.K, self.CP, self.n_pilot, self._stream()),
              "dccn_capture_acquire_grouped")
        return self.first
