"""The label-free classical detector of the receive path: frames -> packed bits (and max-log LLRs) by the pilot-aided
LS / ALMMSE receivers of :mod:`dl_ofdm_amd.benchmark_gpu`, as ONE launch (``dccn_classical_receive``, include/dccn.h
"classical receive"; kernel: csrc/classical_receive.h).

What it has that the BER-curve tool (``ClassicalReceiverGPU.receive``) lacks: it needs no transmitted bits and no true SNR
(the noise variance is the mean power of the frame's own empty carriers), it returns the receive path's ``packed`` / ``llr``
(:class:`~dl_ofdm_amd.receive.ReceiveResult`), and nothing crosses HBM or the host between its stages.  It needs no training:
a fallback where the equaliser chain floors or was never trained, and the in-product baseline of that chain on real captures.

:class:`ClassicalRxReceiver` takes the front-end arguments of :class:`~dl_ofdm_amd.receive.RxReceiver` with the same meanings,
refusals and launch counts (the front end is that class's own code): the alignment / capture-cut stage writes whole symbols
straight into ``self.x`` and the classical launch stands where ``dccn_rx_receive_step`` stands.

:class:`ClassicalReceiveGroup` carries up to ``dccn_chain_group_max()`` links of one grid through ONE classical launch
(``dccn_classical_receive_grouped``), behind the grouped front end :class:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup` uses.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import ClassicalReceiveArgs, check, ptr, stream_ptr
from .receive import ReceiveResult, _FrontEnd, _GroupFrontEnd, _refuse_group_span, row_bytes
from .sync import _per_link, group_size

METHODS = {"ALMMSE": 2, "LS-Spline": 0, "LS-Linear": 0}      # -> dccn_classical_receive's mode


class ClassicalRxReceiver:
    """Fixed-shape classical receive engine on one GPU: ``receive(x)`` / ``receive_capture(cap, ...)`` ->
    :class:`~dl_ofdm_amd.receive.ReceiveResult` (``prob`` is ``None``).

    ``method``: ``"ALMMSE"``, ``"LS-Spline"`` or ``"LS-Linear"`` (the estimators that need neither the true channel nor a
    long-term profile).  ``advance``: the FFT window starts ``advance`` samples inside the prefix (``ClassicalReceiver``'s
    aligned window for a channel whose centre tap sits that far out), its phase ramp folded into the DFT matrix.
    ``noise_var``: the FFT-domain noise variance per cell (``K * 10**(-snr/10)`` on the generator's frames) when it is known;
    ``None``: estimated per frame from the empty carriers (``ofdm_tx.guardSc``).  ``interp``: any ``[S*K, P]`` interpolation
    matrix in place of the method's own.  Resident buffers: ``x``, ``packed``, ``llr`` (``want_llr``), ``chest``, ``noise``."""

    def __init__(self, FLAGS, batch: int, method: str = "ALMMSE", advance: int = 0, noise_var: Optional[float] = None,
                 interp=None, want_llr: bool = False, mapping: str = "table", device="cuda"):
        from .benchmark import ClassicalReceiver
        from .benchmark_gpu import _cexpand, linear_weights, spline_weights
        if method not in METHODS:
            raise ValueError("method must be one of %s: the other estimators need the true channel or a long-term profile"
                             % ", ".join(METHODS))
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DccnError("ClassicalRxReceiver needs a CUDA (ROCm) device; there is no CPU fallback")
        self.FLAGS, self.method, self.batch = FLAGS, method, int(batch)
        self.host = h = ClassicalReceiver(FLAGS, mapping=mapping)
        o = self.o = h.o
        S, K, CP = int(h.S), int(h.K), int(h.CP)
        self.S, self.K, self.CP, self.nbits = S, K, CP, int(h.nbits)
        self.advance = int(advance)
        if not (0 <= self.advance <= CP):
            raise ValueError("advance must lie in [0, CP = %d]: the FFT window starts inside the prefix" % CP)
        if noise_var is not None and not (np.isfinite(noise_var) and noise_var > 0):
            raise ValueError("noise_var must be finite and > 0 (None: estimated from the empty carriers)")
        self.noise_var = None if noise_var is None else float(noise_var)
        self.pilot_sc = np.asarray(o.pilotSc, dtype=np.int32).reshape(-1)
        self.P, self.D, self.E = len(h.pil), len(h.dat), len(o.guardSc)
        if not self.lib.dccn_classical_receive_supported(S, K, CP, self.P, self.D, self.E, self.nbits):
            raise _lib.DccnError("dccn_classical_receive_supported refused S=%d K=%d CP=%d P=%d D=%d E=%d nbits=%d"
                                 % (S, K, CP, self.P, self.D, self.E, self.nbits))
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.pil = torch.as_tensor(h.pil.astype(np.int32), **i32)
        self.dat = torch.as_tensor(h.dat.astype(np.int32), **i32)
        self.empty = torch.as_tensor(np.asarray(o.guardSc).astype(np.int32), **i32)
        self.table = torch.as_tensor(np.stack([h.table.real, h.table.imag], -1).astype(np.float32), **f32)
        self.labels = torch.as_tensor(np.ascontiguousarray(h.labels, dtype=np.int32), **i32)
        if interp is not None:
            Wm = torch.as_tensor(np.asarray(interp, dtype=np.float64) if not isinstance(interp, torch.Tensor) else interp)
            if tuple(Wm.shape) != (S * K, self.P):
                raise ValueError("interp must be [S*K, P] = [%d, %d]" % (S * K, self.P))
            self.w = Wm.to(self.device).T.contiguous().to(torch.float32)
        elif method == "LS-Linear":
            self.w = torch.as_tensor(np.ascontiguousarray(linear_weights(h.pil, S, K).T, dtype=np.float32), **f32)
        else:
            self.w = spline_weights(h.pil, S, K, self.device).T.contiguous().to(torch.float32)
        F = np.exp(-2j * np.pi * np.outer(np.arange(K), np.arange(K)) / K)                          # F[t, k]
        if self.advance > 0:
            F = F * np.exp(2j * np.pi * np.arange(K) * self.advance / K)[None, :]
        self.dft = torch.as_tensor(_cexpand(F).astype(np.float32), device=self.device)
        B = self.batch
        self.x = torch.zeros(B, S, K + CP, 2, **f32)
        self.packed = torch.zeros(B, row_bytes(self.D, self.nbits), dtype=torch.uint8, device=self.device)
        self.llr = torch.empty(B, self.D, self.nbits, **f32) if want_llr else None
        self.chest = torch.empty(B, S * K, 2, **f32)
        self.noise = torch.empty(B, **f32)
        self.y_freq = None
        self._front = _FrontEnd(type(self).__name__, self.device, self.x, CP, K, self.pilot_sc)    # (it writes whole symbols)
        pv = complex(h.pilot_value)
        self.args = ClassicalReceiveArgs(B, S, K, CP, self.P, self.D, self.E, self.nbits, int(self.table.shape[0]),
                                         CP - self.advance, METHODS[method], 0.0 if self.noise_var is None else self.noise_var,
                                         pv.real, pv.imag,
                                         *map(ptr, (self.dft, self.w, self.pil, self.dat, self.empty, self.table, self.labels,
                                                    self.x, self.packed, self.llr, self.chest, self.y_freq, self.noise)))

    def want_y_freq(self) -> torch.Tensor:
        """from now on the launch also writes the frequency-domain frames: the resident ``y_freq [batch, S*K, 2]``"""
        if self.y_freq is None:
            self.y_freq = torch.empty(self.batch, self.S * self.K, 2, dtype=torch.float32, device=self.device)
            self.args.y_freq = self.y_freq.data_ptr()
        return self.y_freq

    def close_graph(self):
        """(nothing captured: lets a :class:`~dl_ofdm_amd.session.Session` keep receivers next to its engines)"""

    def _detect(self, offset=None, est=None, first=None, est0=None, est_int=None) -> ReceiveResult:
        check(self.lib.dccn_classical_receive(C.byref(self.args), stream_ptr(self.device)), "dccn_classical_receive")
        return ReceiveResult(self.packed, self.llr, None, self.D, self.nbits, offset, est, first, est0, est_int)

    def receive(self, x=None, sync: int = 0, cfo: bool = False) -> ReceiveResult:
        """Stage ``x`` (``None``: whatever ``self.x`` holds; whole symbols ``[batch, S, K + CP, 2]``) and run the classical
        launch on the current stream.  ``sync = W > 0`` / ``cfo=True``: as :meth:`RxReceiver.receive` -- the alignment launch
        takes the place of the copy and writes the aligned frames straight into ``self.x``."""
        return self._detect(*self._front.frames(x, sync, cfo))

    def receive_capture(self, cap, first=None, stride: Optional[int] = None, sync: int = 3, cfo: bool = False, acquire: int = 0,
                        lo: int = 0, cfo_scope: str = "frame", cfo_span: int = 0, scale: Optional[float] = None) -> ReceiveResult:
        """The classical launch on ``batch`` frames that still sit inside one contiguous capture: every argument as
        :meth:`RxReceiver.receive_capture` takes it (acquisition, the cut at each frame's estimated start, per-frame or pooled
        carrier offset, offsets beyond half a spacing, int16 captures), with the same refusals and launch counts."""
        return self._detect(*self._front.capture(cap, first, stride, sync, cfo, acquire, lo, cfo_scope, cfo_span, scale))


GRID_FIELDS = ("S", "K", "CP", "P", "D", "E")                 # what dccn_classical_receive_grouped takes once for every link


class _HostGrid:
    """the grid a link's flags give, before any device work (what :class:`ClassicalRxReceiver` will find for them)"""

    def __init__(self, FLAGS):
        from . import ofdm
        o = ofdm.ofdm_tx(FLAGS)
        self.S, self.K, self.CP = int(o.nSymbol), int(o.K), int(o.CP)
        self.P, self.D, self.E = len(np.asarray(o.pilotSc)), len(np.asarray(o.dataSc)), len(o.guardSc)


def _same_grid(links) -> None:
    """the links of a group share the call's shape; the first field that differs is named"""
    for f in GRID_FIELDS:
        vals = [getattr(l, f) for l in links]
        if any(v != vals[0] for v in vals):
            raise ValueError("ClassicalReceiveGroup: every link must have the same %s (got %s); S, K, CP, P, D and E are the "
                             "call's, not a link's" % (f, vals))


class ClassicalReceiveGroup:
    """Up to ``dccn_chain_group_max()`` links of one grid ``(S, K, CP, P, D, E)`` and any mix of modulations, methods, window
    positions and noise sources whose classical detectors share ONE launch (``dccn_classical_receive_grouped``): a host that
    serves several links issues one call per round of frames.  Link i's results are bit for bit what ``.links[i]`` (a
    :class:`ClassicalRxReceiver`, usable on its own) returns for it alone.

        group = ClassicalReceiveGroup([flags_bpsk, flags_16qam], batch=73, methods=["LS-Spline", "ALMMSE"], want_llr=True)
        results = group.receive([frames_bpsk, frames_16qam])           # one ReceiveResult per link
        results = group.receive(device_frames, sync=3, cfo=True)       # + one alignment launch for all links
        results = group.receive_capture(captures, acquire=16, los=3)   # acquisition (3 launches) + cut (1) for all links

    ``methods`` / ``advances`` / ``noise_vars`` / ``interps``: one value for every link, or a list with one entry per link."""

    _solo_call = "ClassicalRxReceiver.receive_capture"                  # the call that serves one link, for the refusals

    def __init__(self, flags_list, batch: int, methods="ALMMSE", advances=0, noise_vars=None, interps=None,
                 want_llr: bool = False, device="cuda"):
        self.lib = _lib.load()
        n = group_size(self.lib, len(flags_list), "ClassicalReceiveGroup")
        # (an interpolation matrix is array-like itself: only a list or tuple of them is one entry per link)
        per = {k: _per_link(v, n, "ClassicalReceiveGroup(%s)" % k)
               for k, v in (("methods", methods), ("advances", advances), ("noise_vars", noise_vars), ("interps", interps))}
        _same_grid([_HostGrid(F) for F in flags_list])         # (before any engine is built: the refusal needs no device)
        self.batch = int(batch)
        self.links = [ClassicalRxReceiver(F, self.batch, method=per["methods"][i], advance=per["advances"][i],
                                          noise_var=per["noise_vars"][i], interp=per["interps"][i], want_llr=want_llr, device=device)
                      for i, F in enumerate(flags_list)]
        l = self.links[0]
        self.device = l.device
        self._front = _GroupFrontEnd(self, l.K, l.CP, [l.x for l in self.links], [l.pilot_sc for l in self.links])
        self._table, self._table_key = (_lib.ClassicalLink * n)(), None

    def want_y_freq(self) -> list:
        """from now on the launch also writes every link's frequency-domain frames (``.links[i].y_freq``)"""
        return [l.want_y_freq() for l in self.links]

    def _detect(self, offsets, ests, firsts=None, acq_cfo=None) -> list:
        """the one classical launch on what every link's ``x`` holds.  The table restates the links' own argument blocks, and is
        rebuilt only when one of them has changed (``links[i].want_y_freq()`` since the last call, say)"""
        key = b"".join(bytes(l.args) for l in self.links)
        if key != self._table_key:
            for i, l in enumerate(self.links):
                a = l.args
                self._table[i] = _lib.ClassicalLink(a.nbits, a.m, a.mode, a.win, a.noise_var, a.pv_re, a.pv_im, a.dft, a.w, a.pil,
                                                    a.dat, a.empty, a.table, a.labels, a.x, a.packed, a.llr, a.chest, a.y_freq, a.noise)
            self._table_key = key
        l = self.links[0]
        check(self.lib.dccn_classical_receive_grouped(len(self.links), self._table, self.batch, l.S, l.K, l.CP, l.P, l.D, l.E,
                                                      stream_ptr(self.device)), "dccn_classical_receive_grouped")
        none = [None] * len(self.links)
        firsts, acq_cfo = firsts or none, acq_cfo or none
        return [ReceiveResult(l.packed, l.llr, None, l.D, l.nbits, offsets[i], ests[i], firsts[i], acq_cfo[i])
                for i, l in enumerate(self.links)]

    def receive(self, xs, sync: int = 0, cfo: bool = False) -> list:
        """``xs[i]``: link i's frames ``[batch, S, K + CP, 2]`` (host array or device tensor; ``None``: what ``.links[i].x``
        holds): the per-link copies, then ONE classical launch.  ``sync = W > 0`` / ``cfo=True``: as
        :meth:`ClassicalRxReceiver.receive` per link -- every ``xs[i]`` is a device tensor, and ONE alignment launch for all links
        (:class:`~dl_ofdm_amd.sync.FrameSyncGroup`) writes each link's frames into its ``x`` in place of the copies.  One
        :class:`~dl_ofdm_amd.receive.ReceiveResult` per link (``prob`` is ``None``; the links' resident buffers)."""
        if len(xs) != len(self.links):
            raise ValueError("one batch of frames per link")
        return self._detect(*self._front.frames(xs, sync, cfo))

    def receive_capture(self, caps, firsts=None, strides=None, sync: int = 3, cfo: bool = False, acquire: int = 0, los=0,
                        cfo_scope: str = "frame", cfo_span: int = 0) -> list:
        """One round on ``batch`` frames per link that still sit inside contiguous captures, with the meanings and refusals of
        :meth:`~dl_ofdm_amd.equalizer_group.ChainReceiveGroup.receive_capture`: acquisition for all links (``firsts=None,
        acquire=J``: three launches, each link's own ``pilotSc``), the cut for all links (one launch; three with
        ``cfo_scope="capture"``), then the ONE classical launch.  ``firsts[i]``: an integer, or a device ``int64`` tensor of one
        element with ``los[i]``; the two mix.  ``cfo_span > 0`` and int16 captures are refused (:class:`DccnError`): the
        grouped front end is float32-only and has no wide variant -- those go through ``.links[i].receive_capture``."""
        _refuse_group_span(self, cfo_span)
        return self._detect(*self._front.capture(caps, firsts, strides, sync, cfo, acquire, los, cfo_scope))
