"""Several equaliser transfer-learning chains trained in lock-step through ONE launch sequence.

The reference driver runs one (receiver -> equaliser) chain per modulation and per cp / longcp variant, each as an OS process
(dev/py/run_local_ofdm.py:61-118; the loop is dev/py/ofdmreceiver_np_mp.py:394-466).  On an MI355X such a chain is a sequence of
73-frame steps of ~21 dependent launches that keeps a few percent of the chip busy, and the host spends as long issuing a step
as the GPU spends running it.  Here G chains of the same shape share every launch (include/dccn.h "chain groups": the chain
index is a grid dimension): per group step ONE C call carries all G chains' batches -- the step, with the next batch's generator
riding on its bottleneck backward launch (``mobile`` chains: as the step's first launch) and the loop's monitors on its optimizer launch (three calls without those riders).  Every chain keeps its own seeds, draws, early stopping and best-model snapshot: the trained model of a chain
is bit for bit the one :func:`dl_ofdm_amd.receiver_mp.train` produces for it alone (tests/test_gpu_chain_groups.py).

    results = train_group([flags_bpsk, flags_qpsk, ...], [rx_params_bpsk, rx_params_qpsk, ...])

The deployed side of the same chains -- label-free receive calls for several links at once -- is :class:`ChainReceiveGroup`
(``dccn_eq_receive_step_grouped``), at the end of this module.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, epochs, ofdm
from . import receiver_mp as H
from ._lib import check, stream_ptr
from .arena import ChainArena, check_same_layout
from .receive import ReceiveResult, _GroupFrontEnd, _refuse_group_span
from .sync import group_size


def _ptr_array(structs):
    """a C array of pointers to the given ctypes structures (kept alive by the caller)"""
    arr = (C.c_void_p * len(structs))()
    for i, s in enumerate(structs):
        arr[i] = C.addressof(s)
    return arr


class _Chain:
    """one chain's state: what :func:`receiver_mp._train_on_device` keeps in local variables"""

    def __init__(self, FLAGS, rx_params, device, arena_bytes: int):
        from .datagen import DeviceDataGen, FusedStaticGen
        from .equalizer import EqualizerTrainer, _FusedPlan
        self.F = FLAGS
        self.o = ofdm.ofdm_tx(FLAGS)
        self.arena = ChainArena(arena_bytes, device)
        np.random.seed(FLAGS.seed)                                          # as receiver_mp.train does (nothing draws from it here)
        self.tr = EqualizerTrainer(FLAGS, self.o, rx_params, device=device, seed=FLAGS.seed, arena=self.arena).pin_tuning()
        self.B = FLAGS.batch_size // FLAGS.nsymbol
        self.steps = (FLAGS.msg_length // FLAGS.nsymbol) // self.B
        self.gen = DeviceDataGen(FLAGS, self.o, device=self.tr.device, seed=FLAGS.seed, mobile=FLAGS.mobile, mix=FLAGS.mobile)
        if not FusedStaticGen.supported(self.gen):
            raise _lib.DccnError("chain groups need the fused generator (N = 64 grid at CP = 16 or CP = 4, no align_window)")
        self.pl = _FusedPlan(self.tr, self.B, arena=self.arena)
        self.tr._plans[self.B] = self.pl
        self.ev = self.tr.resident(FLAGS.eval_frames)                      # evaluation runs per chain, outside the group
        self.loop = H.DeviceEpochLoop(FLAGS, self.o, self.tr, self.gen, self.pl, self.steps, arena=self.arena)
        if not (self.loop.pipeline and self.loop.virt is not None):
            raise _lib.DccnError("chain groups need the pipelined loop with the virtual next batch (dccn_eq_norm_rides)")
        self.best = epochs.BestSnapshot(os.path.join(FLAGS.save_dir, H.save_model_name(FLAGS)), FLAGS, H.save_checkpoint)
        self.rule, self.best_path, self.history = epochs.BestEpoch(FLAGS.early_stop), "", []
        self.epoch, self.done = 0, False
        self.rs = None
        self.monitors = [self.loop.monitor_of(q) for q in range(2)]

    # an epoch of receiver_mp._train_on_device around the group's steps: the same helpers (epochs.py), stepped from outside ------
    def begin_epoch(self):
        F = self.F
        self.rs = np.random.RandomState((F.seed + 1000003 * (self.epoch + 1)) & 0xFFFFFFFF)
        self.loop.begin_epoch(self.rs.choice(H.TRAIN_SNR_GRID, [self.steps, self.B], p=H.TRAIN_SNR_PROB))

    def end_epoch(self, verbose: bool):
        F = self.F
        a = self.loop.epoch_means()
        snr = self.rs.choice(H.TRAIN_SNR_GRID, [F.eval_frames], p=H.TRAIN_SNR_PROB)           # ofdmreceiver_np_mp.py:438
        em = epochs.eq_evaluate_on_device(F, self.tr, self.gen, self.ev, snr, self.loop.sync)
        self.history.append(epochs.eq_epoch_record(self.epoch, a, em, verbose, tag="[%s] " % F.token))
        improved, stop = self.rule.update(self.epoch, float(a[0]))
        if improved:
            self.best.take(self.tr)
        else:
            self.best.maybe_flush(self.tr)
        self.done = stop or self.epoch + 1 >= F.max_epoch_num
        self.epoch += 1

    def result(self) -> dict:
        return dict(history=self.history, best_path=self.best_path, trainer=self.tr)


def arena_bytes_for(FLAGS, lib=None) -> int:
    """a chain's arena: five parameter-sized arrays, the fused step's workspace, the folded receiver, the loop's buffers"""
    lib = lib or _lib.load()
    o = ofdm.ofdm_tx(FLAGS)
    B = FLAGS.batch_size // FLAGS.nsymbol
    shape = _lib.EqShape(B, FLAGS.nsymbol, o.K, o.CP, 1 if FLAGS.cp else 0, FLAGS.nfilter, o.frame_size, 4, o.pilot_size,
                         len(o.pilotCarriers))
    offs = (C.c_longlong * 21)()
    check(lib.dccn_eq_param_offsets(C.byref(shape), offs), "dccn_eq_param_offsets")
    steps = (FLAGS.msg_length // FLAGS.nsymbol) // B
    n = 5 * 4 * int(offs[20]) + int(lib.dccn_eq_workspace_size(C.byref(shape), 1)) + 4 * int(lib.dccn_eq_rx_folded_floats(C.byref(shape)))
    n += 4 * (2 * FLAGS.nsymbol * FLAGS.nfilter * 2 * o.frame_size + (o.K + o.CP) * 2 * FLAGS.nfilter) + 4096      # frozen receiver
    n += 12 * B * FLAGS.nsymbol * (o.K + o.CP) * 2 * 4          # inputs, outputs, generator frames, channel truth
    n += 2 * B * o.frame_size * 4 * 4 + steps * B * 4 + (1 << 20)
    return (n + (4 << 20)) // 256 * 256


class EqualizerChainGroup:
    def __init__(self, flags_list: Sequence, rx_params_list: Sequence[Dict[str, np.ndarray]], device="cuda"):
        self.lib = _lib.load()
        if not (1 <= len(flags_list) <= int(self.lib.dccn_chain_group_max())):
            raise ValueError("1..%d chains per group" % int(self.lib.dccn_chain_group_max()))
        if any(int(getattr(F, "sync", 0) or 0) > 0 for F in flags_list):
            # (a sync loop materialises every batch: no virtual next batch, no riding generator -- what a group step is built on)
            raise _lib.DccnError("chain groups do not take sync > 0: the aligned batch is materialised per chain "
                                 "(dccn_gen_static_apply_sync carries no chain table); train such chains with receiver_mp.train")
        nbytes = max(arena_bytes_for(F, self.lib) for F in flags_list)
        self.chains: List[_Chain] = [_Chain(F, rx, device, nbytes) for F, rx in zip(flags_list, rx_params_list)]
        check_same_layout([c.arena for c in self.chains])
        c0 = self.chains[0]
        for c in self.chains[1:]:
            if (c.B, c.steps) != (c0.B, c0.steps):
                raise ValueError("the chains of a group step through the same epoch schedule (batch_size, msg_length)")
        if not bool(self.lib.dccn_eq_group_supported(C.byref(c0.pl.shape))):
            raise _lib.DccnError("dccn_eq_group_supported: this batch shape has launches that cannot carry several chains")
        self.device = c0.tr.device
        self.hp = c0.tr.hp
        self._tables = {}

    # ---- one lock-step training step of the chains in `act` -------------------------------------------------------------------
    def _table(self, act: List[_Chain]):
        """pointer tables of an active set: [pipe code][q] -> (shapes, buffers), [q] -> monitors"""
        key = tuple(id(c) for c in act)
        t = self._tables.get(key)
        if t is None:
            t = dict(n=len(act),
                     shapes=[_ptr_array([c.loop.pls[q].shape for c in act]) for q in range(2)],
                     bufs={(pipe, q): _ptr_array([c.loop.pls[q].pipe_buffers[pipe] for c in act]) for pipe in range(4) for q in range(2)},
                     mon=[_ptr_array([c.monitors[q] for c in act]) for q in range(2)],
                     desc=_ptr_array([c.loop.fg.desc for c in act]),
                     x=[(C.c_void_p * len(act))(*[c.loop.pls[q].x.data_ptr() for c in act]) for q in range(2)],
                     npow=[(C.c_void_p * len(act))(*[c.loop.fg.npow[q].data_ptr() for c in act]) if act[0].loop.fg.npow is not None
                           else None for q in range(2)])
            self._tables[key] = t
        return t

    def _stream(self):
        return stream_ptr(self.device)

    def _generate(self, act, t, i: int, q: int, materialise: bool):
        """batch i of the epoch for every chain: ONE fused generator launch (+ one that forms x for an epoch's first batch) -- or
        none at all: the group step that normalises the batch produces it too (dccn_eq_buffers.gen_next_rides), the descriptors
        its buffers hold are armed here"""
        if not materialise and all(c.loop.ride_gen for c in act):
            for c in act:
                lp = c.loop
                lp.fg.arm(lp.pls[q].bits, q, None, lp.H[q], lp.snr_rows[i], into=lp.virt[q ^ 1])
            return
        for c in act:
            lp = c.loop
            lp.fg.arm(lp.pls[q].bits, q, None, lp.H[q], lp.snr_rows[i])                    # (advances the chain's gen.offset)
        st = self._stream()
        check(self.lib.dccn_gen_static_frames_grouped(t["n"], t["desc"], st), "dccn_gen_static_frames_grouped")
        if materialise:
            check(self.lib.dccn_gen_static_apply_grouped(t["n"], t["desc"], t["x"][q], t["npow"][q], st),
                  "dccn_gen_static_apply_grouped")

    def step(self, act: List[_Chain], i: int):
        t = self._table(act)
        steps = act[0].steps
        q = i & 1
        if i == 0:
            self._generate(act, t, 0, 0, True)
        if i + 1 < steps:
            self._generate(act, t, i + 1, q ^ 1, False)              # before step i: its optimizer launch normalises it
        last = i + 1 == steps
        pipe = (3 if last else 0) if i == 0 else (2 if last else 1)
        for c in act:                                                # (_FusedPlan.run's bookkeeping of the shared workspace)
            pl = c.loop.pls[q]
            pl._ahead()[pl.ws.data_ptr()] = pl._partner if pipe in (0, 1) else None
        st = self._stream()
        check(self.lib.dccn_eq_train_step_grouped(t["n"], t["shapes"][q], t["bufs"][(pipe, q)], self.hp, st),
              "dccn_eq_train_step_grouped")
        if not all(c.loop.mon is not None for c in act):             # (else the step's optimizer launch carried the monitors)
            check(self.lib.dccn_eq_monitor_accumulate_grouped(t["n"], t["mon"][q], st), "dccn_eq_monitor_accumulate_grouped")

    # ---- the epoch loop of receiver_mp._train_on_device for all chains ---------------------------------------------------------
    def train(self, verbose: bool = False) -> List[dict]:
        try:
            act = [c for c in self.chains if not c.done]
            while act:
                for c in act:
                    c.begin_epoch()
                for i in range(act[0].steps):
                    self.step(act, i)
                for c in act:
                    c.end_epoch(verbose)
                act = [c for c in act if not c.done]
        finally:
            for c in self.chains:
                c.best_path = c.best.flush(c.tr)                        # also on exceptions / KeyboardInterrupt
        return [c.result() for c in self.chains]


def train_group(flags_list: Sequence, rx_params_list: Sequence[Dict[str, np.ndarray]], device="cuda",
                verbose: bool = False) -> List[dict]:
    """:func:`dl_ofdm_amd.receiver_mp.train` (device_data; static or ``mobile`` channels) for several chains at once; returns one result dict
    per chain (history, best_path, trainer) -- the bits the per-chain function returns"""
    return EqualizerChainGroup(flags_list, rx_params_list, device=device).train(verbose=verbose)


# ---- the receive path of a group: several links' frames per launch sequence ---------------------------------------------------
def _eq_shape(FLAGS, o, batch: int, nbits: int) -> "_lib.EqShape":
    return _lib.EqShape(int(batch), FLAGS.nsymbol, o.K, o.CP, 1 if FLAGS.cp else 0, FLAGS.nfilter, o.frame_size, nbits, o.pilot_size,
                        len(o.pilotCarriers))


def receive_arena_bytes_for(FLAGS, batch: int, lib=None) -> int:
    """a receiving chain's arena: the trainer's five parameter-sized arrays, the fused step's workspace, the folded and the frozen
    receiver, one plan's inputs and outputs, and packed / llr / prob set aside for 16-QAM"""
    from .receive import row_bytes
    lib = lib or _lib.load()
    o = ofdm.ofdm_tx(FLAGS)
    B, S, D, n_sc = int(batch), FLAGS.nsymbol, o.frame_size, o.K + o.CP
    shape = _eq_shape(FLAGS, o, B, 4)
    offs = (C.c_longlong * 21)()
    check(lib.dccn_eq_param_offsets(C.byref(shape), offs), "dccn_eq_param_offsets")
    n = 5 * 4 * int(offs[20]) + int(lib.dccn_eq_workspace_size(C.byref(shape), 1)) + 4 * int(lib.dccn_eq_rx_folded_floats(C.byref(shape)))
    n += 4 * (2 * S * FLAGS.nfilter * 2 * D + n_sc * 2 * FLAGS.nfilter) + 4096      # frozen receiver
    n += 3 * B * S * n_sc * 2 * 4 + B * D * 4 * 4                                   # x, out_eq, chest; label buffer of the plan
    n += B * row_bytes(D, 4) + B * D * 4 * 4 + B * D * 4 * 2 * 4                    # packed, llr, prob
    return (n + (1 << 20)) // 256 * 256


class _ReceiveChain:
    """one link: its arena, the trainer that holds the chain's parameters, the resident plan and the receive outputs"""

    def __init__(self, FLAGS, rx_params, batch: int, device, arena_bytes: int, want_llr: bool, want_prob: bool):
        from .equalizer import EqualizerTrainer, _FusedPlan
        from .receive import row_bytes
        self.F = FLAGS
        self.o = ofdm.ofdm_tx(FLAGS)
        self.arena = ChainArena(arena_bytes, device)
        self.tr = EqualizerTrainer(FLAGS, self.o, rx_params, device=device, seed=int(getattr(FLAGS, "seed", 1)), arena=self.arena)
        self.pl = _FusedPlan(self.tr, batch, arena=self.arena)
        self.tr._plans[int(batch)] = self.pl
        B, D, nbits = int(batch), int(self.o.frame_size), int(FLAGS.nbits)
        self.D, self.nbits = D, nbits
        # set aside for 16-QAM whatever this chain's modulation (the arena layout must not depend on it); each chain's rows keep
        # their own length row_bytes(D, nbits)
        self.packed = self.arena.zeros(B, row_bytes(D, nbits), dtype=torch.uint8, reserve=B * row_bytes(D, 4))
        self.llr = self.arena.empty(B, D, nbits, dtype=torch.float32, reserve=B * D * 4) if want_llr else None
        self.prob = self.arena.empty(B, D, nbits, 2, dtype=torch.float32, reserve=B * D * 4 * 2) if want_prob else None

    def out(self, want_llr: bool, want_prob: bool) -> "_lib.ReceiveOut":
        return _lib.ReceiveOut(self.packed.data_ptr(), self.llr.data_ptr() if want_llr else None,
                               self.prob.data_ptr() if want_prob else None)


class ChainReceiveGroup:
    """Up to ``dccn_chain_group_max()`` (equaliser -> frozen receiver) chains of one shape and any mix of modulations whose
    receive steps share ONE launch sequence (``dccn_eq_receive_step_grouped``): a host that serves several links, each with its
    own trained chain, issues one call per round of frames.  Chain i's results are bit for bit what
    ``EqualizerTrainer.receive`` returns for it alone.

        group = ChainReceiveGroup([flags_bpsk, flags_16qam], [rx_bpsk, rx_16qam], batch=73, want_llr=True)
        receiver_mp.load_checkpoint(path, group.chains[0].tr)          # or .tr.load_params(...): the trained equaliser
        results = group.receive([frames_bpsk, frames_16qam])           # one ReceiveResult per chain
        results = group.receive(device_frames, sync=3, cfo=True)       # + one alignment launch for all chains
        results = group.receive_capture(captures, acquire=16, los=3)   # acquisition (3 launches) + cut (1) for all chains

    ``.chains[i].pl.out_eq`` / ``.chest`` / ``.snr_db`` hold what the chain's ``eval_step`` writes for the same frames."""

    _solo_call = "EqualizerTrainer.receive_capture"                     # the call that serves one link, for the refusals

    def __init__(self, flags_list: Sequence, rx_params_list: Sequence[Dict[str, np.ndarray]], batch: int, device="cuda",
                 want_llr: bool = False, want_prob: bool = False):
        self.lib = _lib.load()
        if group_size(self.lib, len(flags_list), "ChainReceiveGroup") != len(rx_params_list):
            raise ValueError("ChainReceiveGroup: one receiver per chain")
        self.batch = int(batch)
        F0 = flags_list[0]
        if len(flags_list) > 1 and not bool(self.lib.dccn_eq_receive_group_supported(
                C.byref(_eq_shape(F0, ofdm.ofdm_tx(F0), self.batch, int(F0.nbits))))):
            raise _lib.DccnError("dccn_eq_receive_group_supported: a receive step of %d frames of this shape has launches that "
                                 "cannot carry several chains (receive the links one by one)" % self.batch)
        nbytes = max(receive_arena_bytes_for(F, self.batch, self.lib) for F in flags_list)
        self.chains: List[_ReceiveChain] = [_ReceiveChain(F, rx, self.batch, device, nbytes, want_llr, want_prob)
                                            for F, rx in zip(flags_list, rx_params_list)]
        check_same_layout([c.arena for c in self.chains])
        self.device = self.chains[0].tr.device
        self._shapes = _ptr_array([c.pl.shape for c in self.chains])
        self._bufs = _ptr_array([c.pl.buffers for c in self.chains])
        self.want_llr, self.want_prob = bool(want_llr), bool(want_prob)
        self._outs = {}                                        # (llr, prob) asked for -> (the chains' dccn_receive_out, their table)
        o = self.chains[0].o
        self._front = _GroupFrontEnd(self, o.K, o.CP, [c.pl.x for c in self.chains], [c.o.pilotSc for c in self.chains])

    def _out_table(self, want_llr: bool, want_prob: bool):
        key = (want_llr, want_prob)
        if key not in self._outs:
            structs = [c.out(want_llr, want_prob) for c in self.chains]
            self._outs[key] = (structs, _ptr_array(structs))
        return self._outs[key][1]

    def _wants(self, want_llr: Optional[bool], want_prob: Optional[bool]):
        want_llr = self.want_llr if want_llr is None else bool(want_llr)
        want_prob = self.want_prob if want_prob is None else bool(want_prob)
        if (want_llr and not self.want_llr) or (want_prob and not self.want_prob):
            raise ValueError("llr / prob were not set aside when the group was built (want_llr / want_prob)")
        return want_llr, want_prob

    def _step(self, want_llr: bool, want_prob: bool) -> None:
        """the grouped receive step on what every chain's ``pl.x`` holds"""
        for c in self.chains:
            c.pl._ahead()[c.pl.ws.data_ptr()] = None           # (the step normalises into the chain's workspace)
        check(self.lib.dccn_eq_receive_step_grouped(len(self.chains), self._shapes, self._bufs, self._out_table(want_llr, want_prob),
                                                    stream_ptr(self.device)), "dccn_eq_receive_step_grouped")

    def receive(self, xs: Sequence, want_llr: Optional[bool] = None, want_prob: Optional[bool] = None, sync: int = 0,
                cfo: bool = False) -> list:
        """``xs[i]``: chain i's frames ``[batch, S, K + CP, 2]`` (host array or device tensor; ``None``: what ``.chains[i].pl.x``
        holds).  ``want_llr`` / ``want_prob``: as the group was built (default), or ``False`` to leave that output out of this
        call.  Returns one :class:`~dl_ofdm_amd.receive.ReceiveResult` per chain -- the chains' resident buffers: the next
        call overwrites them.

        ``sync = W > 0``: as ``EqualizerTrainer.receive(x, sync=W)`` per chain -- every ``xs[i]`` is a device tensor of frames
        that may sit up to ``W`` samples off the FFT window, and ONE alignment launch for all chains
        (:class:`~dl_ofdm_amd.sync.FrameSyncGroup`) writes each chain's rotated frames into its ``pl.x`` in place of the
        per-chain copies; ``result.offset``.  ``cfo=True`` (needs ``sync > 0``): that launch also takes each frame's
        carrier-frequency offset out; ``result.cfo``."""
        if len(xs) != len(self.chains):
            raise ValueError("one batch of frames per chain")
        want_llr, want_prob = self._wants(want_llr, want_prob)
        offsets, ests = self._front.frames(xs, sync, cfo)
        self._step(want_llr, want_prob)
        return [ReceiveResult(c.packed, c.llr if want_llr else None, c.prob if want_prob else None, c.D, c.nbits, offsets[i], ests[i])
                for i, c in enumerate(self.chains)]

    def receive_capture(self, caps: Sequence, firsts=None, strides=None, sync: int = 3, cfo: bool = False, acquire: int = 0, los=0,
                        want_llr: Optional[bool] = None, want_prob: Optional[bool] = None, cfo_scope: str = "frame",
                        cfo_span: int = 0) -> list:
        """One round on ``batch`` frames per chain that still sit inside contiguous captures: ``caps[i]`` is chain i's capture
        (device tensor ``float32 [n, 2]``; two chains may share one), as ``EqualizerTrainer.receive_capture(caps[i], firsts[i],
        strides[i], sync, cfo, frames=batch, lo=los[i])`` per chain.  ``firsts[i]``: an integer, or a device ``int64`` tensor of
        one element with ``los[i]``; the two mix.  ONE launch (:class:`~dl_ofdm_amd.sync.CaptureSyncGroup`) cuts every chain's
        frames at their estimated starts into its ``pl.x``, then the grouped step runs.

        ``firsts=None, acquire=J, los=...``: acquisition for all chains (:class:`~dl_ofdm_amd.sync.CaptureAcquireGroup`, three
        launches, the pilot cells are each chain's ``pilotSc``) leaves every chain's start inside ``[los[i], los[i] + T)`` on the
        device, where the cut reads it: four front-end launches for the whole group, no host round trip.  Each result carries
        ``offset``, ``cfo``, ``first`` and ``acquired_cfo`` as the solo call returns them.

        ``cfo=True, cfo_scope="capture"``: one carrier offset per chain's capture, pooled over its frames
        (``CaptureSyncGroup(..., cfo_scope="capture")``: three launches for all chains in place of the one).

        ``cfo_span > 0`` is refused (:class:`DccnError`): the grouped link tables carry no integer offset, so carrier offsets
        beyond half a subcarrier spacing go through the solo calls (``EqualizerTrainer.receive_capture(..., cfo_span=M)``)."""
        _refuse_group_span(self, cfo_span)
        want_llr, want_prob = self._wants(want_llr, want_prob)
        offsets, cfos, firsts, acq_cfo = self._front.capture(caps, firsts, strides, sync, cfo, acquire, los, cfo_scope)
        self._step(want_llr, want_prob)
        return [ReceiveResult(c.packed, c.llr if want_llr else None, c.prob if want_prob else None, c.D, c.nbits, offsets[i],
                              cfos[i], firsts[i], acq_cfo[i])
                for i, c in enumerate(self.chains)]
