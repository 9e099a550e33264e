"""What the training drivers share (receiver.train, receiver_mp.train on host and on device data, equalizer_group's chains):
the best-model snapshot, the best-epoch / early-stop rule, the host batch, the checkpoint file, and the equaliser's per-epoch
device evaluation and history record.  Plain helpers: each driver keeps its own epoch loop and calls them."""
from __future__ import annotations

import os
import time
from dataclasses import asdict
from typing import Dict

import numpy as np

from . import radio, tf_bundle, util


class BestSnapshot:
    """The best-train-loss model (ofdmreceiver_np.py:268-272, ofdmreceiver_np_mp.py:456-459), kept on the DEVICE: the reference
    calls ``saver.save`` every time the epoch loss improves; here an improvement is a device-to-device copy of the four arenas
    (28 MB for an equaliser: microseconds) and the file is written when training ends (also when it ends with an exception or
    Ctrl-C: the epoch loops flush in a ``finally``) -- and, checked once per epoch, every ``interval`` seconds in between, so a
    killed run loses at most that much plus one epoch.  Writing the file on every improvement is 25 blocking device-to-host copies
    and a 7 MB archive for a receiver -- hundreds of times per run, a third of a BPSK receiver's training time -- and 60 copies +
    a 21 MB archive for an equaliser, as much as half an epoch of training steps; and (chains training in threads of one process,
    config5.train_models) it is time spent holding the interpreter lock.  The file holds the same bytes either way.

    ``owner``: whatever holds ``params`` / ``adam_m`` / ``adam_v`` / ``adam_state`` (an RxEngine, an EqualizerTrainer), passed per
    call: receiver.train swaps engines as its batch grows, the arenas keep their size.  ``save(path, owner, FLAGS)``: the
    driver's ``save_checkpoint``."""
    NAMES = ("params", "adam_m", "adam_v", "adam_state")

    def __init__(self, path: str, FLAGS, save, interval: float = 60.0):
        self.path, self.FLAGS, self.save, self.interval = path, FLAGS, save, float(interval)
        self.bufs, self.dirty, self.written, self.t_last = None, False, False, time.time()

    def take(self, owner):
        import torch
        if self.bufs is None:
            self.bufs = {n: torch.empty_like(getattr(owner, n)) for n in self.NAMES}
        for n, b in self.bufs.items():
            b.copy_(getattr(owner, n))
        self.dirty = True
        self.maybe_flush(owner)

    def maybe_flush(self, owner):
        """call once per epoch, improved or not: a snapshot taken less than ``interval`` seconds after the last write is
        written by the first later epoch that finds the interval over"""
        if self.dirty and time.time() - self.t_last > self.interval:
            self.flush(owner)

    def flush(self, owner) -> str:
        """write the snapshot (not the owner's current state) to ``path``; the owner is left as it was"""
        if self.dirty:
            import torch
            with torch.no_grad():
                cur = {n: getattr(owner, n).clone() for n in self.NAMES}
                for n, b in self.bufs.items():
                    getattr(owner, n).copy_(b)
                self.save(self.path, owner, self.FLAGS)
                for n, c in cur.items():
                    getattr(owner, n).copy_(c)
            self.dirty, self.written, self.t_last = False, True, time.time()
        return self.path if self.written else ""


class BestEpoch:
    """train loss selects the checkpoint; ``early_stop`` epochs without a better one end the run (ofdmreceiver_np.py:268-274,
    ofdmreceiver_np_mp.py:456-466)"""

    def __init__(self, early_stop: int):
        self.early_stop, self.loss_min, self.epoch_min = int(early_stop), 100.0, 0

    def update(self, epoch: int, loss: float):
        """-> (improved: keep this epoch's model, stop: this was the run's last epoch)"""
        improved = loss < self.loss_min
        if improved:
            self.epoch_min, self.loss_min = epoch, loss
        return improved, epoch - self.early_stop > self.epoch_min


def make_batch(FLAGS, ofdmobj, fading, n_frames: int, snr_db):
    """bits -> OFDM frames -> fading -> AWGN on the host (ofdmreceiver_np.py:220-229, 73-79; ofdmreceiver_np_mp.py:405-413):
    frames, labels, the true channel response, the noise power"""
    ys = util.bit_source(FLAGS.nbits, ofdmobj.frame_size, n_frames)
    iq_cpx, _, _ = ofdmobj.ofdm_tx_frame_np(ys)
    xs, chan = fading.run(iq_cpx)
    snr = snr_db * np.ones((n_frames, 1)) if np.isscalar(snr_db) else snr_db
    xs, noise_pwr = radio.AWGN_channel_np(xs, snr)
    return xs.astype(np.float32), ys.astype(np.int32), chan, noise_pwr


# ---- the checkpoint file: <stem>.npz, next to it (on request / when trained by the reference) the tf.train.Saver bundle ---------
def _stem(path: str) -> str:
    return path[:-4] if path.endswith(".npz") else path


def write_checkpoint(path: str, out: Dict[str, np.ndarray], FLAGS, to_tf):
    """the state dict ``out`` + ``__flags__`` as <stem>.npz; ``FLAGS.tf_checkpoint``: also ``to_tf(out)`` in the reference's own
    format (<stem>.index/.data-00000-of-00001)"""
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    if getattr(FLAGS, "tf_checkpoint", False):
        tf_bundle.write_checkpoint(_stem(path), to_tf(out))
    out["__flags__"] = np.array(repr(asdict(FLAGS)))
    np.savez(_stem(path) + ".npz", **out)
    return path


def read_checkpoint(path: str, from_tf):
    """<stem>.npz, or -- when only the TensorFlow bundle <stem>.index/.data-* exists (a model trained by the reference) -- that,
    mapped by ``from_tf`` to this implementation's names and layouts"""
    stem = _stem(path)
    if not os.path.exists(stem + ".npz") and os.path.exists(stem + ".index"):
        return from_tf(tf_bundle.read_checkpoint(stem))
    z = np.load(stem + ".npz", allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- the equaliser's end of an epoch (ofdmreceiver_np_mp.py:430-455) ------------------------------------------------------------
def eq_evaluate_on_device(FLAGS, trainer, gen, ev, snr, sync: int) -> dict:
    """the per-epoch evaluation batch, drawn on the GPU into the resident plan ``ev`` (aligned when ``sync`` > 0), and its metrics"""
    if sync:
        gen.make_batch(FLAGS.eval_frames, snr, out_x=ev.x, out_bits=ev.bits, sync=sync)
    else:
        tx, _ = gen.transmit(FLAGS.eval_frames, out_bits=ev.bits)
        gen.channel(tx, snr, out_x=ev.x)
        gen.offset += 1
    ev.run(False)
    return trainer._metrics(ev.metrics_buf, ev.tx_power)


def eq_epoch_record(epoch: int, a, em: dict, verbose: bool, tag: str = "") -> dict:
    """the epoch's history record (printed when ``verbose``) from its training means ``a`` = [ce_mean, berlin, tx_power,
    noise_power, chan_rms] (DeviceEpochLoop.epoch_means) and the evaluation metrics ``em``"""
    if verbose:
        print("%sEpoch: %d  Train Loss: %f  Tx Power: %f  Noise Power: %f  SNR MSE: %f | Test Loss: %f  Test BER: %.8f"
              % (tag, epoch, a[0], a[2], a[3], a[4], em["ce_mean"], em["berlin"]))
    return dict(epoch=epoch, train_loss=float(a[0]), train_ber=float(a[1]), chan_rms=float(a[4]),
                test_loss=em["ce_mean"], test_ber=em["berlin"])
