"""dl_ofdm_amd/epochs.py, the pieces every training driver shares, without a GPU or the library: the best-model snapshot on CPU
tensors and stub owners, and the best-epoch / early-stop rule against the values the drivers' former inline rule gives."""
import pytest
import torch

from dl_ofdm_amd.epochs import BestEpoch, BestSnapshot

NAMES = ("params", "adam_m", "adam_v", "adam_state")


class Owner:
    """what a snapshot needs of an RxEngine or an EqualizerTrainer: the four arenas under these names"""

    def __init__(self, base: float):
        self.set(base)

    def set(self, base: float):
        for k, n in enumerate(NAMES):
            t = torch.arange(4 if n == "adam_state" else 37, dtype=torch.float32) * 0.25 + base + 100.0 * k
            if hasattr(self, n):
                getattr(self, n).copy_(t)
            else:
                setattr(self, n, t)

    def state(self):
        return {n: getattr(self, n).clone() for n in NAMES}


class Saver:
    """``save(path, owner, FLAGS)``: records what the owner held at the moment of the write"""

    def __init__(self):
        self.calls = []

    def __call__(self, path, owner, FLAGS):
        self.calls.append((path, owner, FLAGS, owner.state()))
        return path


def _same(a: dict, b: dict) -> bool:
    return all(torch.equal(a[n], b[n]) for n in NAMES)


def test_flush_before_any_take_writes_nothing():
    save = Saver()
    snap = BestSnapshot("ck/model", "flags", save)
    assert snap.flush(Owner(1.0)) == "" and save.calls == []
    snap.maybe_flush(Owner(1.0))
    assert save.calls == []


def test_file_holds_the_snapshot_and_the_owner_is_left_as_it_was():
    save, own = Saver(), Owner(1.0)
    A = own.state()
    snap = BestSnapshot("ck/model", "flags", save, interval=1e9)
    snap.take(own)
    assert save.calls == []                                   # a large interval: only flush writes
    own.set(7.0)
    B = own.state()
    assert not _same(A, B)
    assert snap.flush(own) == "ck/model"
    assert len(save.calls) == 1
    path, who, flags, seen = save.calls[0]
    assert (path, flags) == ("ck/model", "flags") and who is own
    assert _same(seen, A)                                     # all four arenas as they were at take()
    assert _same(own.state(), B)                              # ... and the owner holds B again, bit for bit
    assert snap.flush(own) == "ck/model" and len(save.calls) == 1      # nothing new to write; the path stays


def test_take_through_one_owner_and_flush_through_another_of_the_same_sizes():
    """receiver.train swaps engines as its batch grows: the snapshot outlives the engine it was taken from"""
    save, first, second = Saver(), Owner(1.0), Owner(9.0)
    A, B = first.state(), second.state()
    snap = BestSnapshot("ck/model", None, save, interval=1e9)
    snap.take(first)
    first.set(-3.0)                                           # (the released engine: whatever it holds now is not read)
    assert snap.flush(second) == "ck/model"
    assert save.calls[0][1] is second and _same(save.calls[0][3], A)
    assert _same(second.state(), B)


def test_interval_decides_when_take_writes():
    save, own = Saver(), Owner(2.0)
    A = own.state()
    snap = BestSnapshot("ck/model", None, save, interval=0)
    snap.t_last -= 1.0                                        # (the clock need not have moved since construction)
    snap.take(own)
    assert len(save.calls) == 1 and _same(save.calls[0][3], A)         # interval over: written at once
    late = BestSnapshot("ck/late", None, save, interval=1e9)
    late.take(own)
    late.maybe_flush(own)
    assert len(save.calls) == 1
    assert late.flush(own) == "ck/late" and len(save.calls) == 2


def _former_rule(losses, early_stop):
    """the rule as each driver had it inline: -> (kept epochs, epoch at which the loop broke or None)"""
    loss_min, epoch_min, kept = 100.0, 0, []
    for epoch, loss in enumerate(losses):
        if loss < loss_min:
            epoch_min, loss_min = epoch, loss
            kept.append(epoch)
        if epoch - early_stop > epoch_min:
            return kept, epoch
    return kept, None


@pytest.mark.parametrize("losses,early_stop,kept,stop_at", [
    ([3, 2, 2.5, 2.6, 2.7, 2.8, 1.0], 2, [0, 1], 4),
    ([100.0] * 4, 1, [], 2),                                  # a first loss of exactly 100.0 is not an improvement
    ([5, 4, 3, 2, 1], 0, [0, 1, 2, 3, 4], None),
])
def test_best_epoch_rule(losses, early_stop, kept, stop_at):
    assert _former_rule(losses, early_stop) == (kept, stop_at)
    rule, got, stopped = BestEpoch(early_stop), [], None
    assert (rule.loss_min, rule.epoch_min) == (100.0, 0)
    for epoch, loss in enumerate(losses):
        improved, stop = rule.update(epoch, loss)
        if improved:
            got.append(epoch)
        assert stop == (epoch - early_stop > rule.epoch_min)  # evaluated after the update
        if stop:
            stopped = epoch
            break
    assert (got, stopped) == (kept, stop_at)
    if kept:
        assert (rule.epoch_min, rule.loss_min) == (kept[-1], losses[kept[-1]])
