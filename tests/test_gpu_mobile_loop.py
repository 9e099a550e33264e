"""The reference driver's default workload -- every chain trains with ``mobile = 'True'``, i.e. on mixRayleigh with a Jakes-Doppler
frame in every third slot (dev/py/run_local_ofdm.py:41,101; ofdmreceiver_np_mp.py:389-411) -- on the fused training loop: the
one-launch generator, the virtual next batch, the generator issued by the step itself, and chain groups (``-m gpu``)."""
import pytest
import torch

from test_gpu_chain_groups import _flags, _rx, _state

pytestmark = pytest.mark.gpu
NAMES = ("params", "adam_m", "adam_v", "adam_state", "grads")


def test_mobile_loop_trains_the_same_equaliser_under_every_generator_setting(tmp_path, monkeypatch):
    """receiver_mp.train on mixRayleigh with mobile=True, two epochs of five 73-frame steps: the default loop (the step issues the
    Doppler generator launch of the next batch itself and reads it as its virtual input), generator_rides=False (the loop
    issues that launch) and virtual_next=False (every batch materialised by dccn_gen_static_apply) draw the same batches and
    form the same x bits -- identical arenas and histories -- and each of them took the fused generator."""
    from dl_ofdm_amd import receiver_mp as H
    loops = []

    class Recording(H.DeviceEpochLoop):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            loops.append(self)
    monkeypatch.setattr(H, "DeviceEpochLoop", Recording)
    out = []
    for tag, kw in (("default", {}), ("no_ride", dict(generator_rides=False)), ("no_virtual", dict(virtual_next=False))):
        F = _flags(2, tmp_path / tag, mobile=True, max_epoch_num=2, seed=31, token="mob", **kw)
        res = H.train(F, verbose=False, run_test=False, rx_params=_rx(F, 3))
        torch.cuda.synchronize()
        out.append((_state(res["trainer"]), res["history"]))
    assert len(loops) == 3
    for lp in loops:
        assert lp.fg is not None and lp.fg.has_doppler and lp.gen.mix and lp.per_symbol == 1
    assert loops[0].virt is not None and loops[0].ride_gen and loops[1].virt is not None and not loops[1].ride_gen
    assert loops[2].virt is None
    for st, hist in out[1:]:
        for name, x, y in zip(NAMES, out[0][0], st):
            assert torch.equal(x, y), name
        assert hist == out[0][1]
    assert len(out[0][1]) == 2 and float(out[0][0][3][0]) == 10.0
    assert all(0.0 < h["train_ber"] < 0.6 and h["chan_rms"] > 0.0 for h in out[0][1])


def test_mobile_chains_in_a_group_equal_their_solo_runs_bit_for_bit(tmp_path):
    """two mobile mixRayleigh chains, QPSK and 16-QAM, in one group (ONE generator launch with Doppler frames for both chains
    as the grouped step's first launch) against receiver_mp.train per chain: identical arenas, Adam state and history."""
    from dl_ofdm_amd import receiver_mp as H
    from dl_ofdm_amd.equalizer_group import train_group
    fl = [_flags(nb, tmp_path / "g", mobile=True, max_epoch_num=2, seed=40 + nb, token="mg%d" % nb) for nb in (2, 4)]
    rx = [_rx(F, 3 + i) for i, F in enumerate(fl)]
    grouped = train_group(fl, rx, verbose=False)
    torch.cuda.synchronize()
    for i, (F, r) in enumerate(zip(fl, rx)):
        Fs = _flags(F.nbits, tmp_path / "s", mobile=True, max_epoch_num=2, seed=F.seed, token=F.token)
        solo = H.train(Fs, verbose=False, run_test=False, rx_params=r)
        torch.cuda.synchronize()
        for name, x, y in zip(NAMES, _state(grouped[i]["trainer"]), _state(solo["trainer"])):
            assert torch.equal(x, y), (F.nbits, name)
        assert grouped[i]["history"] == solo["history"] and len(solo["history"]) == 2
