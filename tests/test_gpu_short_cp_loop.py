"""The equaliser's on-device training loop at the short cyclic prefix (N = 64, CP = 4: the ``longcp=False`` half of the reference
driver's grid, dev/py/run_local_ofdm.py:61) on the fused loop -- the one-launch generator, the virtual next batch, the generator
issued by the step itself (as the step's own first launch: the bottleneck backward launch carries the long-prefix body only) --
and what remains refused there: chain groups (``-m gpu``)."""
import pytest
import torch

from test_gpu_chain_groups import _flags, _rx, _state

pytestmark = pytest.mark.gpu
NAMES = ("params", "adam_m", "adam_v", "adam_state", "grads")


@pytest.mark.parametrize("channel,mobile,cp", [("mixRayleigh", True, True), ("EPA", False, False)])
def test_short_prefix_loop_trains_the_same_equaliser_under_every_generator_setting(tmp_path, monkeypatch, channel, mobile, cp):
    """receiver_mp.train with longcp=False, two epochs of five 73-frame steps: the default loop, generator_rides=False (the loop
    issues the generator launch) and virtual_next=False (every batch materialised by dccn_gen_static_apply) draw the same
    batches and form the same x bits -- identical arenas and histories -- and each of them took the fused generator."""
    from dl_ofdm_amd import receiver_mp as H
    loops = []

    class Recording(H.DeviceEpochLoop):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            loops.append(self)
    monkeypatch.setattr(H, "DeviceEpochLoop", Recording)
    out = []
    for tag, kw in (("default", {}), ("no_ride", dict(generator_rides=False)), ("no_virtual", dict(virtual_next=False))):
        F = _flags(2, tmp_path / tag, channel=channel, mobile=mobile, cp=cp, longcp=False, max_epoch_num=2, seed=31, token="scp", **kw)
        res = H.train(F, verbose=False, run_test=False, rx_params=_rx(F, 3))
        torch.cuda.synchronize()
        out.append((_state(res["trainer"]), res["history"]))
    assert len(loops) == 3
    for lp in loops:
        assert lp.fg is not None and lp.gen.CP == 4 and lp.fg.desc.CP == 4 and lp.fg.has_doppler == mobile
    assert loops[0].virt is not None and loops[0].ride_gen and loops[1].virt is not None and not loops[1].ride_gen
    assert loops[2].virt is None
    for st, hist in out[1:]:
        for name, x, y in zip(NAMES, out[0][0], st):
            assert torch.equal(x, y), name
        assert hist == out[0][1]
    assert len(out[0][1]) == 2 and float(out[0][0][3][0]) == 10.0
    assert all(0.0 < h["train_ber"] < 0.6 and h["chan_rms"] > 0.0 for h in out[0][1])


def test_short_prefix_chain_groups_are_refused_by_the_group_query_not_by_the_generator(tmp_path, monkeypatch):
    """two short-prefix chains: the fused generator takes them, the grouped step does not -- the folded receiver matrix has
    k = S * 2 * n_sc = 952 rows, no multiple of 16 (eq_rx_folded_ok) -- so EqualizerChainGroup raises DccnError naming
    dccn_eq_group_supported, and no group step has been issued."""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd import equalizer_group as G
    stepped = []
    monkeypatch.setattr(G.EqualizerChainGroup, "step", lambda self, act, i: stepped.append(i))
    fl = [_flags(nb, tmp_path, longcp=False) for nb in (2, 4)]
    with pytest.raises(_lib.DccnError) as err:
        G.train_group(fl, [_rx(F, 1) for F in fl])
    assert "dccn_eq_group_supported" in str(err.value) and "fused generator" not in str(err.value)
    assert stepped == []
