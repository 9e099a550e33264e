"""Training on frames aligned by the cyclic-prefix estimator (``sync = W`` in receiver.Flags / receiver_mp.Flags), ``-m gpu``: the
equaliser loop materialises and aligns every batch with one launch (``dccn_gen_static_apply_sync``) or, ``fused_sync=False``,
with apply + ``dccn_frame_sync`` -- the same bits; the basic-receiver harness takes the launch-per-stage route; chain groups
refuse the flag."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _eq_flags(tmp, tag, **kw):
    from dl_ofdm_amd import receiver_mp as H
    base = dict(nbits=2, nfilter=64, channel="mixRayleigh", mobile=True, device_data=True, seed=12, max_epoch_num=2, early_stop=200,
                msg_length=7 * 73 * 5, eval_frames=128, token="st_" + tag, save_dir=os.path.join(str(tmp), tag) + "/")
    base.update(kw)
    return H.Flags(**base)


def _rx(F, seed=3):
    from dl_ofdm_amd import ofdm, receiver as R
    from dl_ofdm_amd.engine import glorot_init
    return glorot_init(R.rx_dims(F, ofdm.ofdm_tx(F)), seed)


def _run(tmp, tag, **kw):
    from dl_ofdm_amd import receiver_mp as H
    F = _eq_flags(tmp, tag, **kw)
    res = H.train(F, verbose=False, run_test=False, rx_params=_rx(F))
    torch.cuda.synchronize()
    tr = res["trainer"]
    return res["history"], [t.clone() for t in (tr.params, tr.adam_m, tr.adam_v, tr.adam_state)]


@pytest.mark.parametrize("longcp", [True, False])
def test_equaliser_loop_on_aligned_frames_one_launch_equals_three(tmp_path, longcp):
    """receiver_mp.train, sync=3, QPSK, mixRayleigh mobile, two epochs of five 73-frame steps: fused_sync True / False end with
    identical equaliser arenas and Adam state and identical loss / BER histories (chan_rms to 1e-5 relative: the device ramp
    and the torch ramp on H use different sines); a sync=0 run of the same seed differs."""
    ha, sa = _run(tmp_path, "one", sync=3, fused_sync=True, longcp=longcp)
    hb, sb = _run(tmp_path, "three", sync=3, fused_sync=False, longcp=longcp)
    h0, s0 = _run(tmp_path, "plain", longcp=longcp)
    assert len(ha) == len(hb) == 2 and float(sa[3][0]) == 10.0
    for name, x, y in zip(("params", "adam_m", "adam_v", "adam_state"), sa, sb):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
    for a, b in zip(ha, hb):
        assert set(a) == set(b)
        for k in a:
            if k == "chan_rms":
                assert abs(a[k] - b[k]) <= 1e-5 * abs(b[k]), (a[k], b[k])
            else:
                assert a[k] == b[k], (k, a[k], b[k])
        assert np.isfinite(a["train_loss"]) and 0.0 < a["train_ber"] < 0.6 and np.isfinite(a["chan_rms"])
    assert not torch.equal(sa[0], s0[0])
    assert [h["train_loss"] for h in ha] != [h["train_loss"] for h in h0]


def test_equaliser_loop_launch_per_stage_route_aligns_too(tmp_path):
    """fused_generator=False: DeviceDataGen.make_batch(sync=W) (channel into a staging buffer, then dccn_frame_sync).  Its frames
    equal the fused generator's to rounding only, so the run is held to sanity and to differing from its own sync=0 run."""
    ha, sa = _run(tmp_path, "lps", sync=3, fused_generator=False, max_epoch_num=1)
    h0, s0 = _run(tmp_path, "lps0", fused_generator=False, max_epoch_num=1)
    assert len(ha) == 1 and np.isfinite(ha[0]["train_loss"]) and 0.0 < ha[0]["train_ber"] < 0.6 and np.isfinite(ha[0]["chan_rms"])
    assert not torch.equal(sa[0], s0[0])


@pytest.mark.parametrize("cp", [True, False])
def test_basic_receiver_trains_on_aligned_batches(tmp_path, monkeypatch, cp):
    """receiver.train, sync=3, device_data, EPA, one epoch of 73-frame batches: the fused generate-and-train step is not taken,
    and after every ``_gen_into`` the engine's input equals FrameSync (out_kin = K when cp=False) applied to the batch a
    second generator draws at the same (seed, offset) -- the batch the sync=0 run trains on -- with the same labels."""
    from dl_ofdm_amd import ofdm, receiver as R
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.engine import RxEngine
    from dl_ofdm_amd.sync import FrameSync
    kw = dict(nbits=2, nfilter=64, channel="EPA", SNR=10.0, msg_length=7 * 512, batch_size=512, max_epoch_num=1, early_stop=50,
              eval_frames=128, device_data=True, cp=cp, seed=4)
    F = R.Flags(sync=3, token="rs", save_dir=str(tmp_path / "s") + "/", **kw)
    F0 = R.Flags(token="rp", save_dir=str(tmp_path / "p") + "/", **kw)
    o = ofdm.ofdm_tx(F)
    shadow = DeviceDataGen(F0, o, seed=F.seed)
    kin = o.K + o.CP if cp else o.K
    stages, calls, orig = {}, [], R._gen_into

    def spy(gen, eng, FLAGS, ofdmobj, n, snr, slot=0):
        shadow.offset = gen.offset
        out = orig(gen, eng, FLAGS, ofdmobj, n, snr, slot)
        xs, bs, _ = shadow.make_batch(n, snr)
        if n not in stages:
            stages[n] = FrameSync(7, o.K, o.CP, 3, n, out_kin=kin, want_metric=False)
        want, off = stages[n].run(xs)
        assert torch.equal(eng.x.reshape(want.shape), want)
        assert torch.equal(eng.label_slot(slot) if slot else eng.bits, bs)
        assert torch.equal(gen.sync_offset, off) and gen.offset == shadow.offset
        calls.append(n)
        return out

    def refuse(*a, **k):
        raise AssertionError("sync > 0 must not take train_step_generated")

    monkeypatch.setattr(R, "_gen_into", spy)
    monkeypatch.setattr(RxEngine, "train_step_generated", refuse)
    res = R.train(F, verbose=False, run_test=False)
    torch.cuda.synchronize()
    assert calls.count(73) == 7 and calls.count(128) == 1          # 512 frames / 73 per step, and the epoch's evaluation
    assert np.isfinite(res["history"][0]["train_loss"])
    monkeypatch.undo()
    res0 = R.train(F0, verbose=False, run_test=False)
    assert res0["history"][0]["train_loss"] != res["history"][0]["train_loss"]


def test_sweeps_align_their_frames_with_the_same_window(tmp_path):
    """receiver_mp.test_model_cross with sync=3: the plan's input is FrameSync of what the sync=0 sweep evaluates"""
    from dl_ofdm_amd import ofdm, receiver_mp as H
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.sync import FrameSync
    kw = dict(test_frames=64, snr_lo=20, snr_hi=20, channel="EVA")
    F, F0 = _eq_flags(tmp_path, "sw", sync=3, mobile=False, **kw), _eq_flags(tmp_path, "sw0", mobile=False, **kw)
    o = ofdm.ofdm_tx(F)
    xs = []
    for fl in (F, F0):
        tr = EqualizerTrainer(fl, o, _rx(fl), seed=fl.seed)
        out = H.test_model_cross(fl, tr, o, out_dir=str(tmp_path), verbose=False, channels=("EVA",))
        torch.cuda.synchronize()
        xs.append(tr.resident(64).x.clone())
        assert 0.0 <= out["EVA"][1][0] <= 0.6
    want, off = FrameSync(7, o.K, o.CP, 3, 64, want_metric=False).run(xs[1])
    assert torch.equal(xs[0], want) and int((off != 0).sum()) > 0


def test_chain_groups_refuse_sync_before_any_step(tmp_path, monkeypatch):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd import equalizer_group as G
    issued = []
    monkeypatch.setattr(G.EqualizerChainGroup, "step", lambda self, act, i: issued.append(i))
    fl = [_eq_flags(tmp_path, "g%d" % i, sync=3, seed=20 + i) for i in range(2)]
    with pytest.raises(_lib.DccnError, match="sync"):
        G.train_group(fl, [_rx(F, 3 + i) for i, F in enumerate(fl)], verbose=False)
    assert issued == []
