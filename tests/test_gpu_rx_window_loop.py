"""The basic receiver's one-call generate-and-train loop for ``cp=False`` receivers (``kin = K``: the graph drops the cyclic
prefix, dev/py/model.py:1236-1240; half of the reference driver's grid, dev/py/run_local_ofdm.py:72): the windowed apply, the
windowed virtual input of the normalisation that rides on the optimizer launch, what stays refused, and the harness (``-m gpu``).

Everything here is bit equality: the window is formed by the expression of the full path, the power scale is that of the whole
frames on both sides, and the normalisation reduces every column over the rows in an order that does not depend on the column."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_datagen import flags

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)
STATE = ("params", "adam_m", "adam_v", "adam_state")


def _gens(chan, nbits, seed, mobile, longcp, count=2):
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    F = flags(nbits=nbits, channel=chan, longcp=longcp, cp=False)
    o = ofdm.ofdm_tx(F)
    assert o.K == 64 and o.CP == (16 if longcp else 4)
    # (a mixed channel has Doppler frames under ``mix``, a single profile under ``mobile`` alone)
    return F, o, [DeviceDataGen(F, o, seed=seed, mobile=mobile, mix=mobile and chan.startswith("mix")) for _ in range(count)]


# ---- 1. the windowed apply -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cp,frames,chan,mobile", [(16, 5, "EPA", False), (4, 130, "EPA", False), (4, 73, "mixRayleigh", True)])
def test_windowed_apply_equals_the_crop_of_the_full_apply(cp, frames, chan, mobile):
    """one dccn_gen_static_frames, then dccn_gen_static_apply into [n, S, K+CP, 2] and dccn_gen_static_apply_window into
    [n, S, K, 2]: the window is the full batch cropped, bit for bit, the noise power is the same value, and nothing is written
    behind the windowed batch."""
    from dl_ofdm_amd.datagen import FusedStaticGen
    F, o, (gen,) = _gens(chan, 2, 11, mobile, cp == 16, count=1)
    fg = FusedStaticGen(gen, frames, 6.0, want_noise_power=True)
    assert fg.has_doppler == mobile and fg.desc.CP == cp
    lib, st = gen.lib, gen._stream()
    S, K = gen.S, gen.K
    bits = torch.zeros(frames, o.frame_size, 2, dtype=torch.int32, device="cuda")
    full = torch.full((frames, S, K + cp, 2), -7.0, device="cuda")
    n_win, guard = frames * S * K * 2, 4096
    buf = torch.full((n_win + guard,), -7.0, device="cuda")
    win = buf[:n_win].view(frames, S, K, 2)
    npow = torch.full((2,), -1.0, device="cuda")
    d = fg.arm(bits, 0)
    assert lib.dccn_gen_static_frames(C.byref(d), st) == 0
    assert lib.dccn_gen_static_apply(C.byref(d), full.data_ptr(), npow[0:1].data_ptr(), st) == 0
    assert lib.dccn_gen_static_apply_window(C.byref(d), win.data_ptr(), npow[1:2].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0 and not bool((full == -7.0).any())
    assert torch.equal(win, full[:, :, cp:cp + K, :])
    assert float(npow[0]) == float(npow[1]) and float(npow[0]) > 0
    assert bool((buf[n_win:] == -7.0).all())
    # refused like the full apply: no buffer, a misaligned buffer
    assert lib.dccn_gen_static_apply_window(C.byref(d), None, None, st) == INVALID_ARG
    assert lib.dccn_gen_static_apply_window(C.byref(d), win.data_ptr() + 4, None, st) == INVALID_ARG
    torch.cuda.synchronize()
    assert torch.equal(win, full[:, :, cp:cp + K, :])


# ---- 2. generated steps against pipelined steps on the cropped batches ---------------------------------------------------------
@pytest.mark.parametrize("frames,nbits,chan,mobile,longcp", [(73, 2, "EPA", False, True), (130, 4, "EPA", False, False),
                                                             (36, 1, "mixRayleigh", True, False)])
def test_generated_steps_equal_pipelined_steps_on_the_materialised_cropped_batches(frames, nbits, chan, mobile, longcp):
    """tests/test_gpu_datagen.py test_generated_steps_equal_pipelined_steps_on_the_materialised_batches at cp=False: engine A
    (kin = 64) runs train_step_generated -- the optimizer launch reads the samples behind the cyclic prefix from the generator's
    (y, noise, power partials) -- engine B gets every batch through the FULL apply, cropped with a torch slice, and runs
    train_step_pipelined.  73 frames: an odd batch on the generator's two-frames-per-block grid; 130: a second row slot of the
    normalisation, the 8-float window offset, the stand-alone 16-QAM tail; 36 mobile mixRayleigh: Doppler frames and an FIR
    reaching into the previous symbol.  The same bits in every kept batch, parameter, Adam slot and metric after four steps."""
    from dl_ofdm_amd import receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxEngine
    F, o, gs = _gens(chan, nbits, 21, mobile, longcp)
    dims = R.rx_dims(F, o)
    engs = [RxEngine(dims, frames, train=True, seed=5, want_prob=False, want_z=False) for _ in range(2)]
    ea, eb = engs
    assert ea.shape.kin == 64 and tuple(ea.x.shape) == (frames, 7, 64, 2)
    assert all(FusedStaticGen.supported(g, e) for g, e in zip(gs, engs))
    fgs = [FusedStaticGen(g, frames, 7.0, want_noise_power=True) for g in gs]
    assert fgs[0].has_doppler == mobile
    CP, K = o.CP, o.K
    n = 4
    xs = []
    for i in range(n):
        ea.train_step_generated(fgs[0], slot=i & 1, last=(i + 1 == n), keep_x=True)
        xs.append(ea.x.clone())                       # (batch 0 after the first call, then the batch step i normalised ahead)
    full = torch.empty(frames, 7, K + CP, 2, device="cuda")

    def materialise(slot):
        fgs[1].make_batch(full, eb.label_slot(slot), slot)
        eb.x.copy_(full[:, :, CP:CP + K, :])
    materialise(0)
    eb.prime()
    for i in range(n):
        last = i + 1 == n
        if not last:
            materialise((i + 1) & 1)
            assert torch.equal(eb.x, xs[i]), i
        eb.train_step_pipelined(slot=i & 1, last=last)
    torch.cuda.synchronize()
    assert gs[0].offset == gs[1].offset == n
    for name in STATE:
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name
    ma, mb = ea.metrics(), eb.metrics()
    assert ma["conf"] == mb["conf"] and ma["ce_mean"] == mb["ce_mean"] and ma["tx_power"] == mb["tx_power"]
    assert torch.equal(fgs[0].npow, fgs[1].npow)
    assert np.isfinite(ma["ce_mean"]) and float(ea.adam_state[0]) == float(n)


# ---- 3. what stays refused -------------------------------------------------------------------------------------------------------
def test_a_receiver_that_sees_neither_whole_symbols_nor_the_window_is_refused_before_anything_runs():
    """kin = 70 is neither K + CP nor K: a step handed gen_next returns DCCN_ERR_INVALID_ARG with nothing launched (parameters,
    Adam slots, step counter and x_norm keep their bits), FusedStaticGen.make_batch raises ValueError for a [n, S, 70, 2] buffer
    and leaves it alone, and FusedStaticGen.supported says so beforehand."""
    from dl_ofdm_amd import receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxDims, RxEngine
    F, o, (gen,) = _gens("EPA", 2, 3, False, True, count=1)
    frames = 36
    odd = RxEngine(RxDims(S=7, kin=70, F=64, D=o.frame_size, nbits=2), frames, train=True, seed=1, want_prob=False)
    win = RxEngine(R.rx_dims(F, o), 1536, train=True, seed=1, want_prob=False, want_z=False)
    assert win.shape.kin == 64
    assert FusedStaticGen.supported(gen) and FusedStaticGen.supported(gen, win) and not FusedStaticGen.supported(gen, odd)
    fg = FusedStaticGen(gen, frames, 10.0)
    odd.x.copy_(torch.randn(odd.x.shape, generator=torch.Generator().manual_seed(1)))
    odd.prime()
    torch.cuda.synchronize()
    watched = (odd.params, odd.adam_m, odd.adam_v, odd.adam_state, odd.x_norm)
    before = [t.clone() for t in watched]
    d = fg.arm(odd.label_slot(1), 1)
    bufs = odd._pipe_buffers(0, False, 0, False, 1, 0, C.addressof(d), False)
    rc = odd.lib.dccn_rx_train_step(C.byref(odd.shape), C.byref(bufs), odd.hp, odd._stream())
    torch.cuda.synchronize()
    assert rc == INVALID_ARG
    for a, b in zip(before, watched):
        assert torch.equal(a, b)
    offset = gen.offset
    x70 = torch.full((frames, 7, 70, 2), -7.0, device="cuda")
    with pytest.raises(ValueError):
        fg.make_batch(x70, odd.label_slot(0), 0)
    torch.cuda.synchronize()
    assert bool((x70 == -7.0).all()) and gen.offset == offset


# ---- 4. the harness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("longcp", [True, False])
def test_harness_takes_the_fused_loop_at_cp_false_and_trains_the_same_receiver(tmp_path, monkeypatch, longcp):
    """receiver.train(cp=False, device_data=True), QPSK on AWGN at 10 dB, two epochs: every training step is one
    train_step_generated call, train_step_pipelined is never called and FusedStaticGen.make_batch only materialises each
    epoch's batch 0.  A second run whose train_step_generated is replaced by its materialising twin -- every batch through
    FusedStaticGen.make_batch into eng.x, then train_step_pipelined -- ends with the same parameters, Adam slots and history."""
    from dl_ofdm_amd import receiver as R
    from dl_ofdm_amd.datagen import FusedStaticGen
    from dl_ofdm_amd.engine import RxEngine

    def run(tag):
        Fl = R.Flags(nbits=2, nfilter=64, channel="AWGN", SNR=10.0, msg_length=7 * 1024, batch_size=512, max_epoch_num=2,
                     early_stop=100, token="win", save_dir=str(tmp_path / tag) + "/", seed=5, device_data=True, cp=False,
                     longcp=longcp)
        res = R.train(Fl, verbose=False, run_test=False)
        torch.cuda.synchronize()
        return res

    calls = dict(generated=[], pipelined=0, make_batch=[])
    last_eng = {}
    gen_orig, pipe_orig, mb_orig = RxEngine.train_step_generated, RxEngine.train_step_pipelined, FusedStaticGen.make_batch

    def spy_generated(self, fgen, slot=0, last=False, keep_x=False, side=None):
        calls["generated"].append((self.batch, self.dims.kin, bool(last), bool(self._norm_ready)))
        last_eng["plain"] = self
        return gen_orig(self, fgen, slot=slot, last=last, keep_x=keep_x, side=side)

    def spy_pipelined(self, *a, **kw):
        calls["pipelined"] += 1
        return pipe_orig(self, *a, **kw)

    def spy_make_batch(self, out_x, *a, **kw):
        calls["make_batch"].append(tuple(out_x.shape))
        return mb_orig(self, out_x, *a, **kw)

    monkeypatch.setattr(RxEngine, "train_step_generated", spy_generated)
    monkeypatch.setattr(RxEngine, "train_step_pipelined", spy_pipelined)
    monkeypatch.setattr(FusedStaticGen, "make_batch", spy_make_batch)
    plain = run("plain")
    assert calls["pipelined"] == 0
    epochs, cur = [], []
    for batch, kin, last, primed in calls["generated"]:
        assert kin == 64
        cur.append((batch, primed))
        if last:
            epochs.append(cur)
            cur = []
    assert cur == [] and len(epochs) == 2
    for ep in epochs:                                       # one call per training step: 1024 frames per epoch
        assert len(ep) == 1024 // ep[0][0] and [primed for _, primed in ep] == [False] + [True] * (len(ep) - 1)
    assert calls["make_batch"] == [(ep[0][0], 7, 64, 2) for ep in epochs]          # each epoch's batch 0, windowed
    state_plain = [getattr(last_eng["plain"], name).clone() for name in STATE]

    def twin(self, fgen, slot=0, last=False, keep_x=False, side=None):
        last_eng["twin"] = self
        if not self._norm_ready:
            mb_orig(fgen, self.x, self.label_slot(slot), slot)
            self.prime()
        if not last:
            mb_orig(fgen, self.x, self.label_slot(slot ^ 1), slot ^ 1)
        pipe_orig(self, slot=slot, last=last)

    monkeypatch.setattr(RxEngine, "train_step_generated", twin)
    other = run("twin")
    for name, a in zip(STATE, state_plain):
        assert torch.equal(a, getattr(last_eng["twin"], name)), name
    assert sorted(plain["params"]) == sorted(other["params"])
    for name in plain["params"]:
        assert np.array_equal(plain["params"][name], other["params"][name]), name
    assert plain["history"] == other["history"] and len(plain["history"]) == 2
    assert all(np.isfinite(h["train_loss"]) and 0.0 <= h["test_ber"] < 0.5 for h in plain["history"])
