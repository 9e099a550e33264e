"""checksums of the fused generator's outputs at fixed (seed, offset) -- to compare two builds of the library bit for bit
(DCCN_LIB_PATH=<other build> python tools/genhash.py)"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_ofdm_amd import ofdm, receiver as R      # noqa: E402
from dl_ofdm_amd.datagen import DeviceDataGen, FusedStaticGen      # noqa: E402


def h(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]


# (the long-prefix rows first, as they always were: their lines compare across builds; short-prefix rows -- static, then with
# Doppler frames -- behind them, skipped by a library that has no such instantiation)
for chan, nbits, n, longcp, mobile in (("EPA", 2, 1170, True, False), ("ETU", 4, 73, True, False), ("AWGN", 1, 7, True, False),
                                       ("EVA", 3, 300, True, False), ("EPA", 2, 1170, False, False), ("ETU", 4, 73, False, False),
                                       ("AWGN", 1, 7, False, False), ("ETU", 3, 73, False, True),
                                       ("mixRayleigh", 2, 300, False, True)):
    F = R.Flags(nbits=nbits, nfilter=64, channel=chan, SNR=10.0, longcp=longcp)
    o = ofdm.ofdm_tx(F)
    gen = DeviceDataGen(F, o, seed=5, mobile=mobile, mix=mobile)
    gen.offset = 9
    if not FusedStaticGen.supported(gen):
        print(chan, nbits, n, "CP", gen.CP, "mobile", int(mobile), "not taken by this library's fused generator")
        continue
    fg = FusedStaticGen(gen, n, torch.linspace(0, 25, n).numpy(), want_noise_power=True)
    x = torch.empty(n, gen.S, gen.K + gen.CP, 2, device="cuda")
    bits = torch.empty(n, o.frame_size, nbits, dtype=torch.int32, device="cuda")
    tx = torch.empty(n, gen.S, gen.K + gen.CP, 2, device="cuda")
    _, _, npow = fg.make_batch(x, bits, slot=0, tx_out=tx)
    torch.cuda.synchronize()
    print(chan, nbits, n, *(() if longcp else ("CP", gen.CP, "mobile", int(mobile))), "x", h(x), "bits", h(bits), "tx", h(tx), "y", h(fg.y), "noise", h(fg.noise), "npow", h(npow))

# the launch-per-stage chain (tx grid, IDFT GEMM, taps, FIR, AWGN kernels): a static, a Doppler and a frame-interleaved descriptor
for chan, nbits, mobile, mix in (("EPA", 2, False, False), ("ETU", 3, True, False), ("mixRayleigh", 2, True, True)):
    F = R.Flags(nbits=nbits, nfilter=64, channel=chan, SNR=10.0)
    gen = DeviceDataGen(F, ofdm.ofdm_tx(F), seed=5, mobile=mobile, mix=mix)
    gen.offset = 9
    tx, bits = gen.transmit(9)
    x, npow, H = gen.channel(tx, torch.linspace(0, 25, 9, device="cuda"), want_H=True)
    torch.cuda.synchronize()
    print("per-stage", chan, nbits, 9, "mobile", int(mobile), "mix", int(mix), "x", h(x), "H", h(torch.view_as_real(H)), "npow", h(npow))

# the optimizer side: three generated pipelined steps at 73 frames, cp=True and cp=False (the windowed optimizer launch)
from dl_ofdm_amd.engine import RxEngine      # noqa: E402
for cp in (True, False):
    F = R.Flags(nbits=2, nfilter=64, channel="EPA", SNR=10.0, cp=cp)
    o = ofdm.ofdm_tx(F)
    gen = DeviceDataGen(F, o, seed=5)
    eng = RxEngine(R.rx_dims(F, o), 73, train=True, seed=5, want_prob=False, want_z=False)
    if not FusedStaticGen.supported(gen, eng):
        print("steps cp", int(cp), "not taken by this library's generated loop")
        continue
    fg = FusedStaticGen(gen, 73, 7.0, want_noise_power=True)
    for i in range(3):
        eng.train_step_generated(fg, slot=i & 1, last=(i == 2))
    torch.cuda.synchronize()
    print("steps cp", int(cp), "kin", eng.shape.kin, "params", h(eng.params), "adam_m", h(eng.adam_m), "adam_v", h(eng.adam_v))

# the driver: receiver.train over each feeding route, 2 epochs of 4 steps of 73 frames -- and one BPSK run at the default epoch
# length whose batch grows after the first epoch (the engine is swapped under the optimizer state and the best-model snapshot);
# every row also hashes the arrays of the best-model file
import tempfile      # noqa: E402

import numpy as np      # noqa: E402

import dl_ofdm_amd.engine as E      # noqa: E402

made = []


class Recording(RxEngine):
    """receiver.train returns the parameters only: keep the engines it builds, for their optimizer state"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        made.append(self)


E.RxEngine = Recording              # (receiver.train looks the class up when it is called)

small = dict(nbits=2, msg_length=7 * 73 * 5, max_epoch_num=2, eval_frames=128)
for name, kw in (("fused generator", dict(device_data=True, **small)),
                 ("side-stream feeder", dict(device_data=True, no_fused_generator=True, **small)),
                 ("host batches", dict(device_data=False, **small)),
                 ("cp off", dict(device_data=True, cp=False, **small)),
                 ("batch grows", dict(device_data=True, nbits=1, channel="AWGN", max_epoch_num=2))):
    with tempfile.TemporaryDirectory() as tmp:
        kw = dict(dict(nfilter=64, channel="EPA", SNR=10.0, seed=7, early_stop=200, token="t", save_dir=tmp + "/"), **kw)
        extra = {k: kw.pop(k) for k in ("no_fused_generator",) if k in kw}      # (read by the driver, not a declared flag)
        F = R.Flags(**kw)
        for k, v in extra.items():
            setattr(F, k, v)
        del made[:]
        res = R.train(F, verbose=False, run_test=False)
        torch.cuda.synchronize()
        eng = [e for e in made if e.train][-1]               # (the batch only grows: the last training engine holds the final state)
        z = np.load(res["best_path"] + ".npz", allow_pickle=False)
        saved = hashlib.sha256(b"".join(z[k].tobytes() for k in sorted(z.files) if k != "__flags__")).hexdigest()[:16]
        print("train", name, "batch", [e["batch_size"] for e in res["history"]], *sum(((n, h(getattr(eng, n))) for n in
              ("params", "adam_m", "adam_v", "adam_state")), ()), "history",
              hashlib.sha256(repr(res["history"]).encode()).hexdigest()[:16], "saved", saved)
