"""checksums of what the equaliser's entry points leave behind at fixed seeds -- to compare two builds of the library bit for bit
(DCCN_LIB_PATH=<other build> python tools/eqhash.py): the fused step (eager, then replayed from a graph) at 73 and 1170 frames with
cp on and off, the stand-alone monitors, one epoch of the on-device loop (generator and monitors riding on the step), a training
group and a receive group of mixed modulations"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_ofdm_amd import ofdm, receiver_mp as H      # noqa: E402
from dl_ofdm_amd.engine import glorot_init           # noqa: E402
from dl_ofdm_amd.equalizer import EqualizerTrainer   # noqa: E402
from dl_ofdm_amd.equalizer_group import ChainReceiveGroup, train_group      # noqa: E402
from dl_ofdm_amd.receiver import rx_dims              # noqa: E402


def h(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]


def state(tr):
    return " ".join("%s %s" % (n, h(getattr(tr, n))) for n in ("params", "adam_m", "adam_v", "adam_state", "grads"))


# the fused step
for B, nbits, cp in ((73, 2, True), (73, 4, False), (1170, 2, True), (1170, 3, False)):
    F = H.Flags(nbits=nbits, nfilter=64, channel="EPA", cp=cp)
    tx = ofdm.ofdm_tx(F)
    tr = EqualizerTrainer(F, tx, glorot_init(rx_dims(F, tx), 1), seed=1)
    g = torch.Generator().manual_seed(B + nbits)
    pl = tr._plan(B)
    pl.set_batch(torch.randn(B, 7, tx.K + tx.CP, 2, generator=g).cuda(),
                 torch.randint(0, 2, (B, tx.frame_size, nbits), generator=g, dtype=torch.int32).cuda())
    for graph in (False, False, True, True):
        pl.run(True, graph)
    pl.run(False, False)
    torch.cuda.synchronize()
    print("step", B, nbits, "cp", int(cp), state(tr), "out_eq", h(pl.out_eq), "chest", h(pl.chest), "snr_db", h(pl.snr_db), "metrics",
          h(pl.metrics_buf))
    if B == 73:
        r = tr.receive(pl.x, want_llr=True, want_prob=True)
        torch.cuda.synchronize()
        print("receive", B, nbits, "cp", int(cp), "packed", h(r.packed), "llr", h(r.llr), "prob", h(r.prob))

with tempfile.TemporaryDirectory() as tmp:
    def flags(nbits, sub, **kw):
        return H.Flags(nbits=nbits, nfilter=64, channel="mixRayleigh", device_data=True, seed=10 + nbits, max_epoch_num=2, early_stop=200,
                       msg_length=7 * 73 * 4, eval_frames=128, token="h%d" % nbits, save_dir=os.path.join(tmp, sub, "ck%d/" % nbits), **kw)

    # the on-device loop: riders on, then the generator, the normalisation's virtual input and the monitors as launches of their own
    for name, kw in (("riders", {}), ("own launches", dict(generator_rides=False, monitor_rides=False))):
        F = flags(2, name.replace(" ", "_"))
        for k, v in kw.items():
            setattr(F, k, v)
        res = H.train(F, verbose=False, run_test=False, rx_params=glorot_init(rx_dims(F, ofdm.ofdm_tx(F)), 3))
        torch.cuda.synchronize()
        print("loop", name, state(res["trainer"]), "history", hashlib.sha256(repr(res["history"]).encode()).hexdigest()[:16])
    mods = (1, 2, 3, 4, 2)
    fl = [flags(nb, "g%d" % i) for i, nb in enumerate(mods)]
    rx = [glorot_init(rx_dims(F, ofdm.ofdm_tx(F)), 3 + i) for i, F in enumerate(fl)]
    for i, res in enumerate(train_group(fl, rx, verbose=False)):
        print("group chain", i, mods[i], state(res["trainer"]), "history", hashlib.sha256(repr(res["history"]).encode()).hexdigest()[:16])
    grp = ChainReceiveGroup(fl, rx, 73, want_llr=True, want_prob=True)
    rng = np.random.RandomState(4)
    out = grp.receive([(rng.standard_normal((73, 7, 80, 2)) * 2).astype(np.float32) for _ in fl])
    torch.cuda.synchronize()
    for i, (r, c) in enumerate(zip(out, grp.chains)):
        print("group receive", i, mods[i], "packed", h(r.packed), "llr", h(r.llr), "prob", h(r.prob), "out_eq", h(c.pl.out_eq), "chest",
              h(c.pl.chest), "snr_db", h(c.pl.snr_db))
