#!/usr/bin/env python
"""What does aligning every training batch (``sync = W``) cost, and what does forming + aligning in ONE launch save?

One process, the variants alternating, --repeats repeats (the way profiles/gen_short_cp.md was measured); per variant the
median and the repeat-to-repeat spread (max - min) / median.  One JSON line per record.

  batch   FusedStaticGen.make_batch on mixRayleigh mobile, 73 and 1170 frames, CP 16 and 4, three ways:
            plain   generator + dccn_gen_static_apply                               (no alignment: the baseline)
            one     generator + dccn_gen_static_apply_sync                          (sync = W, fused_sync = True)
            three   generator + dccn_gen_static_apply + dccn_frame_sync             (sync = W, fused_sync = False, H not requested)
  step    the equaliser's 73-frame training loop (receiver_mp.DeviceEpochLoop) on mixRayleigh mobile, CP 16 and 4:
            default loop (virtual next batch, riding generator), sync = W, sync = W with fused_sync = False

    python tools/syncbench.py [--W 3] [--repeats 7] [--batches 300] [--steps 300] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    v = sorted(ms)
    med = v[len(v) // 2]
    return {"median": round(med, 3), "spread": round((v[-1] - v[0]) / med, 4), "repeats": [round(t, 3) for t in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--only", default="", help="batch | step")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dl_ofdm_amd import _lib, ofdm, receiver as R, receiver_mp as M
    from dl_ofdm_amd.datagen import DeviceDataGen, FusedStaticGen
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    build = _lib.load().dccn_build_id().decode()

    def emit(rec):
        rec["build_id"] = build
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def flags(longcp, **kw):
        return M.Flags(nbits=2, channel="mixRayleigh", nfilter=64, device_data=True, seed=1, mobile=True, longcp=longcp, **kw)

    if a.only in ("", "batch"):
        for longcp in (True, False):
            for n in (73, 1170):
                F = flags(longcp)
                o = ofdm.ofdm_tx(F)
                gen = DeviceDataGen(F, o, seed=1, mobile=True, mix=True)
                fg = FusedStaticGen(gen, n, 20.0, want_noise_power=True)
                x = torch.empty(n, gen.S, gen.n_sc, 2, device="cuda")
                bits = torch.empty(n, gen.D, gen.nbits, dtype=torch.int32, device="cuda")
                variants = {"plain": lambda: fg.make_batch(x, bits), "one": lambda: fg.make_batch(x, bits, sync=a.W),
                            "three": lambda: fg.make_batch(x, bits, sync=a.W, fused_sync=False)}
                times = {k: [] for k in variants}

                def run(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.batches):
                        fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / a.batches * 1e6

                for fn in variants.values():
                    run(fn)                                             # warm-up
                for _ in range(a.repeats):
                    for k, fn in variants.items():
                        times[k].append(run(fn))
                for k in variants:
                    emit(dict(kind="batch", variant=k, frames=n, CP=o.CP, W=a.W, unit="us per batch", **stats(times[k])))

    if a.only in ("", "step"):
        for longcp in (True, False):
            runs = []
            for name, kw in (("default", {}), ("sync_one", dict(sync=a.W)), ("sync_three", dict(sync=a.W, fused_sync=False))):
                F = flags(longcp, **kw)
                o = ofdm.ofdm_tx(F)
                tr = EqualizerTrainer(F, o, glorot_init(R.rx_dims(F, o), 1), device="cuda", seed=1)
                gen = DeviceDataGen(F, o, device=tr.device, seed=1, mobile=True, mix=True)
                B = F.batch_size // F.nsymbol
                loop = M.DeviceEpochLoop(F, o, tr, gen, tr.resident(B), a.steps)
                assert loop.fg is not None and (loop.virt is None) == bool(kw)
                runs.append((name, loop, B, o.CP, []))

            def epoch(loop, B):
                loop.begin_epoch(np.random.choice(M.TRAIN_SNR_GRID, [a.steps, B], p=M.TRAIN_SNR_PROB))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loop.step()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.steps * 1e6

            for _, loop, B, _, _ in runs:
                epoch(loop, B)                                          # warm-up
            for _ in range(a.repeats):
                for _, loop, B, _, ms in runs:
                    ms.append(epoch(loop, B))
            for name, loop, B, CP, ms in runs:
                emit(dict(kind="step", variant=name, frames=B, CP=CP, W=a.W, unit="us per step", **stats(ms)))


if __name__ == "__main__":
    main()
