#!/usr/bin/env python
"""Wall time per step of the equaliser's on-device training loop (dl_ofdm_amd/receiver_mp.py::_train_on_device) and where
it goes: the loop as the harness runs it, the same loop without the torch-side monitors, the generator alone, the fused step
alone.  One JSON line per variant.

    python tools/eqloop.py [--nbits 2] [--channel EPA] [--steps 300]
    python tools/eqloop.py --channel mixRayleigh --mobile 1 --only r04_loop_next [--fused 0]      (the reference driver's default channel)
    python tools/eqloop.py --longcp 0 [--mobile 1 --channel mixRayleigh] --ab 7      (the short cyclic prefix; the pipelined loop with
                                            --fused 1 and --fused 0 alternating in this process, 7 repeats of --steps steps each)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbits", type=int, default=2)
    ap.add_argument("--channel", default="EPA")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    ap.add_argument("--fused", type=int, default=1, help="0: the launch-per-stage generator chain in the loop variants")
    ap.add_argument("--graph", type=int, default=0, help="1: the loop variants replay the step's hipGraph instead of issuing it eagerly")
    ap.add_argument("--virtual", type=int, default=1, help="0: the pipelined loop materialises every batch (no x_next_virtual)")
    ap.add_argument("--mobile", type=int, default=0, help="1: the mobile channel (mixed channels: Doppler on every 3rd / 4th frame)")
    ap.add_argument("--only", default="", help="run the variants whose name contains this")
    ap.add_argument("--longcp", type=int, default=1, help="0: the short cyclic prefix (N = 64: CP = 4)")
    ap.add_argument("--ab", type=int, default=0, help="> 0: the harness's loop with and without the fused generator, alternating, this many repeats")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dl_ofdm_amd import ofdm, receiver as R, receiver_mp as M
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    F = M.Flags(nbits=args.nbits, channel=args.channel, nfilter=64, device_data=True, seed=1) if hasattr(M, "Flags") else None
    if F is None:
        F = M.parse_flags(["--nbits=%d" % args.nbits, "--channel=%s" % args.channel, "--device_data=True"])
    F.fused_generator = bool(args.fused)
    F.virtual_next = bool(args.virtual)
    F.step_graph = bool(args.graph)
    F.mobile = bool(args.mobile)
    F.longcp = bool(args.longcp)
    o = ofdm.ofdm_tx(F)
    if args.ab > 0:
        return ab(args, F, o)
    rx_params = glorot_init(R.rx_dims(F, o), 1)
    tr = EqualizerTrainer(F, o, rx_params, device="cuda", seed=1)
    gen = DeviceDataGen(F, o, device=tr.device, seed=1, mobile=bool(args.mobile), mix=bool(args.mobile))
    B = F.batch_size // F.nsymbol
    pl = tr.resident(B)
    mview = pl.metrics_buf.view(torch.float32)
    acc = torch.zeros(5, dtype=torch.float32, device=tr.device)
    out = open(args.out, "a") if args.out else None

    def full():
        snr = np.random.choice(M.TRAIN_SNR_GRID, [B], p=M.TRAIN_SNR_PROB)
        tx, _ = gen.transmit(B, out_bits=pl.bits)
        _, npow, H = gen.channel(tx, snr, out_x=pl.x, want_H=True)
        gen.offset += 1
        pl.run(True)
        chan_gt = H if H.dim() == 3 else H[:, None, :].expand(-1, F.nsymbol, -1)
        rms = tr.chan_rms(torch.view_as_complex(pl.chest), chan_gt)
        acc[0:2].add_(mview[12:14]); acc[2:3].add_(pl.tx_power); acc[3:4].add_(npow); acc[4:5].add_(rms)

    def no_monitor():
        snr = np.random.choice(M.TRAIN_SNR_GRID, [B], p=M.TRAIN_SNR_PROB)
        tx, _ = gen.transmit(B, out_bits=pl.bits)
        gen.channel(tx, snr, out_x=pl.x, want_H=True)
        gen.offset += 1
        pl.run(True)

    def gen_only():
        tx, _ = gen.transmit(B, out_bits=pl.bits)
        gen.channel(tx, 10.0, out_x=pl.x, want_H=False)
        gen.offset += 1

    def step_graph():
        pl.run(True)

    def step_eager():
        pl.run(True, graph=False)

    variants = [("harness_loop", full), ("no_monitor", no_monitor), ("generator_only", gen_only), ("step_graph", step_graph),
                ("step_eager", step_eager)]
    if hasattr(M, "device_epoch_runner"):
        try:
            variants.insert(0, ("r04_loop_next_batch_normalised_on_the_optimizer_launch",
                                M.device_epoch_runner(F, o, tr, gen, pl, pipeline=True)))
            variants.insert(0, ("r04_loop", M.device_epoch_runner(F, o, tr, gen, pl, pipeline=False)))
        except TypeError:                                             # (an older package)
            variants.insert(0, ("r04_loop", M.device_epoch_runner(F, o, tr, gen, pl)))
    for name, fn in variants:
        if args.only not in name:
            continue
        for _ in range(30):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t0
        rec = {"variant": name, "frames": B, "channel": args.channel, "mobile": args.mobile, "fused": args.fused, "ms_per_step_wall": round(t_all / args.steps * 1e3, 4),
               "ms_per_step_host_issue": round(t_host / args.steps * 1e3, 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")


def ab(args, F, o):
    """two complete loops (trainer, generator, plans) in one process, one per generator path: ms per step of every repeat,
    median and repeat-to-repeat spread (max - min) / median"""
    import copy
    import numpy as np
    import torch
    from dl_ofdm_amd import receiver as R, receiver_mp as M
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    rx_params = glorot_init(R.rx_dims(F, o), 1)
    B = F.batch_size // F.nsymbol
    runs = []
    for fused in (1, 0):
        Fv = copy.copy(F)
        Fv.fused_generator = bool(fused)
        tr = EqualizerTrainer(Fv, o, rx_params, device="cuda", seed=1)
        gen = DeviceDataGen(Fv, o, device=tr.device, seed=1, mobile=bool(args.mobile), mix=bool(args.mobile))
        loop = M.DeviceEpochLoop(Fv, o, tr, gen, tr.resident(B), args.steps)
        assert (loop.fg is not None) == bool(fused)
        runs.append((fused, loop, []))

    def epoch(loop):
        loop.begin_epoch(np.random.choice(M.TRAIN_SNR_GRID, [args.steps, B], p=M.TRAIN_SNR_PROB))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loop.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for _, loop, _ in runs:
        epoch(loop)                                                   # warm-up
    for _ in range(args.ab):
        for _, loop, ms in runs:
            ms.append(epoch(loop))
    for fused, loop, ms in runs:
        v = sorted(ms)
        med = v[len(v) // 2]
        rec = {"variant": "harness_loop_ab", "frames": B, "channel": args.channel, "mobile": args.mobile, "CP": o.CP, "fused": fused,
               "virtual_next": loop.virt is not None, "generator_issued_by_step": loop.ride_gen,
               "ms_per_step_wall": [round(t, 4) for t in ms], "median": round(med, 4), "spread": round((v[-1] - v[0]) / med, 4)}
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
