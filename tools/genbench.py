"""launch time of the fused generator (HIP events over a same-kernel loop); DCCN_GEN_ABL=<bits> for ablations of the static launch

    python tools/genbench.py [--channel EPA] [--mobile 0] [--frames 1170] [--H 0] [--longcp 1]
    python tools/genbench.py --channel mixRayleigh --mobile 1 --frames 73 --H 1      (a Doppler frame in every third slot)
    python tools/genbench.py --longcp 0 --fused 0                   (the launch-per-stage chain at the short cyclic prefix)
    python tools/genbench.py --longcp 0 --frames 73 --repeats 7     (both generators of a batch x, alternating in this process:
                                                                     us per batch of every repeat, median, (max - min) / median)
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl_ofdm_amd import ofdm, receiver as R      # noqa: E402
from dl_ofdm_amd.datagen import DeviceDataGen, FusedStaticGen      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--channel", default="EPA")
ap.add_argument("--mobile", type=int, default=0)
ap.add_argument("--frames", type=int, default=1170)
ap.add_argument("--H", type=int, default=0, help="1: also write the frequency responses [n, S, K]")
ap.add_argument("--longcp", type=int, default=1, help="0: the short cyclic prefix (N = 64: CP = 4)")
ap.add_argument("--fused", type=int, default=1, help="0: the launch-per-stage chain (transmit + channel) instead of the fused launch")
ap.add_argument("--repeats", type=int, default=0,
                help="> 0: time a whole batch x (fused: generator launch + the launch that forms x) by both generators, alternating")
args = ap.parse_args()
F = R.Flags(nbits=2, nfilter=64, channel=args.channel, SNR=10.0, longcp=bool(args.longcp))
o = ofdm.ofdm_tx(F)
gen = DeviceDataGen(F, o, seed=1, mobile=bool(args.mobile), mix=bool(args.mobile))
gen.want_noise_power = False
n = args.frames
bits = torch.empty(n, o.frame_size, 2, dtype=torch.int32, device="cuda")
per_symbol = gen.doppler or gen.mixed
# (one response per symbol where the launch-per-stage chain writes that: Doppler frames, mixed channels -- and for the fused launch alone)
hshape = (n, gen.S, gen.K, 2) if (per_symbol or (args.fused and not args.repeats)) else (n, gen.K, 2)
H = torch.empty(*hshape, device="cuda") if args.H else None
x = torch.empty(n, gen.S, gen.n_sc, 2, device="cuda")
snr = torch.full((n,), 10.0, device="cuda")
st = gen._stream()
fg = FusedStaticGen(gen, n, 10.0) if (args.fused or args.repeats) else None


def fused_launch():
    gen.lib.dccn_gen_static_frames(C.byref(fg.arm(bits, out_H=H)), st)


def fused_batch():
    fg.make_batch(x, bits, out_H=H)


def staged_batch():
    tx, _ = gen.transmit(n, out_bits=bits)
    gen.channel(tx, snr, out_x=x, out_H=H)
    gen.offset += 1


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


tag = "%s mobile=%d frames=%d H=%d CP=%d" % (args.channel, args.mobile, n, args.H, gen.CP)
if args.repeats > 0:
    variants = (("fused", fused_batch), ("launch_per_stage", staged_batch))
    for _, fn in variants:
        for _ in range(50):
            fn()
    us = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            us[name].append(timed(fn, 300))
    for name, _ in variants:
        v = sorted(us[name])
        med = v[len(v) // 2]
        print("%s %s: us per batch %s median %.2f spread %.3f" % (tag, name, " ".join("%.2f" % t for t in us[name]), med, (v[-1] - v[0]) / med))
else:
    fn = fused_launch if args.fused else staged_batch
    for _ in range(50):
        fn()
    print("%s doppler_period=%d fused=%d DCCN_GEN_ABL=%s: %.2f us per %s"
          % (tag, fg.desc.doppler_period if fg else 0, args.fused, os.environ.get("DCCN_GEN_ABL", "0"), timed(fn, 300),
             "launch" if args.fused else "batch"))
