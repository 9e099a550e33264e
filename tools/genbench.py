"""launch time of the fused generator (HIP events over a same-kernel loop); DCCN_GEN_ABL=<bits> for ablations of the static launch

    python tools/genbench.py [--channel EPA] [--mobile 0] [--frames 1170] [--H 0]
    python tools/genbench.py --channel mixRayleigh --mobile 1 --frames 73 --H 1      (a Doppler frame in every third slot)
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
args = ap.parse_args()
F = R.Flags(nbits=2, nfilter=64, channel=args.channel, SNR=10.0)
o = ofdm.ofdm_tx(F)
gen = DeviceDataGen(F, o, seed=1, mobile=bool(args.mobile), mix=bool(args.mobile))
n = args.frames
fg = FusedStaticGen(gen, n, 10.0)
bits = torch.empty(n, o.frame_size, 2, dtype=torch.int32, device="cuda")
H = torch.empty(n, gen.S, gen.K, 2, device="cuda") if args.H else None
st = gen._stream()
for _ in range(50):
    gen.lib.dccn_gen_static_frames(C.byref(fg.arm(bits, out_H=H)), st)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
for _ in range(300):
    gen.lib.dccn_gen_static_frames(C.byref(fg.arm(bits, out_H=H)), st)
e1.record()
torch.cuda.synchronize()
print("%s mobile=%d frames=%d H=%d doppler_period=%d DCCN_GEN_ABL=%s: %.2f us per launch"
      % (args.channel, args.mobile, n, args.H, fg.desc.doppler_period, os.environ.get("DCCN_GEN_ABL", "0"), e0.elapsed_time(e1) * 1e3 / 300))
