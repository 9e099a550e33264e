#!/usr/bin/env python
"""What does the classical detector cost as ONE launch (``ClassicalRxReceiver.receive``) against the launch sequence a caller
had before it (``ClassicalReceiverGPU.receive(..., "ALMMSE", snr, want_bits=True)``: DFT GEMM, pilot LS, interpolation GEMM,
estimate, detect + finish, and a host read-back of the error count), and next to the DCCN receiver (``RxReceiver.receive``)?

One process, the variants alternating, --repeats repeats; device events around --calls calls per repeat; per variant the
median and the repeat-to-repeat spread (max - min) / median.  One JSON line per record.

  one        ClassicalRxReceiver.receive(x)                      (x device-resident: the staging copy + the one launch)
  one_llr    the same with want_llr=True
  sequence   ClassicalReceiverGPU.receive(..., want_bits=True)    (as a caller had it: ends in ``.item()``)
  launches   the same launch sequence WITHOUT the read-back -- the entry points called directly on preallocated buffers, so
             neither the host synchronisation nor the allocations of ``receive`` are in the window
  dccn       RxReceiver.receive(x) of the basic receiver at the same frame count (cp=True, whole symbols)

    python tools/clsrxbench.py [--repeats 7] [--calls 200] [--frames 73,1170,20000] [--out FILE]

``--links G [G ...]`` asks the other question instead: what does ONE grouped launch for G links
(``ClassicalReceiveGroup.receive``, ``dccn_classical_receive_grouped``) cost against the same G links as solo calls back to back
on one stream (``ClassicalRxReceiver.receive`` G times)?  Frames resident in both arms (no staging copies: launches only), ALMMSE,
the same alternation, repeats and spreads; per G and frame count one pair with every link QPSK and one with the links' modulations
cycling through ``--mods`` (default 1 2 3 4).  ``--variants solo`` restricts the first table to the listed variants (an A/B of two
builds of the library runs ``--variants one`` once per build, ``DCCN_LIB_PATH`` selecting it).

  solo_xG    G ClassicalRxReceiver.receive() calls, one per link       grouped    ClassicalReceiveGroup.receive([None] * G)

    python tools/clsrxbench.py --links 2 4 8 [--mods 1 2 3 4] [--frames 73,1170] [--repeats 7] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(us):
    v = sorted(us)
    med = v[len(v) // 2]
    return {"median": round(med, 3), "spread": round((v[-1] - v[0]) / med, 4), "repeats": [round(t, 3) for t in us]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", default="73,1170,20000")
    ap.add_argument("--nbits", default="2,4")
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--links", type=int, nargs="+", default=[], help="group sizes: time G solo calls against one grouped call")
    ap.add_argument("--mods", type=int, nargs="+", default=[1, 2, 3, 4], help="with --links: the mixed arm's modulations (nbits)")
    ap.add_argument("--variants", default="", help="without --links: only these variants (comma separated)")
    a = ap.parse_args()
    import torch
    from dl_ofdm_amd import _lib, ofdm, receiver as R
    from dl_ofdm_amd.benchmark_gpu import ClassicalReceiverGPU
    from dl_ofdm_amd.classical_receive import ClassicalRxReceiver
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.engine import glorot_init
    from dl_ofdm_amd.receive import RxReceiver
    lib = _lib.load()
    build = lib.dccn_build_id().decode()

    def emit(rec):
        rec["build_id"] = build
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3                   # us per call

    def alternate(variants, calls):
        """every variant warmed up, then --repeats rounds with the variants alternating -> {variant: [us per call]}"""
        times = {k: [] for k in variants}
        for fn in variants.values():
            timed(fn, 5)
        for _ in range(a.repeats):
            for k, fn in variants.items():
                times[k].append(timed(fn, calls))
        return times

    if a.links:
        from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
        for n in (int(v) for v in a.frames.split(",")):
            calls = max(10, min(a.calls, 2_000_000 // n))
            for G in a.links:
                for arm, mods in (("qpsk", [2] * G), ("mixed", [a.mods[i % len(a.mods)] for i in range(G)])):
                    flags = [R.Flags(nbits=nb, channel="EPA", nfilter=64) for nb in mods]
                    grp = ClassicalReceiveGroup(flags, n, "ALMMSE")
                    solos = [ClassicalRxReceiver(F, n, "ALMMSE") for F in flags]
                    for i, F in enumerate(flags):                              # every link its own frames, the same in both arms
                        x = DeviceDataGen(F, ofdm.ofdm_tx(F), device="cuda", seed=1 + i).make_batch(n, a.snr)[0]
                        grp.links[i].x.copy_(x.reshape(grp.links[i].x.shape))
                        solos[i].x.copy_(grp.links[i].x)
                    none = [None] * G

                    def solo_calls():
                        for rx in solos:
                            rx.receive()

                    times = alternate({"solo_x%d" % G: solo_calls, "grouped": lambda: grp.receive(none)}, calls)
                    torch.cuda.synchronize()
                    same = all(torch.equal(l.packed, rx.packed) and torch.equal(l.chest, rx.chest) for l, rx in zip(grp.links, solos))
                    for k, v in times.items():
                        emit(dict(kind="clsrx_group", variant=k, arm=arm, links=G, mods=mods, frames=n, calls=calls,
                                  unit="us per round of %d links" % G, grouped_equals_solo=bool(same), **stats(v)))
        return

    only = [v for v in a.variants.split(",") if v]
    for nbits in (int(v) for v in a.nbits.split(",")):
        for n in (int(v) for v in a.frames.split(",")):
            F = R.Flags(nbits=nbits, channel="EPA", nfilter=64)
            o = ofdm.ofdm_tx(F)
            gen = DeviceDataGen(F, o, device="cuda", seed=1)
            x, bits = gen.make_batch(n, a.snr)[:2]
            old = ClassicalReceiverGPU(F, o)
            one = ClassicalRxReceiver(F, n, "ALMMSE", advance=old.advance)
            one_llr = ClassicalRxReceiver(F, n, "ALMMSE", advance=old.advance, want_llr=True)
            dims = R.rx_dims(F, o)
            dccn = RxReceiver(dims, n, glorot_init(dims, 1), CP=o.CP)
            # the old sequence's launches on buffers of their own
            S, K, SK, P, D = old.S, old.K, old.S * old.K, old.P, old.D
            f32 = dict(dtype=torch.float32, device="cuda")
            Y, gp, Gls, G = torch.empty(n * S, 2 * K, **f32), torch.empty(2, n, P, **f32), torch.empty(2 * n, SK, **f32), \
                torch.empty(n, SK, 2, **f32)
            det = torch.empty(n, D, nbits, dtype=torch.int32, device="cuda")
            b32 = bits.to(torch.int32).contiguous()
            dft = old._dft_matrix(old.advance > 0)
            pv = complex(old.host.pilot_value)
            cvar = float(K * 10.0 ** (-a.snr / 10.0) / abs(pv) ** 2)
            xwin = x.view(n * S, 2 * old.n_sc)
            off = 2 * (old.CP - old.advance)

            def launches():
                s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                st = lib.dccn_dense_fwd_ld(xwin.data_ptr() + 4 * off, 2 * old.n_sc, dft.data_ptr(), None, Y.data_ptr(), n * S, 2 * K,
                                           2 * K, s)
                st |= lib.dccn_classical_pilot_ls(Y.data_ptr(), old.pil.data_ptr(), gp.data_ptr(), n, SK, P, pv.real, pv.imag, s)
                st |= lib.dccn_dense_fwd(gp.data_ptr(), old.w_spline.data_ptr(), None, Gls.data_ptr(), 2 * n, P, SK, s)
                st |= lib.dccn_classical_estimate(Gls.data_ptr(), None, G.data_ptr(), n, S, K, 2, cvar, old.ws.data_ptr(), old.nws, s)
                st |= lib.dccn_classical_detect(Y.data_ptr(), G.data_ptr(), old.dat.data_ptr(), old.table.data_ptr(),
                                                old.labels.data_ptr(), b32.data_ptr(), det.data_ptr(), old._err.data_ptr(), n, SK, D,
                                                int(old.table.shape[0]), nbits, SK, 0, old.ws.data_ptr(), old.nws, s)
                assert st == 0

            variants = {"one": lambda: one.receive(x), "one_llr": lambda: one_llr.receive(x),
                        "sequence": lambda: old.receive(x, bits, "ALMMSE", a.snr, want_bits=True), "launches": launches,
                        "dccn": lambda: dccn.receive(x)}
            if only:
                variants = {k: variants[k] for k in only}
            calls = max(10, min(a.calls, 2_000_000 // n))
            times = alternate(variants, calls)                              # (warm-up of every shape in the window first)
            # the two classical paths decide alike (a few cells within rounding of a boundary aside)
            one.receive(x)
            _, _, ref = old.receive(x, bits, "ALMMSE", a.snr, want_bits=True)
            differ = float((one.receive(x).bits().to(torch.int32) != ref).float().mean())
            for k in variants:
                emit(dict(kind="clsrx", variant=k, frames=n, nbits=nbits, calls=calls, unit="us per call", differ_vs_sequence=differ,
                          **stats(times[k])))


if __name__ == "__main__":
    main()
