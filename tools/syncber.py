#!/usr/bin/env python
"""Does per-frame timing alignment from the cyclic prefix (dl_ofdm_amd.sync.FrameSync) change the BER of a trained chain?

One modulation; the basic receiver trained with the reference driver's recipe (AWGN at 5 dB per bit) and the equaliser trained
on --train_channel (default mixRayleigh, the reference driver's stage 2) -- or a chain loaded with --load -- then evaluated on
EPA / EVA / ETU / mixRayleigh at --snrs, the SAME frames three ways:

    plain     the frames as the generator writes them (they arrive (L - 1) // 2 samples early: datagen.py)
    sync      every frame rotated by its own estimated offset (FrameSync, window --W) in front of the evaluation step
    known     every frame delayed by the channel's known advance (what align_window does; single-profile channels only)

next to the share of frames per estimated offset.  That chain is NOT retrained on aligned frames: the three columns measure what
the stage does for a chain trained as the reference trains it.  ``--train_sync W`` trains a SECOND equaliser with ``sync=W`` (every
training batch aligned by the estimator inside the loop: receiver_mp.Flags.sync) on the same basic receiver -- or, ``--rx_sync``,
on a basic receiver whose own training frames were aligned too -- and adds the column

    sync-trained    that chain on the aligned frames

``--cfo EPS[,EPS...]`` asks another question of the same trained chain, through the label-free receive path: every evaluation frame
gets a carrier-frequency offset of its own, eps ~ U(-EPS, EPS) subcarrier spacings (radio.apply_cfo's statement, on the device in
fp64), and the chain's BER is reported on AWGN / EPA / EVA / ETU for

    no offset      receive(x) on the frames before the impairment (the JSON also carries ``no_offset_eval``: the labelled
                   evaluation step's BER on the same frames, which the receive path's bits must reproduce)
    plain          receive(x) on the impaired frames
    sync           receive(x, sync=W)
    sync + cfo     receive(x, sync=W, cfo=True): the launch that estimates the offset from the prefix correlation and removes it

next to the median and the 95th percentile of |estimate - eps| over the frames.

``--capture`` asks it of contiguous captures (the host model ``rayleigh_chan_lte.run_stream``: the frames' full convolutions
overlap-added, one carrier phase running over the capture), EPA / EVA / ETU static, with eps = 0 and with one eps ~ U(-0.2, 0.2)
per capture:

    capture        receive_capture(cap, first, sync=W[, cfo=True]): frames cut linearly at their estimated starts
    cut            receive(x, sync=W[, cfo=True]) on the same capture cut at the nominal starts (the circular frame)
    baseline       receive(x) on the nominal cut of the capture before the carrier offset, no alignment

``--capture --cfo_scope capture`` (or ``--cfo EPS --cfo_scope capture``: eps ~ U(-EPS, EPS) per capture) adds to every impaired
row the estimate pooled over the capture's frames (``receive_capture(..., cfo=True, cfo_scope="capture")``: one offset per
capture, dccn_capture_sync_pooled) next to the per-frame one, and the offset-free arm on the same aligned path:

    capture_pooled       receive_capture(cap, first, sync=W, cfo=True, cfo_scope="capture")
    capture_offset_free  receive_capture(the capture before the carrier offset, first, sync=W)

with |estimate - eps| of the per-frame estimates (median, p95, worst over the frames) and of the pooled one (median, worst over
the captures).

``--acquire J[,J...]`` begins each such capture at a random sample inside frame 0 and asks how often
``receive_capture(first=None, acquire=J, lo=W)`` finds the frame start (within W samples: the refinement behind it absorbs that),
and what the chain's BER is behind it, next to the BER with the start known.  ``--cfo_span M`` draws the fraction from
U(-1/2, 1/2) and adds every capture under eps = m + f, m uniform in [-M, M]: how often ``receive_capture(..., acquire=J,
cfo_span=M)`` finds the start and the whole offset, the BER behind it, and the BER of the narrow call on the same captures.

``--classical METHOD`` (ALMMSE | LS-Spline | LS-Linear) adds rows of the label-free classical detector
(``ClassicalRxReceiver.receive_capture``, pooled offset, ``acquire=16``) on the ``--acquire`` table's captures, with the noise
variance estimated from the empty carriers and with the true one given.  It trains nothing.

No threshold: the numbers are the result.

    python tools/syncber.py --nbits 2 --out syncber_out [--load CKPT --rx_load CKPT] [--seeds 3] [--train_sync 3 [--rx_sync]]
    python tools/syncber.py --nbits 2 --cfo 0.05,0.2 --out syncber_out
    python tools/syncber.py --nbits 2 --capture --snrs 5,29 --frames 2000 --out syncber_out
    python tools/syncber.py --nbits 2 --cfo 0.2 --cfo_scope capture --snrs 5,29 --frames 2000 --out syncber_out
    python tools/syncber.py --nbits 2 --acquire 4,8,16 --snrs 5,30 --frames 73 --captures 30 --out syncber_out
    python tools/syncber.py --nbits 2 --acquire 4,8,16 --cfo_span 7 --snrs 5,30 --frames 73 --captures 30 --out syncber_out
    python tools/syncber.py --nbits 2 --classical ALMMSE --snrs 5,29 --frames 73 --captures 30 --out syncber_out
"""
import argparse
import copy
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHANNELS = ("EPA", "EVA", "ETU", "mixRayleigh")
CFO_CHANNELS = ("AWGN", "EPA", "EVA", "ETU")


def apply_cfo_device(x, eps, K):
    """radio.apply_cfo on the device: float32 of x[n] exp(+2 pi i eps n / K), n over the whole frame, multiplied in fp64"""
    import torch
    frames = x.shape[0]
    y = torch.view_as_complex(x.to(torch.float64).reshape(frames, -1, 2))
    n = torch.arange(y.shape[1], dtype=torch.float64, device=x.device)
    ang = 2.0 * torch.pi * eps.to(torch.float64)[:, None] * n[None, :] / float(K)
    return torch.view_as_real(y * torch.polar(torch.ones_like(ang), ang)).to(torch.float32).reshape(x.shape)


def cfo_rows(a, tr, hf, snrs, log):
    """the --cfo table: one row per (EPS, channel, SNR)"""
    import torch
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    K = int(tr.ofdmobj.K)
    pl = tr.resident(a.frames)
    clean = torch.empty_like(pl.x)
    rows = []

    def ber(res):
        return float((res.bits().to(torch.int32) != pl.bits).to(torch.float32).mean())

    for EPS in [float(v) for v in a.cfo.split(",")]:
        for ch in CFO_CHANNELS:
            fl = copy.deepcopy(hf)
            fl.channel = ch
            gen = DeviceDataGen(fl, ofdm.ofdm_tx(fl), device=tr.device, seed=77)
            gen.want_noise_power = False
            for i, snr in enumerate(snrs):
                got = {"no_offset": [], "no_offset_eval": [], "plain": [], "sync": [], "sync_cfo": []}
                errs = []
                for sd in range(a.seeds):
                    gen.seed, gen.offset = 77 + 13 * i + 1009 * sd, 0
                    gen.make_batch(a.frames, snr, out_x=clean, out_bits=pl.bits)
                    g = torch.Generator(device=tr.device)
                    g.manual_seed(4242 + 13 * i + 1009 * sd)
                    eps = (torch.rand(a.frames, generator=g, device=tr.device, dtype=torch.float64) * 2.0 - 1.0) * EPS
                    x = apply_cfo_device(clean, eps, K)
                    got["no_offset"].append(ber(tr.receive(clean)))
                    pl.run(False)       # cross-check: the labelled evaluation step on the frames that receive call staged
                    got["no_offset_eval"].append(float(tr._metrics(pl.metrics_buf, pl.tx_power)["berlin"]))
                    got["plain"].append(ber(tr.receive(x)))
                    got["sync"].append(ber(tr.receive(x, sync=a.W)))
                    res = tr.receive(x, sync=a.W, cfo=True)
                    got["sync_cfo"].append(ber(res))
                    d = res.cfo.to(torch.float64) - eps
                    errs.append((d - torch.round(d)).abs())
                e = torch.cat(errs)
                row = {"eps_max": EPS, "channel": ch, "snr_db": snr,
                       "cfo_abs_err": {"median": float(e.median()), "p95": float(torch.quantile(e, 0.95))}}
                for k, v in got.items():
                    row[k] = {"ber": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                rows.append(row)
                print(json.dumps(row), flush=True)
    log["cfo_rows"] = rows
    with open(os.path.join(a.out, "syncber_cfo_%dmod.json" % a.nbits), "w") as f:
        json.dump(log, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "syncber_cfo_%dmod.md" % a.nbits), "w") as f:
        cell = lambda c: "%.3g (%.3g .. %.3g)" % (c["ber"], c["min"], c["max"])      # noqa: E731
        f.write("| EPS | channel | SNR [dB] | BER no offset | BER plain | BER sync (W = %d) | BER sync + cfo | abs(est - eps): median, p95 |\n"
                "|---|---|---|---|---|---|---|---|\n" % a.W)
        for r in rows:
            f.write("| %g | %s | %g | %s | %s | %s | %s | %.2g, %.2g |\n"
                    % (r["eps_max"], r["channel"], r["snr_db"], cell(r["no_offset"]), cell(r["plain"]), cell(r["sync"]),
                       cell(r["sync_cfo"]), r["cfo_abs_err"]["median"], r["cfo_abs_err"]["p95"]))


CAPTURE_CHANNELS = ("EPA", "EVA", "ETU")


def capture_rows(a, tr, hf, snrs, log):
    """the --capture table: one row per (channel, SNR, eps = 0 | one eps ~ U(-0.2, 0.2) per capture).  Captures come from the host
    model (radio.rayleigh_chan_lte.run_stream: every frame's full convolution overlap-added, so a frame's tails fall into its
    neighbours; white noise over the whole capture; radio.apply_cfo_stream: one phase running over the capture)."""
    import torch
    from dl_ofdm_amd import ofdm, util
    from dl_ofdm_amd.radio import apply_cfo_stream, rayleigh_chan_lte
    n, W, lead = a.frames, a.W, 64
    EPS = float(a.cfo.split(",")[0]) if a.cfo else 0.2
    pooled = a.cfo_scope == "capture"
    rows = []
    for ch in CAPTURE_CHANNELS:
        fl = copy.deepcopy(hf)
        fl.channel = ch
        o = ofdm.ofdm_tx(fl)
        S, K, CP = int(fl.nsymbol), int(o.K), int(o.CP)
        T = S * (K + CP)
        fading = rayleigh_chan_lte(fl, o.Fs)
        for i, snr in enumerate(snrs):
            for impaired in (False, True):
                got = {"capture": [], "cut": [], "baseline": []}
                if pooled and impaired:
                    got.update(capture_pooled=[], capture_offset_free=[])
                hist, errs, eps_used, pooled_errs = {}, [], [], []
                for sd in range(a.seeds):
                    np.random.seed(77 + 13 * i + 1009 * sd)
                    bits = util.bit_source(fl.nbits, o.frame_size, n)
                    iq, _, _ = o.ofdm_tx_frame_np(bits)
                    c, _ = fading.run_stream(iq, lead)
                    c = c.astype(np.complex128)
                    c /= np.sqrt(np.mean(np.abs(c[lead:lead + n * T]) ** 2))          # unit mean power over the frames
                    std = np.sqrt(0.5) * 10.0 ** (-snr / 20.0)
                    c = c + std * (np.random.randn(c.shape[0]) + 1j * np.random.randn(c.shape[0]))
                    eps = float(np.random.uniform(-EPS, EPS)) if impaired else 0.0
                    eps_used.append(eps)
                    clean = np.stack([c.real, c.imag], axis=-1).astype(np.float32)
                    cap = torch.as_tensor(apply_cfo_stream(clean, eps, K) if impaired else clean, device=tr.device)
                    lab = torch.as_tensor(bits.astype(np.int32), device=tr.device)
                    ber = lambda res: float((res.bits().to(torch.int32) != lab).to(torch.float32).mean())   # noqa: E731
                    res = tr.receive_capture(cap, lead, sync=W, cfo=impaired)
                    got["capture"].append(ber(res))
                    for v, cnt in zip(*[t.tolist() for t in torch.unique(res.offset, return_counts=True)]):
                        hist[int(v)] = hist.get(int(v), 0) + int(cnt)
                    if impaired:
                        d = res.cfo.to(torch.float64) - eps
                        errs.append((d - torch.round(d)).abs())
                    if pooled and impaired:
                        resp = tr.receive_capture(cap, lead, sync=W, cfo=True, cfo_scope="capture")
                        got["capture_pooled"].append(ber(resp))
                        d = float(resp.cfo[0]) - eps
                        pooled_errs.append(abs(d - round(d)))
                        got["capture_offset_free"].append(ber(tr.receive_capture(torch.as_tensor(clean, device=tr.device), lead, sync=W)))
                    x_nom = cap[lead:lead + n * T].view(n, S, K + CP, 2)              # the same capture cut at the nominal starts
                    got["cut"].append(ber(tr.receive(x_nom, sync=W, cfo=impaired)))
                    x_free = torch.as_tensor(clean[lead:lead + n * T], device=tr.device).view(n, S, K + CP, 2)
                    got["baseline"].append(ber(tr.receive(x_free)))                   # no offset, no alignment
                row = {"channel": ch, "snr_db": snr, "impaired": impaired, "eps": eps_used,
                       "offset_share": {str(k): round(v / (n * a.seeds), 4) for k, v in sorted(hist.items())}}
                if errs:
                    e = torch.cat(errs)
                    row["cfo_abs_err"] = {"median": float(e.median()), "p95": float(torch.quantile(e, 0.95)), "max": float(e.max())}
                if pooled_errs:
                    row["cfo_pooled_abs_err"] = {"median": float(np.median(pooled_errs)), "max": float(np.max(pooled_errs)),
                                                 "per_capture": pooled_errs}
                for k, v in got.items():
                    row[k] = {"ber": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                rows.append(row)
                print(json.dumps(row), flush=True)
    log["capture_rows"] = rows
    log["eps_max"] = EPS
    with open(os.path.join(a.out, "syncber_capture_%dmod.json" % a.nbits), "w") as f:
        json.dump(log, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "syncber_capture_%dmod.md" % a.nbits), "w") as f:
        cell = lambda c: "%.3g (%.3g .. %.3g)" % (c["ber"], c["min"], c["max"])      # noqa: E731
        f.write("| channel | SNR [dB] | eps | BER receive_capture | BER receive(sync=%d[, cfo]) on the nominal cut | BER baseline (no offset, "
                "no alignment) | offsets (share of frames) |\n|---|---|---|---|---|---|---|\n" % a.W)
        for r in rows:
            f.write("| %s | %g | %s | %s | %s | %s | %s |\n"
                    % (r["channel"], r["snr_db"], "U(-0.2, 0.2) per capture" if r["impaired"] else "0", cell(r["capture"]),
                       cell(r["cut"]), cell(r["baseline"]), ", ".join("%s: %.1f %%" % (k, 100 * v) for k, v in r["offset_share"].items())))
        if pooled:
            f.write("\n| channel | SNR [dB] | BER offset-free (receive_capture, eps = 0) | BER per-frame estimate | BER pooled estimate | "
                    "abs(est - eps) per frame: median, p95, worst | abs(est - eps) pooled: median, worst over the captures |\n"
                    "|---|---|---|---|---|---|---|\n")
            for r in rows:
                if r["impaired"]:
                    e, q = r["cfo_abs_err"], r["cfo_pooled_abs_err"]
                    f.write("| %s | %g | %s | %s | %s | %.2g, %.2g, %.2g | %.2g, %.2g |\n"
                            % (r["channel"], r["snr_db"], cell(r["capture_offset_free"]), cell(r["capture"]), cell(r["capture_pooled"]),
                               e["median"], e["p95"], e["max"], q["median"], q["max"]))


def noisy_stream(fl, o, fading, n_tx, T, lead, snr, seed, EPS):
    """one capture of the --acquire / --classical tables: ``n_tx`` frames through ``fading.run_stream``, unit mean power over the
    frames, white noise at ``snr`` dB, one carrier offset eps ~ U(-EPS, EPS) -> (bits, the noisy stream before the offset, eps,
    a random cut inside frame 0, the stream float32 [n, 2] under the offset)"""
    from dl_ofdm_amd import util
    from dl_ofdm_amd.radio import apply_cfo_stream
    np.random.seed(seed)
    bits = util.bit_source(fl.nbits, o.frame_size, n_tx)
    iq, _, _ = o.ofdm_tx_frame_np(bits)
    c, _ = fading.run_stream(iq, lead)
    c = c.astype(np.complex128)
    c /= np.sqrt(np.mean(np.abs(c[lead:lead + n_tx * T]) ** 2))
    std = np.sqrt(0.5) * 10.0 ** (-snr / 20.0)
    c = c + std * (np.random.randn(c.shape[0]) + 1j * np.random.randn(c.shape[0]))
    eps = float(np.random.uniform(-EPS, EPS))
    cut = int(np.random.randint(0, T))
    full = apply_cfo_stream(np.stack([c.real, c.imag], axis=-1).astype(np.float32), eps, int(o.K))
    return bits, c, eps, cut, full


def classical_rows(a, hf, snrs, log):
    """the --classical table: the label-free classical detector (``ClassicalRxReceiver``, method --classical) behind the SAME
    front end on the SAME captures as the --acquire table (noisy_stream: same seeds; ``receive_capture(first=None, acquire=16,
    cfo=True, cfo_scope="capture")``), one row per (channel, SNR): BER with the start known and behind acquisition, with the
    noise variance estimated from the empty carriers and with the true one given.  No training."""
    import torch
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.benchmark import ClassicalReceiver
    from dl_ofdm_amd.classical_receive import ClassicalRxReceiver
    from dl_ofdm_amd.radio import rayleigh_chan_lte
    n, W, lead, J = a.frames, a.W, 64, 16
    lo = W
    rows = []
    for ch in CAPTURE_CHANNELS:
        fl = copy.deepcopy(hf)
        fl.channel = ch
        o = ofdm.ofdm_tx(fl)
        S, K, CP = int(fl.nsymbol), int(o.K), int(o.CP)
        T = S * (K + CP)
        n_tx = max(n, J) + 4
        fading = rayleigh_chan_lte(fl, o.Fs)
        adv = min(ClassicalReceiver.advance_of(fading), CP)
        for i, snr in enumerate(snrs):
            rx = {"estimated": ClassicalRxReceiver(fl, n, a.classical, advance=adv),
                  "given": ClassicalRxReceiver(fl, n, a.classical, advance=adv, noise_var=K * 10.0 ** (-snr / 10.0))}
            got = {k: {"known": [], "acquired": []} for k in rx}
            nv = []
            for c_i in range(a.captures):
                bits, _, _, cut, full = noisy_stream(fl, o, fading, n_tx, T, lead, snr, 177 + 13 * i + 1009 * c_i, 0.2)
                cap = torch.as_tensor(np.ascontiguousarray(full[lead + cut:]), device="cuda")
                m0 = -(-(lo + cut) // T)
                true = m0 * T - cut
                lab = torch.as_tensor(bits[m0:m0 + n].astype(np.int32), device="cuda")
                ber = lambda res: float((res.bits().to(torch.int32) != lab).to(torch.float32).mean())   # noqa: E731
                for k, r in rx.items():
                    got[k]["known"].append(ber(r.receive_capture(cap, true, sync=W, cfo=True, cfo_scope="capture")))
                    got[k]["acquired"].append(ber(r.receive_capture(cap, sync=W, cfo=True, cfo_scope="capture", acquire=J, lo=lo)))
                nv.append(float(rx["estimated"].noise.median()) / (K * 10.0 ** (-snr / 10.0)))
            row = {"channel": ch, "snr_db": snr, "captures": a.captures, "frames": n, "method": a.classical, "advance": adv,
                   "noise_estimate_over_true": float(np.median(nv)),
                   "ber": {k: {q: float(np.mean(v)) for q, v in g.items()} for k, g in got.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    log["classical_rows"] = rows
    with open(os.path.join(a.out, "syncber_classical_%dmod.json" % a.nbits), "w") as f:
        json.dump(log, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "syncber_classical_%dmod.md" % a.nbits), "w") as f:
        f.write("| channel | SNR [dB] | BER %s, start known | BER behind acquire = 16 | BER, true noise variance given, start known | "
                "median noise estimate / true |\n|---|---|---|---|---|---|\n" % a.classical)
        for r in rows:
            f.write("| %s | %g | %.3g | %.3g | %.3g | %.3f |\n" % (r["channel"], r["snr_db"], r["ber"]["estimated"]["known"],
                                                                r["ber"]["estimated"]["acquired"], r["ber"]["given"]["known"],
                                                                r["noise_estimate_over_true"]))


def acquire_rows(a, tr, hf, snrs, log):
    """the --acquire table: one row per (channel, SNR): the share of captures whose start acquisition finds (within W samples of
    the true frame start: the refinement behind it absorbs that) at each J, and the chain's BER behind it against the BER with the
    start known.  Captures as in capture_rows (run_stream, white noise, one eps ~ U(-0.2, 0.2) per capture), each beginning at a
    random sample inside frame 0; the search starts at lo = W.

    ``--cfo_span M``: the fraction is drawn from U(-1/2, 1/2) and every capture exists twice, under eps = f (the columns above, the
    narrow path) and under eps = m + f, m uniform in [-M, M]: there ``receive_capture(..., acquire=J, cfo_span=M)`` must find the
    start and the whole offset (|m^ + eps^ - eps| < 0.1), and the narrow call at the largest J shows what the offset costs it."""
    import torch
    from dl_ofdm_amd import ofdm, util
    from dl_ofdm_amd.radio import apply_cfo_stream, rayleigh_chan_lte
    M = int(a.cfo_span)
    n, W, lead, EPS = a.frames, a.W, 64, (0.5 if M else 0.2)
    Js = [int(v) for v in a.acquire.split(",")]
    lo = W
    rows = []
    for ch in CAPTURE_CHANNELS:
        fl = copy.deepcopy(hf)
        fl.channel = ch
        o = ofdm.ofdm_tx(fl)
        S, K, CP = int(fl.nsymbol), int(o.K), int(o.CP)
        T = S * (K + CP)
        n_tx = max(n, max(Js)) + 4
        fading = rayleigh_chan_lte(fl, o.Fs)
        for i, snr in enumerate(snrs):
            right = {J: 0 for J in Js}
            err = {J: {} for J in Js}
            ber_right = {J: [] for J in Js}
            ber_all = {J: [] for J in Js}
            ber_known = []
            wide = {J: {"right": 0, "int_right": 0, "ber_right": [], "ber_all": []} for J in Js}
            ber_narrow_on_wide = []
            for c_i in range(a.captures):
                bits, c, eps, cut, full = noisy_stream(fl, o, fading, n_tx, T, lead, snr, 177 + 13 * i + 1009 * c_i, EPS)
                cap = torch.as_tensor(np.ascontiguousarray(full[lead + cut:]), device=tr.device)
                m0 = -(-(lo + cut) // T)                                              # the first transmitted frame that starts at or after lo
                true = m0 * T - cut
                lab = torch.as_tensor(bits[m0:m0 + n].astype(np.int32), device=tr.device)
                ber = lambda res: float((res.bits().to(torch.int32) != lab).to(torch.float32).mean())   # noqa: E731
                ber_known.append(ber(tr.receive_capture(cap, true, sync=W, cfo=True, frames=n)))
                for J in Js:
                    res = tr.receive_capture(cap, sync=W, cfo=True, frames=n, acquire=J, lo=lo)
                    d = (int(res.first[0]) - true + T // 2) % T - T // 2
                    err[J][d] = err[J].get(d, 0) + 1
                    b = ber(res)
                    ber_all[J].append(b)
                    if abs(d) <= W:
                        right[J] += 1
                        ber_right[J].append(b)
                if M:
                    m = int(np.random.randint(-M, M + 1))
                    full = apply_cfo_stream(np.stack([c.real, c.imag], axis=-1).astype(np.float32), m + eps, K)
                    capw = torch.as_tensor(np.ascontiguousarray(full[lead + cut:]), device=tr.device)
                    for J in Js:
                        res = tr.receive_capture(capw, sync=W, cfo=True, frames=n, acquire=J, lo=lo, cfo_span=M)
                        d = (int(res.first[0]) - true + T // 2) % T - T // 2
                        whole = abs(int(res.acquired_cfo_int[0]) + float(res.acquired_cfo[0]) - (m + eps)) < 0.1
                        b = ber(res)
                        wide[J]["ber_all"].append(b)
                        wide[J]["int_right"] += bool(whole)
                        if abs(d) <= W and whole:
                            wide[J]["right"] += 1
                            wide[J]["ber_right"].append(b)
                    ber_narrow_on_wide.append(ber(tr.receive_capture(capw, sync=W, cfo=True, frames=n, acquire=max(Js), lo=lo)))
            row = {"channel": ch, "snr_db": snr, "captures": a.captures, "frames": n,
                   "ber_known": float(np.mean(ber_known)),
                   "acquire": {str(J): {"share_right": right[J] / a.captures,
                                        "first_minus_true": {str(k): v for k, v in sorted(err[J].items())},
                                        "ber_where_right": float(np.mean(ber_right[J])) if ber_right[J] else None,
                                        "ber_all": float(np.mean(ber_all[J]))} for J in Js}}
            if M:
                row["cfo_span"] = M
                row["wide"] = {str(J): {"share_right": q["right"] / a.captures, "share_offset_right": q["int_right"] / a.captures,
                                        "ber_where_right": float(np.mean(q["ber_right"])) if q["ber_right"] else None,
                                        "ber_all": float(np.mean(q["ber_all"]))} for J, q in wide.items()}
                row["ber_narrow_on_wide_offsets"] = float(np.mean(ber_narrow_on_wide))
            rows.append(row)
            print(json.dumps(row), flush=True)
    log["acquire_rows"] = rows
    with open(os.path.join(a.out, "syncber_acquire_%dmod.json" % a.nbits), "w") as f:
        json.dump(log, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "syncber_acquire_%dmod.md" % a.nbits), "w") as f:
        f.write("| channel | SNR [dB] | BER, start known | " + " | ".join("J = %d: acquired / BER where acquired / BER over all" % J for J in Js)
                + " |\n|---|---|---|" + "---|" * len(Js) + "\n")
        for r in rows:
            cells = []
            for J in Js:
                q = r["acquire"][str(J)]
                cells.append("%d of %d / %s / %.3g" % (round(q["share_right"] * r["captures"]), r["captures"],
                                                      "-" if q["ber_where_right"] is None else "%.3g" % q["ber_where_right"], q["ber_all"]))
            f.write("| %s | %g | %.3g | %s |\n" % (r["channel"], r["snr_db"], r["ber_known"], " | ".join(cells)))
        if M:
            f.write("\neps = m + f, |m| <= %d, cfo_span = %d\n\n| channel | SNR [dB] | " % (M, M)
                    + " | ".join("J = %d: start and offset found / BER where found / BER over all" % J for J in Js)
                    + " | BER, cfo_span = 0 at J = %d |\n|---|---|" % max(Js) + "---|" * (len(Js) + 1) + "\n")
            for r in rows:
                cells = []
                for J in Js:
                    q = r["wide"][str(J)]
                    cells.append("%d of %d / %s / %.3g" % (round(q["share_right"] * r["captures"]), r["captures"],
                                                          "-" if q["ber_where_right"] is None else "%.3g" % q["ber_where_right"],
                                                          q["ber_all"]))
                f.write("| %s | %g | %s | %.3g |\n" % (r["channel"], r["snr_db"], " | ".join(cells), r["ber_narrow_on_wide_offsets"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbits", type=int, default=2)
    ap.add_argument("--train_channel", default="mixRayleigh")
    ap.add_argument("--snrs", default="5,11,20,29,40")
    ap.add_argument("--frames", type=int, default=20000, help="frames per point and seed")
    ap.add_argument("--seeds", type=int, default=3, help="independent evaluation batches per point (the spread is over them)")
    ap.add_argument("--W", type=int, default=3)
    ap.add_argument("--rx_epochs", type=int, default=0)
    ap.add_argument("--eq_epochs", type=int, default=0)
    ap.add_argument("--load", default=None, help="equaliser checkpoint (receiver_mp.save_checkpoint) instead of training")
    ap.add_argument("--rx_load", default=None, help="basic-receiver checkpoint stem that goes with --load")
    ap.add_argument("--train_sync", type=int, default=0, help="W > 0: also train an equaliser with sync=W and evaluate it on aligned frames")
    ap.add_argument("--rx_sync", action="store_true", help="with --train_sync: the second chain's basic receiver trains on aligned frames too")
    ap.add_argument("--cfo", default=None, help="EPS[,EPS...]: per-frame carrier-frequency offsets ~ U(-EPS, EPS) subcarrier spacings "
                                                "on the evaluation frames; reports the receive path with and without cfo=True")
    ap.add_argument("--capture", action="store_true",
                    help="contiguous captures from the host model (run_stream): receive_capture against receive(sync=W[, cfo=True]) on the "
                         "same capture cut at the nominal starts, and the offset-free unaligned baseline; EPA / EVA / ETU at --snrs")
    ap.add_argument("--cfo_scope", "--cfo-scope", default="frame", choices=["frame", "capture"],
                    help="capture: the --capture table (also selected by --cfo EPS --cfo_scope capture, eps ~ U(-EPS, EPS) per capture) "
                         "with the estimate pooled over each capture next to the per-frame one")
    ap.add_argument("--acquire", default=None,
                    help="J[,J...]: captures that begin inside frame 0 (host model as --capture, one eps ~ U(-0.2, 0.2) each): the share "
                         "whose start receive_capture(first=None, acquire=J) finds, and the chain's BER behind it; --frames per capture")
    ap.add_argument("--captures", type=int, default=30, help="--acquire: captures per channel and SNR")
    ap.add_argument("--cfo_span", "--cfo-span", type=int, default=0,
                    help="M, with --acquire: every capture also under eps = m + f, m uniform in [-M, M], f ~ U(-1/2, 1/2), received "
                         "with receive_capture(..., acquire=J, cfo_span=M), next to the narrow path on eps = f and on eps = m + f")
    ap.add_argument("--classical", default=None, metavar="METHOD",
                    help="ALMMSE | LS-Spline | LS-Linear: the classical detector (ClassicalRxReceiver) behind the same front end on the "
                         "--acquire table's captures (receive_capture, pooled offset, acquire = 16); trains nothing; --frames per capture")
    ap.add_argument("--out", default="syncber_out")
    a = ap.parse_args()
    if a.cfo_span and not a.acquire:
        ap.error("--cfo_span M goes with --acquire J[,J...]: the whole spacings are only known through acquisition")
    if a.cfo_scope == "capture":
        if not (a.capture or a.cfo) or a.acquire:
            ap.error("--cfo_scope capture goes with --capture or --cfo EPS")
        a.capture = True
    import torch
    from dl_ofdm_amd import _lib, ofdm, receiver as R, receiver_mp as H
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.sync import FrameSync
    os.makedirs(a.out, exist_ok=True)
    nb, snrs = a.nbits, [float(s) for s in a.snrs.split(",")]
    save = tempfile.mkdtemp(prefix="dccn_syncber_") + "/"
    t0 = time.time()
    log = {"build_id": _lib.load().dccn_build_id().decode(), "nbits": nb, "W": a.W, "frames": a.frames, "seeds": a.seeds,
           "train_channel": a.train_channel, "snrs": snrs}
    hf = H.Flags(nbits=nb, nfilter=64, channel=a.train_channel, max_epoch_num=a.eq_epochs if a.eq_epochs > 0 else 4000 * nb,
                 early_stop=200, token="syncber", save_dir=save, device_data=True, seed=10 + nb, test_frames=a.frames)
    if a.classical:
        classical_rows(a, hf, snrs, log)
        return
    if a.load:
        from dl_ofdm_amd.equalizer import EqualizerTrainer
        from dl_ofdm_amd.session import Session, load_model_np
        sess = Session(device="cuda", seed=1)
        load_model_np(a.rx_load, sess)
        tr = EqualizerTrainer(hf, ofdm.ofdm_tx(hf), dict(sess.params), seed=hf.seed)
        H.load_checkpoint(a.load, tr, with_optimizer=False)
        log["loaded"] = [a.rx_load, a.load]
    else:
        rf = R.Flags(nbits=nb, nfilter=64, channel="AWGN", SNR=5.0 * nb, max_epoch_num=a.rx_epochs if a.rx_epochs > 0 else 1200 * nb,
                     early_stop=200, token="syncber_%dmod" % nb, save_dir=save, device_data=True, seed=nb)
        res = R.train(rf, verbose=False, run_test=False)
        log["receiver"] = {"epochs": len(res["history"]), "seconds": round(time.time() - t0, 1),
                           "best_train_loss": min(h["train_loss"] for h in res["history"])}
        t1 = time.time()
        out = H.train(hf, verbose=False, run_test=False, rx_params=res["params"])
        H.load_checkpoint(out["best_path"], out["trainer"], with_optimizer=False)
        tr = out["trainer"]
        best = min(out["history"], key=lambda h: h["train_loss"])
        log["equalizer"] = {"epochs": len(out["history"]), "seconds": round(time.time() - t1, 1), "best_train_loss": best["train_loss"],
                            "best_epoch": best["epoch"], "test_ber_at_best": best["test_ber"]}
    tr2 = None
    if a.train_sync > 0:
        if a.load:
            raise SystemExit("--train_sync trains its own chains: not together with --load")
        t2 = time.time()
        rx2 = res["params"]
        if a.rx_sync:
            rf2 = copy.deepcopy(rf)
            rf2.sync, rf2.token = a.train_sync, rf.token + "_sync"
            res2 = R.train(rf2, verbose=False, run_test=False)
            rx2 = res2["params"]
            log["receiver_sync"] = {"epochs": len(res2["history"]), "best_train_loss": min(h["train_loss"] for h in res2["history"])}
        hf2 = copy.deepcopy(hf)
        hf2.sync, hf2.token = a.train_sync, hf.token + "_sync"
        out2 = H.train(hf2, verbose=False, run_test=False, rx_params=rx2)
        H.load_checkpoint(out2["best_path"], out2["trainer"], with_optimizer=False)
        tr2 = out2["trainer"]
        best2 = min(out2["history"], key=lambda h: h["train_loss"])
        log["equalizer_sync"] = {"W": a.train_sync, "rx_sync": bool(a.rx_sync), "epochs": len(out2["history"]),
                                 "seconds": round(time.time() - t2, 1), "best_train_loss": best2["train_loss"],
                                 "best_epoch": best2["epoch"], "test_ber_at_best": best2["test_ber"]}
    print(json.dumps(log), flush=True)
    if a.acquire:
        acquire_rows(a, tr, hf, snrs, log)
        return
    if a.capture:
        capture_rows(a, tr, hf, snrs, log)
        return
    if a.cfo:
        cfo_rows(a, tr, hf, snrs, log)
        return
    o = tr.ofdmobj
    S, K, CP = int(hf.nsymbol), int(o.K), int(o.CP)
    pl = tr.resident(a.frames)
    scratch = torch.empty_like(pl.x)
    fs = FrameSync(S, K, CP, a.W, a.frames, tr.device, want_metric=False)

    def ber():
        pl.run(False)
        return float(tr._metrics(pl.metrics_buf, pl.tx_power)["berlin"])

    pl2 = tr2.resident(a.frames) if tr2 is not None else None
    fs2 = FrameSync(S, K, CP, a.train_sync, a.frames, tr.device, want_metric=False) if (tr2 is not None and a.train_sync != a.W) else fs

    def ber2():
        """the sync-trained chain on the frames aligned with ITS window"""
        fs2.run(scratch, out=pl2.x)
        pl2.bits.copy_(pl.bits)
        pl2.run(False)
        return float(tr2._metrics(pl2.metrics_buf, pl2.tx_power)["berlin"])

    rows = []
    for ch in CHANNELS:
        fl = copy.deepcopy(hf)
        fl.channel = ch
        gen = DeviceDataGen(fl, ofdm.ofdm_tx(fl), device=tr.device, seed=77)
        gen.want_noise_power = False
        adv = 0 if gen.mixed else (gen.L - 1) // 2
        for i, snr in enumerate(snrs):
            got = {"plain": [], "sync": [], "known": [], "sync_trained": []}
            hist = {}
            for sd in range(a.seeds):
                gen.seed, gen.offset = 77 + 13 * i + 1009 * sd, 0
                gen.make_batch(a.frames, snr, out_x=scratch, out_bits=pl.bits)
                pl.x.copy_(scratch)
                got["plain"].append(ber())
                _, off = fs.run(scratch, out=pl.x)
                got["sync"].append(ber())
                if tr2 is not None:
                    got["sync_trained"].append(ber2())
                for v, c in zip(*[t.tolist() for t in torch.unique(off, return_counts=True)]):
                    hist[int(v)] = hist.get(int(v), 0) + int(c)
                if not gen.mixed:
                    pl.x.copy_(torch.roll(scratch.view(a.frames, -1, 2), adv, dims=1).view_as(pl.x))
                    got["known"].append(ber())
            row = {"channel": ch, "snr_db": snr, "known_advance": None if gen.mixed else adv,
                   "offset_share": {str(k): round(v / (a.frames * a.seeds), 4) for k, v in sorted(hist.items())}}
            for k, v in got.items():
                row[k] = None if not v else {"ber": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    log["rows"] = rows
    log["total_seconds"] = round(time.time() - t0, 1)
    with open(os.path.join(a.out, "syncber_%dmod.json" % nb), "w") as f:
        json.dump(log, f, indent=1)
        f.write("\n")
    with open(os.path.join(a.out, "syncber_%dmod.md" % nb), "w") as f:
        cell = lambda c: "-" if c is None else "%.3g (%.3g .. %.3g)" % (c["ber"], c["min"], c["max"])      # noqa: E731
        shares = lambda r: ", ".join("%s: %.1f %%" % (k, 100 * v) for k, v in r["offset_share"].items())   # noqa: E731
        if tr2 is None:
            f.write("| channel | SNR [dB] | BER plain | BER sync (W = %d) | BER known advance | offsets (share of frames) |\n|---|---|---|---|---|---|\n" % a.W)
            for r in rows:
                f.write("| %s | %g | %s | %s | %s | %s |\n" % (r["channel"], r["snr_db"], cell(r["plain"]), cell(r["sync"]), cell(r["known"]), shares(r)))
        else:
            f.write("| channel | SNR [dB] | plain-trained, plain frames | plain-trained, aligned frames (W = %d) | sync-trained (W = %d), aligned frames |\n"
                    "|---|---|---|---|---|\n" % (a.W, a.train_sync))
            for r in rows:
                f.write("| %s | %g | %s | %s | %s |\n" % (r["channel"], r["snr_db"], cell(r["plain"]), cell(r["sync"]), cell(r["sync_trained"])))


if __name__ == "__main__":
    main()
