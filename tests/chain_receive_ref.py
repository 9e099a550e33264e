"""The checker of the chain's receive step (include/dccn.h ``dccn_eq_receive_step``: IQ frames -> equaliser -> frozen receiver ->
packed bits, LLRs, probabilities) and the cases the host test (tests/test_chain_receive_checker.py) and the GPU test
(tests/test_gpu_chain_receive.py) share.

``check_receive`` takes one receive call's tensors and makes two sets of checks, each under a name of its own:

  stages          ``check_forward`` of tests/test_gpu_equalizer_stages.py on the step's own workspace tensors: R0 through dense_5
                  and the pilot SNR, each against float64 on the step's OWN input to that stage, at that checker's 1e-5 with its
                  |h| margin and cap.  (Its labels are zeros here; its ce_mean / confusion table are not used.)
  llr, prob       the frozen receiver in float64 (``O.rx_forward(..., keep=True)``) on the step's own ``out_eq`` -- the window
                  behind the prefix when ``cp`` is off: ``llr`` against ``u1 - u0`` of the post-leaky-ReLU logits, ``prob``
                  against the softmax pairs, each to TOL = 1e-5 of the reference tensor's maximum (RTOL of test_gpu_receive.py,
                  TOL of the stage checker).
  decisions       ``packed`` unpacked against the oracle's argmax: exact on every cell with |p1 - p0| >= TIE_MARGIN = 2e-5 (the
                  margin of the stage checker's _check_metrics: float32 and float64 may fall on either side of a tie)
  ties            the cells inside that margin number at most 5e-3 cells + 4 (the cap of test_receive_matches_the_fp64_oracle)
  padding         the padding bits of each row's last byte are 0
  layout          row f is ``numpy.packbits(hard[f].reshape(-1))``: ``receive.pack_bits`` of the bits numpy itself unpacks
                  (``numpy.unpackbits``: most significant bit first, independent of ``receive.unpack_bits``) gives ``packed``
                  back, ``receive.unpack_bits`` agrees with numpy, and -- a round trip cannot tell one bit order from the other --
                  the bits read most-significant-first fit the step's own outputs (the signs of its LLRs or the argmax of its
                  ``prob``, whichever they fit best) on more cells than the bits read least-significant-first do
  prob coherence  all cells: hard == (prob[..., 1] > prob[..., 0]) on the step's own ``prob``
  llr coherence   where |llr| > 1e-6: hard == (llr > 0) on the step's own ``llr``

``check_receive`` returns the names that failed and the figures; the caller asserts.  Bits packed in the wrong order fail
``layout`` and ``decisions`` and -- by the definition of the two coherence checks, which read the same bits -- both of those.
"""
import ctypes as C

import numpy as np

from oracle import dccn_oracle as O

TOL = 1e-5
TIE_MARGIN = 2e-5
LLR_FLOOR = 1e-6
CHECKS = ("stages", "llr", "prob", "decisions", "ties", "padding", "layout", "prob coherence", "llr coherence")


def tie_cap(cells):
    return 5e-3 * cells + 4


def _geo(nfft, longcp, cp):
    return dict(nfft=nfft, longcp=longcp, cp=cp, rx_bias=0.05)


def _route(fold_k, group, rides, bn, rx_k, grid, window):
    """what `route_of` must answer: fold_k: the folded matrix's row count S * 2 n_sc (dccn_eq_rx_folded_floats); group:
    dccn_eq_receive_group_supported (at N = 64, where rides and bn are 1: the few-row receiver is folded into one matrix);
    rides / bn: dccn_eq_norm_rides / dccn_eq_bottleneck_supported; tail_eval: dccn_rx_dense_tail_fused(rsh, 0), 1 in every case;
    rx_k: the k extent of the receiver's dense layer as the step runs it (fold_k where folded, else S * 2 F); grid: (grid kind,
    tile rows, ragged rows, blocks) of dccn_dense_tail_grid(B, rx_k, 2 D, nbits) for nbits <= 2 (grid kind 1: the 16-row few-row
    tiles), None for 8-QAM / 16-QAM, whose decision is a launch of its own; decide: dccn_dense_decide_supported at the same
    extents, 1 in every case; window: byte offset, modulo 16, of the window behind the prefix"""
    return dict(fold_k=fold_k, group=group, rides=rides, bn=bn, tail_eval=1, rx_k=rx_k, grid=grid, decide=1, window=window)


# The routes are the queries' own answers (host only; tests/test_chain_receive_checker.py asserts them without a device too).
# frames: RandomState(500 + B + nbits); chain: test_gpu_equalizer._trainer(nbits, seed=71 + B, rx_bias=0.05, **geometry)
CASES = {
    # a / a1: folded few-row decide, K = 1120 with zero prefix rows (QPSK, BPSK instantiation); group-supported
    "a": dict(nbits=2, B=73, geometry=_geo(64, True, False), route=_route(1120, 1, 1, 1, 1120, (1, 16, 0, 200), 0)),
    "a1": dict(nbits=1, B=73, geometry=_geo(64, True, False), route=_route(1120, 1, 1, 1, 1120, (1, 16, 0, 200), 0)),
    # a3: folded few-row dense storing z, then the stand-alone decision kernel
    "a3": dict(nbits=3, B=73, geometry=_geo(64, True, False), route=_route(1120, 1, 1, 1, 1120, None, 0)),
    # b: the smallest batch without the few-row plan: C-Conv on the 128 B window, 48-row tiles storing z (one row left in the
    # third tile row), decision kernel
    "b": dict(nbits=4, B=97, geometry=_geo(64, True, False), route=_route(1120, 0, 1, 1, 896, None, 0)),
    # c: few-row receiver NOT folded (952 % 16 = 8): its own C-Conv at ld = 136, few-row decide at K = 896
    "c": dict(nbits=2, B=73, geometry=_geo(64, False, True), route=_route(952, 0, 1, 1, 896, (1, 16, 0, 200), 0)),
    # d: 32 B window, few-row dense + decision kernel
    "d": dict(nbits=3, B=73, geometry=_geo(64, False, False), route=_route(952, 0, 1, 1, 896, None, 0)),
    # d2: dense + decide on 48x64 tiles, ragged last tile row (97 = 2 * 48 + 1: three tile rows of ten tiles)
    "d2": dict(nbits=2, B=97, geometry=_geo(64, False, False), route=_route(952, 0, 1, 1, 896, (0, 48, 0, 30), 0)),
    # e: one partial 16-row tile
    "e": dict(nbits=1, B=12, geometry=_geo(64, False, True), route=_route(952, 0, 1, 1, 896, (1, 16, 0, 40), 0)),
    # f: K = 1792, N = 1280, D = 640; multi-launch norm, bottleneck as GEMMs; 274-float rows
    "f": dict(nbits=2, B=12, geometry=_geo(128, False, True), route=_route(1918, 0, 0, 0, 1792, (0, 48, 0, 20), 0)),
    # g: 72 B window (8 mod 16), 16-QAM float4 LLR stores
    "g": dict(nbits=4, B=12, geometry=_geo(128, False, False), route=_route(1918, 0, 0, 0, 1792, None, 8)),
    # h: BPSK, 129 rows at N = 1280 (three tile rows of twenty tiles); row_bytes = 80
    "h": dict(nbits=1, B=129, geometry=_geo(128, False, True), route=_route(1918, 0, 0, 0, 1792, (0, 48, 0, 60), 0)),
    # i: 320-float rows; 8-QAM rows of 240 bytes
    "i": dict(nbits=3, B=73, geometry=_geo(128, True, True), route=_route(2240, 0, 1, 0, 1792, None, 0)),
}


def case_config(name):
    """(F, tx, ecfg, rcfg, pe, pr) of the case's chain, host only: what test_gpu_equalizer._trainer builds its trainer from"""
    from test_gpu_equalizer import _trainer_config
    c = CASES[name]
    return _trainer_config(c["nbits"], 71 + c["B"], **c["geometry"])


def case_rng(name):
    c = CASES[name]
    return np.random.RandomState(500 + c["B"] + c["nbits"])


def case_frames(rng, B, ecfg):
    """the case's frames, the first draw of its stream (the labels of the evaluation step are drawn after them)"""
    return (rng.standard_normal((B, ecfg.S, ecfg.n_sc, 2)) * 2).astype(np.float32)


def route_of(lib, B, ecfg, rcfg, rx_k):
    """what the library's own queries (host only, nothing is launched) say a receive step of this shape runs; rx_k: the k extent
    the case expects of the receiver's dense layer, at which the grid and the decide queries are asked"""
    from dl_ofdm_amd import _lib
    from test_gpu_equalizer_stages import eq_shape
    sh = eq_shape(B, ecfg, rcfg)
    rsh = _lib.RxShape(B, rcfg.S, rcfg.kin, rcfg.F, rcfg.D, rcfg.nbits)
    dN = 2 * rcfg.D
    n = int(lib.dccn_eq_rx_folded_floats(C.byref(sh)))
    assert (n - dN) % dN == 0
    group = int(lib.dccn_eq_receive_group_supported(C.byref(sh)))
    if group:                                   # a group runs on the folded matrix alone
        assert rx_k == (n - dN) // dN, (rx_k, (n - dN) // dN)
    grid = None
    if rcfg.nbits <= 2:
        g = [C.c_int() for _ in range(4)]
        assert lib.dccn_dense_tail_grid(B, rx_k, dN, rcfg.nbits, *[C.byref(v) for v in g]) == 0, (B, rx_k, dN)
        grid = tuple(int(v.value) for v in g)
    return dict(fold_k=(n - dN) // dN, group=group, rides=int(lib.dccn_eq_norm_rides(C.byref(sh))),
                bn=int(lib.dccn_eq_bottleneck_supported(B, ecfg.S * ecfg.K * 2, 2 * ecfg.pilot_size)),
                tail_eval=int(lib.dccn_rx_dense_tail_fused(C.byref(rsh), 0)), rx_k=rx_k, grid=grid,
                decide=int(lib.dccn_dense_decide_supported(B, rx_k, dN, rcfg.nbits)), window=(0 if ecfg.cp else 8 * ecfg.CP) % 16)


def window(ecfg):
    """first sample of a row that the frozen receiver reads: 0, or CP (the K samples behind the cyclic prefix)"""
    return 0 if ecfg.cp else ecfg.CP


def oracle_decision(pr64, out_eq, ecfg, rcfg):
    """the frozen receiver in float64 on out_eq [B, S, n_sc, 2]: llr [B, D, nbits], prob [B, D, nbits, 2], hard (argmax, first
    index on ties), near (cells inside the tie margin)"""
    B = out_eq.shape[0]
    prob, t = O.rx_forward(pr64, np.asarray(out_eq, np.float64)[:, :, window(ecfg):, :], rcfg, keep=True)
    u = t["u"].reshape(B, rcfg.D, rcfg.nbits, 2)
    return dict(llr=u[..., 1] - u[..., 0], prob=prob, hard=(prob[..., 1] > prob[..., 0]).astype(np.uint8),
                near=np.abs(prob[..., 1] - prob[..., 0]) < TIE_MARGIN)


def numpy_unpack(packed, D, nbits):
    """uint8 [frames, row bytes] -> uint8 [frames, D, nbits] by numpy.unpackbits (most significant bit first)"""
    p = np.ascontiguousarray(np.asarray(packed, np.uint8))
    return np.unpackbits(p, axis=1)[:, :D * nbits].reshape(p.shape[0], D, nbits)


def padding_clear(packed, D, nbits):
    """the padding bits of each row's last byte (its low bits) are 0"""
    pad = packed.shape[1] * 8 - D * nbits
    assert 0 <= pad < 8
    return not pad or not (np.asarray(packed, np.uint8)[:, -1] & ((1 << pad) - 1)).any()


def check_receive(v, P, ecfg, rcfg, pr, packed, llr, prob, label=""):
    """v: name -> float64 array of the step's forward workspace tensors (FWD_NAMES of the stage checker) + "x", "h", "out_eq",
    "snr_db"; P: the equaliser's parameters (TF shapes, float64); pr: the frozen receiver's parameters; packed / llr / prob: the
    call's outputs (host arrays).  Returns (the set of failed check names, figures: name -> number)."""
    import torch
    from dl_ofdm_amd.receive import pack_bits, row_bytes, unpack_bits
    from oracle.torch_ref import LiteralRx
    from test_gpu_equalizer_stages import Stage, check_forward, rel
    D, nbits = rcfg.D, rcfg.nbits
    B = v["x"].shape[0]
    pr64 = {k: np.asarray(a, np.float64) for k, a in pr.items()}
    failed, fig = set(), {}

    # ---- forward stages ----------------------------------------------------------------------------------------------------
    st = Stage()
    lit_rx = LiteralRx(pr64, rcfg, dtype=torch.float64, literal_conv=False)
    check_forward(v, P, ecfg, lit_rx, np.zeros((B, D, nbits), np.int32), st)
    assert len(st.rows) == 15, [n for n, _, _ in st.rows]
    worst = max(st.rows, key=lambda r: r[1])
    fig["stages"], fig["worst stage"] = worst[1], worst[0]
    if any(not e <= tol for _, e, tol in st.rows):
        failed.add("stages")
        fig["failed stages"] = ["%s %.2e" % (n, e) for n, e, tol in st.rows if not e <= tol]

    # ---- decision stage ----------------------------------------------------------------------------------------------------
    ref = oracle_decision(pr64, v["out_eq"].reshape(B, ecfg.S, ecfg.n_sc, 2), ecfg, rcfg)
    llr, prob = np.asarray(llr, np.float64), np.asarray(prob, np.float64)
    packed = np.ascontiguousarray(np.asarray(packed, np.uint8))
    assert packed.shape == (B, row_bytes(D, nbits)) and llr.shape == (B, D, nbits) and prob.shape == (B, D, nbits, 2)
    fig["llr"], fig["prob"] = rel(llr, ref["llr"]), rel(prob, ref["prob"])
    for name in ("llr", "prob"):
        if not fig[name] <= TOL:
            failed.add(name)
    hard = numpy_unpack(packed, D, nbits)
    safe = ~ref["near"]
    fig["ties"], fig["cells"] = int(ref["near"].sum()), int(ref["near"].size)
    fig["ones"] = float(ref["hard"].mean())
    if fig["ties"] > tie_cap(fig["cells"]):
        failed.add("ties")
    fig["decisions"] = int((hard[safe] != ref["hard"][safe]).sum())
    if fig["decisions"]:
        failed.add("decisions")
    if not padding_clear(packed, D, nbits):
        failed.add("padding")
    lsb = np.unpackbits(packed, axis=1, bitorder="little")[:, :D * nbits].reshape(B, D, nbits)
    sign, arg = llr > 0, prob[..., 1] > prob[..., 0]
    big = np.abs(llr) > LLR_FLOOR
    fig["prob coherence"] = int((hard != arg).sum())
    fig["llr coherence"] = int((hard != sign)[big].sum())
    # (either of the step's own outputs may itself be the wrong one: the reading is judged by the one it fits best)
    fig["layout msb"] = min(fig["llr coherence"], fig["prob coherence"])
    fig["layout lsb"] = min(int((lsb != sign)[big].sum()), int((lsb != arg).sum()))
    if not (np.array_equal(pack_bits(hard), packed) and np.array_equal(unpack_bits(packed, D, nbits), hard)
            and np.array_equal(np.packbits(hard.reshape(B, -1), axis=1), packed)
            and (fig["layout msb"] == 0 or fig["layout msb"] < fig["layout lsb"])):
        failed.add("layout")
    for name in ("prob coherence", "llr coherence"):
        if fig[name]:
            failed.add(name)
    print("%s worst stage %.2e (%s) | llr %.2e | prob %.2e | near ties %d of %d (cap %d) | ones %.3f | failed: %s"
          % (label, fig["stages"], fig["worst stage"], fig["llr"], fig["prob"], fig["ties"], fig["cells"],
             int(tie_cap(fig["cells"])), fig["ones"], sorted(failed) or "none"))
    return failed, fig
