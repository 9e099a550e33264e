"""The label-free receive path on the GPU (``-m gpu``): IQ frames -> packed bits / LLRs / probabilities, held to the
evaluation step (exactly) and to the fp64 oracle (at the project's bounds).

Inputs: the five cases and the generator of tests/test_gpu_engine.py, re-stated here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def relerr(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def make_case(batch, nbits, kin=80, F=64, D=320, S=7, seed=0):
    from dl_ofdm_amd.engine import RxDims
    rng = np.random.RandomState(seed)
    dims = RxDims(S=S, kin=kin, F=F, D=D, nbits=nbits)
    cfg = O.RxConfig(S=S, kin=kin, F=F, D=D, nbits=nbits)
    x = (rng.randn(batch, S, kin, 2) * rng.uniform(0.5, 2.0, (S, kin, 2)) + 0.1 * rng.randn(S, kin, 2)).astype(np.float32)
    bits = rng.randint(0, 2, (batch, D, nbits)).astype(np.int32)
    p = O.init_params(cfg, seed=seed + 1)
    for k in p:
        if k.endswith("bias"):
            p[k] = rng.uniform(-0.05, 0.05, p[k].shape).astype(np.float32)
    p["demodulation/dense_1/kernel"] = (p["demodulation/dense_1/kernel"] * 1.0).astype(np.float32)
    return dims, cfg, x, bits, p


CASES = [  # (name, batch frames, nbits, kin, F, D)
    ("C1_bpsk_256sym", 36, 1, 80, 64, 320),
    ("C2_qpsk_8192sym", 1170, 2, 80, 64, 320),
    ("C3_16qam", 1170, 4, 80, 64, 320),
    ("qam8_nocp", 100, 3, 64, 64, 320),
    ("ragged", 13, 2, 20, 12, 50),
]


def host_conf(hard, bits):
    """the 2x2 table conf[label, pred] tallied on the host"""
    h, b = np.asarray(hard).reshape(-1).astype(np.int64), np.asarray(bits).reshape(-1).astype(np.int64)
    return [[int(((b == l) & (h == q)).sum()) for q in (0, 1)] for l in (0, 1)]


def unpack(res, D, nbits):
    from dl_ofdm_amd.receive import unpack_bits
    return unpack_bits(res.packed.cpu().numpy(), D, nbits)


@pytest.mark.parametrize("name,batch,nbits,kin,F,D", CASES)
def test_receive_agrees_exactly_with_the_eval_step(name, batch, nbits, kin, F, D):
    from dl_ofdm_amd.engine import RxEngine
    from dl_ofdm_amd.receive import RxReceiver, row_bytes
    dims, cfg, x, bits, p = make_case(batch, nbits, kin, F, D)
    eng = RxEngine(dims, batch, params=p, train=False, want_prob=True)
    eng.eval_step(x, bits)
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True)
    res = rcv.receive(x)
    torch.cuda.synchronize()
    assert res.packed.dtype == torch.uint8 and tuple(res.packed.shape) == (batch, row_bytes(D, nbits))
    hard = unpack(res, D, nbits)
    pe = eng.prob.cpu().numpy()
    assert np.array_equal(hard, (pe[..., 1] > pe[..., 0]).astype(np.uint8))
    assert np.array_equal(res.bits().cpu().numpy(), hard)                     # device-side unpack
    assert torch.equal(rcv.x_norm, eng.x_norm)
    assert torch.equal(rcv.fft_out, eng.fft_out)
    assert torch.equal(res.prob, eng.prob)
    m = eng.metrics()
    assert host_conf(hard, bits) == [[int(v) for v in row] for row in np.asarray(m["conf"]).reshape(2, 2)]
    # padding bits of the last byte of every row are 0
    pad = row_bytes(D, nbits) * 8 - D * nbits
    if pad:
        assert not (res.packed.cpu().numpy()[:, -1] & ((1 << pad) - 1)).any()


@pytest.mark.parametrize("name,batch,nbits,kin,F,D", CASES)
def test_receive_matches_the_fp64_oracle(name, batch, nbits, kin, F, D):
    from dl_ofdm_amd.receive import RxReceiver
    dims, cfg, x, bits, p = make_case(batch, nbits, kin, F, D)
    rcv = RxReceiver(dims, batch, p, want_llr=True)
    res = rcv.receive(x)
    torch.cuda.synchronize()
    hard = unpack(res, D, nbits).reshape(-1)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    xn, _, _ = O.batch_moment_norm(x.reshape(batch, -1).astype(np.float64))
    prob, sv = O.rx_forward(p64, xn.reshape(x.shape), cfg, keep=True)
    pr = prob.reshape(-1, 2)
    safe = np.abs(pr[:, 1] - pr[:, 0]) > 1e-5
    n_unsafe = int((~safe).sum())
    print("%s: %d of %d cells inside the 1e-5 margin" % (name, n_unsafe, pr.shape[0]))
    assert n_unsafe <= 5e-3 * pr.shape[0] + 4
    assert np.array_equal(hard[safe], (pr[:, 1] > pr[:, 0])[safe].astype(np.uint8))
    u = sv["u"].reshape(batch, D, nbits, 2)
    err = relerr(res.llr.cpu().numpy(), u[..., 1] - u[..., 0])
    print("%s: llr max|diff| / max|ref| = %.3g" % (name, err))
    assert err <= RTOL


def _tail_arena(p):
    return np.concatenate([p[n].reshape(-1) for n in ("demodulation/conv2d/kernel", "demodulation/conv2d/bias",
                                                      "demodulation/dense_1/kernel", "demodulation/dense_1/bias")]).astype(np.float32)


@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
@pytest.mark.parametrize("frames,D", [(13, 50), (37, 320)])
def test_stand_alone_decision_kernel(nbits, frames, D):
    from dl_ofdm_amd import _lib, ops
    from dl_ofdm_amd.receive import row_bytes, unpack_bits
    lib = _lib.load()
    cfg = O.RxConfig(S=7, kin=80, F=64, D=D, nbits=nbits)
    p = O.init_params(cfg, seed=3 + nbits)
    rng = np.random.RandomState(17 * nbits + D)
    for k in p:
        if k.endswith("bias"):
            p[k] = rng.uniform(-0.05, 0.05, p[k].shape).astype(np.float32)
    assert lib.dccn_tail_param_count(nbits) == _tail_arena(p).size
    z = (rng.randn(frames * D, 2) * 1.5).astype(np.float32)
    labels = rng.randint(0, 2, (frames * D, nbits)).astype(np.int32)     # for the evaluation tail: the oracle comparison ignores them
    dev = "cuda"
    zt, tp = torch.as_tensor(z, device=dev), torch.as_tensor(_tail_arena(p), device=dev)
    packed = torch.full((frames, row_bytes(D, nbits)), 0xAA, dtype=torch.uint8, device=dev)
    llr = torch.empty(frames, D, nbits, dtype=torch.float32, device=dev)
    prob = torch.empty(frames, D, nbits, 2, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.dccn_demod_decide(zt.data_ptr(), tp.data_ptr(), packed.data_ptr(), llr.data_ptr(), prob.data_ptr(), frames, D,
                                     nbits, st), "dccn_demod_decide")
    torch.cuda.synchronize()
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    tl = O.tail_forward_backward(z.astype(np.float64), labels, p64["demodulation/conv2d/kernel"],
                                 p64["demodulation/conv2d/bias"], p64["demodulation/dense_1/kernel"],
                                 p64["demodulation/dense_1/bias"], nbits)
    pt = tl["prob"].reshape(-1, 2)
    tie = np.abs(pt[:, 1] - pt[:, 0]) < 1e-6
    hard = unpack_bits(packed.cpu().numpy(), D, nbits).reshape(-1)
    assert np.array_equal(hard[~tie], (pt[:, 1] > pt[:, 0])[~tie].astype(np.uint8))
    u = O.leaky(tl["pre2"]).reshape(-1, 2)
    assert relerr(llr.cpu().numpy().reshape(-1), u[:, 1] - u[:, 0]) <= RTOL
    assert relerr(prob.cpu().numpy().reshape(-1, 2), pt) <= RTOL
    pad = row_bytes(D, nbits) * 8 - D * nbits
    if pad:
        assert not (packed.cpu().numpy()[:, -1] & ((1 << pad) - 1)).any()
    # sign coherence of the two outputs
    lv = llr.cpu().numpy().reshape(-1)
    big = np.abs(lv) > 1e-6
    assert np.array_equal(hard[big], (lv > 0)[big].astype(np.uint8))
    # the decision kernel and the evaluation tail call the same forward and softmax (tail.h tail_fwd_logits / tail_softmax): the
    # same floats, so the same decisions at EVERY cell (no tie mask) and the confusion table the evaluation tallies
    _, prob_eval, mbuf = ops.demod_tail_eval(zt, tp, torch.as_tensor(labels, device=dev), nbits)
    assert torch.equal(prob.reshape(-1, nbits, 2), prob_eval.reshape(-1, nbits, 2))
    pe = prob_eval.cpu().numpy().reshape(-1, 2)
    assert np.array_equal(hard, (pe[:, 1] > pe[:, 0]).astype(np.uint8))
    lab = labels.reshape(-1)
    conf = [[int(((lab == l) & (hard == h)).sum()) for h in (0, 1)] for l in (0, 1)]
    assert conf == ops.read_metrics(mbuf)["conf"]


@pytest.mark.parametrize("M,K,N,nbits", [(1170, 896, 640, 1), (1170, 896, 640, 2), (36, 896, 640, 1), (73, 896, 640, 2),
                                         (13, 168, 100, 2), (100, 896, 640, 3), (1170, 896, 640, 4),
                                         # odd k-tile counts of the two-ahead schedule (3 and 5 tiles of 64)
                                         (53, 192, 100, 2), (53, 320, 100, 2)])
def test_dense_decide_equals_dense_then_decide(M, K, N, nbits):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import row_bytes
    lib = _lib.load()
    assert lib.dccn_dense_decide_supported(M, K, N, nbits) == 1
    rng = np.random.RandomState(M + nbits)
    dev, f32 = "cuda", torch.float32
    x = torch.as_tensor(rng.randn(M, K).astype(np.float32), device=dev)
    w = torch.as_tensor((rng.randn(K, N) / math.sqrt(K)).astype(np.float32), device=dev)
    b = torch.as_tensor((0.05 * rng.randn(N)).astype(np.float32), device=dev)
    cfg = O.RxConfig(S=7, kin=80, F=64, D=N // 2, nbits=nbits)
    tp = torch.as_tensor(_tail_arena(O.init_params(cfg, seed=9)), device=dev)
    D, RB = N // 2, row_bytes(N // 2, nbits)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z1, z2 = torch.empty(M, N, dtype=f32, device=dev), torch.empty(M, N, dtype=f32, device=dev)
    pk1 = torch.full((M, RB), 0x55, dtype=torch.uint8, device=dev)
    pk2 = torch.full((M, RB), 0xAA, dtype=torch.uint8, device=dev)
    pk3 = torch.full((M, RB), 0x33, dtype=torch.uint8, device=dev)
    l1, l2 = torch.empty(M, D, nbits, dtype=f32, device=dev), torch.empty(M, D, nbits, dtype=f32, device=dev)
    q1, q2 = torch.empty(M, D, nbits, 2, dtype=f32, device=dev), torch.empty(M, D, nbits, 2, dtype=f32, device=dev)
    _lib.check(lib.dccn_dense_decide_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), z1.data_ptr(), tp.data_ptr(), pk1.data_ptr(),
                                         l1.data_ptr(), q1.data_ptr(), M, K, N, nbits, st), "dccn_dense_decide_fwd")
    _lib.check(lib.dccn_dense_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), z2.data_ptr(), M, K, N, st), "dccn_dense_fwd")
    _lib.check(lib.dccn_demod_decide(z2.data_ptr(), tp.data_ptr(), pk2.data_ptr(), l2.data_ptr(), q2.data_ptr(), M, D, nbits, st),
               "dccn_demod_decide")
    if nbits <= 2:     # z is optional in the one-launch form; the bits do not depend on it
        _lib.check(lib.dccn_dense_decide_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, tp.data_ptr(), pk3.data_ptr(),
                                             None, None, M, K, N, nbits, st), "dccn_dense_decide_fwd")
    torch.cuda.synchronize()
    assert torch.equal(pk1, pk2)
    assert torch.equal(z1, z2) and torch.equal(l1, l2) and torch.equal(q1, q2)
    if nbits <= 2:
        assert torch.equal(pk3, pk1)
    assert relerr(z1.cpu().numpy(), x.cpu().numpy().astype(np.float64) @ w.cpu().numpy().astype(np.float64)
                  + b.cpu().numpy().astype(np.float64)) <= RTOL


@pytest.fixture(scope="module")
def large_cases():
    """The cached operands and float64 references of tests/test_gpu_dense_tail_large.py (built here when that module did not
    run first; released when this module is done)."""
    import test_gpu_dense_tail_large as T
    yield T
    T._cases.clear()


@pytest.mark.parametrize("M,K,N,nbits,route", [(4960, 192, 640, 1, (0, 80, 0, 620)),      # uniform 80x64 tiles
                                               (4960, 192, 640, 2, (0, 80, 0, 620)),
                                               (4961, 192, 640, 2, (2, 80, 1, 630)),      # ragged grid, one row
                                               (4992, 192, 640, 1, (2, 80, 32, 630)),     # ragged grid, a full 32-row block
                                               (4960, 192, 640, 4, (0, 80, 0, 620))])     # two launches
def test_dense_decide_on_the_grids_of_large_layers(large_cases, M, K, N, nbits, route):
    """dccn_dense_decide_fwd where dense_tail_route leaves the 48x64 tiles (dccn_dense_tail_grid proves it).  There
    dccn_dense_fwd may run another tile family, so z is held to what the header promises instead: the bits of
    dccn_dense_tail_fwd's z.  prob likewise; packed is numpy.packbits of that prob's decisions and -- the tail-side test
    holds that prob to the oracle, and no cell of these inputs is near a tie -- of the oracle's; llr, prob and packed are those
    of the stand-alone decision kernel on that z; all-NULL optional outputs (nbits <= 2) give the same packed; 64 guard
    bytes behind packed stay untouched."""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import row_bytes
    T = large_cases
    lib = _lib.load()
    assert T.grid_of(lib, M, K, N, nbits) == route
    assert lib.dccn_dense_decide_supported(M, K, N, nbits) == 1
    c = T.large_case(M, K, N, nbits)
    tail = T.run_tail(lib, c, bwd=False)
    D, RB, GB = N // 2, row_bytes(N // 2, nbits), 64
    dev = "cuda"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, w, b, tp = (c[k].data_ptr() for k in ("d_x", "d_w", "d_b", "d_flat"))

    def outputs(fill):
        return (torch.full((M * RB + GB,), fill, dtype=torch.uint8, device=dev), T.Guarded(M * D * nbits),
                T.Guarded(M * D * nbits * 2))

    def packed_rows(pk, fill, what):
        h = pk.cpu().numpy()
        assert (h[M * RB:] == fill).all(), "%s: bytes behind packed written" % what
        return h[:M * RB].reshape(M, RB)

    z1 = T.Guarded(M * N)
    pk1, l1, q1 = outputs(0x55)
    _lib.check(lib.dccn_dense_decide_fwd(x, w, b, z1.ptr, tp, pk1.data_ptr(), l1.ptr, q1.ptr, M, K, N, nbits, st),
               "dccn_dense_decide_fwd")
    torch.cuda.synchronize()
    zh = z1.get("z")
    T.assert_same_bits(zh.reshape(M, N), tail["z"], "z against dccn_dense_tail_fwd")
    qh = q1.get("prob").reshape(M, D, nbits, 2)
    T.assert_same_bits(qh, tail["prob"], "prob against dccn_dense_tail_fwd")
    ph = packed_rows(pk1, 0x55, "decide")
    hard = tail["prob"][..., 1] > tail["prob"][..., 0]
    # (numpy.packbits pads a row's last byte with zero bits)
    assert np.array_equal(ph, np.packbits(hard.reshape(M, D * nbits), axis=1))
    assert np.array_equal(ph, np.packbits(c["hard"].reshape(M, D * nbits), axis=1))
    # the stand-alone decision kernel on the same z
    z2 = torch.as_tensor(zh, device=dev)
    pk2, l2, q2 = outputs(0xAA)
    _lib.check(lib.dccn_demod_decide(z2.data_ptr(), tp, pk2.data_ptr(), l2.ptr, q2.ptr, M, D, nbits, st), "dccn_demod_decide")
    torch.cuda.synchronize()
    assert np.array_equal(packed_rows(pk2, 0xAA, "stand-alone"), ph)
    T.assert_same_bits(l2.get("llr"), l1.get("llr"), "llr against dccn_demod_decide")
    T.assert_same_bits(q2.get("prob").reshape(qh.shape), qh, "prob against dccn_demod_decide")
    if nbits <= 2:
        pk3 = torch.full((M * RB + GB,), 0x33, dtype=torch.uint8, device=dev)
        _lib.check(lib.dccn_dense_decide_fwd(x, w, b, None, tp, pk3.data_ptr(), None, None, M, K, N, nbits, st),
                   "dccn_dense_decide_fwd")
        torch.cuda.synchronize()
        assert np.array_equal(packed_rows(pk3, 0x33, "packed only"), ph)


@pytest.mark.parametrize("name,batch,nbits,kin,F,D", CASES)
def test_sign_coherence_and_nullable_outputs(name, batch, nbits, kin, F, D):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import RxReceiver
    dims, cfg, x, bits, p = make_case(batch, nbits, kin, F, D)
    full = RxReceiver(dims, batch, p, want_llr=True, want_prob=True)
    r = full.receive(x)
    torch.cuda.synchronize()
    hard = unpack(r, D, nbits).reshape(-1)
    lv = r.llr.cpu().numpy().reshape(-1)
    big = np.abs(lv) > 1e-6
    assert np.array_equal(hard[big], (lv > 0)[big].astype(np.uint8))
    ref = r.packed.clone()
    for want_llr, want_prob in ((False, False), (True, False), (False, True)):
        rc = RxReceiver(dims, batch, p, want_llr=want_llr, want_prob=want_prob)
        rr = rc.receive(x)
        torch.cuda.synchronize()
        assert (rr.llr is not None) == want_llr and (rr.prob is not None) == want_prob
        assert torch.equal(rr.packed, ref)
        if want_llr:
            assert torch.equal(rr.llr, r.llr)
        if want_prob:
            assert torch.equal(rr.prob, r.prob)
    # packed == NULL: refused by the entry's own validation, nothing launched (sentinels stay)
    lib = _lib.load()
    full.x_norm.fill_(123.0)
    full.fft_out.fill_(-7.0)
    full.llr.fill_(5.0)
    full.prob.fill_(9.0)
    torch.cuda.synchronize()
    vals = {f: getattr(full.buffers, f) for f, _ in _lib.RxReceiveBuffers._fields_}
    vals["packed"] = None
    bad = _lib.RxReceiveBuffers(*[vals[f] for f, _ in _lib.RxReceiveBuffers._fields_])
    assert lib.dccn_rx_receive_step(C.byref(full.shape), C.byref(bad), full._stream()) == -1
    torch.cuda.synchronize()
    assert bool((full.x_norm == 123.0).all()) and bool((full.fft_out == -7.0).all())
    assert bool((full.llr == 5.0).all()) and bool((full.prob == 9.0).all())


# ---- equaliser + receiver chain ---------------------------------------------------------------------------
class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer(nbits, seed=21):
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    F = _Flags()
    F.nbits, F.opt, F.init_learning, F.cp = nbits, 0, 1e-3, True
    tx = ofdm_tx(F)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size,
                      pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=nbits)
    pe = E.init_params(ecfg, seed=seed, bias_scale=0.05)
    pr = O.init_params(rcfg, seed=seed + 1)
    tr = EqualizerTrainer(F, tx, pr, seed=3)
    tr.load_params(pe)
    return tx, tr


@pytest.mark.parametrize("nbits", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [73, 130])
def test_chain_receive_agrees_exactly_with_the_chain_eval_step(nbits, B):
    tx, tr = _trainer(nbits)
    D = tx.frame_size
    rng = np.random.RandomState(40 + nbits + B)
    x = (rng.standard_normal((B, 7, 80, 2)) * 2).astype(np.float32)
    bits = rng.randint(0, 2, (B, D, nbits)).astype(np.int32)
    m = tr.eval_step(x, bits, graph=False)
    torch.cuda.synchronize()
    pl = tr.resident(B)
    out_eq, chest = pl.out_eq.clone(), pl.chest.clone()
    pl.out_eq.fill_(0.0)
    pl.chest.fill_(0.0)
    r = tr.receive(x, want_llr=True)
    torch.cuda.synchronize()
    assert torch.equal(pl.out_eq, out_eq) and torch.equal(pl.chest, chest)
    hard = unpack(r, D, nbits)
    assert host_conf(hard, bits) == [[int(v) for v in row] for row in np.asarray(m["conf"]).reshape(2, 2)]
    lv = r.llr.cpu().numpy().reshape(-1)
    big = np.abs(lv) > 1e-6
    assert np.array_equal(hard.reshape(-1)[big], (lv > 0)[big].astype(np.uint8))
    assert torch.equal(tr.receive(x).packed, r.packed) and tr.receive(x).llr is None


# ---- graph-name API -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,batch,cp", [(1, 36, True), (2, 130, True), (2, 64, False), (4, 48, True)])
def test_session_serves_label_free_fetches(tmp_path, nbits, batch, cp):
    from dl_ofdm_amd import receiver
    from dl_ofdm_amd.engine import RxDims, RxEngine
    from dl_ofdm_amd.session import Session, load_model_np
    kin = 80 if cp else 64
    cfg = O.RxConfig(S=7, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(cfg, seed=5)
    rng = np.random.RandomState(nbits)
    p["demodulation/dense/bias"] = (rng.randn(640) * 0.1).astype(np.float32)
    eng = RxEngine(RxDims(7, kin, 64, 320, nbits), 8, params=p, train=True)
    path = receiver.save_checkpoint(str(tmp_path / "OFDM_x"), eng, receiver.Flags(nbits=nbits, cp=cp, nfilter=64))
    sess = Session(seed=3)
    tup = load_model_np(path, sess)
    y, xph, iq_receiver, outputs, ce_mean = tup[0], tup[1], tup[2], tup[3], tup[12]
    frames = (rng.randn(batch, 7, kin, 2) * rng.uniform(0.3, 3.0, (7, kin, 2))).astype(np.float32)
    bits = rng.randint(0, 2, (batch, 320, nbits)).astype(np.int32)
    free = sess.run(outputs, {xph: frames})
    fed = sess.run(outputs, {xph: frames, y: bits})
    assert free.shape == (batch, 320, nbits, 2) and np.array_equal(free, fed)
    g = sess.get_tensor_by_name
    names = ["input:0", "receiver/fft_like/fft_out:0", "output:0", "tx_ofdm:0"]
    a = sess.run([g(n) for n in names], {xph: frames})
    b = sess.run([g(n) for n in names], {xph: frames, y: bits})
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for bad in (ce_mean, g("conf_matrix:0"), g("tx_power:0"), g("bits_in:0")):
        with pytest.raises(ValueError, match="bits_in:0"):
            sess.run(bad, {xph: frames})
    with pytest.raises(ValueError, match="bits_in:0"):
        sess.run([outputs, ce_mean], {xph: frames})
    sess.close()


# ---- closed form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,snr_db", [(1, 1.0), (2, 4.0)])
def test_receive_ber_equals_eval_ber_on_the_analytic_receiver(nbits, snr_db):
    """The analytically initialised DFT receiver of tests/test_gpu_harness.py: the BER counted from
    the received bits equals the BER the evaluation step reports on the same batch exactly, so it inherits that test's
    Q-function check (repeated here at the same tolerance)."""
    from dl_ofdm_amd import ofdm, radio, receiver
    from dl_ofdm_amd.engine import RxEngine
    from dl_ofdm_amd.receive import RxReceiver
    from tests.test_gpu_harness import dft_receiver_params, flags, qfunc
    F = flags(nbits=nbits)
    o = ofdm.ofdm_tx(F)
    dims = receiver.rx_dims(F, o)
    frames = 6000
    np.random.seed(1234 + nbits)
    fading = radio.rayleigh_chan_lte(F, o.Fs)
    xs, ys, _ = receiver.make_batch(F, o, fading, frames, snr_db)
    params = dft_receiver_params(dims, o, nbits)
    eng = RxEngine(dims, frames, train=False, params=params, want_prob=False)
    eng.eval_step(xs, ys)
    m = eng.metrics()
    r = RxReceiver(dims, frames, params).receive(xs)
    torch.cuda.synchronize()
    hard = unpack(r, o.frame_size, nbits)
    wrong = int((hard.reshape(-1) != np.asarray(ys).reshape(-1)).sum())
    conf = np.asarray(m["conf"]).reshape(2, 2)
    assert wrong == int(conf[0, 1] + conf[1, 0])
    n_bits = frames * o.frame_size * nbits
    ber = wrong / n_bits
    assert np.float32(ber) == np.float32(m["berlin"])
    sigma2 = 10.0 ** (-snr_db / 10.0)
    per_dim = (64.0 / 24.0 if nbits == 1 else 64.0 / 48.0) / sigma2
    theory = qfunc(math.sqrt(per_dim))
    assert abs(ber - theory) <= 4.0 * math.sqrt(theory * (1 - theory) / n_bits) + 0.02 * theory
