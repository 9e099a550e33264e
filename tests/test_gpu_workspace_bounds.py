"""No operator writes behind the workspace it asked for (``-m gpu``).

Every workspace-taking operator runs once at the smallest shape that reaches each place where it cuts its workspace into
pieces, on a workspace of exactly the size its query answers, followed by a 4 KiB band of a sentinel byte: the band is
intact afterwards, and the outputs are bit for bit those of the same call through the Python wrapper on the wrapper's own
workspace.  (The wrappers take their workspace from ops.workspace or keep it in an attribute; the banded run swaps that
allocation and nothing else.  dccn_rx_backward has no wrapper: its reference is the same call on a plain, larger workspace.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND, SENTINEL = 4096, 0xA5


class Bands:
    """workspaces of the queried size with a sentinel band behind them"""

    def __init__(self):
        self.made = []

    def alloc(self, nbytes, device="cuda", key=None):
        t = torch.full((int(nbytes) + BAND,), SENTINEL, dtype=torch.uint8, device=device)
        self.made.append((t, int(nbytes)))
        return t

    def check(self, expect=None):
        torch.cuda.synchronize()
        assert self.made and (expect is None or len(self.made) == expect), len(self.made)
        for t, n in self.made:
            assert bool((t[n:] == SENTINEL).all()), "an operator wrote behind its %d-byte workspace" % n


def same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        if u is None or v is None:
            assert u is None and v is None
        else:
            assert u.dtype == v.dtype and torch.equal(u, v)


def both_ways(monkeypatch, fn, allocs=None):
    """fn() through the wrapper as it is, then with every ops.workspace allocation banded: same outputs, bands intact"""
    from dl_ofdm_amd import ops
    ref = fn()
    bands = Bands()
    with monkeypatch.context() as m:
        m.setattr(ops, "workspace", bands.alloc)
        out = fn()
    bands.check(allocs)
    same(ref, out)


def rnd(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32)).cuda()


# ---- the receiver's steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [2, 4])
@pytest.mark.parametrize("train", [True, False])
def test_receiver_step(nbits, train):
    from dl_ofdm_amd.engine import RxDims, RxEngine
    from oracle import dccn_oracle as O
    batch = 36
    dims = RxDims(S=7, kin=80, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=7, kin=80, F=64, D=320, nbits=nbits), seed=1)
    rng = np.random.RandomState(nbits)
    x = rng.randn(batch, 7, 80, 2).astype(np.float32)
    bits = rng.randint(0, 2, (batch, 320, nbits)).astype(np.int32)
    outs, bands = [], Bands()
    for banded in (False, True):
        eng = RxEngine(dims, batch, params=p, train=train)
        if banded:
            eng.ws = bands.alloc(eng.buffers.workspace_bytes)
            eng.buffers.workspace = eng.ws.data_ptr()
        if train:
            eng.train_step(x, bits)
        else:
            eng.eval_step(x, bits)
        torch.cuda.synchronize()
        outs.append([eng.prob.clone(), eng.metrics_buf.clone(), eng.params.clone(), eng.x_norm.clone(), eng.fft_out.clone()] +
                    ([eng.grads.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.dz.clone()] if train else []))
    bands.check(1)
    same(outs[0], outs[1])


def test_rx_backward():
    from dl_ofdm_amd import _lib
    lib = _lib.load()
    B, S, kin, F, D = 64, 7, 80, 64, 320
    assert lib.dccn_rx_bwd_fused_supported(C.byref(_lib.RxShape(B, S, kin, F, D, 2)))
    xn, fft, dz, w = rnd(1, B, S * kin * 2), rnd(2, B, S * 2 * F), rnd(3, B, 2 * D), rnd(4, S * 2 * F, 2 * D)
    nws = lib.dccn_rx_backward_workspace_size(B, S, kin, F, D)
    bands, outs = Bands(), []
    for ws in (torch.zeros(2 * nws, dtype=torch.uint8, device="cuda"), bands.alloc(nws)):
        o = [torch.zeros(S * 2 * F, 2 * D, device="cuda"), torch.zeros(2 * D, device="cuda"), torch.zeros(kin, 2 * F, device="cuda"),
             torch.zeros(2 * F, device="cuda")]
        _lib.check(lib.dccn_rx_backward(xn.data_ptr(), fft.data_ptr(), dz.data_ptr(), w.data_ptr(), None, o[0].data_ptr(),
                                        o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), B, S, kin, F, D, 1, ws.data_ptr(), nws,
                                        None), "dccn_rx_backward")
        outs.append(o)
    bands.check(1)
    same(outs[0], outs[1])
    assert float(outs[0][0].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0


# ---- operators behind ops.workspace -----------------------------------------------------------------------------------
# (73, 896, 896): few rows, one unsplit grid; (300, 896, 640): split-K slabs on the grouped k-major launch
@pytest.mark.parametrize("M,K,N", [(73, 896, 896), (300, 896, 640)])
def test_dense_bwd(monkeypatch, M, K, N):
    from dl_ofdm_amd import ops
    x, w, b, dy = rnd(1, M, K), rnd(2, K, N), rnd(3, N), rnd(4, M, N)

    def run():
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        ops.dense(xs, ws, bs).backward(dy)
        return [xs.grad, ws.grad, bs.grad]
    both_ways(monkeypatch, run, 1)


def test_cconv_gemm_bwd_w(monkeypatch):
    from dl_ofdm_amd import ops
    x, w, b, dout = rnd(1, 511, 80, 2), rnd(2, 80, 128), rnd(3, 128), rnd(4, 511, 64, 2)

    def run():
        ws, bs = (t.clone().requires_grad_(True) for t in (w, b))
        ops.cconv_gemm(x, ws, bs).backward(dout)
        return [ws.grad, bs.grad]
    both_ways(monkeypatch, run, 1)


@pytest.mark.parametrize("nbits", [2, 4])
def test_demod_tail_loss_fwd_bwd(monkeypatch, nbits):
    from dl_ofdm_amd import ops
    z, tailp = rnd(1, 36, 320, 2), 0.3 * rnd(2, ops.tail_param_count(nbits))
    bits = torch.from_numpy(np.random.RandomState(3).randint(0, 2, (36, 320, nbits)).astype(np.int32)).cuda()

    def run():
        zs, ts = z.clone().requires_grad_(True), tailp.clone().requires_grad_(True)
        ce, prob, mbuf = ops.demod_tail_loss(zs, ts, bits, nbits)
        ce.backward()
        return [ce.detach(), prob, mbuf, zs.grad, ts.grad]
    both_ways(monkeypatch, run, 1)


def test_dense_tail_fwd_bwd(monkeypatch):
    from dl_ofdm_amd import ops
    M, K, N, nbits = 36, 896, 640, 2
    x, w, b, tailp = rnd(1, M, K), 0.05 * rnd(2, K, N), rnd(3, N), 0.3 * rnd(4, ops.tail_param_count(nbits))
    bits = torch.from_numpy(np.random.RandomState(5).randint(0, 2, (M, N // 2, nbits)).astype(np.int32)).cuda()

    def run():
        xs, ws, bs, ts = (t.clone().requires_grad_(True) for t in (x, w, b, tailp))
        ce, prob, mbuf = ops.dense_demod_tail_loss(xs, ws, bs, ts, bits, nbits)
        ce.backward()
        return [ce.detach(), prob, mbuf, xs.grad, ws.grad, bs.grad, ts.grad]
    both_ways(monkeypatch, run, 2)             # the fused forward's workspace, then the grouped backward's


def test_cconv1d_bwd(monkeypatch):
    """the smallest shape dccn_cconv1d_bwd supports: one frame, two channels, F = 32, one tap"""
    from dl_ofdm_amd import _lib, ops
    B, L, Cc, F, ntl = 1, 4, 2, 32, 1
    assert _lib.load().dccn_cconv1d_bwd_supported(B, L, Cc, L, ntl, 1, F) == 1
    x, w, b, dout = rnd(1, B, L, 1, Cc, 2), rnd(2, ntl * Cc, 2 * F), rnd(3, 2 * F), rnd(4, B * L, F, 2)

    def run():
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        ops.cconv_patch(xs, ws, bs, L, 1, range(ntl), range(1), (1, 1), (0, 0)).backward(dout)
        return [xs.grad, ws.grad, bs.grad]
    both_ways(monkeypatch, run, 1)


# ---- the channel stage's three entry points, 6 frames of T = 560 -------------------------------------------------------
@pytest.mark.parametrize("chan,mobile,mix,entry", [("EPA", False, False, "dccn_channel_awgn"),
                                                   ("EPA", True, False, "dccn_channel_doppler_awgn"),
                                                   ("mixAll", True, True, "dccn_channel_groups_awgn")])
def test_channel_stage(chan, mobile, mix, entry):
    from dl_ofdm_amd import ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.receiver import Flags
    F = Flags(channel=chan, nfilter=64, nbits=2, SNR=5.0)
    o = ofdm.ofdm_tx(F)
    n = 6
    outs, bands = [], Bands()
    for banded in (False, True):
        gen = DeviceDataGen(F, o, seed=13, mobile=mobile, mix=mix)
        assert gen.T == 560 and gen.mixed == (entry == "dccn_channel_groups_awgn") and \
            (gen.mixed or gen.doppler == (entry == "dccn_channel_doppler_awgn"))
        tx, bits = gen.transmit(n)
        if banded:                      # the entry point's own query, not the wrapper's maximum over the three
            q = {"dccn_channel_awgn": lambda: gen.lib.dccn_channel_awgn_workspace_size(n, gen.T, gen.L),
                 "dccn_channel_doppler_awgn": lambda: gen.lib.dccn_channel_doppler_awgn_workspace_size(n, gen.T, gen.L, gen.S),
                 "dccn_channel_groups_awgn": lambda: gen.lib.dccn_channel_groups_awgn_workspace_size(n, gen.T, gen.S)}[entry]()
            w = gen._workspace(n)
            assert 0 < q <= w["nws"]
            w["ws"], w["nws"] = bands.alloc(q), q
        x, npow, H = gen.channel(tx, np.linspace(2.0, 20.0, n), want_H=True)
        torch.cuda.synchronize()
        outs.append([tx, bits, x.clone(), npow.clone(), torch.view_as_real(H).clone()])
    bands.check(1)
    same(outs[0], outs[1])


def test_ingraph_awgn():
    from dl_ofdm_amd import _lib, session
    from dl_ofdm_amd.engine import RxDims, RxEngine
    lib = _lib.load()
    B, S, kin = 4, 7, 80
    eng = RxEngine(RxDims(S=S, kin=kin, F=64, D=320, nbits=2), B, train=False)
    eng.x_norm.copy_(rnd(1, *eng.x_norm.shape))
    snr = np.array([3.0, 7.0, 11.0, 15.0], np.float32)
    ref = session.monitor_tensors(eng, snr, seed=5, call=2)
    pairs = S * kin
    assert pairs == 560
    bands = Bands()
    nws = lib.dccn_ingraph_awgn_workspace_size(B, pairs)
    ws = bands.alloc(nws)
    snr_t = torch.from_numpy(snr).cuda()
    txs = torch.empty(B, S, kin, 2, device="cuda")
    iq_tx, iq_rx = (torch.empty(B * pairs, 2, dtype=torch.float16, device="cuda") for _ in range(2))
    npw = torch.zeros(1, device="cuda")
    _lib.check(lib.dccn_ingraph_awgn(eng.x_norm.data_ptr(), snr_t.data_ptr(), txs.data_ptr(), iq_tx.data_ptr(), iq_rx.data_ptr(),
                                     npw.data_ptr(), B, pairs, 8.0, 5, 2, ws.data_ptr(), nws, None), "dccn_ingraph_awgn")
    bands.check(1)
    same([ref["tx_signal"], ref["iq_tx"], ref["iq_rx"], ref["noise_power"]], [txs, iq_tx, iq_rx, npw])


def test_classical_gain_and_detect():
    """4 frames through the wrapper: LMMSE-Fast runs dccn_classical_gain, the estimator and dccn_classical_detect"""
    from dl_ofdm_amd import benchmark_gpu as G, ofdm
    from dl_ofdm_amd.datagen import DeviceDataGen
    from dl_ofdm_amd.receiver import Flags
    F = Flags(nbits=2, channel="EPA", nfilter=64)
    o = ofdm.ofdm_tx(F)
    x, bits, _, H = DeviceDataGen(F, o, seed=9).make_batch(4, 15.0, want_H=True)
    outs, bands = [], Bands()
    for banded in (False, True):
        rx = G.ClassicalReceiverGPU(F, o)
        if banded:
            rx.ws = bands.alloc(rx.nws)
        res = []
        for method in ("LMMSE-Fast", "LS-Spline"):
            err, cnt, det = rx.receive(x, bits, method, 15.0, H_true=H, want_bits=True)
            res += [torch.tensor([err, cnt]), det.clone()]
        outs.append(res)
    bands.check(1)
    same(outs[0], outs[1])
