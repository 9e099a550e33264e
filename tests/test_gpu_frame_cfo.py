"""Carrier-frequency offset from the cyclic-prefix correlation on the GPU (``-m gpu``): ``dccn_frame_sync_cfo`` held to the fp64
restatement of its definition (tests/frame_cfo_ref.py: tolerances and their derivation are stated there), its timing side held
bit for bit to ``dccn_frame_sync``, and the ``cfo=True`` argument of the receive path held to a plain receive call on the frames
``FrameSync(..., cfo=True)`` writes.

Inputs: the frames of tests/frame_sync_ref.py impaired by a per-frame offset ~ U(-0.4, 0.4) subcarrier spacings, and exact-prefix
frames built in tests/frame_cfo_ref.py; a case of n frames takes the leading n of the case's batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_cfo_ref as F
import frame_sync_ref as R
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = R.S, R.K
GUARD = 64
SENT_X, SENT_OFF, SENT_C, SENT_M = 777.0, -99, 333.0, 555.0
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


def dev(a) -> torch.Tensor:
    """a (read-only) host array as a device tensor of its own"""
    return torch.from_numpy(np.array(a)).to(DEV)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Run:
    """one dccn_frame_sync_cfo call (``cfo=False``: one dccn_frame_sync call) on guarded, sentinel-filled outputs"""

    def __init__(self, lib, x, cp, w, out_kin=None, want_out=True, want_metric=True, cfo=True, s=S, k=K):
        n = x.shape[0]
        self.n, self.W, self.S, self.out_kin = n, w, s, (k + cp if out_kin is None else out_kin)
        self.n_out, self.n_met = n * s * self.out_kin * 2, n * (2 * w + 1)
        self.out_buf = torch.full((self.n_out + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.off_buf = torch.full((n + GUARD,), SENT_OFF, dtype=torch.int32, device=DEV)
        self.cfo_buf = torch.full((n + GUARD,), SENT_C, dtype=torch.float32, device=DEV)
        self.met_buf = torch.full((self.n_met + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        head = (x.data_ptr(), n, s, k, cp, w, self.out_kin, self.out_buf.data_ptr() if want_out else None, self.off_buf.data_ptr())
        tail = (self.met_buf.data_ptr() if want_metric else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if cfo:
            self.status = lib.dccn_frame_sync_cfo(*head, self.cfo_buf.data_ptr(), *tail)
        else:
            self.status = lib.dccn_frame_sync(*head, *tail)
        torch.cuda.synchronize()

    @property
    def out(self):
        return self.out_buf[:self.n_out].view(self.n, self.S, self.out_kin, 2)

    @property
    def offset(self):
        return self.off_buf[:self.n]

    @property
    def cfo(self):
        return self.cfo_buf[:self.n]

    @property
    def metric(self):
        return self.met_buf[:self.n_met].view(self.n, 2 * self.W + 1)

    def guards_intact(self):
        return (bool((self.out_buf[self.n_out:] == SENT_X).all()) and bool((self.off_buf[self.n:] == SENT_OFF).all())
                and bool((self.cfo_buf[self.n:] == SENT_C).all()) and bool((self.met_buf[self.n_met:] == SENT_M).all()))


def frame_peak(x):
    """max |y| of every frame, fp64 [frames]"""
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2).reshape(x.shape[0], -1).max(axis=1)


def derotation_error(x, run, k, cp=None):
    """max over the frames of |out - out64| / (DEROT_TOL max|y|), out64 from the input, the GPU's own offsets and the GPU's own
    estimates promoted to fp64; ``cp``: ``run`` is the cropped form (the K samples behind each symbol's prefix)"""
    off = run.offset.cpu().numpy().astype(np.int64)
    est = run.cfo.cpu().numpy().astype(np.float64)
    want = F.derotated(x, off, est, k)
    if cp is not None:
        want = want[:, :, cp:cp + k]
    d = run.out.cpu().numpy().astype(np.float64) - want
    err = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2).reshape(d.shape[0], -1).max(axis=1)
    return float((err / (F.DEROT_TOL * frame_peak(x))).max())


# ---- 1. estimate against fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("CP,W,channel,snr", R.all_cases())
def test_estimate_against_fp64(lib, CP, W, channel, snr):
    xs = F.case_frames(channel, snr, CP)
    off64, lam64, phi64, ok, gamma64, cfo64 = F.case_reference(channel, snr, CP, W)
    bound = F.cfo_bound(phi64, gamma64)
    for n in R.FRAME_COUNTS:
        x = dev(xs[:n])
        r = Run(lib, x, CP, W)
        assert r.status == 0 and r.guards_intact()
        plain = Run(lib, x, CP, W, cfo=False)
        assert plain.status == 0
        assert same_bits(r.metric, plain.metric) and torch.equal(r.offset, plain.offset)       # (the timing side is dccn_frame_sync's)
        off = r.offset.cpu().numpy().astype(np.int64)
        est = r.cfo.cpu().numpy().astype(np.float64)
        use = ok[:n]
        wrong = int((off[use] != off64[:n][use]).sum())
        ratio = float((F.circle(est - cfo64[:n]) / bound[:n])[use].max()) if use.any() else 0.0
        print("%s %g dB CP %d W %d, %d frames: %d undecidable; %d offsets differ on the rest; max |cfo - cfo64| / bound = %.3g"
              % (channel, snr, CP, W, n, int((~use).sum()), wrong, ratio))
        assert (~use).sum() <= R.CAP * n
        assert wrong == 0
        assert (off >= -W).all() and (off <= W).all()
        assert np.isfinite(est).all() and (np.abs(est) <= 0.5).all()
        assert ratio <= 1.0


# ---- 2. derotation against fp64 on the GPU's own estimates ----------------------------------------------------------
@pytest.mark.parametrize("CP,W", [(CP, W) for (_, _, CP) in R.SHAPES for W in R.WINDOWS[CP]])
@pytest.mark.parametrize("n", R.FRAME_COUNTS)
def test_derotation_against_fp64(lib, CP, W, n):
    """ETU at 5 dB: offsets of both parities and both signs inside one batch, every frame with its own carrier offset."""
    xs = F.case_frames("ETU", 5.0, CP)[:n]
    x = dev(xs)
    x0 = x.clone()
    full = Run(lib, x, CP, W)
    assert full.status == 0 and full.guards_intact()
    e_full = derotation_error(xs, full, K)
    crop = Run(lib, x, CP, W, out_kin=K)
    assert crop.status == 0 and crop.guards_intact()
    assert torch.equal(crop.offset, full.offset) and same_bits(crop.cfo, full.cfo) and same_bits(crop.metric, full.metric)
    e_crop = derotation_error(xs, crop, K, cp=CP)
    print("CP %d W %d, %d frames: max |out - out64| / (1e-5 max|y|) = %.3g full, %.3g crop" % (CP, W, n, e_full, e_crop))
    assert e_full <= 1.0 and e_crop <= 1.0
    # the cropped rows are the full rows behind each prefix, bit for bit
    assert same_bits(crop.out, full.out[:, :, CP:CP + K].contiguous())
    # estimates only: x_out = NULL, then also metric = NULL
    for want_metric in (True, False):
        only = Run(lib, x, CP, W, want_out=False, want_metric=want_metric)
        assert only.status == 0 and only.guards_intact() and bool((only.out_buf == SENT_X).all())
        assert torch.equal(only.offset, full.offset) and same_bits(only.cfo, full.cfo)
        assert same_bits(only.metric, full.metric) if want_metric else bool((only.met_buf == SENT_M).all())
    quiet = Run(lib, x, CP, W, want_metric=False)
    assert quiet.status == 0 and bool((quiet.met_buf == SENT_M).all())
    assert same_bits(quiet.out_buf, full.out_buf) and torch.equal(quiet.off_buf, full.off_buf) and same_bits(quiet.cfo_buf, full.cfo_buf)
    again = Run(lib, x, CP, W)
    assert (torch.equal(again.off_buf, full.off_buf) and same_bits(again.cfo_buf, full.cfo_buf)
            and same_bits(again.out_buf, full.out_buf) and same_bits(again.met_buf, full.met_buf))
    assert same_bits(x, x0)
    if n >= 73:
        assert len(torch.unique(full.offset)) >= (3 if W > 1 else 2)      # the batch does exercise several shifts
        assert float(full.cfo.max()) > 0.2 and float(full.cfo.min()) < -0.2


# ---- 3. a small odd shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [-2, 0, 1])
@pytest.mark.parametrize("eps", [-0.3, 0.2])
def test_small_odd_shape(lib, d, eps):
    """S = 3, K = 12 (no power of two), CP = 4, W = 2: T = 48, less than one pass of the wave's 64 lanes"""
    s, k, cp, w, n = 3, 12, 4, 2, 5
    assert lib.dccn_frame_sync_supported(s, k, cp, w) == 1
    xs = F.exact_prefix_frames(n, s, k, cp, seed=7, eps=eps, roll=d)
    x = dev(xs)
    x0 = x.clone()
    full = Run(lib, x, cp, w, s=s, k=k)
    assert full.status == 0 and full.guards_intact()
    assert (full.offset.cpu().numpy() == d).all()
    crop = Run(lib, x, cp, w, out_kin=k, s=s, k=k)
    assert crop.status == 0 and crop.guards_intact() and torch.equal(crop.offset, full.offset) and same_bits(crop.cfo, full.cfo)
    e_full, e_crop = derotation_error(xs, full, k), derotation_error(xs, crop, k, cp=cp)
    print("d %d eps %g: max |out - out64| / (1e-5 max|y|) = %.3g full, %.3g crop; cfo %s"
          % (d, eps, e_full, e_crop, full.cfo.cpu().numpy()))
    assert e_full <= 1.0 and e_crop <= 1.0
    assert same_bits(x, x0)
    if d == 0:
        off64, lam64, phi64, gamma64, cfo64 = F.reference(xs, k, cp, w)
        assert (off64 == 0).all()
        err = F.circle(full.cfo.cpu().numpy().astype(np.float64) - eps)
        assert (err <= F.cfo_bound(phi64, gamma64) + 1e-6).all()


# ---- 4. zero offset: the identity on top of the timing stage ------------------------------------------------------
@pytest.mark.parametrize("CP,W", [(16, 3), (4, 4)])
@pytest.mark.parametrize("d", [0, -1])
def test_zero_offset_gives_the_bits_of_frame_sync(lib, CP, W, d):
    n = 73
    x = dev(F.exact_prefix_frames(n, S, K, CP, seed=90 + CP, eps=0.0, roll=d))
    for out_kin in (K + CP, K):
        r = Run(lib, x, CP, W, out_kin=out_kin)
        plain = Run(lib, x, CP, W, out_kin=out_kin, cfo=False)
        assert r.status == 0 and plain.status == 0 and r.guards_intact()
        assert (r.offset.cpu().numpy() == d).all() and torch.equal(r.offset, plain.offset)
        assert bool((r.cfo == 0).all())                  # u conj(u) has no imaginary part: the angle is 0 exactly
        assert same_bits(r.out, plain.out) and same_bits(r.metric, plain.metric)


# ---- 5. the receive path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,batch", [(2, 36), (4, 8)])
@pytest.mark.parametrize("cp", [True, False])
def test_receiver_cfo_equals_receive_of_the_frames_the_stage_writes(nbits, batch, cp):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import FrameSync
    CP, W = 16, 3
    kin = K + CP if cp else K
    dims = RxDims(S=S, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=kin, F=64, D=320, nbits=nbits), seed=11 + nbits)
    x = dev(F.case_frames("ETU", 30.0, CP)[:batch])
    x0 = x.clone()
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True, CP=CP if cp else None)
    # cfo without sync: refused before anything is launched
    before = [t.clone() for t in (rcv.x, rcv.packed, rcv.llr, rcv.prob)]
    with pytest.raises(_lib.DccnError):
        rcv.receive(x, cfo=True)
    torch.cuda.synchronize()
    assert same_bits(before[0], rcv.x) and torch.equal(before[1], rcv.packed)
    assert same_bits(before[2], rcv.llr) and same_bits(before[3], rcv.prob)
    res = rcv.receive(x, sync=W, cfo=True)
    torch.cuda.synchronize()
    assert res.offset is not None and res.offset.dtype == torch.int32 and tuple(res.offset.shape) == (batch,)
    assert res.cfo is not None and res.cfo.dtype == torch.float32 and tuple(res.cfo.shape) == (batch,)
    got = [t.clone() for t in (res.packed, res.llr, res.prob, rcv.x, res.offset, res.cfo)]
    fs = FrameSync(S, K, CP, W, batch, DEV, out_kin=kin, cfo=True)
    want_x, off_fs = fs.run(x)
    torch.cuda.synchronize()
    assert torch.equal(got[4], off_fs) and same_bits(got[5], fs.cfo) and bool((got[5] != 0).all())
    assert same_bits(x, x0)
    assert same_bits(got[3], want_x)
    # the estimates alone: FrameSync.offsets writes no frame and leaves the same offset / cfo bits
    kept = want_x.clone()
    fs.cfo.fill_(SENT_C)
    assert torch.equal(fs.offsets(x), got[4]) and same_bits(fs.cfo, got[5]) and same_bits(fs.out, kept)
    ref = rcv.receive(want_x.clone())
    torch.cuda.synchronize()
    assert ref.offset is None and ref.cfo is None
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
    # and timing alignment alone gives other bits: the derotation is not a no-op on this batch
    timing = rcv.receive(x, sync=W)
    torch.cuda.synchronize()
    assert timing.cfo is None and torch.equal(timing.offset, got[4]) and not same_bits(timing.llr, got[1])


class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer(nbits, seed=21):
    """the chain of tests/test_gpu_receive.py, re-stated"""
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    fl = _Flags()
    fl.nbits, fl.opt, fl.init_learning, fl.cp = nbits, 0, 1e-3, True
    tx = ofdm_tx(fl)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size,
                      pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=nbits)
    tr = EqualizerTrainer(fl, tx, O.init_params(rcfg, seed=seed + 1), seed=3)
    tr.load_params(E.init_params(ecfg, seed=seed, bias_scale=0.05))
    return tx, tr


def test_chain_cfo_equals_chain_receive_of_the_frames_the_stage_writes():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import chain_receive
    from dl_ofdm_amd.sync import FrameSync
    CP, W, B = 16, 3, 73
    tx, tr = _trainer(2)
    x = dev(F.case_frames("ETU", 30.0, CP)[:B])
    x0 = x.clone()
    with pytest.raises(_lib.DccnError):
        chain_receive(tr, x, cfo=True)
    res = tr.receive(x, want_llr=True, want_prob=True, sync=W, cfo=True)
    torch.cuda.synchronize()
    got = [t.clone() for t in (res.packed, res.llr, res.prob, tr.resident(B).x, tr.resident(B).out_eq, res.offset, res.cfo)]
    fs = FrameSync(S, K, CP, W, B, DEV, cfo=True)
    want_x, off_fs = fs.run(x)
    torch.cuda.synchronize()
    assert torch.equal(got[5], off_fs) and same_bits(got[6], fs.cfo) and bool((got[6] != 0).all()) and same_bits(x, x0)
    assert same_bits(got[3], want_x)
    ref = chain_receive(tr, want_x.clone(), want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert ref.offset is None and ref.cfo is None
    assert same_bits(got[4], tr.resident(B).out_eq)
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
    assert chain_receive(tr, x0, sync=W).cfo is None


# ---- 6. the old path is untouched -----------------------------------------------------------------------------------
def test_sync_alone_is_what_it_was_before_any_cfo_call():
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    CP, W, batch, nbits = 16, 3, 36, 2
    dims = RxDims(S=S, kin=K + CP, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=K + CP, F=64, D=320, nbits=nbits), seed=13)
    x = dev(F.case_frames("EVA", 30.0, CP)[:batch])
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True, CP=CP)
    first = rcv.receive(x, sync=W)
    torch.cuda.synchronize()
    assert first.cfo is None
    keep = [t.clone() for t in (first.packed, first.llr, first.prob, rcv.x, first.offset)]
    with_cfo = rcv.receive(x, sync=W, cfo=True)
    torch.cuda.synchronize()
    assert with_cfo.cfo is not None and not same_bits(rcv.x, keep[3])
    after = rcv.receive(x, sync=W)
    torch.cuda.synchronize()
    assert after.cfo is None
    assert torch.equal(after.packed, keep[0]) and same_bits(after.llr, keep[1]) and same_bits(after.prob, keep[2])
    assert same_bits(rcv.x, keep[3]) and torch.equal(after.offset, keep[4])
