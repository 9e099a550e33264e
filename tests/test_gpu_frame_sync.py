"""Per-frame timing alignment from the cyclic prefix on the GPU (``-m gpu``): ``dccn_frame_sync`` held to the fp64 restatement
of its definition (tests/frame_sync_ref.py: tolerances and their derivation are stated there), its data movement held bit for
bit, and the ``sync=W`` argument of the receive path held to a receive call on frames rolled by the returned offsets.

Inputs: the host substrate's QPSK frames through AWGN / EPA / EVA / ETU at 5 and 30 dB, at both prefix lengths of the driver
grid; a case of n frames takes the leading n of the case's batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_sync_ref as R
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
S, K = R.S, R.K
GUARD = 64
SENT_X, SENT_OFF, SENT_M = 777.0, -99, 555.0
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


def rolled(x: torch.Tensor, off: torch.Tensor) -> torch.Tensor:
    """frame f as torch.roll(x[f].view(T, 2), -off[f], 0), in x's shape"""
    n = x.shape[0]
    flat = x.reshape(n, -1, 2)
    out = torch.empty_like(flat)
    for o in torch.unique(off).tolist():
        m = off == o
        out[m] = torch.roll(flat[m], -int(o), 1)
    return out.reshape(x.shape)


class Run:
    """one dccn_frame_sync call on guarded, sentinel-filled outputs"""

    def __init__(self, lib, x, cp, w, out_kin=None, want_out=True, want_metric=True, over=None):
        """``over``: arguments of the C call by name (x, frames, S, K, CP, W, out_kin, x_out, offset, metric), replacing the
        ones worked out here"""
        n, CP, W = x.shape[0], cp, w
        self.n, self.W, self.out_kin = n, W, (K + CP if out_kin is None else out_kin)
        self.n_out, self.n_met = n * S * self.out_kin * 2, n * (2 * W + 1)
        self.out_buf = torch.full((self.n_out + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
        self.off_buf = torch.full((n + GUARD,), SENT_OFF, dtype=torch.int32, device=DEV)
        self.met_buf = torch.full((self.n_met + GUARD,), SENT_M, dtype=torch.float32, device=DEV)
        a = dict(x=x.data_ptr(), frames=n, S=S, K=K, CP=CP, W=W, out_kin=self.out_kin,
                 x_out=self.out_buf.data_ptr() if want_out else None, offset=self.off_buf.data_ptr(),
                 metric=self.met_buf.data_ptr() if want_metric else None)
        a.update(over or {})
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.status = lib.dccn_frame_sync(a["x"], a["frames"], a["S"], a["K"], a["CP"], a["W"], a["out_kin"], a["x_out"],
                                          a["offset"], a["metric"], st)
        torch.cuda.synchronize()

    @property
    def out(self):
        return self.out_buf[:self.n_out].view(self.n, S, self.out_kin, 2)

    @property
    def offset(self):
        return self.off_buf[:self.n]

    @property
    def metric(self):
        return self.met_buf[:self.n_met].view(self.n, 2 * self.W + 1)

    def guards_intact(self):
        return (bool((self.out_buf[self.n_out:] == SENT_X).all()) and bool((self.off_buf[self.n:] == SENT_OFF).all())
                and bool((self.met_buf[self.n_met:] == SENT_M).all()))

    def untouched(self):
        return (bool((self.out_buf == SENT_X).all()) and bool((self.off_buf == SENT_OFF).all())
                and bool((self.met_buf == SENT_M).all()))


# ---- 1. offsets and metric against fp64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("CP,W,channel,snr", R.all_cases())
def test_offsets_and_metric_against_fp64(lib, CP, W, channel, snr):
    xs = R.case_frames(channel, snr, CP)
    off64, lam64, phi64, ok = R.case_reference(channel, snr, CP, W)
    scale = phi64.max(axis=1)
    for n in R.FRAME_COUNTS:
        r = Run(lib, dev(xs[:n]), CP, W)
        assert r.status == 0 and r.guards_intact()
        lam = r.metric.cpu().numpy().astype(np.float64)
        off = r.offset.cpu().numpy().astype(np.int64)
        err = float((np.abs(lam - lam64[:n]).max(axis=1) / scale[:n]).max())
        use = ok[:n]
        wrong = int((off[use] != off64[:n][use]).sum())
        print("%s %g dB CP %d W %d, %d frames: max |dLambda| / max Phi = %.3g; %d undecidable; %d offsets differ on the rest"
              % (channel, snr, CP, W, n, err, int((~use).sum()), wrong))
        assert err <= R.METRIC_TOL
        assert (~use).sum() <= R.CAP * n
        assert wrong == 0
        assert (off >= -W).all() and (off <= W).all()
        # the offset is the kernel's own argmax of the metric it reports: the smallest lag among the largest values
        assert np.array_equal(off, np.argmax(r.metric.cpu().numpy(), axis=1) - W)


# ---- 2. data movement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("CP,W", [(CP, W) for (_, _, CP) in R.SHAPES for W in R.WINDOWS[CP]])
@pytest.mark.parametrize("n", R.FRAME_COUNTS)
def test_data_movement_is_exact(lib, CP, W, n):
    """ETU at 5 dB: offsets of both parities and both signs inside one batch."""
    x = dev(R.case_frames("ETU", 5.0, CP)[:n])
    x0 = x.clone()
    full = Run(lib, x, CP, W)
    assert full.status == 0 and full.guards_intact()
    off = full.offset.clone()
    want = rolled(x0, off)
    assert same_bits(full.out, want)
    assert same_bits(x, x0)
    crop = Run(lib, x, CP, W, out_kin=K)
    assert crop.status == 0 and crop.guards_intact()
    assert torch.equal(crop.offset, off) and same_bits(crop.metric, full.metric)
    assert same_bits(crop.out, want[:, :, CP:CP + K].contiguous())
    # offsets only: x_out = NULL, then also metric = NULL
    for want_metric in (True, False):
        only = Run(lib, x, CP, W, want_out=False, want_metric=want_metric)
        assert only.status == 0 and only.guards_intact() and bool((only.out_buf == SENT_X).all())
        assert torch.equal(only.offset, off)
        assert same_bits(only.metric, full.metric) if want_metric else bool((only.met_buf == SENT_M).all())
    again = Run(lib, x, CP, W)
    assert torch.equal(again.off_buf, full.off_buf) and same_bits(again.met_buf, full.met_buf) and same_bits(again.out_buf, full.out_buf)
    assert same_bits(x, x0)
    if n >= 73:
        assert len(torch.unique(off)) >= (3 if W > 1 else 2)      # the batch does exercise several shifts


# ---- 3. pure roll -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("CP,W", [(16, 16), (16, 3), (4, 4), (4, 1)])
def test_a_pure_roll_moves_the_offset_by_the_roll(lib, CP, W):
    n = 73
    xs = R.case_frames("AWGN", 30.0, CP)[:n]
    _, lam0, phi0 = R.reference(xs, K, CP, W)
    ok0 = R.decidable(lam0, phi0)
    base = Run(lib, dev(xs), CP, W)
    assert base.status == 0
    off0 = base.offset.cpu().numpy().astype(np.int64)
    checked = 0
    for d in range(-W, W + 1):
        xr = R.roll_frames(xs, d)
        _, lam, phi = R.reference(xr, K, CP, W)
        r = Run(lib, dev(xr), CP, W)
        assert r.status == 0 and r.guards_intact()
        off = r.offset.cpu().numpy().astype(np.int64)
        use = ok0 & R.decidable(lam, phi) & (np.abs(off0 + d) <= W)
        assert np.array_equal(off[use], off0[use] + d), d
        checked += int(use.sum())
    assert checked >= 0.9 * n * (2 * W + 1)


# ---- 4. the receive path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,batch", [(2, 36), (4, 8)])
@pytest.mark.parametrize("cp", [True, False])
def test_receiver_sync_equals_receive_of_the_rolled_frames(nbits, batch, cp):
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    from dl_ofdm_amd.sync import FrameSync
    CP, W = 16, 3
    kin = K + CP if cp else K
    dims = RxDims(S=S, kin=kin, F=64, D=320, nbits=nbits)
    p = O.init_params(O.RxConfig(S=S, kin=kin, F=64, D=320, nbits=nbits), seed=11 + nbits)
    x = dev(R.case_frames("ETU", 30.0, CP)[:batch])
    x0 = x.clone()
    rcv = RxReceiver(dims, batch, p, want_llr=True, want_prob=True, CP=CP if cp else None)
    res = rcv.receive(x, sync=W)
    torch.cuda.synchronize()
    assert res.offset is not None and res.offset.dtype == torch.int32 and tuple(res.offset.shape) == (batch,)
    off = res.offset.clone()
    got = [t.clone() for t in (res.packed, res.llr, res.prob, rcv.x)]
    fs = FrameSync(S, K, CP, W, batch, DEV)
    _, off_fs = fs.run(x)
    torch.cuda.synchronize()
    assert torch.equal(off, off_fs) and bool((off != 0).any())
    assert same_bits(x, x0)
    want_x = rolled(x0, off)
    if not cp:
        want_x = want_x[:, :, CP:CP + K].contiguous()
    ref = rcv.receive(want_x)
    torch.cuda.synchronize()
    assert ref.offset is None
    assert same_bits(got[3], want_x)
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
    # and the frames as they came give other bits: the alignment is not a no-op on this batch
    plain = rcv.receive(x0 if cp else x0[:, :, CP:CP + K].contiguous())
    torch.cuda.synchronize()
    assert not same_bits(plain.llr, got[1])


def test_receiver_sync_refusals():
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.engine import RxDims
    from dl_ofdm_amd.receive import RxReceiver
    p = O.init_params(O.RxConfig(S=S, kin=80, F=64, D=320, nbits=2), seed=3)
    rcv = RxReceiver(RxDims(S=S, kin=80, F=64, D=320, nbits=2), 8, p)          # whole symbols, no CP given
    xs = R.case_frames("EVA", 30.0, 16)[:8]
    with pytest.raises(_lib.DccnError):
        rcv.receive(dev(xs), sync=3)
    rcv = RxReceiver(RxDims(S=S, kin=80, F=64, D=320, nbits=2), 8, p, CP=16)
    with pytest.raises(_lib.DccnError):
        rcv.receive(xs, sync=3)                                               # a host array
    with pytest.raises(_lib.DccnError):
        rcv.receive(dev(xs), sync=17)                 # W > CP


class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


def _trainer(nbits, seed=21):
    """the chain of tests/test_gpu_receive.py, re-stated"""
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.ofdm import ofdm_tx
    F = _Flags()
    F.nbits, F.opt, F.init_learning, F.cp = nbits, 0, 1e-3, True
    tx = ofdm_tx(F)
    ecfg = E.EqConfig(S=7, K=tx.K, CP=tx.CP, cp=True, pilot_size=tx.pilot_size,
                      pilot_carriers=tuple(int(v) for v in tx.pilotCarriers))
    rcfg = O.RxConfig(S=7, kin=tx.K + tx.CP, F=64, D=tx.frame_size, nbits=nbits)
    tr = EqualizerTrainer(F, tx, O.init_params(rcfg, seed=seed + 1), seed=3)
    tr.load_params(E.init_params(ecfg, seed=seed, bias_scale=0.05))
    return tx, tr


@pytest.mark.parametrize("B", [8, 73])
def test_chain_sync_equals_chain_receive_of_the_rolled_frames(B):
    from dl_ofdm_amd.receive import chain_receive
    from dl_ofdm_amd.sync import FrameSync
    CP, W = 16, 3
    tx, tr = _trainer(2)
    x = dev(R.case_frames("ETU", 30.0, CP)[:B])
    x0 = x.clone()
    res = chain_receive(tr, x, want_llr=True, want_prob=True, sync=W)
    torch.cuda.synchronize()
    off = res.offset.clone()
    got = [t.clone() for t in (res.packed, res.llr, res.prob, tr.resident(B).x, tr.resident(B).out_eq)]
    _, off_fs = FrameSync(S, K, CP, W, B, DEV).run(x)
    torch.cuda.synchronize()
    assert torch.equal(off, off_fs) and bool((off != 0).any()) and same_bits(x, x0)
    want_x = rolled(x0, off)
    ref = tr.receive(want_x, want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert ref.offset is None
    assert same_bits(got[3], want_x) and same_bits(got[4], tr.resident(B).out_eq)
    assert torch.equal(got[0], ref.packed) and same_bits(got[1], ref.llr) and same_bits(got[2], ref.prob)
    assert chain_receive(tr, x0, sync=0).offset is None


# ---- 5. refusals --------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing(lib):
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.sync import FrameSync
    CP, W, n = 16, 3, 9
    xs = R.case_frames("EVA", 30.0, CP)[:n]
    # x with room in front and behind, so that shifted pointers stay inside the allocation
    store = torch.zeros(2 * n * S * (K + CP) * 2 + 64, dtype=torch.float32, device=DEV)
    x = store[16:16 + xs.size].view(xs.shape)
    x.copy_(dev(xs))
    x0 = store.clone()
    assert x.data_ptr() % 16 == 0
    ok = Run(lib, x, CP, W)
    assert ok.status == 0 and not ok.untouched()
    cases = {
        "W = 0": dict(W=0), "W = CP + 1": dict(W=CP + 1), "2 W + CP > 64": dict(K=48, CP=32, W=17),
        "odd T": dict(K=63, out_kin=63 + CP), "S = 0": dict(S=0),
        "frames = 0": dict(frames=0), "frames < 0": dict(frames=-3),
        "x NULL": dict(x=None), "offset NULL": dict(offset=None),
        "x off 16 bytes": dict(x=x.data_ptr() + 4),
        "out_kin": dict(out_kin=K + CP - 1), "out_kin 0": dict(out_kin=0),
        "x_out is x": dict(x_out=x.data_ptr()),
        "x_out inside x": dict(x_out=x.data_ptr() + 16 * 5),
        "x_out ends inside x": dict(x_out=x.data_ptr() - 64),
    }
    for what, over in cases.items():
        r = Run(lib, x, CP, W, over=over)
        assert r.status == -1, what
        assert r.untouched(), what
        assert same_bits(store, x0), what
    spare = torch.full((xs.size + GUARD,), SENT_X, dtype=torch.float32, device=DEV)
    for what in ("x_out", "metric"):                 # one float off a 16-byte boundary
        r = Run(lib, x, CP, W, over={what: spare.data_ptr() + 4})
        assert r.status == -1 and r.untouched() and bool((spare == SENT_X).all()), what
    assert same_bits(store, x0)
    # the cropped form with an odd S K: rows that are no multiple of 16 bytes
    assert lib.dccn_frame_sync_supported(1, 5, 3, 1) == 1
    small = torch.zeros(4, 1, 8, 2, dtype=torch.float32, device=DEV)
    r = Run(lib, small, 3, 1, out_kin=5, over=dict(S=1, K=5))
    assert r.status == -1 and r.untouched()
    with pytest.raises(_lib.DccnError):
        FrameSync(S, K, CP, CP + 1, n, DEV)
    with pytest.raises(_lib.DccnError):
        FrameSync(S, 1024, 256, 16, n, DEV)
    fs = FrameSync(S, K, CP, W, n, DEV)
    with pytest.raises(_lib.DccnError):
        fs.run(torch.from_numpy(np.array(xs)))                                  # a CPU tensor
    with pytest.raises(_lib.DccnError):
        fs.run(xs)                                                   # a host array
    with pytest.raises(_lib.DccnError):
        fs.run(x, out=x)                                             # overlapping: refused by the library
    aligned, off = fs.run(x)
    torch.cuda.synchronize()
    assert torch.equal(off, ok.offset) and same_bits(aligned, ok.out)
