"""The chain's receive step (include/dccn.h dccn_eq_receive_step; EqualizerTrainer.receive, chain_receive, group_receive) away
from N = 64 / CP = 16 / FLAGS.cp on, held to float64 (``-m gpu``).

Every case of chain_receive_ref.CASES first asserts its route through the library's own host-only queries, then runs one receive
call and hands its tensors to chain_receive_ref.check_receive: the forward stages R0 .. dense_5 and the pilot SNR on the step's
own workspace tensors, ``llr`` and ``prob`` against the frozen receiver in float64 on the step's own ``out_eq`` (1e-5 of the
reference's maximum), the packed decisions (exact outside the 2e-5 tie margin, capped inside), padding, row layout and the
coherence of the three outputs.  Then the evaluation step on the same frames: ``out_eq`` / ``chest`` / ``snr_db`` bit for bit,
and the confusion table it tallies is the table of the received bits.  The grouped receive at ``cp`` off and the alignment stage
in front of the chain at two more geometries are held bit for bit to the calls they are made of.

Measured (MI355X; worst stage / llr / prob error, near ties): DESIGN.md section 4."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_receive_ref as R
from oracle import equalizer_oracle as E

pytestmark = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT_F32 = float(np.frombuffer(bytes([SENT_BYTE] * 4), np.float32)[0])
DEV = "cuda"


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _trainer(nbits, B, **geometry):
    from test_gpu_equalizer import _trainer as mk
    return mk(nbits=nbits, seed=71 + B, **geometry)


def _fill_outputs(pl, B, D, nbits):
    """packed / llr / prob of the plan's receive calls (created here where the plan has none yet) and the step's own outputs,
    all filled with the sentinel"""
    from dl_ofdm_amd.receive import row_bytes
    out = pl._receive_out
    shapes = dict(packed=((B, row_bytes(D, nbits)), torch.uint8), llr=((B, D, nbits), torch.float32),
                  prob=((B, D, nbits, 2), torch.float32))
    for name, (shp, dt) in shapes.items():
        if name not in out:
            out[name] = torch.empty(*shp, dtype=dt, device=pl.tr.device)
        assert tuple(out[name].shape) == shp
        out[name].view(torch.uint8).fill_(SENT_BYTE)
    for t in (pl.out_eq, pl.chest, pl.snr_db):
        t.fill_(SENT_F32)
    return out


def _is_sentinel(t: torch.Tensor) -> bool:
    return bool((t.contiguous().view(torch.uint8) == SENT_BYTE).all())


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_chain_receive_at_every_prefix_and_window(case):
    from dl_ofdm_amd.receive import unpack_bits
    from test_gpu_equalizer_stages import FWD_NAMES, _outputs, _ws
    from test_gpu_receive import host_conf
    cs = R.CASES[case]
    nbits, B = cs["nbits"], cs["B"]
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer(nbits, B, **cs["geometry"])
    D = rcfg.D
    got = R.route_of(tr.lib, B, ecfg, rcfg, cs["route"]["rx_k"])
    assert got == cs["route"], "route: the library answers %r, the case expects %r" % (got, cs["route"])
    rng = R.case_rng(case)
    x = R.case_frames(rng, B, ecfg)
    bits = rng.randint(0, 2, (B, D, nbits)).astype(np.int32)                     # (drawn after the frames)
    shp = E.param_shapes(ecfg)
    P = {n: a.astype(np.float64).reshape(shp[n]) for n, a in tr.get_params().items()}
    pl = tr.resident(B)

    # ---- one receive call with every output, against float64 -----------------------------------------------------------------
    out = _fill_outputs(pl, B, D, nbits)
    r = tr.receive(x, want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert r.packed is out["packed"] and r.llr is out["llr"] and r.prob is out["prob"] and (r.D, r.nbits) == (D, nbits)
    v = _outputs({n: _ws(tr, pl, n, train=0) for n in FWD_NAMES}, pl)
    v["x"] = x
    first = {n: t.clone() for n, t in dict(packed=r.packed, llr=r.llr, prob=r.prob, out_eq=pl.out_eq, chest=pl.chest,
                                           snr_db=pl.snr_db).items()}
    failed, fig = R.check_receive(v, P, ecfg, rcfg, pr, first["packed"].cpu().numpy(), first["llr"].cpu().numpy(),
                                  first["prob"].cpu().numpy(), label="case %s:" % case)
    assert not failed, "case %s fails %s: %r" % (case, sorted(failed), fig)

    # ---- the evaluation step on the same frames: the same equaliser outputs, and it tallies these decisions -------------------
    hard = unpack_bits(first["packed"].cpu().numpy(), D, nbits)
    for t in (pl.out_eq, pl.chest, pl.snr_db):
        t.fill_(SENT_F32)
    m = tr.eval_step(x, bits, graph=False)
    torch.cuda.synchronize()
    for name in ("out_eq", "chest", "snr_db"):
        assert same_bits(getattr(pl, name), first[name]), name
    assert host_conf(hard, bits) == [[int(c) for c in row] for row in np.asarray(m["conf"]).reshape(2, 2)]

    # ---- no optional outputs: the same packed bits, llr / prob not written ---------------------------------------------------
    out = _fill_outputs(pl, B, D, nbits)
    r2 = tr.receive(x)
    torch.cuda.synchronize()
    assert r2.llr is None and r2.prob is None
    assert torch.equal(r2.packed, first["packed"])
    assert _is_sentinel(out["llr"]) and _is_sentinel(out["prob"])
    for name in ("out_eq", "chest", "snr_db"):
        assert same_bits(getattr(pl, name), first[name]), name

    # ---- the same call again: the same bits ---------------------------------------------------------------------------------
    r3 = tr.receive(x, want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert torch.equal(r3.packed, first["packed"]) and same_bits(r3.llr, first["llr"]) and same_bits(r3.prob, first["prob"])


# ---- grouped receive with FLAGS.cp off -------------------------------------------------------------------------------------------
def test_grouped_receive_without_cp_equals_the_solo_receive_bit_for_bit():
    """N = 64, the long prefix, FLAGS.cp off (case a of the stage checker's GEOMETRY_CASES: dccn_eq_group_supported and
    dccn_eq_receive_group_supported answer 1): the folded matrix carries zero rows for the prefix samples, one per chain"""
    import test_gpu_group_receive as G
    from dl_ofdm_amd.equalizer import EqualizerTrainer
    from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
    from dl_ofdm_amd.receive import row_bytes
    from oracle import dccn_oracle as O
    from test_gpu_equalizer import _trainer_config
    mods, B = (1, 2, 3, 4), 73
    chains = []
    for i, nb in enumerate(mods):
        F, tx, ecfg, rcfg, pe, pr = _trainer_config(nb, seed=21 + 10 * i + nb, cp=False, rx_bias=0.05)
        assert (ecfg.cp, rcfg.kin, ecfg.n_sc) == (False, 64, 80)
        chains.append((F, tx, pe, pr, ecfg, rcfg))
    F0, _, _, _, ecfg0, rcfg0 = chains[0]
    from dl_ofdm_amd import _lib
    from test_gpu_equalizer_stages import eq_shape
    lib = _lib.load()
    assert int(lib.dccn_eq_receive_group_supported(C.byref(eq_shape(B, ecfg0, rcfg0)))) == 1
    grp = ChainReceiveGroup([c[0] for c in chains], [c[3] for c in chains], B, want_llr=True, want_prob=True)
    for ch, c in zip(grp.chains, chains):
        ch.tr.load_params(c[2])
    assert int(grp.lib.dccn_eq_receive_group_supported(C.byref(grp.chains[0].pl.shape))) == 1
    assert grp.chains[0].pl.shape.cp == 0
    G._fill_sentinels(grp, B)
    xs = [(np.random.RandomState(600 + 17 * i + nb + B).standard_normal((B, 7, 80, 2)) * 2).astype(np.float32)
          for i, nb in enumerate(mods)]
    res = grp.receive(xs)
    torch.cuda.synchronize()
    for i, (nb, ch, r, c) in enumerate(zip(mods, grp.chains, res, chains)):
        tr = EqualizerTrainer(c[0], c[1], c[3], seed=3)
        tr.load_params(c[2])
        ref = tr.receive(xs[i], want_llr=True, want_prob=True)
        torch.cuda.synchronize()
        pl = tr.resident(B)
        assert r.nbits == nb and tuple(r.packed.shape) == (B, row_bytes(ch.D, nb))
        assert torch.equal(r.packed, ref.packed), (i, nb, "packed")
        assert same_bits(r.llr, ref.llr) and same_bits(r.prob, ref.prob), (i, nb)
        for name in ("out_eq", "chest", "snr_db"):
            assert same_bits(getattr(ch.pl, name), getattr(pl, name)), (i, nb, name)
        assert not _is_sentinel(r.packed) and bool(r.packed.any())


# ---- the alignment stage in front of the chain, away from the default geometry ----------------------------------------------------
def _offset_frames(B, S, K, CP, W, seed, eps):
    """frames with an exact cyclic prefix, a carrier-frequency offset per frame (eps: its largest magnitude, in subcarrier
    spacings) and a delay per frame in [-W, W] (tests/frame_cfo_ref.py exact_prefix_frames, tests/frame_sync_ref.py aligned)"""
    import frame_cfo_ref as FC
    import frame_sync_ref as FS
    rs = np.random.RandomState(seed)
    x = FC.exact_prefix_frames(B, S, K, CP, seed, eps=rs.uniform(-eps, eps, B))
    d = rs.randint(-W, W + 1, B)
    d[:2] = (W, -W)
    x = FS.aligned(x, -d) + 0.01 * rs.standard_normal(x.shape)
    return np.ascontiguousarray(x.astype(np.float32)), d


@pytest.mark.parametrize("cfo", [False, True])
@pytest.mark.parametrize("nfft,longcp,cp,W", [(64, False, False, 4), (128, True, True, 16)])
def test_chain_sync_away_from_the_default_geometry(nfft, longcp, cp, W, cfo):
    """chain_receive(x, sync=W, cfo=...) == FrameSync(...).run followed by chain_receive of the frames it wrote, bit for bit; the
    offsets (and carrier-frequency offsets) returned are the stage's"""
    from dl_ofdm_amd.receive import chain_receive
    from dl_ofdm_amd.sync import FrameSync
    B, nbits = 12, 2
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer(nbits, B, nfft=nfft, longcp=longcp, cp=cp, rx_bias=0.05)
    S, K, CP = ecfg.S, ecfg.K, ecfg.CP
    xs, d = _offset_frames(B, S, K, CP, W, seed=900 + nfft + W, eps=0.2 if cfo else 0.0)
    x = torch.from_numpy(xs).to(DEV)
    x0 = x.clone()
    pl = tr.resident(B)
    _fill_outputs(pl, B, rcfg.D, nbits)
    res = chain_receive(tr, x, want_llr=True, want_prob=True, sync=W, cfo=cfo)
    torch.cuda.synchronize()
    assert (res.cfo is not None) == cfo
    got = {n: t.clone() for n, t in dict(packed=res.packed, llr=res.llr, prob=res.prob, x=pl.x, out_eq=pl.out_eq, chest=pl.chest,
                                         snr_db=pl.snr_db, offset=res.offset).items()}
    if cfo:
        got["cfo"] = res.cfo.clone()
    fs = FrameSync(S, K, CP, W, B, DEV, cfo=cfo)
    want_x, off = fs.run(x)
    torch.cuda.synchronize()
    assert same_bits(x, x0)
    assert torch.equal(got["offset"], off) and bool((off != 0).any())
    assert np.array_equal(off.cpu().numpy(), d)                      # exact prefixes, 1 % noise: the delays drawn are the estimates
    if cfo:
        assert same_bits(got["cfo"], fs.cfo) and bool((fs.cfo != 0).all())
    assert same_bits(got["x"], want_x)
    _fill_outputs(pl, B, rcfg.D, nbits)
    ref = chain_receive(tr, want_x.clone(), want_llr=True, want_prob=True)
    torch.cuda.synchronize()
    assert ref.offset is None and ref.cfo is None
    assert torch.equal(got["packed"], ref.packed) and same_bits(got["llr"], ref.llr) and same_bits(got["prob"], ref.prob)
    for name in ("out_eq", "chest", "snr_db"):
        assert same_bits(got[name], getattr(pl, name)), name


@pytest.mark.parametrize("cfo", [False, True])
def test_chain_sync_refuses_an_odd_frame_length_and_launches_nothing(cfo):
    """N = 128 with the short prefix: T = 7 * 137 = 959 samples, odd -- the alignment stage cannot run (dccn_frame_sync_supported),
    the call raises before anything is staged or launched"""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.receive import chain_receive
    B, nbits, W = 12, 2, 4
    F, tx, ecfg, rcfg, pe, pr, tr = _trainer(nbits, B, nfft=128, longcp=False, cp=True, rx_bias=0.05)
    assert (ecfg.S * ecfg.n_sc) % 2 == 1 and ecfg.S * ecfg.n_sc == 959
    assert tr.lib.dccn_frame_sync_supported(ecfg.S, ecfg.K, ecfg.CP, W) == 0
    pl = tr.resident(B)
    out = _fill_outputs(pl, B, rcfg.D, nbits)
    pl.x.fill_(SENT_F32)
    x = torch.from_numpy(R.case_frames(np.random.RandomState(7), B, ecfg)).to(DEV)
    with pytest.raises(_lib.DccnError):
        chain_receive(tr, x, want_llr=True, want_prob=True, sync=W, cfo=cfo)
    torch.cuda.synchronize()
    for t in (out["packed"], out["llr"], out["prob"], pl.out_eq, pl.chest, pl.x):
        assert _is_sentinel(t)
