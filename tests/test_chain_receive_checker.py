"""CPU check of the receive checker of tests/chain_receive_ref.py (what tests/test_gpu_chain_receive.py holds the chain's receive
step to): fed with the float64 whole-graph oracle's values, rounded to float32 and packed by ``receive.pack_bits``, in the place of
the GPU's tensors, every check passes at four geometries and every modulation; six mutations of those values each fail exactly
the checks they must; every GPU case lands on the route its table states (the library's host-only queries); and with every GPU
case's own seeds the oracle alone stays inside the near-tie cap and decides both ways."""
import os

import numpy as np
import pytest

import chain_receive_ref as R
from oracle import dccn_oracle as O
from oracle import equalizer_oracle as E
from test_equalizer_stage_checker import oracle_values

# (K, CP, cp) -> nbits: every modulation once over the four
GEOMETRIES = {(64, 16, False): 2, (64, 4, True): 1, (64, 4, False): 3, (128, 9, False): 4}
COHERENCE = {"prob coherence", "llr coherence"}


def gpu_like(K, CP, cp, nbits):
    """the whole-graph oracle's values at B = 5 as a receive call would leave them: every tensor rounded to float32, the
    decisions packed.  Returns (v, P, ecfg, rcfg, pr, out) with out = dict(packed, llr, prob) and the unrounded out_eq."""
    from dl_ofdm_amd.receive import pack_bits
    v, pe, _, c, lit_rx, _, _, _ = oracle_values(K, CP, cp, B=5, nbits=nbits, seed=3)
    rc = lit_rx.cfg
    assert rc.nbits == nbits
    pr = {k: t.detach().numpy().copy() for k, t in lit_rx.p.items()}
    ref = R.oracle_decision(pr, v["out_eq"], c, rc)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)      # noqa: E731
    v32 = {k: f32(a) for k, a in v.items()}
    out = dict(packed=pack_bits(ref["hard"]), llr=f32(ref["llr"]), prob=f32(ref["prob"]), hard=ref["hard"], near=ref["near"],
               out_eq=v["out_eq"])
    return v32, pe, c, rc, pr, out


@pytest.fixture(scope="module")
def values():
    """one oracle run per geometry, shared and left unchanged (the mutation tests copy what they change)"""
    cache = {}

    def get(K, CP, cp):
        if (K, CP, cp) not in cache:
            cache[(K, CP, cp)] = gpu_like(K, CP, cp, GEOMETRIES[(K, CP, cp)])
        return cache[(K, CP, cp)]
    return get


def _failed(vals, **over):
    v, P, c, rc, pr, out = vals
    o = dict(out, **over)
    return R.check_receive(v, P, c, rc, pr, o["packed"], o["llr"], o["prob"])[0]


@pytest.mark.parametrize("K,CP,cp", sorted(GEOMETRIES))
def test_checker_passes_on_the_whole_graph_oracle(values, K, CP, cp):
    v, P, c, rc, pr, out = values(K, CP, cp)
    failed, fig = R.check_receive(v, P, c, rc, pr, out["packed"], out["llr"], out["prob"])
    assert not failed, (failed, fig)
    # float64 values rounded once to float32: every figure is at rounding level, far below the 1e-5 the GPU is held to
    assert fig["stages"] <= 1e-6 and fig["llr"] <= 1e-6 and fig["prob"] <= 1e-6, fig
    assert fig["cells"] == 5 * rc.D * rc.nbits


@pytest.mark.parametrize("K,CP,cp", sorted(GEOMETRIES))
def test_llr_off_by_1e4_fails_llr_only(values, K, CP, cp):
    vals = values(K, CP, cp)
    assert _failed(vals, llr=vals[5]["llr"] * (1 + 1e-4)) == {"llr"}


def test_swapped_llrs_of_a_qpsk_cell_fail_llr_and_its_coherence(values):
    vals = values(64, 16, False)
    assert vals[3].nbits == 2
    assert _failed(vals, llr=vals[5]["llr"][..., ::-1].copy()) == {"llr", "llr coherence"}


@pytest.mark.parametrize("K,CP,cp", sorted(GEOMETRIES))
def test_one_flipped_bit_fails_decisions_and_coherence(values, K, CP, cp):
    from dl_ofdm_amd.receive import pack_bits
    vals = values(K, CP, cp)
    out = vals[5]
    hard = out["hard"].copy()
    f, d, b = [int(i[0]) for i in np.nonzero(~out["near"] & (np.abs(out["llr"]) > 1e-3))]      # a cell outside the margin
    hard[f, d, b] ^= 1
    assert _failed(vals, packed=pack_bits(hard)) == {"decisions"} | COHERENCE


@pytest.mark.parametrize("K,CP,cp", sorted(GEOMETRIES))
def test_bits_packed_lsb_first_fail_layout_and_decisions(values, K, CP, cp):
    """(and the two coherence checks, which read the same bits)"""
    vals = values(K, CP, cp)
    hard = vals[5]["hard"]
    lsb = np.packbits(hard.reshape(hard.shape[0], -1), axis=1, bitorder="little")
    assert lsb.shape == vals[5]["packed"].shape
    assert _failed(vals, packed=lsb) == {"layout", "decisions"} | COHERENCE


@pytest.mark.parametrize("K,CP,cp", [g for g in sorted(GEOMETRIES) if not g[2]])
def test_a_window_one_sample_off_fails_llr_prob_and_decisions(values, K, CP, cp):
    """the receiver fed out_eq rolled by one sample along the subcarrier axis (a window read one sample off), cp off"""
    from dl_ofdm_amd.receive import pack_bits
    vals = values(K, CP, cp)
    v, P, c, rc, pr, out = vals
    off = R.oracle_decision(pr, np.roll(out["out_eq"], 1, axis=2), c, rc)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    assert _failed(vals, packed=pack_bits(off["hard"]), llr=f32(off["llr"]), prob=f32(off["prob"])) == {"llr", "prob", "decisions"}


@pytest.mark.parametrize("K,CP,cp", sorted(GEOMETRIES))
def test_swapped_prob_pairs_fail_prob_and_its_coherence(values, K, CP, cp):
    vals = values(K, CP, cp)
    assert _failed(vals, prob=vals[5]["prob"][..., ::-1].copy()) == {"prob", "prob coherence"}


def test_nonzero_padding_bits_are_seen():
    """no GPU case has padding bits (D nbits is a multiple of 8 at every geometry of the grid), so the check is proven here on
    its own: D = 3 cells of QPSK leave two padding bits"""
    from dl_ofdm_amd.receive import pack_bits, row_bytes
    hard = np.array([[[1, 0], [0, 1], [1, 1]]], np.uint8)
    good = pack_bits(hard)
    assert row_bytes(3, 2) == 1 and good.tolist() == [[0b10011100]]
    assert np.array_equal(R.numpy_unpack(good, 3, 2), hard) and R.padding_clear(good, 3, 2)
    for bad in (good | 1, good | 2):
        assert np.array_equal(R.numpy_unpack(bad, 3, 2), hard) and not R.padding_clear(bad, 3, 2)
        assert not np.array_equal(pack_bits(R.numpy_unpack(bad, 3, 2)), bad)           # the round trip of the layout check


# ---- the GPU cases, host side ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_every_gpu_case_lands_on_the_route_its_table_states(lib, case):
    """the library's host-only queries (nothing is launched): what the GPU test asserts again before it issues the step"""
    _, tx, c, rc, _, _ = R.case_config(case)
    cs = R.CASES[case]
    got = R.route_of(lib, cs["B"], c, rc, cs["route"]["rx_k"])
    assert got == cs["route"], "route: the library answers %r, the case expects %r" % (got, cs["route"])
    assert cs["B"] <= 129


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_margins_of_the_gpu_cases_stay_inside_their_caps(case):
    """every case of tests/test_gpu_chain_receive.py with its own seeds, float64 oracle alone: the cells inside the tie margin
    are within the cap (5e-3 cells + 4), and both decisions occur (the share of ones lies between 0.2 and 0.85)"""
    _, tx, c, rc, pe, pr = R.case_config(case)
    cs = R.CASES[case]
    pe = {k: v.astype(np.float64) for k, v in pe.items()}
    pr = {k: v.astype(np.float64) for k, v in pr.items()}
    x = R.case_frames(R.case_rng(case), cs["B"], c)
    out, _, _ = E.equalizer_forward(pe, O.batch_moment_norm(x.astype(np.float64))[0], c)
    ref = R.oracle_decision(pr, out, c, rc)
    ties, cells, ones = int(ref["near"].sum()), int(ref["near"].size), float(ref["hard"].mean())
    print("%s: %d of %d cells (%.4f %%) inside the tie margin, cap %d; share of ones %.3f"
          % (case, ties, cells, 100.0 * ties / cells, int(R.tie_cap(cells)), ones))
    assert cells == cs["B"] * rc.D * rc.nbits
    assert ties <= R.tie_cap(cells)
    assert 0.2 <= ones <= 0.85
