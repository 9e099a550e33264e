"""The host half of the step timeline (dl_ofdm_amd/steptrace.py) on synthetic rings: no GPU, no library.

``decode_ring`` turns the words a traced run left in the device ring into step records, ``summarise`` turns the records of several
bursts into the per-launch table bench.py prints as ``step.boundaries``.  Every number here is built by hand from the layout
include/dccn.h documents -- ring x launches x blocks x {wall at entry, cycles at entry, wall at exit, cycles at exit} -- so
that an expected value never comes from the code under test.
"""
import numpy as np
import pytest

from dl_ofdm_amd.steptrace import SLOT_NAMES, WALL_HZ, decode_ring, summarise

GEO = (8, 16, 4)                 # launches, blocks, words: the library's geometry with fewer blocks


def empty(ring):
    return np.zeros((ring,) + GEO, dtype=np.uint64)


def put(t, entry, slot, block, w0, w1, c0=1000, c1=None):
    """one workgroup's four words; w1 = 0: it entered and never left"""
    t[entry, slot, block] = (w0, c0, w1, 0 if w1 == 0 else (c1 if c1 is not None else c0 + 24 * (w1 - w0)))


def rec(start, end, sclk=None):
    return dict(start=start, end=end, blocks=1, sclk_mhz=sclk, block_us_median=(end - start) * 1e6 / WALL_HZ)


# ---- decode_ring: which entries, in which order -------------------------------------------------------------------------
def stamped_ring(ring, n):
    """step i of n leaves one block in slot 1 of entry i % ring, entering at 1000 * (i + 1)"""
    t = empty(ring)
    for i in range(n):
        t[i % ring] = 0
        put(t, i % ring, 1, 0, 1000 * (i + 1), 1000 * (i + 1) + 7)
    return t


@pytest.mark.parametrize("ring,n,steps", [(4, 0, []), (4, 1, [0]), (4, 3, [0, 1, 2]), (4, 4, [0, 1, 2, 3]), (4, 5, [1, 2, 3, 4]),
                                          (3, 5, [2, 3, 4]), (3, 7, [4, 5, 6]), (1, 9, [8])])
def test_ring_wrap_order(ring, n, steps):
    got = decode_ring(stamped_ring(ring, n).reshape(-1), n, ring, GEO)
    assert [r[1]["start"] for r in got] == [1000 * (i + 1) for i in steps]
    assert all(set(r) == {1} and r[1]["end"] == r[1]["start"] + 7 for r in got)


def test_no_steps_counted_reads_nothing_even_from_a_written_ring():
    """n is the library's count since the last enable: stale words of an earlier run are not steps"""
    assert decode_ring(stamped_ring(4, 4), 0, 4, GEO) == []


def test_decode_accepts_the_int64_words_a_torch_tensor_gives():
    t = stamped_ring(3, 2)
    put(t, 1, 2, 5, 2 ** 63 + 10, 2 ** 63 + 30)          # a counter past the sign bit of int64 words
    got = decode_ring(t.view(np.int64).reshape(-1), 2, 3, GEO)
    assert got[1][2]["end"] - got[1][2]["start"] == 20


def test_an_unwritten_step_is_an_empty_record_and_keeps_its_place():
    t = empty(4)
    put(t, 0, 1, 0, 100, 110)
    put(t, 2, 1, 0, 300, 310)
    got = decode_ring(t, 3, 4, GEO)
    assert [sorted(r) for r in got] == [[1], [], [1]]


def test_slots_and_blocks_are_read_where_the_header_puts_them():
    t = empty(2)
    put(t, 1, 4, 0, 500, 560)
    put(t, 1, 4, 3, 480, 590)
    put(t, 1, 4, 15, 510, 520)
    put(t, 1, 6, 1, 700, 705)
    r = decode_ring(t, 2, 2, GEO)[1]
    assert sorted(r) == [4, 6]
    assert (r[4]["start"], r[4]["end"], r[4]["blocks"]) == (480, 590, 3)
    assert (r[6]["start"], r[6]["end"], r[6]["blocks"]) == (700, 705, 1)
    assert r[4]["block_us_median"] == pytest.approx(60 * 1e6 / WALL_HZ)           # durations 60, 110, 10 ticks


# ---- a block that entered and never exited ------------------------------------------------------------------------------
def test_a_block_that_never_exited_counts_as_a_block_and_nowhere_else():
    t = empty(1)
    put(t, 0, 2, 0, 100, 400, c0=0, c1=7200)
    put(t, 0, 2, 1, 120, 0)                            # entered, no exit words
    r = decode_ring(t, 1, 1, GEO)[0][2]
    assert r["blocks"] == 2 and (r["start"], r["end"]) == (100, 400)
    assert r["block_us_median"] == pytest.approx(3.0) and r["sclk_mhz"] == pytest.approx(2400.0)


def test_a_launch_none_of_whose_blocks_exited_ends_at_its_last_entry():
    t = empty(1)
    put(t, 0, 2, 0, 100, 0)
    put(t, 0, 2, 1, 130, 0)
    r = decode_ring(t, 1, 1, GEO)[0][2]
    assert (r["start"], r["end"], r["blocks"]) == (100, 130, 2)
    assert r["sclk_mhz"] is None and r["block_us_median"] is None


# ---- the shader clock -----------------------------------------------------------------------------------------------------
def test_shader_clock_from_the_two_counters():
    """400 ticks of the 100 MHz counter = 4 us; 9600 cycles in 4 us = 2400 MHz"""
    t = empty(1)
    put(t, 0, 1, 0, 1000, 1400, c0=50_000, c1=59_600)
    assert decode_ring(t, 1, 1, GEO)[0][1]["sclk_mhz"] == pytest.approx(2400.0, rel=1e-12)


def test_short_blocks_do_not_vote_on_the_clock():
    """under 300 ticks one tick of rounding is more than 0.3 % of the ratio: the 299-tick block (at 100 MHz x 10 = 1000 MHz)
    is left out, the 300-tick one (2400 MHz) is in"""
    t = empty(1)
    put(t, 0, 1, 0, 1000, 1299, c0=0, c1=2990)
    put(t, 0, 1, 1, 1000, 1300, c0=0, c1=7200)
    assert decode_ring(t, 1, 1, GEO)[0][1]["sclk_mhz"] == pytest.approx(2400.0, rel=1e-12)
    put(t, 0, 1, 1, 1000, 1250, c0=0, c1=6000)
    assert decode_ring(t, 1, 1, GEO)[0][1]["sclk_mhz"] is None


def test_the_clock_is_the_median_over_the_long_blocks():
    t = empty(1)
    for b, mhz in enumerate((2100, 2400, 1200)):
        put(t, 0, 1, b, 1000, 1500, c0=0, c1=5 * mhz)
    assert decode_ring(t, 1, 1, GEO)[0][1]["sclk_mhz"] == pytest.approx(2100.0, rel=1e-12)


# ---- summarise --------------------------------------------------------------------------------------------------------------
TICK_US = 0.01


def burst(t0s, d1, g12, d2, clk=None):
    """steps starting at t0s: slot 1 runs d1[i] ticks, then a gap of g12[i], then slot 2 for d2[i]"""
    out = []
    for i, t0 in enumerate(t0s):
        e1 = t0 + d1[i]
        s2 = e1 + g12[i]
        out.append({1: rec(t0, e1, clk), 2: rec(s2, s2 + d2[i], clk)})
    return out


def rows(res):
    return {r["slot"]: r for r in res["launches"]}


def test_medians_and_p90_of_durations_and_gaps():
    d1 = [100, 200, 300, 400, 1000]
    g12 = [10, 20, 30, 40, 500]
    d2 = [50, 50, 50, 50, 50]
    t0s = [0, 2000, 4000, 6000, 8000]
    res = summarise([burst(t0s, d1, g12, d2)])
    r = rows(res)
    assert r[1]["us"] == pytest.approx(np.median(d1) * TICK_US) and r[1]["us_p90"] == pytest.approx(np.percentile(d1, 90) * TICK_US)
    assert r[2]["gap_before_us"] == pytest.approx(0.3) and r[2]["gap_before_us_p90"] == pytest.approx(np.percentile(g12, 90) * TICK_US)
    # the gap in front of slot 1 runs from the previous step's slot 2: four of them, none for the burst's first step
    g1 = [t0s[i + 1] - (t0s[i] + d1[i] + g12[i] + d2[i]) for i in range(4)]
    assert r[1]["gap_before_us"] == pytest.approx(np.median(g1) * TICK_US)
    assert r[1]["gap_before_us_p90"] == pytest.approx(round(np.percentile(g1, 90) * TICK_US, 2))
    assert res["sum_launch_us"] == pytest.approx(r[1]["us"] + r[2]["us"])
    assert res["sum_gap_us"] == pytest.approx(r[1]["gap_before_us"] + r[2]["gap_before_us"])


def test_the_period_is_first_launch_to_first_launch():
    t0s = [0, 1000, 2500, 4500, 7000]                     # periods 1000, 1500, 2000, 2500 ticks
    res = summarise([burst(t0s, [10] * 5, [1] * 5, [10] * 5)])
    assert res["samples"] == 4
    assert res["period_us"] == pytest.approx(17.5) and res["period_us_p90"] == pytest.approx(round(np.percentile([10, 15, 20, 25], 90), 2))


def test_nothing_is_measured_across_a_burst_border():
    """two bursts a second apart: neither a gap nor a period spans the read-back between them"""
    a = burst([0, 1000], [100, 100], [10, 10], [50, 50])
    b = burst([100_000_000, 100_001_000], [100, 100], [10, 10], [50, 50])
    res = summarise([a, b])
    r = rows(res)
    assert res["samples"] == 2 and res["period_us"] == pytest.approx(10.0) and res["period_us_p90"] == pytest.approx(10.0)
    assert r[1]["gap_before_us"] == pytest.approx(8.4) and r[1]["gap_before_us_p90"] == pytest.approx(8.4)
    assert r[2]["gap_before_us_p90"] == pytest.approx(0.1)


def test_a_burst_of_one_step_has_durations_but_no_period():
    res = summarise([burst([0], [100], [10], [50])])
    assert res["samples"] == 0 and "period_us" not in res
    r = rows(res)
    assert r[1]["us"] == pytest.approx(1.0) and np.isnan(r[1]["gap_before_us"]) and r[2]["gap_before_us"] == pytest.approx(0.1)


def test_launches_are_ordered_by_their_start_not_by_their_slot():
    """slot 5 running before slot 4: the gap in front of 4 is measured from 5"""
    step = {4: rec(500, 600), 5: rec(100, 400)}
    r = rows(summarise([[step]]))
    assert r[4]["gap_before_us"] == pytest.approx(1.0) and np.isnan(r[5]["gap_before_us"])


def test_an_empty_step_record_is_skipped():
    res = summarise([[{1: rec(0, 10)}, {}, {1: rec(1000, 1010)}]])
    assert res["samples"] == 1 and res["period_us"] == pytest.approx(10.0)


def test_the_clock_column_is_the_median_of_the_steps_that_have_one():
    steps = [{1: rec(0, 10, 2400.0)}, {1: rec(100, 110, None)}, {1: rec(200, 210, 2100.0)}, {1: rec(300, 310, 2000.0)}]
    assert rows(summarise([steps]))[1]["sclk_mhz"] == 2100.0
    assert rows(summarise([[{1: rec(0, 10)}]]))[1]["sclk_mhz"] is None


# ---- slot names ---------------------------------------------------------------------------------------------------------
def test_slot_names_cover_exactly_the_slots_the_library_writes():
    """include/dccn.h: slots 1-6 are written, 0 and 7 never"""
    assert sorted(SLOT_NAMES) == [1, 2, 3, 4, 5, 6] and len(set(SLOT_NAMES.values())) == 6
    step = {s: rec(100 * s, 100 * s + 50) for s in range(1, 7)}
    assert [r["name"] for r in summarise([[step]])["launches"]] == [SLOT_NAMES[s] for s in range(1, 7)]


def test_the_header_states_the_same_slot_table():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dccn.h")).read()
    para = text[text.index("step timeline: in-situ"):text.index("size_t dccn_step_trace_bytes")]
    flat = re.sub(r"\s*\*?\s+", " ", para)
    for s in SLOT_NAMES:
        assert re.search(r"\b%d [A-Za-z]" % s, flat[flat.index("Slots:"):]), s
    assert "0 and 7 are never written" in flat
