"""The device-side accumulators behind the published numbers (``-m gpu``): ``dccn_metrics_table_add`` / ``dccn_metrics_table_set``
(a row of a sweep's BER table, dl_ofdm_amd/receiver.py, bench.py) and ``dccn_step_monitor_add`` (the per-epoch monitors of the
training loop).  Each is a handful of additions in a fixed order, so the expected values are the same additions in the same
order on the host -- Python floats for the double rows, ``np.float32`` for the monitors -- and the comparison is bit for bit.
The records come from three real evaluation steps on three different batches of 13 QPSK frames.
"""
import numpy as np
import pytest
import torch

from test_gpu_engine import make_case

pytestmark = pytest.mark.gpu
INVALID_ARG = -1                        # DCCN_ERR_INVALID_ARG (include/dccn.h)
BATCH, NBITS = 13, 2


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def records():
    """three evaluation steps: per step the device record (a copy of the engine's dccn_metrics), its tx_power on the device,
    and both as `eng.metrics()` reads them back"""
    from dl_ofdm_amd.engine import RxEngine
    dims, _, _, _, p = make_case(BATCH, NBITS, seed=0)
    eng = RxEngine(dims, BATCH, params=p, train=False)
    out = []
    for seed in (0, 1, 2):
        _, _, x, bits, _ = make_case(BATCH, NBITS, seed=seed)
        eng.eval_step(x, bits)
        torch.cuda.synchronize()
        out.append(dict(dev=eng.metrics_buf.clone(), tx=eng.tx_power.clone(), host=eng.metrics()))
    cells = BATCH * dims.D * NBITS
    for r in out:
        m = r["host"]
        assert m["count"] == cells == sum(map(sum, m["conf"])) and 0 < m["count"] < 2 ** 53 and m["ce_sum"] > 0.0
    assert len({r["host"]["ce_sum"] for r in out}) == 3 and len({r["host"]["ce_mean"] for r in out}) == 3     # three different batches
    return out


def row_of(m):
    return [float(m["conf"][0][0]), float(m["conf"][0][1]), float(m["conf"][1][0]), float(m["conf"][1][1]), m["ce_sum"],
            float(m["count"])]


def bits64(values):
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


def bits32(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32).tolist()


def test_table_add_sums_in_call_order(lib, records):
    row = torch.zeros(6, dtype=torch.float64, device="cuda")
    want = [0.0] * 6
    for r in records:
        assert lib.dccn_metrics_table_add(r["dev"].data_ptr(), row.data_ptr(), None) == 0
        want = [a + b for a, b in zip(want, row_of(r["host"]))]
    torch.cuda.synchronize()
    assert bits64(row.cpu().numpy()) == bits64(want)
    # the other order is a different double for ce_sum unless the three happen to commute: the call order is what is pinned
    assert want[5] == 3 * records[0]["host"]["count"] and sum(want[:4]) == want[5]


def test_table_add_adds_to_what_the_row_holds(lib, records):
    start = [1.0, 2.0, 3.0, 4.0, 0.125, 10.0]
    row = torch.tensor(start, dtype=torch.float64, device="cuda")
    assert lib.dccn_metrics_table_add(records[1]["dev"].data_ptr(), row.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bits64(row.cpu().numpy()) == bits64([a + b for a, b in zip(start, row_of(records[1]["host"]))])


def test_table_set_overwrites_a_nan_row_with_the_last_record(lib, records):
    whole = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    row = whole[1:7]
    for r in records:
        assert lib.dccn_metrics_table_set(r["dev"].data_ptr(), row.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert bits64(got[1:7]) == bits64(row_of(records[-1]["host"]))
    assert np.isnan(got[0]) and np.isnan(got[7])


def test_step_monitor_add_is_three_float32_sums(lib, records):
    acc = torch.zeros(3, dtype=torch.float32, device="cuda")
    noise = [torch.tensor([v], dtype=torch.float32, device="cuda") for v in (0.1, 0.2, 0.30000001)]
    want = np.zeros(3, np.float32)
    for r, nz in zip(records, noise):
        assert lib.dccn_step_monitor_add(r["dev"].data_ptr(), r["tx"].data_ptr(), nz.data_ptr(), acc.data_ptr(), None) == 0
        want[0] = want[0] + np.float32(r["host"]["ce_mean"])
        want[1] = want[1] + np.float32(r["tx"].item())
        want[2] = want[2] + np.float32(nz.item())
    torch.cuda.synchronize()
    assert bits32(acc.cpu().numpy()) == bits32(want)
    assert want[0] > 0 and want[1] > 0


@pytest.mark.parametrize("missing", ["tx_power", "noise_power", "both"])
def test_step_monitor_add_leaves_the_element_of_a_null_input(lib, records, missing):
    start = np.array([0.5, 7.25, -3.5], np.float32)
    whole = torch.full((5,), float("nan"), dtype=torch.float32, device="cuda")
    acc = whole[1:4]
    acc.copy_(torch.from_numpy(start))
    r = records[2]
    noise = torch.tensor([0.75], dtype=torch.float32, device="cuda")
    tx = None if missing in ("tx_power", "both") else r["tx"].data_ptr()
    nz = None if missing in ("noise_power", "both") else noise.data_ptr()
    assert lib.dccn_step_monitor_add(r["dev"].data_ptr(), tx, nz, acc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want = start.copy()
    want[0] = want[0] + np.float32(r["host"]["ce_mean"])
    if tx is not None:
        want[1] = want[1] + np.float32(r["tx"].item())
    if nz is not None:
        want[2] = want[2] + np.float32(0.75)
    got = whole.cpu().numpy()
    assert bits32(got[1:4]) == bits32(want) and np.isnan(got[0]) and np.isnan(got[4])


def test_null_arguments_are_refused_and_launch_nothing(lib, records):
    r = records[0]
    row = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda")
    acc = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    rec = r["dev"].clone()
    torch.cuda.synchronize()
    assert lib.dccn_metrics_table_add(None, row.data_ptr(), None) == INVALID_ARG
    assert lib.dccn_metrics_table_add(rec.data_ptr(), None, None) == INVALID_ARG
    assert lib.dccn_metrics_table_set(None, row.data_ptr(), None) == INVALID_ARG
    assert lib.dccn_metrics_table_set(rec.data_ptr(), None, None) == INVALID_ARG
    assert lib.dccn_step_monitor_add(None, r["tx"].data_ptr(), r["tx"].data_ptr(), acc.data_ptr(), None) == INVALID_ARG
    assert lib.dccn_step_monitor_add(rec.data_ptr(), r["tx"].data_ptr(), r["tx"].data_ptr(), None, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(row).all()) and bool(torch.isnan(acc).all()) and torch.equal(rec, r["dev"])
