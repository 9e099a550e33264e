"""Host side of the grouped receive step (include/dccn.h dccn_eq_receive_step_grouped): the query that says where a group of
receiving chains shares one launch sequence, and the argument checks that need no device.  Nothing here launches."""
import ctypes as C
import os

import pytest


class _Flags:
    nfft, nsymbol, nbits, npilot, nguard, nfilter = 64, 7, 2, 8, 8, 64
    cp, longcp, pilot, channel = True, True, "lte", "EPA"


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _shape(batch, longcp=True, nbits=2):
    """the N = 64, S = 7, F = 64 geometry of the equaliser tests (cp on); longcp: CP = 16, else CP = 4"""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.ofdm import ofdm_tx
    F = _Flags()
    F.longcp, F.nbits = longcp, nbits
    tx = ofdm_tx(F)
    assert (tx.K, tx.CP) == (64, 16 if longcp else 4)
    return _lib.EqShape(batch, 7, tx.K, tx.CP, 1, 64, tx.frame_size, nbits, tx.pilot_size, len(tx.pilotCarriers))


@pytest.mark.parametrize("batch", [8, 73, 96])
def test_few_row_batches_are_supported(lib, batch):
    for nbits in (1, 2, 3, 4):
        assert int(lib.dccn_eq_receive_group_supported(C.byref(_shape(batch, nbits=nbits)))) == 1


@pytest.mark.parametrize("batch", [97, 130])
def test_larger_batches_are_not(lib, batch):
    """more than 96 frames leave the few-row plan: the receiver is not folded, the step has launches without a chain index"""
    assert int(lib.dccn_eq_receive_group_supported(C.byref(_shape(batch)))) == 0


def test_short_prefix_is_not(lib):
    """CP = 4: the folded receiver's k extent is S * 2 * (K + CP) = 952, no multiple of 16"""
    sh = _shape(73, longcp=False)
    assert 7 * 2 * (sh.K + sh.CP) == 952
    assert int(lib.dccn_eq_receive_group_supported(C.byref(sh))) == 0


def test_invalid_shape_is_not(lib):
    bad = _shape(73)
    bad.nbits = 5
    assert int(lib.dccn_eq_receive_group_supported(C.byref(bad))) == 0
    zero = _shape(73)
    zero.batch = 0
    assert int(lib.dccn_eq_receive_group_supported(C.byref(zero))) == 0
    assert int(lib.dccn_eq_receive_group_supported(None)) == 0


def test_grouped_call_checks_the_chain_count_and_the_tables(lib):
    """n_chains outside 1..dccn_chain_group_max() and null tables: DCCN_ERR_INVALID_ARG, before any pointer is followed"""
    from dl_ofdm_amd import _lib
    from dl_ofdm_amd.equalizer_group import _ptr_array
    assert int(lib.dccn_chain_group_max()) == 8
    n = 9
    shapes = [_shape(73) for _ in range(n)]
    bufs = [_lib.EqBuffers() for _ in range(n)]
    outs = [_lib.ReceiveOut() for _ in range(n)]
    ps, pb, po = _ptr_array(shapes), _ptr_array(bufs), _ptr_array(outs)
    for k in (0, 9, -1):
        assert lib.dccn_eq_receive_step_grouped(k, ps, pb, po, None) == -1
    assert lib.dccn_eq_receive_step_grouped(2, None, pb, po, None) == -1
    assert lib.dccn_eq_receive_step_grouped(2, ps, None, po, None) == -1
    assert lib.dccn_eq_receive_step_grouped(2, ps, pb, None, None) == -1
    # a table with a null entry, and outputs without `packed`
    hole = (C.c_void_p * 2)(C.addressof(shapes[0]), None)
    assert lib.dccn_eq_receive_step_grouped(2, hole, pb, po, None) == -1
    assert lib.dccn_eq_receive_step_grouped(2, ps, pb, po, None) == -1
