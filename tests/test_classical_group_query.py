"""Every refusal ``dccn_classical_receive_grouped`` adds to the solo entry's, and the solo rules applied to one link among good
ones, on a box without a GPU: the pointers are small host buffers that a refused call never follows (as
tests/test_classical_receive_query.py does it), so ``-1`` means the call was judged before any device work.  Then the Python
side's own refusals (``ClassicalReceiveGroup``), which are raised before a device is touched."""
import ctypes as C
import os

import pytest

S, K, CP, P, D, E = 7, 64, 16, 32, 320, 112
FRAMES = 3
STEP = 1 << 20         # bytes between the fake buffers: beyond the largest range of this shape (dft: 64 KB; x: 107 KB)


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


INPUTS = ("dft", "w", "pil", "dat", "empty", "table", "labels", "x")
OUTPUTS = ("packed", "llr", "chest", "y_freq", "noise")


def table(n, nbits=(1, 2, 3, 4, 1, 2, 3, 4), shared_inputs=True):
    """n links that would be accepted: fake 256-byte aligned addresses far apart, never dereferenced.  The inputs are shared by all
    links (``shared_inputs``) or each link's own; the outputs are each link's own."""
    from dl_ofdm_amd import _lib
    t = (_lib.ClassicalLink * max(n, 1))()
    base = 1 << 32
    for i in range(n):
        nb = nbits[i]
        own = base + (1 + i) * 32 * STEP
        ins = {k: (base if shared_inputs else own) + j * STEP for j, k in enumerate(INPUTS)}
        outs = {k: own + (len(INPUTS) + j) * STEP for j, k in enumerate(OUTPUTS)}
        t[i] = _lib.ClassicalLink(nb, 1 << nb, 2, CP, 0.0, 3.0, 3.0, ins["dft"], ins["w"], ins["pil"], ins["dat"], ins["empty"],
                                  ins["table"], ins["labels"], ins["x"], outs["packed"], outs["llr"], outs["chest"], outs["y_freq"],
                                  outs["noise"])
    return t


def call(lib, n, t, frames=FRAMES):
    return lib.dccn_classical_receive_grouped(n, t, frames, S, K, CP, P, D, E, None)


def test_struct_size_matches_the_header():
    from dl_ofdm_amd import _lib
    assert C.sizeof(_lib.ClassicalLink) == 136
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "sizeof(dccn_classical_link) == 136" in open(os.path.join(root, "include", "dccn.h")).read()


def test_the_calls_own_refusals(lib):
    assert call(lib, 0, table(4)) == -1
    assert call(lib, 9, table(8)) == -1                      # (judged by the count alone: the ninth entry is never read)
    assert lib.dccn_chain_group_max() == 8
    assert call(lib, 4, None) == -1
    assert call(lib, 4, table(4), frames=0) == -1
    assert call(lib, 4, table(4), frames=-2) == -1


@pytest.mark.parametrize("bad", [1, 3])
@pytest.mark.parametrize("field,value", [("mode", 1), ("win", CP + 1), ("m", 32), ("packed", None), ("x", "+8"), ("nbits", 5)])
def test_one_bad_link_among_good_ones(lib, bad, field, value):
    t = table(4)
    if isinstance(value, str):
        value = getattr(t[bad], field) + int(value)
    setattr(t[bad], field, value)
    assert call(lib, 4, t) == -1


def test_m_must_be_the_links_own_two_to_the_nbits(lib):
    t = table(4)
    t[0].m, t[1].m = t[1].m, t[0].m                          # each a valid m -- of the other link's modulation
    assert call(lib, 4, t) == -1


@pytest.mark.parametrize("field", ["llr", "chest", "y_freq", "noise"])
def test_an_output_for_some_links_only(lib, field):
    for missing in (0, 2):
        t = table(3)
        setattr(t[missing], field, None)
        assert call(lib, 3, t) == -1


@pytest.mark.parametrize("other", ["chest", "x", "packed", "llr", "dft", "labels"])
def test_an_output_of_one_link_inside_a_range_of_another(lib, other):
    t = table(2, shared_inputs=False)
    t[0].packed = getattr(t[1], other) + 16                  # inside link 1's range (every range here is longer than 16 bytes)
    assert call(lib, 2, t) == -1
    t = table(2, shared_inputs=False)
    t[0].packed = getattr(t[1], other) - 1                   # link 0's rows run into the start of link 1's range
    assert call(lib, 2, t) == -1


def test_the_last_byte_of_a_range_counts(lib):
    """link 0's packed rows (3 frames of 40 bytes: BPSK) end one byte inside link 1's chest.  (A byte earlier they end where chest
    starts and the call passes the plan: not made here, it would launch.)"""
    RB0 = (D * 1 + 7) // 8
    t = table(2, shared_inputs=False)
    t[0].packed = t[1].chest - FRAMES * RB0 + 1
    assert call(lib, 2, t) == -1


def test_shared_inputs_are_not_what_is_refused(lib):
    """Every table above shares ALL inputs between its links (x, dft, w, the lists, the tables) and differs from an accepted call
    in the one field the test names; the accepted calls themselves are made on the GPU (tests/test_gpu_classical_group.py, where
    two links read one x).  Here: with shared inputs an output placed on the SHARED x is still refused -- for link 1 that x is
    another link's input -- so sharing does not switch the collision check off either."""
    t = table(2)
    assert t[0].x == t[1].x and t[0].dft == t[1].dft and t[0].labels == t[1].labels
    t[0].noise = t[1].x + 32
    assert call(lib, 2, t) == -1


def _flags(nbits, **kw):
    from dl_ofdm_amd.receiver import Flags
    return Flags(nbits=nbits, channel="EPA", **kw)


def test_python_mismatched_grids_name_the_field():
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    with pytest.raises(ValueError, match=r"same CP"):
        ClassicalReceiveGroup([_flags(2), _flags(4, longcp=False)], 3, device="cpu")
    with pytest.raises(ValueError, match=r"same K"):
        ClassicalReceiveGroup([_flags(2), _flags(2, nfft=128)], 3, device="cpu")


@pytest.mark.parametrize("kw", [dict(methods=["ALMMSE"]), dict(advances=[0, 1, 2]), dict(noise_vars=[1.0]), dict(interps=[None])])
def test_python_lists_of_the_wrong_length(kw):
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    with pytest.raises(ValueError, match="one entry per link"):
        ClassicalReceiveGroup([_flags(2), _flags(4)], 3, device="cpu", **kw)


def test_python_group_size(lib):
    from dl_ofdm_amd.classical_receive import ClassicalReceiveGroup
    with pytest.raises(ValueError, match=r"1\.\.8 links"):
        ClassicalReceiveGroup([_flags(2)] * 9, 3, device="cpu")
    with pytest.raises(ValueError, match=r"1\.\.8 links"):
        ClassicalReceiveGroup([], 3, device="cpu")


def test_lazy_export():
    from dl_ofdm_amd import classical_receive, receive
    assert receive.ClassicalReceiveGroup is classical_receive.ClassicalReceiveGroup
    assert receive.ClassicalRxReceiver is classical_receive.ClassicalRxReceiver
