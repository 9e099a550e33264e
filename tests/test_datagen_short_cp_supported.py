"""The fused generator launch at the short cyclic prefix (N = 64, CP = round(0.07 * 64) = 4: the ``longcp=False`` half of the
reference driver's grid): which shapes the library says it is instantiated for (dccn_gen_static_supported) and which channels
datagen.FusedStaticGen.supported / doppler_plan take there.  No device."""
import ctypes as C

import pytest

from dl_ofdm_amd import _lib
from dl_ofdm_amd.datagen import FusedStaticGen
from test_datagen_mobile_supported import gen_like


@pytest.mark.parametrize("chan", ["AWGN", "Flat", "EPA", "EVA", "ETU", "mixRayleigh", "mixAll"])
@pytest.mark.parametrize("mobile", [False, True])
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("align_window", [False, True])
def test_supported_truth_table_at_the_short_prefix(chan, mobile, mix, align_window):
    g = gen_like(chan, mobile, mix, align_window, CP=4)
    assert FusedStaticGen.supported(g) == (not align_window)
    mixed = chan.startswith("mix")
    want_doppler = mobile and (mix if mixed else chan != "AWGN")           # as at the long prefix
    assert FusedStaticGen.doppler_plan(g) == want_doppler
    assert FusedStaticGen.doppler_plan(g) == FusedStaticGen.doppler_plan(gen_like(chan, mobile, mix, align_window))


def test_the_library_names_both_prefix_lengths_of_the_n64_grid_and_nothing_else():
    lib = _lib.load()
    for shape in ((7, 64, 4), (7, 64, 16)):
        assert int(lib.dccn_gen_static_supported(*shape)) == 1, shape
    for shape in ((7, 64, 8), (7, 64, 0), (6, 64, 4), (7, 128, 9), (7, 128, 32)):
        assert int(lib.dccn_gen_static_supported(*shape)) == 0, shape


def test_descriptor_mirrors_keep_their_size():
    assert C.sizeof(_lib.GenStatic) == 200 and C.sizeof(_lib.GenProfile) == 32
