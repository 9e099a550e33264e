"""Which channels the fused generator launch takes (datagen.FusedStaticGen.supported / doppler_plan), decided from a generator's
attributes alone: no device.  The attributes are the ones DeviceDataGen.__init__ derives from the channel profiles."""
import types

import pytest

from dl_ofdm_amd import _lib, radio
from dl_ofdm_amd.datagen import FusedStaticGen


def gen_like(chan, mobile, mix, align_window=False, S=7, K=64, CP=16):
    """the attributes of DeviceDataGen(Flags(channel=chan, align_window=...), mobile=mobile, mix=mix) that the decision reads"""
    chan = chan.lower()
    g = types.SimpleNamespace(lib=_lib.load(), S=S, K=K, CP=CP, align_window=align_window, mix=bool(mix))
    g.mixed = chan in ("mixrayleigh", "mixall")
    g.identity = chan == "awgn"
    alphas = radio._alpha_matrices()
    if g.mixed:
        names = ("flat", "etu", "eva", "epa") if chan == "mixrayleigh" else ("awgn", "flat", "etu", "eva", "epa")
        g.period = 3 if chan == "mixrayleigh" else 4
        g.profiles = []
        for nm in names:
            pr = radio._Profile(nm, bool(mobile), alphas)
            g.profiles.append(dict(identity=(nm == "awgn"), Fd=float(pr.Fd), n_taps=int(pr.n_taps), L=int(pr.alpha.shape[1])))
    prof = radio._Profile("flat" if g.mixed else chan, bool(mobile), alphas)
    g.Fd = float(prof.Fd)
    g.doppler = (not g.identity) and g.Fd > 0.1
    g.n_taps, g.L = int(prof.n_taps), 1 if g.identity else int(prof.alpha.shape[1])
    return g


@pytest.mark.parametrize("chan", ["AWGN", "Flat", "EPA", "EVA", "ETU", "mixRayleigh", "mixAll"])
@pytest.mark.parametrize("mobile", [False, True])
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("align_window", [False, True])
def test_supported_truth_table(chan, mobile, mix, align_window):
    g = gen_like(chan, mobile, mix, align_window)
    assert FusedStaticGen.supported(g) == (not align_window)             # every N = 64 channel, Doppler frames or not
    mixed = chan.startswith("mix")
    want_doppler = mobile and (mix if mixed else chan != "AWGN")
    assert FusedStaticGen.doppler_plan(g) == want_doppler


def test_supported_keeps_its_bounds():
    assert not FusedStaticGen.supported(gen_like("mixRayleigh", True, True, K=128, CP=32))      # the N = 64 grid only
    g = gen_like("mixRayleigh", True, True)
    g.profiles[1]["L"] = 65
    assert not FusedStaticGen.supported(g)
    g = gen_like("mixAll", True, True)
    g.profiles[2]["n_taps"] = 17
    assert not FusedStaticGen.supported(g)
    g = gen_like("mixAll", True, True)
    g.profiles = g.profiles + g.profiles[:2]                             # 7 profiles
    assert not FusedStaticGen.supported(g)


def test_descriptor_mirrors_keep_their_size_and_the_new_fields_sit_in_the_old_padding():
    """the C structs are static_assert'ed to 200 / 32 bytes (csrc/dccn_abi_gen.hip); Fd / doppler_period / t_sym fill the three
    4-byte holes of dccn_gen_static, and a profile's Fd is the old `reserved` int"""
    import ctypes as C
    assert C.sizeof(_lib.GenStatic) == 200 and C.sizeof(_lib.GenProfile) == 32
    assert (_lib.GenStatic.Fd.offset, _lib.GenStatic.doppler_period.offset, _lib.GenStatic.t_sym.offset) == (68, 172, 196)
    assert _lib.GenProfile.Fd.offset == 28
    d = _lib.GenStatic()
    assert d.doppler_period == 0 and d.t_sym == 0.0 and d.Fd == 0.0      # all-zero: the static launch
