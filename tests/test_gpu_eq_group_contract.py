"""The layout contract of a chain group (include/dccn.h "chain groups"), field by field: every device pointer of chain g lies at ONE
byte offset from chain 0's.  The arenas of the Python callers always have one layout, so the bit-for-bit group tests
(test_gpu_chain_groups.py, test_gpu_group_receive.py) cannot see a pointer field that a grouped entry point forgot to check.  Here
three chains of one shape and one arena layout are built; every call names two chains -- chain 0 and a COPY of chain 1's structs in
which exactly one pointer field is chain 2's pointer for that field (a valid buffer of the right size at the wrong offset), or NULL
where the field is nullable -- and must return DCCN_ERR_INVALID_ARG having launched nothing: after a synchronise every chain's
arena (parameters, Adam slots, gradients, workspaces, out_eq, chest, metrics, packed / llr / prob: all of a chain's device memory)
is bit for bit what it was.  Every pointer any call carries is a live device buffer of the chain it names, so even a call that were
wrongly accepted stays inside valid memory.

The field lists come from the ctypes mirrors of the structs (dl_ofdm_amd/_lib.py, held to the header by test_lib_abi.py), not from
the lists in csrc/dccn_abi_eq.hip.  A field that is NULL in the callers' layout (dccn_gen_static.tx_out, dccn_eq_monitor.rms_out) is
given a spare buffer at one arena offset in every chain first."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -6
B_TRAIN, B_RECEIVE = 73, 8
# host pointers (followed on the host, not part of the arena) and what a training group refuses outright
HOST_FIELDS = {"EqBuffers": ("x_next_virtual", "tuning", "monitor"), "GenStatic": ("profiles",)}
# the fields of dccn_eq_buffers a forward-only step uses (include/dccn.h dccn_eq_receive_step_grouped)
FORWARD_FIELDS = ("x", "eq_params", "rx_params", "rx_folded", "out_eq", "chest", "snr_db", "pilot_carriers", "workspace")
NORM_FIELDS = ("y", "noise", "power_partial", "noise_partial", "noise_power_out")      # read from x_next_virtual by the normalisation
NULL_IN_LAYOUT = {"GenStatic": {"tx_out"}, "EqMonitor": {"rms_out"}, "EqBuffers": set(), "ReceiveOut": set(), "GenProfile": set()}


def _pointer_fields(struct):
    skip = HOST_FIELDS.get(struct.__name__, ())
    return [f for f, t in struct._fields_ if t is C.c_void_p and f not in skip]


def _copy(s):
    return type(s).from_buffer_copy(s)


def _ptrs(structs):
    from dl_ofdm_amd.equalizer_group import _ptr_array
    return _ptr_array(structs)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Untouched:
    """every chain's whole arena, before; check(): still the same bytes"""

    def __init__(self, chains):
        torch.cuda.synchronize()
        self.chains = chains
        self.before = [c.arena.buf.clone() for c in chains]

    def check(self, what):
        torch.cuda.synchronize()
        for i, (c, b) in enumerate(zip(self.chains, self.before)):
            assert torch.equal(c.arena.buf, b), "chain %d's arena changed: %s" % (i, what)


def _fill_null_fields(structs, spares):
    """fields NULL in every chain get the chains' spare buffers (one arena offset); returns their names"""
    names = []
    for f in _pointer_fields(type(structs[0])):
        if all(not getattr(s, f) for s in structs):
            for s, sp in zip(structs, spares):
                setattr(s, f, sp.data_ptr())
            names.append(f)
    assert set(names) <= NULL_IN_LAYOUT[type(structs[0]).__name__], names
    return names


def _one_field_cases(structs, fields=None):
    """(field, chain 2's pointer): one wrong-offset case per pointer field of the chains' structs"""
    out = []
    for f in fields or _pointer_fields(type(structs[0])):
        p = [getattr(s, f) for s in structs]
        assert all(p) and len(set(p)) == 3, (type(structs[0]).__name__, f, p)
        out.append((f, p[2]))
    return out


def _refused(call, obj, field, value, want, seen, failures, what):
    """obj.field = value for one call; the status must be `want` and nothing may have been written"""
    keep = getattr(obj, field)
    setattr(obj, field, value)
    try:
        rc = call()
    finally:
        setattr(obj, field, keep)
    if rc != want:
        failures.append("%s: status %d, expected %d" % (what, rc, want))
    seen.check(what)


# ---- the training side: a three-chain training group, one real step taken --------------------------------------------------------
def _train_flags(nbits, tmp, i):
    from dl_ofdm_amd import receiver_mp as H
    return H.Flags(nbits=nbits, nfilter=64, channel="mixRayleigh", device_data=True, seed=10 + 7 * i + nbits, max_epoch_num=1,
                   early_stop=200, msg_length=7 * B_TRAIN * 3, eval_frames=128, token="ctr%d_%d" % (i, nbits),
                   save_dir=os.path.join(str(tmp), "ck%d/" % i))


def _rx(F, seed):
    from dl_ofdm_amd import ofdm, receiver as R
    from dl_ofdm_amd.engine import glorot_init
    return glorot_init(R.rx_dims(F, ofdm.ofdm_tx(F)), seed)


class _TrainGroup:
    """three chains after the first step of an epoch, so every buffer holds real data, and private copies of what the group's
    SECOND step takes for them: plan 1 continuing the pipeline (x_prenormalised, x_next, x_next_virtual armed for the third batch
    with gen_next_rides, the monitors); for the generator entry points the descriptor of the first batch"""

    def __init__(self, tmp):
        from dl_ofdm_amd.equalizer_group import EqualizerChainGroup
        fl = [_train_flags(nb, tmp, i) for i, nb in enumerate((2, 4, 2))]
        self.grp = grp = EqualizerChainGroup(fl, [_rx(F, 3 + i) for i, F in enumerate(fl)])
        self.lib, self.hp, self.chains = grp.lib, grp.hp, grp.chains
        for c in self.chains:
            c.begin_epoch()
        grp.step(self.chains, 0)
        for c in self.chains:                   # (what EqualizerChainGroup.step does ahead of step 1)
            lp = c.loop
            lp.fg.arm(lp.pls[0].bits, 0, None, lp.H[0], lp.snr_rows[2], into=lp.virt[1])
        o = self.chains[0].o
        self.spares = [c.arena.zeros(B_TRAIN * 7 * (o.K + o.CP) * 2) for c in self.chains]
        self.shapes, self.bufs, self.virt, self.prof, self.mon, self.desc, self.dprof = [], [], [], [], [], [], []
        for c in self.chains:
            lp, pl = c.loop, c.loop.pls[1]
            assert pl.batch == B_TRAIN and c.steps == 3 and lp.ride_gen and lp.mon is not None
            b, m = _copy(pl.pipe_buffers[1]), _copy(lp.mon[1])
            v, pr = self._descriptor(lp.virt[1])
            d, dpr = self._descriptor(lp.fg.desc)
            b.x_next_virtual, b.monitor = C.addressof(v), C.addressof(m)
            assert b.gen_next_rides == 1 and b.x_prenormalised == 1 and b.x_next and not b.prob
            self.shapes.append(pl.shape)
            for lst, s in ((self.bufs, b), (self.virt, v), (self.prof, pr), (self.mon, m), (self.desc, d), (self.dprof, dpr)):
                lst.append(s)
        self.x_out = [c.loop.pls[0].x.data_ptr() for c in self.chains]
        self.npow = [c.loop.fg.npow[0].data_ptr() for c in self.chains]
        for structs in (self.virt, self.mon, self.desc):
            _fill_null_fields(structs, self.spares)
        self.seen = _Untouched(self.chains)

    @staticmethod
    def _descriptor(src):
        from dl_ofdm_amd import _lib
        v = _copy(src)
        assert v.n_profiles > 0 and v.bits_out and v.H_out
        pr = (_lib.GenProfile * v.n_profiles).from_buffer_copy((_lib.GenProfile * v.n_profiles).from_address(v.profiles))
        v.profiles = C.addressof(pr)
        return v, pr

    def step(self, shapes=None, bufs=None):
        return self.lib.dccn_eq_train_step_grouped(2, _ptrs((shapes or self.shapes)[:2]), _ptrs((bufs or self.bufs)[:2]), self.hp, _stream())

    def monitors(self):
        return self.lib.dccn_eq_monitor_accumulate_grouped(2, _ptrs(self.mon[:2]), _stream())

    def frames(self):
        return self.lib.dccn_gen_static_frames_grouped(2, _ptrs(self.desc[:2]), _stream())

    def apply(self, x_out=None, npow=None, no_npow=False):
        x = (C.c_void_p * 2)(*(x_out or self.x_out)[:2])
        n = None if no_npow else (C.c_void_p * 2)(*(npow or self.npow)[:2])
        return self.lib.dccn_gen_static_apply_grouped(2, _ptrs(self.desc[:2]), x, n, _stream())


@pytest.fixture(scope="module")
def train(tmp_path_factory):
    return _TrainGroup(tmp_path_factory.mktemp("contract"))


def test_training_group_holds_every_buffer_field_to_the_contract(train):
    t, failures = train, []
    cases = _one_field_cases(t.bufs, [f for f in _pointer_fields(type(t.bufs[0])) if f != "prob"])
    assert len(cases) == 18
    for f, p in cases:
        _refused(t.step, t.bufs[1], f, p, INVALID_ARG, t.seen, failures, "dccn_eq_buffers.%s of chain 1 at chain 2's offset" % f)
    for f in ("snr_db", "tx_power", "reg_coef", "x_next", "monitor"):
        _refused(t.step, t.bufs[1], f, None, INVALID_ARG, t.seen, failures, "dccn_eq_buffers.%s NULL in chain 1 only" % f)
    assert not failures, failures


def test_training_group_holds_the_nested_monitor_to_the_contract(train):
    t, failures = train, []
    cases = _one_field_cases(t.mon)
    assert len(cases) == 8
    for f, p in cases:
        _refused(t.step, t.mon[1], f, p, INVALID_ARG, t.seen, failures, "monitor.%s of chain 1 at chain 2's offset" % f)
    for f in ("tx_power", "noise_power"):
        _refused(t.step, t.mon[1], f, None, INVALID_ARG, t.seen, failures, "monitor.%s NULL in chain 1 only" % f)
    assert not failures, failures


def test_training_group_holds_the_next_batch_descriptor_to_the_contract(train):
    """gen_next_rides = 1: the step arms and runs the generator, every pointer of the descriptor counts (one profile's tables
    among them); gen_next_rides = 0: the caller's launch filled it, the step reads the five fields of the normalisation"""
    t, failures = train, []
    cases = _one_field_cases(t.virt)
    assert len(cases) == 14 and set(NORM_FIELDS) <= {f for f, _ in cases}
    for f, p in cases:
        _refused(t.step, t.virt[1], f, p, INVALID_ARG, t.seen, failures, "armed x_next_virtual.%s of chain 1 at chain 2's offset" % f)
    for f, p in _one_field_cases([pr[0] for pr in t.prof]):
        _refused(t.step, t.prof[1][0], f, p, INVALID_ARG, t.seen, failures, "armed x_next_virtual.profiles[0].%s at chain 2's offset" % f)
    _refused(t.step, t.virt[1], "noise_partial", None, INVALID_ARG, t.seen, failures, "x_next_virtual.noise_partial NULL in chain 1 only")
    for b in t.bufs:
        b.gen_next_rides = 0
    try:
        for f, p in cases:
            if f in NORM_FIELDS:
                _refused(t.step, t.virt[1], f, p, INVALID_ARG, t.seen, failures, "x_next_virtual.%s of chain 1 at chain 2's offset" % f)
    finally:
        for b in t.bufs:
            b.gen_next_rides = 1
    assert not failures, failures


def test_training_group_status_codes(train):
    """rx_folded missing in every chain: the group has a launch that cannot carry chains (DCCN_ERR_UNSUPPORTED); a shape of
    another batch: DCCN_ERR_INVALID_ARG"""
    from dl_ofdm_amd import _lib
    t = train
    nofold = [_copy(b) for b in t.bufs]
    for b in nofold:
        b.rx_folded = None
    assert t.step(bufs=nofold) == UNSUPPORTED
    t.seen.check("rx_folded NULL in every chain")
    other = _lib.EqShape.from_buffer_copy(t.shapes[1])
    other.batch = 64
    assert t.step(shapes=[t.shapes[0], other]) == INVALID_ARG
    t.seen.check("a shape of another batch")


def test_monitor_group_holds_every_field_to_the_contract(train):
    t, failures = train, []
    for f, p in _one_field_cases(t.mon):
        _refused(t.monitors, t.mon[1], f, p, INVALID_ARG, t.seen, failures, "dccn_eq_monitor.%s of chain 1 at chain 2's offset" % f)
    for f in ("tx_power", "noise_power"):
        _refused(t.monitors, t.mon[1], f, None, INVALID_ARG, t.seen, failures, "dccn_eq_monitor.%s NULL in chain 1 only" % f)
    assert not failures, failures


def test_generator_groups_hold_every_field_to_the_contract(train):
    t, failures = train, []
    cases = _one_field_cases(t.desc)
    assert len(cases) == 14
    for name, call in (("frames", t.frames), ("apply", t.apply)):
        for f, p in cases:
            _refused(call, t.desc[1], f, p, INVALID_ARG, t.seen, failures, "%s: dccn_gen_static.%s of chain 1 at chain 2's offset" % (name, f))
        for f, p in _one_field_cases([pr[0] for pr in t.dprof]):
            _refused(call, t.dprof[1][0], f, p, INVALID_ARG, t.seen, failures, "%s: profiles[0].%s at chain 2's offset" % (name, f))
    swapped = lambda v: [v[0], v[2]]          # noqa: E731
    for what, kw in (("x_out at chain 2's offset", dict(x_out=swapped(t.x_out))), ("noise_power at chain 2's offset", dict(npow=swapped(t.npow))),
                     ("noise_power NULL in chain 1 only", dict(npow=[t.npow[0], None]))):
        rc = t.apply(**kw)
        if rc != INVALID_ARG:
            failures.append("apply: %s: status %d" % (what, rc))
        t.seen.check(what)
    assert not failures, failures


def test_the_unbroken_training_tables_are_accepted(train):
    """the copies every case above starts from are a valid group: generator, materialised input, step, monitors"""
    t = train
    assert t.frames() == 0 and t.apply() == 0 and t.apply(no_npow=True) == 0
    assert t.step() == 0 and t.monitors() == 0
    t.seen = _Untouched(t.chains)


# ---- the receive side ------------------------------------------------------------------------------------------------------------------
class _ReceiveGroup:
    def __init__(self, tmp):
        import numpy as np
        from dl_ofdm_amd import receiver_mp as H
        from dl_ofdm_amd.equalizer_group import ChainReceiveGroup
        fl = [H.Flags(nbits=nb, nfilter=64, channel="mixRayleigh", seed=10 + nb + i, token="crx%d" % i, save_dir=os.path.join(str(tmp), "r%d/" % i))
              for i, nb in enumerate((2, 4, 1))]
        self.grp = grp = ChainReceiveGroup(fl, [_rx(F, 5 + i) for i, F in enumerate(fl)], B_RECEIVE, want_llr=True, want_prob=True)
        self.lib, self.chains = grp.lib, grp.chains
        rng = np.random.RandomState(7)
        grp.receive([(rng.standard_normal((B_RECEIVE, 7, 80, 2)) * 2).astype(np.float32) for _ in fl])
        self.shapes = [c.pl.shape for c in self.chains]
        self.bufs = [_copy(c.pl.buffers) for c in self.chains]
        self.outs = [c.out(True, True) for c in self.chains]
        self.seen = _Untouched(self.chains)

    def step(self, shapes=None, bufs=None):
        return self.lib.dccn_eq_receive_step_grouped(2, _ptrs((shapes or self.shapes)[:2]), _ptrs((bufs or self.bufs)[:2]),
                                                     _ptrs(self.outs[:2]), _stream())


@pytest.fixture(scope="module")
def receive(tmp_path_factory):
    return _ReceiveGroup(tmp_path_factory.mktemp("contract_rx"))


def test_receive_group_holds_buffers_and_outputs_to_the_contract(receive):
    r, failures = receive, []
    for f, p in _one_field_cases(r.bufs, FORWARD_FIELDS):
        _refused(r.step, r.bufs[1], f, p, INVALID_ARG, r.seen, failures, "dccn_eq_buffers.%s of chain 1 at chain 2's offset" % f)
    cases = _one_field_cases(r.outs)
    assert [f for f, _ in cases] == ["packed", "llr", "prob"]
    for f, p in cases:
        _refused(r.step, r.outs[1], f, p, INVALID_ARG, r.seen, failures, "dccn_receive_out.%s of chain 1 at chain 2's offset" % f)
    _refused(r.step, r.bufs[1], "snr_db", None, INVALID_ARG, r.seen, failures, "dccn_eq_buffers.snr_db NULL in chain 1 only")
    for f in ("llr", "prob"):
        _refused(r.step, r.outs[1], f, None, INVALID_ARG, r.seen, failures, "dccn_receive_out.%s NULL in chain 1 only" % f)
    assert not failures, failures


def test_receive_group_status_codes(receive):
    """rx_folded missing in every chain is an argument error here (DCCN_ERR_INVALID_ARG), as is a shape of another batch"""
    from dl_ofdm_amd import _lib
    r = receive
    nofold = [_copy(b) for b in r.bufs]
    for b in nofold:
        b.rx_folded = None
    assert r.step(bufs=nofold) == INVALID_ARG
    r.seen.check("rx_folded NULL in every chain")
    other = _lib.EqShape.from_buffer_copy(r.shapes[1])
    other.batch = 7
    assert r.step(shapes=[r.shapes[0], other]) == INVALID_ARG
    r.seen.check("a shape of another batch")
    assert r.step() == 0                    # ... and the same tables, unbroken, are accepted
    r.seen = _Untouched(r.chains)
