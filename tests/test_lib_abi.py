"""The C-ABI library loads on a GPU-less box and exports every symbol include/dccn.h declares
(no compute calls here); host-side argument validation that needs no device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dl_ofdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dccn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dccn_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from dl_ofdm_amd import _lib
    names = header_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libdccn.so does not export %s" % n
    assert sorted(_lib.SIGNATURES) == names, set(names) ^ set(_lib.SIGNATURES)


def test_struct_sizes_match_header(lib):
    from dl_ofdm_amd import _lib
    assert C.sizeof(_lib.Metrics) == 64
    assert C.sizeof(_lib.AdamState) == 16
    assert C.sizeof(_lib.AdamHParams) == 24
    assert C.sizeof(_lib.RxShape) == 24
    # 18 pointers/sizes + x_next + x_prenormalised (padded) + x_norm_next + (norm_slot, keep_dense_grad) + reg_uniform_dense (padded)
    assert C.sizeof(_lib.RxBuffers) == 26 * 8          # ... + x_next_ready + gen_next + tuning
    assert C.sizeof(_lib.GenStatic) == 200             # (static_assert'ed against the C struct in csrc/dccn_abi.hip)
    assert C.sizeof(_lib.GenProfile) == 32
    assert C.sizeof(_lib.CconvPatchPlan) == 16 * 4     # dccn_cconv_patch_plan: sixteen ints



def test_host_side_queries(lib):
    from dl_ofdm_amd import _lib
    assert lib.dccn_version() >= 100
    assert lib.dccn_strerror(0) == b"ok" and b"workspace" in lib.dccn_strerror(-2)
    assert [lib.dccn_tail_param_count(b) for b in (1, 2, 3, 4)] == [16, 40, 90, 200]
    assert lib.dccn_tail_param_count(5) < 0
    sh = _lib.RxShape(1170, 7, 80, 64, 320, 2)
    offs = (C.c_longlong * 6)()
    assert lib.dccn_rx_param_offsets(C.byref(sh), offs) == 0
    assert list(offs) == [0, 10240, 10368, 583808, 584448, 584488]        # 584 488 live params
    assert lib.dccn_rx_workspace_size(C.byref(sh), 1) > lib.dccn_rx_workspace_size(C.byref(sh), 0) > 0
    bad = _lib.RxShape(1170, 7, 80, 64, 320, 5)
    assert lib.dccn_rx_param_offsets(C.byref(bad), offs) == -1
    assert lib.dccn_rx_workspace_size(C.byref(bad), 1) == 0
    # argument validation happens before any device work
    assert lib.dccn_dense_fwd(None, None, None, None, 4, 4, 4, None) == -1
    assert lib.dccn_cconv_gemm_fwd(None, None, None, None, 0, 80, 64, None) == -1


def test_dense_tail_grid_query(lib):
    """dccn_dense_tail_grid against the route worked out by hand from the comments on dense_tail_route (256 CUs): 80x64 tiles
    from ceil(M / 48) * ceil(N / 64) >= 1024 tiles on; there, BPSK / QPSK with 1 <= M % 80 <= 32 rows left over run those
    rows as one row of 32x64 blocks (knob 27); M <= 96 on BPSK / QPSK runs the few-row 16x16 tiles."""
    TILES, FEWROW, RAGGED = 0, 1, 2

    def q(M, K, N, nbits):
        g = [C.c_int(-7) for _ in range(4)]
        st = lib.dccn_dense_tail_grid(M, K, N, nbits, *[C.byref(v) for v in g])
        assert (st == 0) == (lib.dccn_dense_tail_supported(M, K, N, nbits) == 1)
        return st, tuple(v.value for v in g)

    assert q(1170, 896, 640, 2) == (0, (TILES, 48, 0, 250))             # 25 x 10 tiles of 48x64
    # 13 x 125 = 1625 >= 1024; 585 = 7 x 80 + 25: 7 x 125 blocks of 80x64 + 125 of 32x64
    assert q(585, 14336, 8000, 2) == (0, (RAGGED, 80, 25, 1000))
    assert q(585, 14336, 8000, 4) == (0, (TILES, 80, 0, 1000))          # the ragged grid is BPSK / QPSK only: 8 x 125
    default = lib.dccn_get_tuning(27)
    try:
        assert lib.dccn_set_tuning(27, 0) == 0
        assert q(585, 14336, 8000, 2) == (0, (TILES, 80, 0, 1000))
    finally:
        lib.dccn_set_tuning(27, default)
    assert lib.dccn_get_tuning(27) == default == 1
    assert q(4960, 192, 640, 2) == (0, (TILES, 80, 0, 620))             # 104 x 10 = 1040 >= 1024; 62 x 10 blocks
    assert q(4880, 192, 640, 2) == (0, (TILES, 48, 0, 1020))            # 102 x 10 = 1020 < 1024: just below the threshold
    assert q(4961, 192, 640, 2) == (0, (RAGGED, 80, 1, 630))            # 62 x 10 + 10
    assert q(4992, 192, 640, 1) == (0, (RAGGED, 80, 32, 630))
    assert q(4993, 192, 640, 2) == (0, (TILES, 80, 0, 630))             # 33 rows left: 63 x 10 uniform tiles
    assert q(4976, 896, 580, 2) == (0, (RAGGED, 80, 16, 630))           # 10 column tiles, the last of 4 columns
    assert q(4976, 192, 640, 4) == (0, (TILES, 80, 0, 630))
    assert q(36, 896, 640, 2) == (0, (FEWROW, 16, 0, 3 * 40))           # 3 x 40 tiles of 16x16
    assert q(36, 896, 640, 4)[1][:3] == (TILES, 48, 0)                  # few-row tiles carry the tail at BPSK / QPSK only
    # refused exactly where dccn_dense_tail_supported answers 0; the outputs stay as they were
    for bad in ((1170, 898, 640, 2), (1170, 896, 642, 2), (1170, 896, 640, 5), (0, 896, 640, 2)):
        assert q(*bad) == (-1, (-7, -7, -7, -7)), bad
    # the outputs are nullable
    assert lib.dccn_dense_tail_grid(1170, 896, 640, 2, None, None, None, None) == 0


def test_eq_workspace_tensor_lookup(lib):
    """dccn_eq_workspace_tensor: a host-side query (no device work): named intermediates of the fused equaliser step lie
    inside the sized workspace on 256-byte boundaries; unknown names and training-only tensors of an evaluation workspace
    are refused."""
    from dl_ofdm_amd import _lib
    sh = _lib.EqShape(12, 7, 64, 16, 1, 64, 320, 2, 16, 8)
    off, cnt = C.c_size_t(), C.c_size_t()
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, b"y", C.byref(off), C.byref(cnt)) == 0 and cnt.value == 12 * 7 * 128
    total = lib.dccn_eq_workspace_size(C.byref(sh), 1)
    assert off.value % 256 == 0 and off.value + 4 * cnt.value <= total
    seen = set()
    for name in (b"x_norm", b"ln", b"t1", b"d1", b"d2", b"d3", b"d4", b"eq", b"corr", b"cat", b"dz", b"dout", b"deqc", b"dcorc",
                 b"deq", b"dcorr", b"dy", b"dh", b"dd4", b"dd3", b"dd2", b"dflat", b"dt1"):
        assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, name, C.byref(off), C.byref(cnt)) == 0, name
        assert off.value % 256 == 0 and cnt.value > 0 and off.value + 4 * cnt.value <= total and off.value not in seen
        seen.add(off.value)
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 0, b"dh", C.byref(off), C.byref(cnt)) == -1          # training only
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 0, b"y", C.byref(off), C.byref(cnt)) == 0
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, b"nope", C.byref(off), C.byref(cnt)) == -1
    assert lib.dccn_eq_workspace_tensor(C.byref(sh), 1, None, C.byref(off), C.byref(cnt)) == -1


def test_short_workspace_is_refused_before_device_work(lib):
    """Every entry point that takes a workspace, called with otherwise valid arguments and one byte less than its size query
    asks for, answers DCCN_ERR_WORKSPACE (-2) -- before anything touches a device: the pointers are small host buffers that a
    refused call never dereferences (this runs on a box without a GPU).  (dccn_rx_graph_create / dccn_eq_graph_create open a
    stream capture around the same step and need a device for that; the step they capture is the one checked here.)"""
    from dl_ofdm_amd import _lib
    store = (C.c_char * 8192)()
    p = C.c_void_p((C.addressof(store) + 255) // 256 * 256)          # 256-byte aligned, like every device allocation
    hp = _lib.AdamHParams.default()
    got = {}

    def short(name, query, call):
        n = query()
        assert n > 0, name
        got[name] = call(n - 1)

    L = lib
    short("batch_moment_norm_fwd", lambda: L.dccn_batch_moment_norm_workspace_size(36, 1120),
          lambda n: L.dccn_batch_moment_norm_fwd(p, p, p, p, 36, 1120, 1e-9, p, n, None))
    short("clip_power", lambda: L.dccn_clip_power_workspace_size(2240), lambda n: L.dccn_clip_power(p, p, p, 2240, 8.0, p, n, None))
    short("cconv_gemm_bwd_w", lambda: L.dccn_cconv_gemm_bwd_w_workspace_size(511, 80, 64),
          lambda n: L.dccn_cconv_gemm_bwd_w(p, p, p, p, 511, 80, 64, p, n, None))
    for M, K, N in ((73, 896, 896), (300, 896, 640)):
        q = lambda: L.dccn_dense_bwd_w_workspace_size(M, K, N)      # noqa: E731
        short("dense_bwd_w %d" % M, q, lambda n: L.dccn_dense_bwd_w(p, p, p, p, M, K, N, p, n, None))
        short("dense_bwd %d" % M, q, lambda n: L.dccn_dense_bwd(p, p, p, p, p, p, M, K, N, p, n, None))
        short("dense_bwd_slabs %d" % M, q, lambda n: L.dccn_dense_bwd_slabs(p, p, p, p, p, p, M, K, N, p, n, None, None))
    for nb in (2, 4):
        q = lambda: L.dccn_demod_tail_workspace_size(36 * 320, nb)      # noqa: E731
        short("demod_tail_loss_fwd %d" % nb, q, lambda n: L.dccn_demod_tail_loss_fwd(p, p, p, p, p, 36 * 320, nb, p, n, None))
        short("demod_tail_loss_fwd_bwd %d" % nb, q,
              lambda n: L.dccn_demod_tail_loss_fwd_bwd(p, p, p, p, p, p, p, 36 * 320, nb, p, n, None))
        q = lambda: L.dccn_dense_tail_workspace_size(36, 640, nb)      # noqa: E731
        short("dense_tail_fwd %d" % nb, q, lambda n: L.dccn_dense_tail_fwd(p, p, p, p, p, p, p, p, 36, 896, 640, nb, p, n, None))
        short("dense_tail_fwd_bwd %d" % nb, q,
              lambda n: L.dccn_dense_tail_fwd_bwd(p, p, p, p, p, p, p, p, p, p, 36, 896, 640, nb, p, n, None))
    short("rx_backward", lambda: L.dccn_rx_backward_workspace_size(64, 7, 80, 64, 320),
          lambda n: L.dccn_rx_backward(p, p, p, p, p, p, p, p, p, 64, 7, 80, 64, 320, 1, p, n, None))
    for nb in (2, 4):
        sh = _lib.RxShape(36, 7, 80, 64, 320, nb)

        def rx_buffers(n):
            b = _lib.RxBuffers()
            for f in ("x", "bits", "params", "grads", "adam_m", "adam_v", "adam", "x_norm", "fft_out", "z", "prob", "dz", "dfft",
                      "metrics", "workspace"):
                setattr(b, f, p.value)
            b.workspace_bytes = n
            return b
        short("rx_eval_step %d" % nb, lambda: L.dccn_rx_workspace_size(C.byref(sh), 0),
              lambda n: L.dccn_rx_eval_step(C.byref(sh), C.byref(rx_buffers(n)), None))
        short("rx_train_step %d" % nb, lambda: L.dccn_rx_workspace_size(C.byref(sh), 1),
              lambda n: L.dccn_rx_train_step(C.byref(sh), C.byref(rx_buffers(n)), hp, None))
        short("rx_normalise %d" % nb, lambda: L.dccn_rx_workspace_size(C.byref(sh), 1),
              lambda n: L.dccn_rx_normalise(C.byref(sh), C.byref(rx_buffers(n)), None))
        short("rx_receive_step %d" % nb, lambda: L.dccn_rx_receive_workspace_size(C.byref(sh)),
              lambda n: L.dccn_rx_receive_step(C.byref(sh), C.byref(_lib.RxReceiveBuffers(p.value, p.value, p.value, p.value, p.value,
                                                                                         p.value, None, None, p.value, n, None)), None))
    geo = (2, 12, 10, 2, 10, 8, 3, 3, 0, 0, 1, 1, 0, 0, 16)             # B, L, Wd, C, Lo, Wo, ntl, ntw, tl0, tw0, sL, sW, pl0, pw0, F
    short("cconv_patch_bwd_w", lambda: L.dccn_cconv_patch_bwd_w_workspace_size(2, 10, 8, 2, 3, 3, 16),
          lambda n: L.dccn_cconv_patch_bwd_w(p, p, p, p, *geo, p, n, None))
    short("cconv_patch_bwd_x", lambda: L.dccn_cconv_patch_bwd_x_workspace_size(2, 3, 3, 16),
          lambda n: L.dccn_cconv_patch_bwd_x(p, p, p, *geo, p, n, None))
    assert L.dccn_cconv1d_bwd_supported(2, 64, 2, 64, 3, 1, 32) == 1
    short("cconv1d_bwd", lambda: L.dccn_cconv1d_bwd_workspace_size(32),
          lambda n: L.dccn_cconv1d_bwd(p, p, p, p, p, p, 2, 64, 2, 64, 3, 0, 1, 0, 32, p, n, None))
    short("channel_awgn", lambda: L.dccn_channel_awgn_workspace_size(6, 560, 9),
          lambda n: L.dccn_channel_awgn(p, None, p, p, 9, 9, 0, p, None, p, None, 0, p, 6, 560, 1, 0, p, n, None))
    short("channel_doppler_awgn", lambda: L.dccn_channel_doppler_awgn_workspace_size(6, 560, 9, 7),
          lambda n: L.dccn_channel_doppler_awgn(p, None, p, p, 9, 9, 70.0, 7e-5, 7, 80, p, None, p, None, 0, p, 6, 1, 0, p, n, None))
    grp = (_lib.ChannelGroup * 1)(_lib.ChannelGroup(None, 6, p.value, p.value, 9, 9, 0, 70.0))
    short("channel_groups_awgn", lambda: L.dccn_channel_groups_awgn_workspace_size(6, 560, 7),
          lambda n: L.dccn_channel_groups_awgn(p, grp, 1, None, None, 7e-5, 7, 80, p, None, p, None, 0, p, 6, 1, 0, p, n, None))
    cq = L.dccn_classical_workspace_size
    short("classical_gain", cq, lambda n: L.dccn_classical_gain(p, p, p, p, 4, 448, 8, 1.0, 0.0, p, p, n, None))
    short("classical_estimate", cq, lambda n: L.dccn_classical_estimate(p, p, p, 4, 7, 64, 0, 0.0, p, n, None))
    short("classical_detect", cq, lambda n: L.dccn_classical_detect(p, p, p, p, p, p, p, p, 4, 448, 320, 4, 2, 448, 1, p, n, None))
    short("ingraph_awgn", lambda: L.dccn_ingraph_awgn_workspace_size(4, 560),
          lambda n: L.dccn_ingraph_awgn(p, p, p, p, p, p, 4, 560, 8.0, 1, 0, p, n, None))
    short("eq_monitor_accumulate", lambda: L.dccn_eq_monitor_workspace_size(12, 7, 64),
          lambda n: L.dccn_eq_monitor_accumulate(p, p, 0, 12, 7, 64, p, p, p, p, p, p, n, None))
    assert L.dccn_eq_bottleneck_supported(12, 896, 16) == 1
    short("eq_bottleneck_bwd", lambda: L.dccn_eq_bottleneck_workspace_size(12, 896, 16),
          lambda n: L.dccn_eq_bottleneck_bwd(*([p] * 11), 12, 896, 16, p, n, None))
    es = _lib.EqShape(12, 7, 64, 16, 1, 64, 320, 2, 16, 8)

    def eq_buffers(n):
        b = _lib.EqBuffers()
        for f in ("x", "bits", "eq_params", "eq_grads", "adam_m", "adam_v", "adam", "rx_params", "out_eq", "chest", "snr_db",
                  "pilot_carriers", "prob", "metrics", "workspace"):
            setattr(b, f, p.value)
        b.workspace_bytes = n
        return b
    short("eq_eval_step", lambda: L.dccn_eq_workspace_size(C.byref(es), 0),
          lambda n: L.dccn_eq_eval_step(C.byref(es), C.byref(eq_buffers(n)), None))
    short("eq_train_step", lambda: L.dccn_eq_workspace_size(C.byref(es), 1),
          lambda n: L.dccn_eq_train_step(C.byref(es), C.byref(eq_buffers(n)), hp, None))
    short("eq_receive_step", lambda: L.dccn_eq_workspace_size(C.byref(es), 0),
          lambda n: L.dccn_eq_receive_step(C.byref(es), C.byref(eq_buffers(n)), C.byref(_lib.ReceiveOut(p.value, None, None)), None))
    assert len(got) == 41 and all(v == -2 for v in got.values()), {k: v for k, v in got.items() if v != -2}


def test_fused_dense_forward_refuses_operands_that_are_not_vector_legal(lib):
    """The fused dense forward (+ tail, + decision) runs on tiles without scalar loaders: x or w one float off a 16-byte
    boundary, or a K that is no multiple of 4, is answered DCCN_ERR_INVALID_ARG (-1) before anything touches a device (host
    buffers that a refused call never dereferences), and dccn_dense_tail_supported says the same of the shape.  The same
    arguments with aligned operands pass the argument checks: with a workspace one byte short they get as far as
    DCCN_ERR_WORKSPACE (-2)."""
    store = (C.c_char * 8192)()
    a = (C.addressof(store) + 255) // 256 * 256
    p = C.c_void_p(a)
    L = lib
    M, K, N, nb = 36, 128, 64, 2
    n = L.dccn_dense_tail_workspace_size(M, N, nb)
    assert n > 0 and L.dccn_dense_tail_supported(M, K, N, nb) == 1 and L.dccn_dense_decide_supported(M, K, N, nb) == 1

    def tails(x, w, k, nbytes):
        return {"dense_tail_fwd": L.dccn_dense_tail_fwd(x, w, p, p, p, p, p, p, M, k, N, nb, p, nbytes, None),
                "dense_tail_fwd_bwd": L.dccn_dense_tail_fwd_bwd(x, w, p, p, p, p, p, p, p, p, M, k, N, nb, p, nbytes, None)}

    # (aligned operands: only the two calls that a short workspace stops -- dccn_dense_decide_fwd takes none and would launch)
    got = tails(p, p, K, n - 1)
    assert all(v == -2 for v in got.values()), got
    off = C.c_void_p(a + 4)                                        # 4-byte aligned, not 16
    for what, x, w, k in (("x off by one float", off, p, K), ("w off by one float", p, off, K), ("K = 130", p, p, 130)):
        got = tails(x, w, k, n)
        got["dense_decide_fwd"] = L.dccn_dense_decide_fwd(x, w, p, p, p, p, p, p, M, k, N, nb, None)
        assert all(v == -1 for v in got.values()), (what, got)
    assert L.dccn_dense_tail_supported(M, 130, N, nb) == 0


def test_fused_backward_is_not_offered_where_dz_outgrows_the_fast_loaders(lib):
    """The one-launch backward reads dz [batch, 2 D] through loaders with 32-bit byte offsets.  A short (S x 2 F = 64), very wide
    dense layer under a long batch passes every tile-count test of the plan while dz is 2 GiB or more: the plan must not
    offer the launch there (the step then takes the composed backward), and dccn_rx_backward refuses before any launch.  One
    row less of D and dz fits: offered."""
    from dl_ofdm_amd import _lib
    wide = _lib.RxShape(65408, 1, 64, 32, 32704, 2)                 # dz: 65408 x 65408 floats = 16 GiB
    assert 4 * wide.batch * 2 * wide.D >= 2 ** 31
    assert lib.dccn_rx_bwd_fused_supported(C.byref(wide)) == 0
    store = (C.c_char * 1024)()
    p = C.c_void_p((C.addressof(store) + 255) // 256 * 256)
    assert lib.dccn_rx_backward(p, p, p, p, p, p, p, p, p, 65408, 1, 64, 32, 32704, 1, p, 1 << 40, None) == -1
    fits = _lib.RxShape(8192, 1, 64, 32, 32704, 2)                  # the same layer, dz just under 2 GiB
    assert 4 * fits.batch * 2 * fits.D < 2 ** 31
    assert lib.dccn_rx_bwd_fused_supported(C.byref(fits)) == 1


def test_ops_refuse_cpu_tensors():
    import torch
    from dl_ofdm_amd import _lib, ops
    with pytest.raises(_lib.DccnError):
        ops.batch_moment_norm(torch.zeros(4, 7, 80, 2))
    with pytest.raises(_lib.DccnError):
        ops.dense(torch.zeros(4, 8), torch.zeros(8, 8), None)
    from dl_ofdm_amd.engine import RxDims, RxEngine
    with pytest.raises(_lib.DccnError):
        RxEngine(RxDims(7, 80, 64, 320, 2), 4, device="cpu")


def test_bench_reports_traffic_only_for_the_build_it_was_measured_on(tmp_path):
    """bench.traffic_for: the PMC counters kept in profiles/pmc_traffic.json are stamped with the id of the library they were
    collected on (dccn_build_id); for any other build the bench line carries null + traffic_stale instead of an old number."""
    import json
    import sys
    ROOT_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if ROOT_ not in sys.path:
        sys.path.insert(0, ROOT_)
    import bench
    from dl_ofdm_amd import _lib
    bid = _lib.load().dccn_build_id().decode()
    assert len(bid) == 16 and int(bid, 16) >= 0
    f = tmp_path / "pmc_traffic.json"
    f.write_text(json.dumps({"c2": {"rx_backward": 7.0e7}, "build_id": bid}))
    assert bench.traffic_for(str(f), "c2", "rx_backward", bid) == (7.0e7, False, bid)
    f.write_text(json.dumps({"c2": {"rx_backward": 7.0e7}, "build_id": "0123456789abcdef"}))
    assert bench.traffic_for(str(f), "c2", "rx_backward", bid) == (None, True, "0123456789abcdef")
    f.write_text(json.dumps({"c2": {"rx_backward": 7.0e7}}))                      # a file from before the stamp existed
    assert bench.traffic_for(str(f), "c2", "rx_backward", bid) == (None, True, None)
    assert bench.traffic_for(str(tmp_path / "missing.json"), "c2", "rx_backward", bid) == (None, False, None)
