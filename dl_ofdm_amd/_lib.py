"""ctypes binding of libdccn.so (include/dccn.h).

The library is the product: every op of this package calls it, and there is NO CPU or
PyTorch fallback -- a missing library or a missing GPU raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCCN_LIB_PATH") or os.path.join(_HERE, "lib", "libdccn.so")     # override: kernel experiments


class DccnError(RuntimeError):
    pass


class Metrics(C.Structure):
    """dccn_metrics"""
    _fields_ = [("ce_sum", c_double), ("conf", c_longlong * 4), ("count", c_longlong),
                ("ce_mean", c_float), ("berlin", c_float), ("log_ber", c_float), ("reserved", c_float)]


class AdamState(C.Structure):
    """dccn_adam_state"""
    _fields_ = [("global_step", c_float), ("beta1_power", c_float), ("beta2_power", c_float), ("alpha", c_float)]


class AdamHParams(C.Structure):
    """dccn_adam_hparams (ofdmreceiver_np.py:185-189 defaults)"""
    _fields_ = [("lr0", c_float), ("decay_steps", c_float), ("decay_rate", c_float),
                ("beta1", c_float), ("beta2", c_float), ("eps", c_float)]

    @classmethod
    def default(cls, lr0: float = 1e-3):
        return cls(lr0, 500.0, 0.98, 0.9, 0.999, 1e-8)


class RxShape(C.Structure):
    """dccn_rx_shape"""
    _fields_ = [("batch", c_int), ("S", c_int), ("kin", c_int), ("F", c_int), ("D", c_int), ("nbits", c_int)]


class GemmRoute(C.Structure):
    """dccn_gemm_route: what dccn_gemm_route_query reports (ops and families: the DCCN_ROUTE_* / DCCN_FAMILY_* ids of dccn.h)"""
    _fields_ = [("family", c_int), ("variant", c_int), ("tile_rows", c_int), ("tile_cols", c_int), ("tile_k", c_int),
                ("w_tile_rows", c_int), ("w_tile_cols", c_int), ("splits", c_int), ("klen", c_int), ("nranges", c_int),
                ("koff", c_int * 9), ("stage", c_int)]


ROUTE_OPS = dict(dense_fwd=0, dense_bwd_x=1, dense_bwd_w=2, dense_bwd=3, cconv_fwd=4, cconv_bwd_w=5, rx_backward=6)
ROUTE_FAMILIES = dict(generic=0, gemm16=1, skinny=2, fewrow=3, kmajor=4, staged=5, grouped_big=6, grouped_kmajor=7, grouped=8,
                      two_launch=9, rx_fused=10)


class CconvPatchPlan(C.Structure):
    """dccn_cconv_patch_plan: what dccn_cconv_patch_plan_query reports (ops and kernels: the DCCN_PATCH_* ids of dccn.h)"""
    _fields_ = [("kernel", c_int), ("tile_rows", c_int), ("tile_cols", c_int), ("tile_k", c_int), ("splits", c_int),
                ("klen", c_int), ("col_tiles", c_int), ("depth", c_int), ("bt_lds", c_int), ("taps_fastest", c_int),
                ("phases", c_int), ("tiles", c_int), ("positions", c_int), ("chunks", c_int), ("items", c_int), ("grid", c_int)]


PATCH_OPS = dict(fwd=0, bwd_w=1, bwd_x=2, bwd_1d=3)
PATCH_KERNELS = dict(gemm=0, kmajor=1, dx_narrow=2, conv1d_fused=3)


class RxBuffers(C.Structure):
    """dccn_rx_buffers"""
    _fields_ = [("x", c_void_p), ("bits", c_void_p), ("params", c_void_p), ("grads", c_void_p),
                ("adam_m", c_void_p), ("adam_v", c_void_p), ("reg_coef", c_void_p), ("adam", c_void_p),
                ("x_norm", c_void_p), ("fft_out", c_void_p), ("z", c_void_p), ("prob", c_void_p),
                ("dz", c_void_p), ("dfft", c_void_p), ("metrics", c_void_p), ("tx_power", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("x_next", c_void_p), ("x_prenormalised", c_int), ("x_norm_next", c_void_p), ("norm_slot", c_int),
                ("keep_dense_grad", c_int), ("reg_uniform_dense", c_int), ("x_next_ready", c_void_p),
                ("gen_next", c_void_p), ("tuning", c_void_p)]


class RxReceiveBuffers(C.Structure):
    """dccn_rx_receive_buffers"""
    _fields_ = [("x", c_void_p), ("params", c_void_p), ("x_norm", c_void_p), ("fft_out", c_void_p), ("z", c_void_p),
                ("packed", c_void_p), ("llr", c_void_p), ("prob", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("tuning", c_void_p)]


class ReceiveOut(C.Structure):
    """dccn_receive_out"""
    _fields_ = [("packed", c_void_p), ("llr", c_void_p), ("prob", c_void_p)]


class GenStatic(C.Structure):
    """dccn_gen_static"""
    _fields_ = [("bits_out", c_void_p), ("cell_map", c_void_p), ("const_tab", c_void_p), ("pilot_re", c_float),
                ("pilot_im", c_float), ("idft", c_void_p), ("coeff", c_void_p), ("alpha", c_void_p), ("n_taps", c_int),
                ("L", c_int), ("identity", c_int), ("Fd", c_float), ("snr_db", c_void_p), ("y", c_void_p), ("noise", c_void_p),
                ("power_partial", c_void_p), ("noise_partial", c_void_p), ("noise_power_out", c_void_p), ("tx_out", c_void_p),
                ("frames", c_int), ("S", c_int), ("K", c_int), ("CP", c_int), ("D", c_int), ("nbits", c_int),
                ("seed", C.c_ulonglong), ("offset", C.c_uint),
                ("n_profiles", c_int), ("tap_stride", c_int), ("doppler_period", c_int), ("profiles", c_void_p),
                ("H_out", c_void_p), ("h_rep", c_int), ("t_sym", c_float)]


class GenProfile(C.Structure):
    """dccn_gen_profile"""
    _fields_ = [("coeff", c_void_p), ("alpha", c_void_p), ("n_taps", c_int), ("L", c_int), ("identity", c_int),
                ("Fd", c_float)]


class EqShape(C.Structure):
    """dccn_eq_shape"""
    _fields_ = [("batch", c_int), ("S", c_int), ("K", c_int), ("CP", c_int), ("cp", c_int), ("F", c_int),
                ("D", c_int), ("nbits", c_int), ("pilot_size", c_int), ("P", c_int)]


class EqBuffers(C.Structure):
    """dccn_eq_buffers"""
    _fields_ = [("x", c_void_p), ("bits", c_void_p), ("eq_params", c_void_p), ("eq_grads", c_void_p),
                ("adam_m", c_void_p), ("adam_v", c_void_p), ("reg_coef", c_void_p), ("adam", c_void_p),
                ("rx_params", c_void_p), ("out_eq", c_void_p), ("chest", c_void_p), ("snr_db", c_void_p),
                ("pilot_carriers", c_void_p), ("prob", c_void_p), ("metrics", c_void_p), ("tx_power", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("reg_uniform", c_int), ("rx_folded", c_void_p),
                ("x_next", c_void_p), ("x_prenormalised", c_int), ("norm_slot", c_int), ("x_next_virtual", c_void_p),
                ("tuning", c_void_p), ("gen_next_rides", c_int), ("monitor", c_void_p)]


class EqMonitor(C.Structure):
    """dccn_eq_monitor"""
    _fields_ = [("chest", c_void_p), ("chan", c_void_p), ("chan_per_symbol", c_int), ("B", c_int), ("S", c_int), ("K", c_int),
                ("metrics", c_void_p), ("tx_power", c_void_p), ("noise_power", c_void_p), ("acc5", c_void_p),
                ("rms_out", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


class ChannelGroup(C.Structure):
    """dccn_channel_group"""
    _fields_ = [("frames", c_void_p), ("n_frames", c_int), ("coeff", c_void_p), ("alpha", c_void_p),
                ("n_taps", c_int), ("L", c_int), ("identity", c_int), ("Fd", c_float)]


class FrameLink(C.Structure):
    """dccn_frame_link"""
    _fields_ = [("x", c_void_p), ("x_out", c_void_p), ("offset", c_void_p), ("cfo", c_void_p), ("metric", c_void_p)]


class CaptureLink(C.Structure):
    """dccn_capture_link"""
    _fields_ = [("cap", c_void_p), ("n_samples", c_longlong), ("first", c_longlong), ("first_dev", c_void_p), ("lo", c_longlong),
                ("stride", c_longlong), ("x_out", c_void_p), ("offset", c_void_p), ("cfo", c_void_p), ("metric", c_void_p)]


class AcquireLink(C.Structure):
    """dccn_acquire_link"""
    _fields_ = [("cap", c_void_p), ("n_samples", c_longlong), ("lo", c_longlong), ("pilot_sc", c_void_p), ("first_out", c_void_p),
                ("cfo_out", c_void_p), ("sym_metric", c_void_p), ("phase_metric", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t)]


class PooledLink(C.Structure):
    """dccn_pooled_link"""
    _fields_ = CaptureLink._fields_ + [("workspace", c_void_p), ("workspace_bytes", c_size_t)]


class ClassicalReceiveArgs(C.Structure):
    """dccn_classical_receive_args"""
    _fields_ = [(n, c_int) for n in ("frames", "S", "K", "CP", "P", "D", "E", "nbits", "m", "win", "mode")] + \
               [(n, c_float) for n in ("noise_var", "pv_re", "pv_im")] + \
               [(n, c_void_p) for n in ("dft", "w", "pil", "dat", "empty", "table", "labels", "x", "packed", "llr", "chest",
                                        "y_freq", "noise")]


class ClassicalLink(C.Structure):
    """dccn_classical_link"""
    _fields_ = [(n, c_int) for n in ("nbits", "m", "mode", "win")] + \
               [(n, c_float) for n in ("noise_var", "pv_re", "pv_im")] + \
               [(n, c_void_p) for n in ("dft", "w", "pil", "dat", "empty", "table", "labels", "x", "packed", "llr", "chest",
                                        "y_freq", "noise")]


METRICS_BYTES = C.sizeof(Metrics)
ADAM_STATE_BYTES = C.sizeof(AdamState)

_vp, _i, _ll, _f, _sz = c_void_p, c_int, c_longlong, c_float, c_size_t

# name -> (restype, argtypes); must list every symbol include/dccn.h declares
SIGNATURES = {
    "dccn_strerror": (c_char_p, [_i]),
    "dccn_version": (_i, []),
    "dccn_build_id": (c_char_p, []),
    "dccn_last_hip_error": (_i, []),
    "dccn_device_info": (_i, [POINTER(c_int), POINTER(c_int), POINTER(c_size_t), c_char_p, _i]),
    "dccn_batch_moment_norm_workspace_size": (_sz, [_i, _i]),
    "dccn_batch_moment_norm_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _sz, _vp]),
    "dccn_clip_power_workspace_size": (_sz, [_ll]),
    "dccn_clip_power": (_i, [_vp, _vp, _vp, _ll, _f, _vp, _sz, _vp]),
    "dccn_cconv_gemm_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_cconv_gemm_bwd_w_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_cconv_gemm_bwd_w": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "dccn_cconv_gemm_bwd_x": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_dense_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_dense_bwd_x": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_dense_bwd_w_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_dense_bwd_w": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "dccn_dense_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "dccn_dense_bwd_slabs": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, POINTER(c_int), _vp]),
    "dccn_tail_param_count": (_i, [_i]),
    "dccn_demod_tail_workspace_size": (_sz, [_ll, _i]),
    "dccn_demod_tail_loss_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _sz, _vp]),
    "dccn_demod_tail_loss_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ll, _i, _vp, _sz, _vp]),
    "dccn_dense_tail_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_dense_tail_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "dccn_dense_tail_fwd_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "dccn_cconv_im2col": (_i, [_vp, _vp] + [_i] * 14 + [_vp]),
    "dccn_eq_bottleneck_supported": (_i, [_i] * 3),
    "dccn_eq_bottleneck_workspace_size": (C.c_size_t, [_i] * 3),
    "dccn_eq_bottleneck_fwd": (_i, [_vp] * 7 + [_i] * 3 + [_vp]),
    "dccn_eq_bottleneck_bwd": (_i, [_vp] * 11 + [_i] * 3 + [_vp, C.c_size_t, _vp]),
    "dccn_cconv_patch_supported": (_i, [_i] * 9),
    "dccn_cconv_patch_fwd": (_i, [_vp, _vp, _vp, _vp] + [_i] * 15 + [_vp]),
    "dccn_cconv_col2im": (_i, [_vp, _vp] + [_i] * 14 + [_vp]),
    "dccn_rx_gen_next_supported": (_i, [POINTER(RxShape)]),
    "dccn_step_monitor_add": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "dccn_tuning_count": (_i, []),
    "dccn_tuning_snapshot": (_i, [_vp, _i]),
    "dccn_chain_group_max": (_i, []),
    "dccn_eq_group_supported": (_i, [POINTER(EqShape)]),
    "dccn_eq_train_step_grouped": (_i, [_i, _vp, _vp, AdamHParams, _vp]),
    "dccn_eq_receive_group_supported": (_i, [POINTER(EqShape)]),
    "dccn_eq_receive_step_grouped": (_i, [_i, _vp, _vp, _vp, _vp]),
    "dccn_gen_static_frames_grouped": (_i, [_i, _vp, _vp]),
    "dccn_gen_static_apply_grouped": (_i, [_i, _vp, _vp, _vp, _vp]),
    "dccn_eq_monitor_accumulate_grouped": (_i, [_i, _vp, _vp]),
    "dccn_cconv_patch_bwd_supported": (_i, [_i] * 11),
    "dccn_cconv1d_bwd_supported": (_i, [_i] * 7),
    "dccn_cconv1d_bwd_workspace_size": (_sz, [_i]),
    "dccn_cconv1d_bwd": (_i, [_vp] * 6 + [_i] * 9 + [_vp, _sz, _vp]),
    "dccn_cconv_patch_bwd_w_workspace_size": (C.c_size_t, [_i] * 7),
    "dccn_cconv_patch_bwd_w": (_i, [_vp, _vp, _vp, _vp] + [_i] * 15 + [_vp, C.c_size_t, _vp]),
    "dccn_cconv_patch_bwd_x_workspace_size": (C.c_size_t, [_i] * 4),
    "dccn_cconv_patch_bwd_x": (_i, [_vp, _vp, _vp] + [_i] * 15 + [_vp, C.c_size_t, _vp]),
    "dccn_cconv_patch_plan_query": (_i, [_i] * 12 + [POINTER(CconvPatchPlan)]),
    "dccn_metrics_table_add": (_i, [_vp, _vp, _vp]),
    "dccn_metrics_table_set": (_i, [_vp, _vp, _vp]),
    "dccn_ingraph_awgn_workspace_size": (_sz, [_i, _i]),
    "dccn_ingraph_awgn": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, C.c_ulonglong, C.c_uint, _vp, _sz, _vp]),
    "dccn_classical_workspace_size": (_sz, []),
    "dccn_dense_fwd_ld": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_classical_pilot_ls": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _f, _vp]),
    "dccn_classical_gain": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _sz, _vp]),
    "dccn_classical_estimate": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "dccn_classical_detect": (_i, [_vp] * 8 + [_i] * 7 + [_vp, _sz, _vp]),
    "dccn_classical_receive_supported": (_i, [_i] * 7),
    "dccn_classical_receive": (_i, [POINTER(ClassicalReceiveArgs), _vp]),
    "dccn_classical_receive_grouped": (_i, [_i, POINTER(ClassicalLink)] + [_i] * 7 + [_vp]),
    "dccn_set_tuning": (_i, [_i, _i]),
    "dccn_get_tuning": (_i, [_i]),
    "dccn_dense_tail_supported": (_i, [_i, _i, _i, _i]),
    "dccn_dense_tail_grid": (_i, [_i, _i, _i, _i] + [POINTER(c_int)] * 4),
    "dccn_gemm_route_query": (_i, [_i] * 6 + [POINTER(GemmRoute)]),
    "dccn_rx_bwd_fused_supported": (_i, [POINTER(RxShape)]),
    "dccn_rx_dense_tail_fused": (_i, [POINTER(RxShape), _i]),
    "dccn_rx_norm_rides_backward": (_i, [POINTER(RxShape)]),
    "dccn_rx_backward_workspace_size": (_sz, [_i, _i, _i, _i, _i]),
    "dccn_rx_backward": (_i, [_vp] * 9 + [_i] * 6 + [_vp, _sz, _vp]),
    "dccn_adam_tf_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, AdamHParams, _ll, _vp]),
    "dccn_rx_param_offsets": (_i, [POINTER(RxShape), POINTER(c_longlong)]),
    "dccn_rx_workspace_size": (_sz, [POINTER(RxShape), _i]),
    "dccn_rx_eval_step": (_i, [POINTER(RxShape), POINTER(RxBuffers), _vp]),
    "dccn_rx_train_step": (_i, [POINTER(RxShape), POINTER(RxBuffers), AdamHParams, _vp]),
    # receive path (IQ frames -> packed bits / LLRs, no labels)
    "dccn_demod_decide": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dccn_dense_decide_supported": (_i, [_i, _i, _i, _i]),
    "dccn_dense_decide_fwd": (_i, [_vp] * 8 + [_i] * 4 + [_vp]),
    "dccn_rx_receive_workspace_size": (_sz, [POINTER(RxShape)]),
    "dccn_rx_receive_fused": (_i, [POINTER(RxShape)]),
    "dccn_rx_receive_step": (_i, [POINTER(RxShape), POINTER(RxReceiveBuffers), _vp]),
    "dccn_eq_receive_step": (_i, [POINTER(EqShape), POINTER(EqBuffers), POINTER(ReceiveOut), _vp]),
    # timing alignment from the cyclic prefix (in front of the receive path)
    "dccn_frame_sync_supported": (_i, [_i] * 4),
    "dccn_frame_sync": (_i, [_vp] + [_i] * 6 + [_vp] * 4),
    "dccn_frame_sync_cfo": (_i, [_vp] + [_i] * 6 + [_vp] * 5),
    "dccn_capture_sync_supported": (_i, [_i] * 4),
    "dccn_capture_sync": (_i, [_vp] + [c_longlong] * 3 + [_i] * 6 + [_vp] * 5),
    "dccn_capture_sync_at": (_i, [_vp, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 5),
    # coarse acquisition inside a capture (the first frame's start, left on the device for dccn_capture_sync_at)
    "dccn_capture_acquire_supported": (_i, [_i] * 5),
    "dccn_capture_acquire_workspace_size": (_sz, [_i] * 5),
    "dccn_capture_acquire": (_i, [_vp, c_longlong, c_longlong] + [_i] * 4 + [_vp, _i] + [_vp] * 5 + [_sz, _vp]),
    # the same stages for several links per launch (a host table of per-link descriptors)
    "dccn_frame_sync_grouped": (_i, [_i, POINTER(FrameLink)] + [_i] * 6 + [_vp]),
    "dccn_capture_sync_grouped": (_i, [_i, POINTER(CaptureLink)] + [_i] * 6 + [_vp]),
    "dccn_capture_acquire_grouped": (_i, [_i, POINTER(AcquireLink)] + [_i] * 5 + [_vp]),
    # one carrier offset per capture, pooled over its frames (three launches, a caller-owned workspace per link)
    "dccn_capture_sync_pooled_workspace_size": (_sz, [_i]),
    "dccn_capture_sync_pooled": (_i, [_vp, c_longlong, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 5 + [_sz, _vp]),
    "dccn_capture_sync_pooled_grouped": (_i, [_i, POINTER(PooledLink)] + [_i] * 6 + [_vp]),
    # carrier offsets beyond half a subcarrier spacing: acquisition over (q, m), the cuts with the whole offset taken out
    "dccn_capture_acquire_wide_supported": (_i, [_i] * 6),
    "dccn_capture_acquire_wide_workspace_size": (_sz, [_i] * 6),
    "dccn_capture_acquire_wide": (_i, [_vp, c_longlong, c_longlong] + [_i] * 4 + [_vp, _i, _i] + [_vp] * 6 + [_sz, _vp]),
    "dccn_capture_sync_wide": (_i, [_vp, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 7),
    "dccn_capture_sync_pooled_wide_workspace_size": (_sz, [_i]),
    "dccn_capture_sync_pooled_wide": (_i, [_vp, c_longlong, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 7
                                      + [_sz, _vp]),
    # 16-bit integer I/Q captures (int16 [n, 2] and a scale), converted inside the launches
    "dccn_capture_sync_sc16": (_i, [_vp, c_longlong, _f, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 5),
    "dccn_capture_sync_pooled_sc16": (_i, [_vp, c_longlong, _f, c_longlong, _vp, c_longlong, c_longlong] + [_i] * 6 + [_vp] * 5
                                      + [_sz, _vp]),
    "dccn_capture_acquire_sc16": (_i, [_vp, c_longlong, _f, c_longlong] + [_i] * 4 + [_vp, _i] + [_vp] * 5 + [_sz, _vp]),
    "dccn_rx_normalise": (_i, [POINTER(RxShape), POINTER(RxBuffers), _vp]),
    "dccn_rx_graph_create": (_i, [POINTER(RxShape), POINTER(RxBuffers), _i, AdamHParams, _vp, POINTER(c_void_p)]),
    "dccn_rx_graph_launch": (_i, [_vp, _vp]),
    "dccn_rx_graph_destroy": (_i, [_vp]),
    "dccn_timer_create": (_i, [POINTER(c_void_p)]),
    "dccn_timer_start": (_i, [_vp, _vp]),
    "dccn_timer_stop": (_i, [_vp, _vp]),
    "dccn_timer_elapsed_ms": (_i, [_vp, POINTER(c_float)]),
    "dccn_timer_destroy": (_i, [_vp]),
    "dccn_stream_synchronize": (_i, [_vp]),
    "dccn_eq_rx_folded_floats": (_sz, [POINTER(EqShape)]),
    "dccn_eq_norm_rides": (_i, [POINTER(EqShape)]),
    "dccn_eq_rx_fold": (_i, [POINTER(EqShape), _vp, _vp, _vp]),
    "dccn_eq_monitor_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_eq_monitor_accumulate": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dccn_step_trace_bytes": (_sz, [_i]),
    "dccn_step_trace_enable": (_i, [_vp, _sz, _i]),
    "dccn_step_trace_steps": (_ll, []),
    "dccn_step_trace_geometry": (None, [POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    # equaliser stage
    "dccn_layer_norm_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "dccn_layer_norm_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "dccn_tanh_fwd": (_i, [_vp, _vp, _ll, _vp]),
    "dccn_tanh_bwd": (_i, [_vp, _vp, _vp, _ll, _vp]),
    "dccn_equalize_fwd": (_i, [_vp, _vp, _vp, _vp, _ll, _vp]),
    "dccn_equalize_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _ll, _vp]),
    "dccn_pilot_snr": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dccn_cconv2d_same_expand": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dccn_cconv2d_same_reduce": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dccn_eq_param_offsets": (_i, [POINTER(EqShape), POINTER(c_longlong)]),
    "dccn_eq_workspace_size": (_sz, [POINTER(EqShape), _i]),
    "dccn_gen_static_supported": (_i, [_i, _i, _i]),
    "dccn_gen_static_partials": (_i, [_i]),
    "dccn_gen_static_frames": (_i, [POINTER(GenStatic), _vp]),
    "dccn_gen_static_apply": (_i, [POINTER(GenStatic), _vp, _vp, _vp]),
    "dccn_gen_static_apply_window": (_i, [POINTER(GenStatic), _vp, _vp, _vp]),
    "dccn_gen_static_apply_sync_supported": (_i, [_i] * 4),
    "dccn_gen_static_apply_sync": (_i, [POINTER(GenStatic), _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "dccn_eq_workspace_tensor": (_i, [POINTER(EqShape), _i, C.c_char_p, POINTER(C.c_size_t), POINTER(C.c_size_t)]),
    "dccn_eq_eval_step": (_i, [POINTER(EqShape), POINTER(EqBuffers), _vp]),
    "dccn_eq_train_step": (_i, [POINTER(EqShape), POINTER(EqBuffers), AdamHParams, _vp]),
    "dccn_eq_graph_create": (_i, [POINTER(EqShape), POINTER(EqBuffers), _i, AdamHParams, _vp, POINTER(c_void_p)]),
    # device-side input generator
    "dccn_philox_fill": (_i, [_vp, _ll, C.c_uint, C.c_uint, C.c_ulonglong, _vp]),
    "dccn_ofdm_tx_frames": (_i, [_vp, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.c_ulonglong,
                                 C.c_uint, _vp]),
    "dccn_channel_awgn_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_channel_doppler_awgn_workspace_size": (_sz, [_i, _i, _i, _i]),
    "dccn_channel_doppler_awgn": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _f, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i,
                                       C.c_ulonglong, C.c_uint, _vp, _sz, _vp]),
    "dccn_channel_groups_awgn_workspace_size": (_sz, [_i, _i, _i]),
    "dccn_channel_groups_awgn": (_i, [_vp, POINTER(ChannelGroup), _i, _vp, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _i, _vp,
                                      _i, C.c_ulonglong, C.c_uint, _vp, _sz, _vp]),
    "dccn_crc32c": (C.c_uint32, [C.c_uint32, _vp, _sz]),
    "dccn_channel_awgn": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, C.c_ulonglong,
                               C.c_uint, _vp, _sz, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """dlopen libdccn.so (built in-tree by ``__graft_entry__.build()`` / ``make -C dl_ofdm_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DccnError(
            "libdccn.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dl_ofdm_amd/csrc`; this package has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)      # AttributeError if the symbol is missing
        except AttributeError:
            # kernel experiments against an OLDER build of the library (tools/build_rev.sh): tolerate entry points it lacks
            if os.environ.get("DCCN_LIB_PATH") and os.environ.get("DCCN_LIB_ALLOW_MISSING"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # kernel experiments: DCCN_TUNE="key=value,key=value" applies dccn_set_tuning pairs at load time
    for kv in filter(None, os.environ.get("DCCN_TUNE", "").split(",")):
        k, v = kv.split("=")
        if lib.dccn_set_tuning(int(k), int(v)) != 0:
            raise DccnError("DCCN_TUNE: bad tuning pair %r" % kv)
    return lib


# Held over "device synchronize + dccn_*_graph_create".  hipDeviceSynchronize fails with hipErrorStreamCaptureUnsupported
# while ANY stream of the process is capturing, whatever the capture mode and whichever thread began it, so two host threads
# that each train on a stream of their own (config5.train_models) must not interleave one's capture with the other's
# synchronize.  Captures are rare (once per plan and mode) and short: the lock orders nothing else.
capture_lock = threading.Lock()


def check(status: int, what: str = "dccn call") -> None:
    if status != 0:
        lib = load()
        msg = lib.dccn_strerror(status).decode()
        raise DccnError("%s failed: %s (status %d, hipError %d)" % (what, msg, status, lib.dccn_last_hip_error()))


def ptr(t):
    """``t.data_ptr()``; ``None`` (a NULL pointer) for a tensor the call does without"""
    return None if t is None else t.data_ptr()


def stream_ptr(device) -> c_void_p:
    """the current stream of ``device``, as the ``dccn_stream_t`` every launch entry takes last"""
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_info():
    """(cu_count, wavefront, hbm_bytes, arch) of the current HIP device; raises without a GPU."""
    lib = load()
    cu, wf, hbm = c_int(0), c_int(0), c_size_t(0)
    arch = C.create_string_buffer(64)
    check(lib.dccn_device_info(C.byref(cu), C.byref(wf), C.byref(hbm), arch, 64), "dccn_device_info")
    return cu.value, wf.value, hbm.value, arch.value.decode()
