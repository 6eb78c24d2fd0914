"""aum_hip -- ctypes binding of libaum_hip.so (the C ABI in include/aum_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here (device memory, streams); every op below enqueues hand-written gfx950 kernels on the
current HIP stream through the C ABI.  There is NO fallback: if the shared library is missing the import of
the product path fails loudly (`python audio-mamba-aum_amd/csrc/build.py` builds it with hipcc).

The functions mirror the reference's extension modules:
  scan_fwd / scan_bwd          <- selective_scan_cuda.fwd / .bwd   (SSI:37, 62-65, 499-505, 541-552)
  conv1d_fwd / conv1d_bwd      <- causal_conv1d_cuda.causal_conv1d_fwd / _bwd (SSI:463, 594-596)
  rmsnorm_fwd / rmsnorm_bwd    <- _layer_norm_fwd / _layer_norm_bwd (LN:123-177, 293-377)
  rmsnorm_drop_fwd / _bwd      <- the same behind timm's DropPath on x (MM:90, MM:650): the per-sample factor inside the kernels
  rmsnorm_pool_fwd / _bwd      <- the final add + norm and hidden_states.mean(dim=1) of a cls-free model (MM:649-669) in one pass
"""
import ctypes as C
import math
import os
import typing

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libaum_hip.so")

AUM_F32, AUM_BF16, AUM_F16 = 0, 1, 2
SCAN_SOFTPLUS, SCAN_REVERSE, SCAN_GENERIC, SCAN_ROWPAIR, SCAN_ACCUMULATE = 1, 2, 4, 8, 16
SCAN_DELTA_ACTIVATED = 32       # token-major scans: delta already holds softplus(raw + delta_bias) (xdt_tm_fwd(..., delta_softplus=True))
XDT_DELTA_SOFTPLUS = 1
CONV_SILU, CONV_REVERSE, CONV_GENERIC = 1, 2, 4     # AUM_CONV_*: CONV_GENERIC forces the any-width kernel
NORM_GENERIC = 2                                    # AUM_NORM_GENERIC: forces the any-cols kernel
_DT = {torch.float32: AUM_F32, torch.bfloat16: AUM_BF16, torch.float16: AUM_F16}
_ERR = {-1: "AUM_E_NULL", -2: "AUM_E_SHAPE", -3: "AUM_E_DTYPE", -4: "AUM_E_UNSUPPORTED", -5: "AUM_E_WORKSPACE",
        -6: "AUM_E_LAUNCH"}

_i64, _i32, _u32, _vp, _fp = C.c_int64, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p
ABI_VERSION = 13


class _Debug:
    """Kernel-selection switches for A/B runs and ablations (tools/kbench.py, tests).  They are attributes set by the tool that
    wants them; the environment is consulted ONCE, at import, and only when AUM_DEBUG=1 -- a stray variable in a training
    environment cannot change which kernel runs."""

    def __init__(self):
        self.ablate = 0            # AUM_DBG_* bits (upper half of the kernel `flags`)
        self.rowpair = False       # general row-pair kernels instead of the specialised ones
        self.no_ckpt = False       # long rows: no chunk-entry checkpoint
        self.no_accumulate = False  # long rows: second direction does not accumulate into the first one's tensors
        self.no_lane_ckpt = False  # L = 513 rows: scan_lane_ckpt() hands out no checkpoint
        self.proj_splits = 0       # token splits of the projection weight-gradient kernel (0: aum_proj_bwd_weight_splits)
        self.torch_sums = False    # partial results summed by torch.sum instead of aum_sum_rows
        self.sums_one_by_one = False   # sum_rows_multi: one aum_sum_rows launch per partial set (the launches of rounds 2-4; A/B)
        self.stream_fused = True   # Mamba.step_chunk: conv + x/dt + scan in one launch (stream_block) where it takes the shapes
        if os.environ.get("AUM_DEBUG") == "1":
            self.ablate = int(os.environ.get("AUM_ABLATE", "0"))
            self.rowpair = os.environ.get("AUM_SCAN_ROWPAIR") == "1"
            self.no_ckpt = os.environ.get("AUM_SCAN_NO_CKPT") == "1"
            self.no_accumulate = os.environ.get("AUM_SCAN_NO_ACCUMULATE") == "1"
            self.no_lane_ckpt = os.environ.get("AUM_SCAN_NO_LANE_CKPT") == "1"
            self.torch_sums = os.environ.get("AUM_TORCH_SUMS") == "1"
            self.sums_one_by_one = os.environ.get("AUM_SUMS_ONE_BY_ONE") == "1"
            self.stream_fused = os.environ.get("AUM_STREAM_FUSED", "1") != "0"


debug = _Debug()


class ScanFwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "A", "A_b", "D", "delta_bias", "out", "out_pre",
                                    "last_state", "workspace")]
                + [(n, _i64) for n in ("workspace_bytes", "u_bs", "u_ds", "delta_bs", "delta_ds", "z_bs", "z_ds", "B_bs",
                                       "B_ns", "C_bs", "C_ns", "out_bs", "out_ds")]
                + [(n, _i32) for n in ("batch", "dim", "len", "dstate", "dtype")] + [("flags", _u32), ("x_ck", _vp), ("x_lane", _vp)])


class ScanBwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "dout", "out_pre", "A", "A_b", "D", "delta_bias", "du",
                                    "ddelta", "dz", "dA", "dA_b", "dB", "dC", "dD", "ddelta_bias", "workspace")]
                + [(n, _i64) for n in ("workspace_bytes", "u_bs", "u_ds", "delta_bs", "delta_ds", "z_bs", "z_ds", "B_bs",
                                       "B_ns", "C_bs", "C_ns", "dout_bs", "dout_ds", "out_bs", "out_ds", "du_bs", "du_ds",
                                       "ddelta_bs", "ddelta_ds", "dz_bs", "dz_ds", "dB_bs", "dB_ns", "dC_bs", "dC_ns")]
                + [(n, _i32) for n in ("batch", "dim", "len", "dstate", "dtype")] + [("flags", _u32), ("x_ck", _vp), ("x_lane", _vp)])


class ScanTmFwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "A", "A_b", "D", "delta_bias", "out", "out_pre", "ckpt")]
                + [(n, _i64) for n in ("u_bs", "u_ts", "delta_bs", "delta_ts", "z_bs", "z_ts", "B_bs", "B_ts", "C_bs", "C_ts",
                                       "out_bs", "out_ts", "pre_bs", "pre_ts")]
                + [(n, _i32) for n in ("batch", "dim", "len", "dstate", "dtype")] + [("flags", _u32)])


class ScanTmBwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "dout", "out_pre", "A", "A_b", "D", "delta_bias", "ckpt", "du",
                                    "ddelta", "dz", "dA", "dA_b", "dBC", "dD", "ddelta_bias", "workspace")]
                + [(n, _i64) for n in ("workspace_bytes", "u_bs", "u_ts", "delta_bs", "delta_ts", "z_bs", "z_ts", "B_bs", "B_ts",
                                       "C_bs", "C_ts", "dout_bs", "dout_ts", "pre_bs", "pre_ts", "du_bs", "du_ts", "ddelta_bs",
                                       "ddelta_ts", "dz_bs", "dz_ts")]
                + [(n, _i32) for n in ("batch", "dim", "len", "dstate", "dtype")] + [("flags", _u32), ("dA_xA", _vp), ("dA_b_xA", _vp)])


class ScanTmSegFwdArgs(C.Structure):
    _fields_ = [("base", ScanTmFwdArgs), ("carry", _vp), ("carry_bytes", _i64), ("segments", _i32), ("reserved", _i32)]


class ScanTmSegBwdArgs(C.Structure):
    _fields_ = [("base", ScanTmBwdArgs), ("segments", _i32), ("reserved", _i32)]


class ScanTmFwdStateArgs(C.Structure):
    _fields_ = [("base", ScanTmFwdArgs), ("state_in", _vp), ("state_out", _vp), ("carry", _vp), ("carry_bytes", _i64), ("segments", _i32),
                ("reserved", _i32)]


class ConvArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "dy", "weight", "bias", "y", "dx", "dweight", "dbias")]
                + [(n, _i64) for n in ("x_bs", "x_ds", "y_bs", "y_ds", "dy_bs", "dy_ds", "dx_bs", "dx_ds")]
                + [(n, _i32) for n in ("batch", "dim", "len", "width", "dtype")] + [("flags", _u32)])


class ConvTmArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "dy", "weight", "bias", "y", "dx", "dw_part", "db_part")]
                + [(n, _i64) for n in ("x_bs", "x_ts", "y_bs", "y_ts", "dy_bs", "dy_ts", "dx_bs", "dx_ts")]
                + [(n, _i32) for n in ("batch", "dim", "len", "width", "dtype")] + [("flags", _u32)])


class NormArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "residual", "dy", "dresidual_out", "weight", "rstd_in", "y", "residual_out",
                                    "dx", "dresidual_in", "rstd_out", "dweight_partial")]
                + [(n, _i64) for n in ("row_stride_x", "row_stride_res", "row_stride_y", "row_stride_res_out",
                                       "row_stride_dy", "row_stride_dres_out", "row_stride_dx", "row_stride_dres_in")]
                + [("eps", C.c_float)] + [(n, _i32) for n in ("rows", "cols", "x_dtype", "res_dtype", "y_dtype")]
                + [("flags", _u32)])


class NormDropArgs(C.Structure):
    _fields_ = [("base", NormArgs), ("row_scale", _vp), ("rows_per_scale", _i32), ("reserved", _i32)]


class NormPoolArgs(C.Structure):
    _fields_ = ([("base", NormArgs), ("pooled", _vp), ("dpooled", _vp), ("pool_partial", _vp), ("row_stride_pooled", _i64),
                 ("row_stride_dpooled", _i64), ("rows_per_sample", _i32), ("reserved", _i32)])


class FbankArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("wave", "window", "twiddle", "mel_start_f", "mel_count_f", "mel_w", "out")]
                + [(n, _i64) for n in ("wave_bs", "out_bs")]
                + [(n, _i32) for n in ("batch", "n_samples", "win", "shift", "padded", "num_frames", "target_length",
                                       "num_mel", "mel_wstride")]
                + [(n, C.c_float) for n in ("preemph", "norm_mean", "norm_inv2std", "log_floor")]
                + [("aug", _vp), ("noise", _vp)])


class StftArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("wave", "window", "twiddle", "mel_start_f", "mel_count_f", "mel_w", "n_valid", "out")]
                + [(n, _i64) for n in ("wave_bs", "out_bs")]
                + [(n, _i32) for n in ("batch", "n_samples", "win", "hop", "n_fft", "num_mel", "mel_wstride", "target_length")]
                + [("eps", C.c_float), ("reserved", _i32)])


class TimeWarpArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("in_", "table", "out")] + [(n, _i64) for n in ("in_bs", "out_bs")]
                + [(n, _i32) for n in ("batch", "frames", "num_mel", "reserved")])


class FrontendArgs(C.Structure):
    _fields_ = ([("fbank", FbankArgs)] + [(n, _vp) for n in ("weight", "bias", "pos", "cls_row", "tokens", "patches")]
                + [("tokens_bs", _i64)] + [(n, _i32) for n in ("dim", "cls_pos", "dtype", "out_dtype")] + [("flags", _u32)])


class FbankStreamArgs(C.Structure):
    _fields_ = ([("fbank", FbankArgs)] + [(n, _vp) for n in ("cu_samples", "cu_frames", "tail_len", "idx", "first_frame", "n_real", "tails")]
                + [(n, _i32) for n in ("total_samples", "total_frames", "nseq", "nrows", "cap", "reserved")])


class ProjArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("act", "w_x", "w_dt", "x_dbl", "out_act", "dB", "dC")]
                + [(n, _i64) for n in ("dB_bs", "dB_ns", "dC_bs", "dC_ns", "ntok")]
                + [(n, _i32) for n in ("dim", "dt_rank", "dstate", "len", "dtype", "w_ld")])


class ProjWArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "y", "out")] + [("ntok", _i64)]
                + [(n, _i32) for n in ("dim", "nrows", "nsplit", "transpose_out", "dtype")])


class GemmArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("a", "b", "c")] + [(n, _i32) for n in ("m", "n", "k", "lda", "ldb", "ldc", "dtype")] + [("flags", _u32)])


class XdtBwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("ddelta", "dbc", "wdt_t", "wx_t", "du", "dx_dbl")] + [("ntok", _i64)]
                + [(n, _i32) for n in ("dim", "rank", "ncols", "ldd", "lddbc", "ldwdt", "ldwx", "ldu", "ldx", "dtype")])


class GemmWArgs(C.Structure):
    _fields_ = [("y", C.c_void_p), ("x", C.c_void_p), ("part", C.c_void_p), ("t", C.c_int64), ("ldy", C.c_int64), ("ldx", C.c_int64),
                ("n", C.c_int32), ("k", C.c_int32), ("splits", C.c_int32), ("dtype", C.c_int32)]


SUM_MAX_JOBS = 8        # AUM_SUM_MAX_JOBS


class SumJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("outer", C.c_int64), ("inner", C.c_int64), ("tr_cols", C.c_int32), ("reserved", C.c_int32)]


class ConvUpdateArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("conv_state", C.c_void_p), ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("batch", C.c_int32), ("dim", C.c_int32), ("width", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_uint32)]


class StateUpdateArgs(C.Structure):
    _fields_ = [("state", C.c_void_p), ("x", C.c_void_p), ("dt", C.c_void_p), ("z", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
                ("A", C.c_void_p), ("D", C.c_void_p), ("dt_bias", C.c_void_p), ("out", C.c_void_p),
                ("batch", C.c_int32), ("dim", C.c_int32), ("dstate", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_uint32)]


class ConvTmChunkArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "conv_state", "weight", "bias", "y")] + [(n, _i64) for n in ("x_bs", "x_ts", "y_bs", "y_ts")]
                + [(n, _i32) for n in ("batch", "dim", "len", "width", "dtype")] + [("flags", _u32)])


class ScanTmChunkArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out")]
                + [(n, _i64) for n in ("u_bs", "u_ts", "delta_bs", "delta_ts", "z_bs", "z_ts", "B_bs", "B_ts", "C_bs", "C_ts", "out_bs", "out_ts")]
                + [(n, _i32) for n in ("batch", "dim", "len", "dstate", "dtype")] + [("flags", _u32)])


class ConvTmChunkVarArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "conv_state", "weight", "bias", "y", "cu_seqlens", "state_indices")] + [(n, _i64) for n in ("x_ts", "y_ts")]
                + [(n, _i32) for n in ("total", "nseq", "nrows", "dim", "width", "dtype")] + [("flags", _u32)])


class ScanTmChunkVarArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out", "cu_seqlens", "state_indices")]
                + [(n, _i64) for n in ("u_ts", "delta_ts", "z_ts", "B_ts", "C_ts", "out_ts")]
                + [(n, _i32) for n in ("total", "nseq", "nrows", "dim", "dstate", "dtype")] + [("flags", _u32)])


class ConvTmChunkPeeksArgs(C.Structure):
    _fields_ = [("base", ConvTmChunkVarArgs), ("peek_every", _i32), ("reserved", _i32)]


class ScanTmChunkPeeksArgs(C.Structure):
    _fields_ = [("base", ScanTmChunkVarArgs), ("peek_every", _i32), ("reserved", _i32)]


class ScanTmPeeksFwdArgs(C.Structure):
    _fields_ = [("base", ScanTmChunkVarArgs), ("ckpt", _vp), ("ckpt_bytes", _i64), ("peek_every", _i32), ("reserved", _i32)]


class ScanTmPeeksBwdArgs(C.Structure):
    _fields_ = ([("base", ScanTmChunkVarArgs)] + [(n, _vp) for n in ("ckpt", "du", "ddelta", "dz", "workspace")]
                + [(n, _i64) for n in ("ckpt_bytes", "workspace_bytes", "du_ts", "ddelta_ts", "dz_ts")] + [("peek_every", _i32), ("reserved", _i32)])


class ConvTmPeeksBwdArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "dy", "weight", "bias", "dx", "workspace", "cu_seqlens")]
                + [(n, _i64) for n in ("workspace_bytes", "x_ts", "dy_ts", "dx_ts")]
                + [(n, _i32) for n in ("total", "nseq", "dim", "width", "dtype")] + [("flags", _u32), ("peek_every", _i32), ("reserved", _i32)])


class ConvTmPrefillVarArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "conv_state", "weight", "bias", "y", "cu_seqlens", "state_indices")] + [(n, _i64) for n in ("x_ts", "y_ts")]
                + [(n, _i32) for n in ("total", "nseq", "nrows", "dim", "width", "dtype")] + [("flags", _u32), ("max_len", _i32)])


class ScanTmFwdStateVarArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "delta", "z", "B", "C", "A", "D", "delta_bias", "state", "out", "cu_seqlens", "state_indices")]
                + [(n, _i64) for n in ("u_ts", "delta_ts", "z_ts", "B_ts", "C_ts", "out_ts")]
                + [(n, _i32) for n in ("total", "nseq", "nrows", "dim", "dstate", "dtype")] + [("flags", _u32)]
                + [(n, _i32) for n in ("range_len", "max_len", "reserved")] + [("carry", _vp), ("carry_bytes", _i64)])


class StreamBlockArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "z", "conv_state", "state", "conv_weight", "conv_bias", "wx", "wdt", "A", "D", "delta_bias", "y", "scratch",
                                    "cu_seqlens", "state_indices")]
                + [(n, _i64) for n in ("x_ts", "z_ts", "y_ts", "scratch_bytes")]
                + [(n, _i32) for n in ("total", "nseq", "nrows", "max_len", "dim", "width", "dstate", "rank", "ncols", "ldwx", "ldwdt", "dtype")]
                + [("flags", _u32)])


class DtProjArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("x", "w", "out")] + [("ntok", _i64)] + [(n, _i32) for n in ("dim", "rank", "ldx", "ldw", "ldo", "dtype")])


class XdtArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("u", "wx", "wdt", "x_dbl", "delta")] + [("ntok", _i64)]
                + [(n, _i32) for n in ("dim", "rank", "ncols", "ldu", "ldwx", "ldwdt", "ldx", "ldd", "dtype")]
                + [("delta_bias", _vp), ("flags", _u32)])


PARK_MAX_TENSORS = 64       # AUM_PARK_MAX_TENSORS
PARK_RESTORE = 1            # AUM_PARK_RESTORE: blob -> pool


class ParkArgs(C.Structure):
    _fields_ = ([("base", _vp * PARK_MAX_TENSORS)] + [(n, _i64 * PARK_MAX_TENSORS) for n in ("row_stride", "row_bytes", "blob_off")]
                + [("rows", _vp), ("blob", _vp), ("blob_stride", _i64), ("n_tensors", _i32), ("n_sessions", _i32), ("flags", _u32)])


class StreamInArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("hidden", "residual_in", "norm_weight", "w_in", "residual_out", "xz")] + [("hidden_ts", _i64), ("xz_ts", _i64)]
                + [(n, _i32) for n in ("total", "d_model", "dim", "ldw", "dtype")] + [("eps", C.c_float)])


class StreamOutArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("y", "w_out", "out")] + [("y_ts", _i64), ("out_ts", _i64)]
                + [(n, _i32) for n in ("total", "d_model", "dim", "ldw", "dtype", "reserved")])


STREAM_LAYER_POINTERS = ("norm_weight", "w_in", "conv_weight", "conv_bias", "wx", "wdt", "A", "D", "delta_bias", "w_out", "conv_state", "state")


class StreamLayer(C.Structure):
    _fields_ = [(n, _vp) for n in STREAM_LAYER_POINTERS]


class StreamLayersArgs(C.Structure):
    _fields_ = ([(n, _vp) for n in ("layers", "hidden", "residual_in", "hidden_out", "residual_out", "workspace", "cu_seqlens", "state_indices")]
                + [("hidden_ts", _i64), ("workspace_bytes", _i64)]
                + [(n, _i32) for n in ("depth", "total", "nseq", "nrows", "max_len", "d_model", "dim", "rank", "ncols", "ldwx", "ldwdt", "dtype")]
                + [("flags", _u32), ("eps", C.c_float)])


# Every entry point of include/aum_hip.h: name -> (argtypes, restype).  The launches take (const Args*, void* stream) and return an AUM_E_*
# code; only the other forms are spelled out.  Lib sets these on load; EXPORTS (what tests/test_abi.py holds against the header) is the keys.
_SIGNATURES = {name: ([_vp, _vp], C.c_int) for name in (
    "aum_selective_scan_fwd", "aum_selective_scan_bwd", "aum_causal_conv1d_fwd", "aum_causal_conv1d_bwd", "aum_rmsnorm_fwd", "aum_rmsnorm_bwd",
    "aum_fbank_fwd", "aum_frontend_tokens_fwd", "aum_stft_logmel_fwd", "aum_spec_time_warp", "aum_proj_fwd", "aum_proj_bwd_data",
    "aum_proj_bwd_weight", "aum_scan_tm_fwd", "aum_scan_tm_bwd", "aum_scan_tm_seg_fwd", "aum_scan_tm_seg_bwd", "aum_conv1d_tm_fwd",
    "aum_conv1d_tm_bwd", "aum_gemm_tn", "aum_gemm_wgrad", "aum_dtproj_tm_fwd", "aum_xdt_tm_fwd", "aum_xdt_tm_bwd", "aum_causal_conv1d_update",
    "aum_selective_state_update", "aum_conv1d_tm_chunk", "aum_scan_tm_chunk", "aum_conv1d_tm_chunk_var", "aum_scan_tm_chunk_var", "aum_stream_block_tm", "aum_scan_tm_fwd_state",
    "aum_conv1d_tm_prefill_var", "aum_scan_tm_fwd_state_var", "aum_conv1d_tm_chunk_peeks", "aum_scan_tm_chunk_peeks", "aum_fbank_stream_fwd",
    "aum_scan_tm_peeks_fwd_ckpt", "aum_scan_tm_peeks_bwd", "aum_conv1d_tm_peeks_bwd", "aum_stream_park", "aum_stream_in_tm", "aum_stream_out_tm",
    "aum_stream_layers", "aum_rmsnorm_drop_fwd", "aum_rmsnorm_drop_bwd", "aum_rmsnorm_pool_fwd", "aum_rmsnorm_pool_bwd")}
_SIGNATURES.update({
    "aum_abi_version": ([], C.c_int), "aum_scan_max_single_pass_len": ([], C.c_int),
    "aum_selective_scan_workspace_bytes": ([_i32] * 6, _i64), "aum_selective_scan_ckpt_bytes": ([_i32] * 4, _i64),
    "aum_selective_scan_lane_ckpt_bytes": ([_i32] * 5, _i64), "aum_scan_tm_workspace_bytes": ([_i32] * 5, _i64),
    "aum_scan_tm_seg_carry_bytes": ([_i32] * 6, _i64), "aum_scan_tm_seg_workspace_bytes": ([_i32] * 6, _i64),
    "aum_rmsnorm_bwd_partials": ([_i32], C.c_int), "aum_rmsnorm_bwd_partial_rows": ([_i32, _i32, _u32], C.c_int),
    "aum_scan_tm_nck": ([_i32], _i32), "aum_scan_tm_ckpt_rows": ([_i32], _i32), "aum_conv1d_tm_nparts": ([_i32, _i32], _i32),
    "aum_proj_bwd_weight_splits": ([_i32, _i64], C.c_int), "aum_hbm_copy": ([_vp, _vp, _i64, _vp], C.c_int),
    "aum_selftest_wave_scan": ([_vp, _vp, C.c_int, _vp], C.c_int), "aum_selftest_wave_sum32": ([_vp, _vp, _vp], C.c_int),
    "aum_sum_rows": ([_vp, _vp, _i64, _i64, _i64, _i32, _vp], C.c_int), "aum_sum_rows_multi": ([_vp, _i32, _vp], C.c_int),
    "aum_cast_bank": ([_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp], C.c_int),
    "aum_stream_block_scratch_bytes": ([_i32] * 3, _i64), "aum_stream_block_max_len": ([], _i32),
    "aum_scan_tm_fwd_state_var_carry_bytes": ([_i32] * 4, _i64),
    "aum_scan_tm_peeks_ckpt_bytes": ([_i32] * 4, _i64), "aum_scan_tm_peeks_bwd_workspace_bytes": ([_i32] * 4, _i64),
    "aum_conv1d_tm_peeks_bwd_workspace_bytes": ([_i32] * 3, _i64),
    "aum_stream_layers_scratch_bytes": ([_i32] * 4, _i64),
    "aum_rmsnorm_pool_partial_rows": ([_i32], C.c_int),
})
EXPORTS = list(_SIGNATURES)


class Lib:
    """A loaded C-ABI library.  `host=True` marks the tests-only lane-array build that takes host pointers."""

    def __init__(self, path, host=False):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: the HIP extension is not built.  Run `python audio-mamba-aum_amd/csrc/build.py` "
                "(hipcc, gfx950).  There is no CPU fallback on the product path.")
        self.path, self.host = path, host
        self.c = C.CDLL(path)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(self.c, name)   # AttributeError if a declared symbol is missing
            fn.argtypes, fn.restype = argtypes, restype
        if self.c.aum_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {self.c.aum_abi_version()}, this binding speaks {ABI_VERSION} -- rebuild the library "
                               "(python audio-mamba-aum_amd/csrc/build.py)")
        self.max_single_pass_len = int(self.c.aum_scan_max_single_pass_len())

    def stream(self, t):
        if self.host:
            return None
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def check_tensor(self, t):
        if t is None:
            return
        if self.host:
            if t.device.type != "cpu":
                raise RuntimeError("lane-array (test) library takes host tensors")
        elif t.device.type != "cuda":
            raise RuntimeError("libaum_hip.so needs device (HIP) tensors; there is no CPU path in the product library")


_product = None


def get():
    """The product library (libaum_hip.so).  Raises ImportError if it has not been built."""
    global _product
    if _product is None:
        so = _SO
        if os.environ.get("AUM_DEBUG") == "1" and os.environ.get("AUM_HIP_LIB"):     # A/B builds (tools/ only)
            so = os.environ["AUM_HIP_LIB"]
        _product = Lib(so, host=False)
    return _product


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {_ERR.get(rc, rc)}")


class LaunchTimer:
    """Optional per-launch timing with HIP events recorded on the stream the kernels are enqueued on (torch's current
    stream).  bench.py enables it to compute the live roofline numbers; off by default (zero overhead)."""

    def __init__(self):
        self.enabled = False
        self.only = None        # optional set of kernel names to time (two events per launch cost ~8 us of host time)
        self.every = 1          # bracket every n-th launch of a name only: an event on the stream is a barrier packet, ~6 us of idle GPU each
                                # (profiles/r06_step_timeline.txt: two 5.8 us gaps around every bracketed launch)
        self.records = {}       # name -> list of (start_event, end_event, meta)
        self.seen = {}          # name -> launches seen since reset()

    def reset(self):
        self.records = {}
        self.seen = {}

    def want(self, name):
        n = self.seen.get(name, 0)
        self.seen[name] = n + 1
        return n % self.every == 0

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in evs]
            out[name] = {"launches": len(ms), "avg_ms": sum(ms) / max(len(ms), 1), "meta": evs[-1][2] if evs else None}
        return out


timer = LaunchTimer()


def C_byref(s):
    return C.cast(C.byref(s), C.c_void_p)


def _launch(fn, args, stream_tensor, lib, name, meta=None):
    if timer.enabled and not lib.host and (timer.only is None or name in timer.only) and timer.want(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(C_byref(args), lib.stream(stream_tensor))
        b.record()
        timer.records.setdefault(name, []).append((a, b, meta))
    else:
        rc = fn(C_byref(args), lib.stream(stream_tensor))
    _chk(rc, name)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _unit(t, name):
    if t is not None and t.stride(-1) != 1 and t.shape[-1] != 1:
        raise RuntimeError(f"{name}: the time axis must be unit-stride (SSI:19-30)")


def _f32c(t):
    """a parameter as the kernels read it: fp32 contiguous.  One that already is comes back as it is -- the callers take its address and shape,
    and a detach() is a microsecond per parameter and launch; anything else is converted off the autograd graph"""
    if t is None or (t.dtype == torch.float32 and t.is_contiguous()):
        return t
    return t.detach().to(torch.float32).contiguous()


def _bc3(t):
    """(batch, 1, dstate, len) -> (batch, dstate, len) view (the G=1 case, SSI:31-36)."""
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise RuntimeError("only one B/C group is supported (G=1), as used by Mamba (SSI:473-493)")
        t = t[:, 0]
    return t


def _alloc(batch, dim, length, dtype, device, dmajor):
    """(batch, dim, len) tensor; dmajor=True stores it channel-major [dim][batch][len] (the layout of the reference's
    xz view, MS:185-189) so the projections on either side of the kernels are transpose-free GEMMs."""
    if dmajor:
        return torch.empty((dim, batch, length), dtype=dtype, device=device).permute(1, 0, 2)
    return torch.empty((batch, dim, length), dtype=dtype, device=device)


def scan_ckpt(u, dstate, lib=None):
    """An empty `x` checkpoint tensor (batch, dim, len/512, dstate) fp32 for rows the chunked kernels take (long-form clips,
    L = 512 m + 1), else None.  Pass it as x_ck to scan_fwd (filled) and then to scan_bwd of the same direction (which then
    skips its pre-pass); not with generic=/rowpair=.  debug.no_ckpt (A/B runs) or debug.rowpair: no checkpoint."""
    lib = lib or get()
    batch, dim, length = u.shape
    if debug.rowpair or debug.no_ckpt:
        return None
    if lib.c.aum_selective_scan_ckpt_bytes(batch, dim, length, dstate) <= 0:
        return None
    return torch.empty((batch, dim, length // 512, dstate), dtype=torch.float32, device=u.device)


def scan_lane_ckpt(u, dstate, bidir, lib=None):
    """An empty lane-entry checkpoint (batch, dim, directions, dstate, 64) fp32 for rows the L = 513 row kernels take, else None.
    Pass it as x_lane to scan_fwd (filled) and to scan_bwd of the same call, which then skips recomputing the forward scan."""
    lib = lib or get()
    batch, dim, length = u.shape
    if debug.rowpair or debug.no_lane_ckpt:
        return None
    if lib.c.aum_selective_scan_lane_ckpt_bytes(batch, dim, length, dstate, int(bool(bidir))) <= 0:
        return None
    return torch.empty((batch, dim, 2 if bidir else 1, dstate, 64), dtype=torch.float32, device=u.device)


def scan_accumulates(u, dstate, lib=None):
    """True when a second-direction call on this shape can add to the first one's tensors (accumulate_into=): the rows the
    chunked kernels take, i.e. exactly when scan_ckpt() gives a checkpoint."""
    lib = lib or get()
    batch, dim, length = u.shape
    if debug.rowpair or debug.no_accumulate:
        return False
    return lib.c.aum_selective_scan_ckpt_bytes(batch, dim, length, dstate) > 0


def _scan_cm_rows(lib, u, delta, z, B, C, A, extra=()):
    """THE operand rule of the channel-major scans (scan_fwd, scan_bwd): B / C as (batch, dstate, len) views (_bc3); every row operand on the
    library's side with a unit time stride; u of a dtype the kernels have and delta, z, B, C of that dtype; A (dim, dstate), B / C (batch,
    dstate, len); delta, z and every (name, tensor | None) of `extra` (scan_bwd: dout, out_pre) of u's dtype and (batch, dim, len) -- the
    kernels are told ONE element type and ONE shape and index every one of them by it.  Returns (B, C, (batch, dim, len, dstate))."""
    B, C = _bc3(B), _bc3(C)
    dt, shape = u.dtype, u.shape
    for n, t in (("u", u), ("delta", delta), ("z", z), ("B", B), ("C", C)):
        _unit(t, n)
        lib.check_tensor(t)
    if dt not in _DT or delta.dtype != dt or B.dtype != dt or C.dtype != dt or (z is not None and z.dtype != dt):
        raise RuntimeError("u, delta, z, B, C must share one dtype in {fp32, bf16, fp16}")
    batch, dim, length = shape
    dstate = A.shape[1]
    if A.shape != (dim, dstate) or B.shape != (batch, dstate, length) or C.shape != B.shape:
        raise RuntimeError("shape mismatch in selective scan arguments")
    if delta.shape != shape or (z is not None and z.shape != shape):
        extra = (("delta", delta), ("z", z)) + tuple(extra)            # the refusal below names the one
    for n, t in extra:
        if t is not None:
            _unit(t, n)
            lib.check_tensor(t)
            if t.dtype != dt or t.shape != shape:
                raise RuntimeError(f"{n}: expected u's dtype and shape ({dt}, {tuple(shape)}), got {t.dtype}, {tuple(t.shape)}")
    return B, C, (batch, dim, length, dstate)


def _check_scan_ck(lib, x_ck, x_lane, dims, bidir):
    """the checkpoints as scan_ckpt / scan_lane_ckpt hand them out: on the library's side, fp32, contiguous, of exactly their shape"""
    if x_ck is None and x_lane is None:         # the usual call: kept short
        return
    batch, dim, length, dstate = dims
    for name, t, shape in (("x_ck", x_ck, (batch, dim, length // 512, dstate)), ("x_lane", x_lane, (batch, dim, 2 if bidir else 1, dstate, 64))):
        if t is None:
            continue
        lib.check_tensor(t)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != shape:
            raise RuntimeError(f"{name}: expected a contiguous fp32 {shape} tensor, got {tuple(t.shape)} {t.dtype}")


def _scan_cm_flags(softplus, reverse, generic, rowpair, accumulate):
    return ((SCAN_SOFTPLUS if softplus else 0) | (SCAN_REVERSE if reverse else 0) | (SCAN_GENERIC if generic else 0)
            | (SCAN_ROWPAIR if rowpair or debug.rowpair else 0) | (SCAN_ACCUMULATE if accumulate else 0)
            | (debug.ablate << 16))   # kernel-ablation bits, set by tools/kbench.py only


def _fill_scan_cm(a, u, delta, z, B, C, A, A_b, D, delta_bias, x_ck, x_lane, dims, flags):
    """Writes what ScanFwdArgs and ScanBwdArgs share: the row operands' pointers and (batch, row) strides, the parameters (fp32 contiguous,
    as the caller converted them), the checkpoints, sizes, dtype and flags."""
    a.u, a.delta, a.z, a.B, a.C = _ptr(u), _ptr(delta), _ptr(z), _ptr(B), _ptr(C)
    a.A, a.A_b, a.D, a.delta_bias = _ptr(A), _ptr(A_b), _ptr(D), _ptr(delta_bias)
    a.x_ck, a.x_lane = _ptr(x_ck), _ptr(x_lane)
    a.u_bs, a.u_ds = u.stride(0), u.stride(1)
    a.delta_bs, a.delta_ds = delta.stride(0), delta.stride(1)
    if z is not None:
        a.z_bs, a.z_ds = z.stride(0), z.stride(1)
    a.B_bs, a.B_ns, a.C_bs, a.C_ns = B.stride(0), B.stride(1), C.stride(0), C.stride(1)
    a.batch, a.dim, a.len, a.dstate = dims
    a.dtype, a.flags = _DT[u.dtype], flags


def scan_fwd(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, reverse=False, A_b=None,
             want_out_pre=False, want_last_state=False, dmajor=False, generic=False, rowpair=False, x_ck=None,
             accumulate_into=None, x_lane=None, lib=None):
    """selective_scan_cuda.fwd.  Returns (out, out_pre|None, last_state|None).  A_b != None: fused bidirectional.
    x_ck: a scan_ckpt() tensor to fill.  accumulate_into: the `out` of the other direction's call (long rows only, see
    scan_accumulates): this call adds to it and returns it."""
    lib = lib or get()
    B, C, dims = _scan_cm_rows(lib, u, delta, z, B, C, A)
    batch, dim, length, dstate = dims
    _check_scan_ck(lib, x_ck, x_lane, dims, A_b is not None)
    A, A_b, D, delta_bias = _f32c(A), _f32c(A_b), _f32c(D), _f32c(delta_bias)
    out = accumulate_into if accumulate_into is not None else _alloc(batch, dim, length, u.dtype, u.device, dmajor)
    if out.shape != u.shape or out.dtype != u.dtype or out.stride(2) != 1:
        raise RuntimeError(f"accumulate_into: expected u's dtype and shape with a unit time stride, got {out.dtype}, {tuple(out.shape)}, {out.stride()}")
    out_pre = _alloc(batch, dim, length, u.dtype, u.device, dmajor) if want_out_pre else None
    last = torch.empty((batch, dim, dstate), dtype=torch.float32, device=u.device) if want_last_state else None
    a = ScanFwdArgs()
    _fill_scan_cm(a, u, delta, z, B, C, A, A_b, D, delta_bias, x_ck, x_lane, dims,
                  _scan_cm_flags(delta_softplus, reverse, generic, rowpair, accumulate_into is not None))
    a.out, a.out_pre, a.last_state = _ptr(out), _ptr(out_pre), _ptr(last)
    a.out_bs, a.out_ds = out.stride(0), out.stride(1)
    _launch(lib.c.aum_selective_scan_fwd, a, u, lib, "scan_fwd_bidir" if A_b is not None else "scan_fwd",
            (batch, dim, length, dstate, u.element_size(), want_out_pre))
    return out, out_pre, last


def scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out_pre, delta_softplus=False, reverse=False, A_b=None,
             dz_out=None, dmajor=False, generic=False, rowpair=False, x_ck=None, accumulate_into=None, x_lane=None, lib=None):
    """selective_scan_cuda.bwd.  Returns dict(du, ddelta, dA, dA_b, dB, dC, dD, dz, ddelta_bias); dB/dC fp32
    (batch, dstate, len).  dz_out: optional preallocated (possibly strided) tensor written in place (SSI:537-545).
    accumulate_into: the dict the other direction's call returned (long rows only, see scan_accumulates): this call adds its
    du, ddelta, dz, dB, dC, dD, ddelta_bias to those tensors and returns them, with its own dA."""
    lib = lib or get()
    B, C, dims = _scan_cm_rows(lib, u, delta, z, B, C, A, (("dout", dout), ("out_pre", out_pre)))
    batch, dim, length, dstate = dims
    if dout is None or (z is not None and out_pre is None):
        raise RuntimeError("dout is required, and out_pre (the forward's pre-gate sum) when z is given")
    _check_scan_ck(lib, x_ck, x_lane, dims, A_b is not None)
    dev = u.device
    A, A_b, D, delta_bias = _f32c(A), _f32c(A_b), _f32c(D), _f32c(delta_bias)
    acc = accumulate_into
    if acc and A_b is not None:
        raise RuntimeError("accumulate_into: one direction per call adds to the other's tensors, not the fused pair (A_b)")
    du = acc["du"] if acc else _alloc(batch, dim, length, u.dtype, dev, dmajor)
    ddelta = acc["ddelta"] if acc else _alloc(batch, dim, length, u.dtype, dev, dmajor)
    dz = None
    if z is not None:
        dz = acc["dz"] if acc else dz_out if dz_out is not None else _alloc(batch, dim, length, u.dtype, dev, dmajor)
        _unit(dz, "dz")
    f32 = dict(dtype=torch.float32, device=dev)
    # one zero-fill for all accumulate-into outputs (dA, dA_b, dD, ddelta_bias, dB, dC) instead of six
    nA, nBC = dim * dstate, batch * dstate * length
    sizes = [nA, nA if A_b is not None else 0, dim if D is not None and not acc else 0,
             dim if delta_bias is not None and not acc else 0, 0 if acc else nBC, 0 if acc else nBC]
    zbuf = torch.zeros((sum(sizes),), **f32)
    parts = torch.split(zbuf, sizes)
    dA = parts[0].view(dim, dstate)
    dA_b = parts[1].view(dim, dstate) if A_b is not None else None
    dD = parts[2] if D is not None else None
    dbias = parts[3] if delta_bias is not None else None
    dB = parts[4].view(batch, dstate, length) if not acc else None
    dC = parts[5].view(batch, dstate, length) if not acc else None
    if acc:      # the reduce stage of the call adds its partial sums to what is there
        dB, dC, dD, dbias = acc["dB"], acc["dC"], acc["dD"], acc["ddelta_bias"]
    ws_bytes = int(lib.c.aum_selective_scan_workspace_bytes(batch, dim, length, dstate, int(A_b is not None), 1))
    ws = torch.empty((max(ws_bytes, 4) // 4,), **f32) if ws_bytes else None
    a = ScanBwdArgs()
    _fill_scan_cm(a, u, delta, z, B, C, A, A_b, D, delta_bias, x_ck, x_lane, dims, _scan_cm_flags(delta_softplus, reverse, generic, rowpair, acc))
    a.dout, a.out_pre, a.du, a.ddelta, a.dz = map(_ptr, (dout, out_pre, du, ddelta, dz))
    a.dA, a.dA_b, a.dB, a.dC, a.dD, a.ddelta_bias = map(_ptr, (dA, dA_b, dB, dC, dD, dbias))
    a.workspace, a.workspace_bytes = _ptr(ws), ws_bytes
    if z is not None:
        a.out_bs, a.out_ds = out_pre.stride(0), out_pre.stride(1)
        a.dz_bs, a.dz_ds = dz.stride(0), dz.stride(1)
    a.dout_bs, a.dout_ds = dout.stride(0), dout.stride(1)
    a.du_bs, a.du_ds = du.stride(0), du.stride(1)
    a.ddelta_bs, a.ddelta_ds = ddelta.stride(0), ddelta.stride(1)
    a.dB_bs, a.dB_ns, a.dC_bs, a.dC_ns = dB.stride(0), dB.stride(1), dC.stride(0), dC.stride(1)
    _launch(lib.c.aum_selective_scan_bwd, a, u, lib, "scan_bwd_bidir" if A_b is not None else "scan_bwd",
            (batch, dim, length, dstate, u.element_size(), True))
    return dict(du=du, ddelta=ddelta, dA=dA, dA_b=dA_b, dB=dB, dC=dC, dD=dD, dz=dz, ddelta_bias=dbias)


# ---- time-serial scan on token-major activations (aum_scan_tm_*, ABI 7) -------------------------------------------------
SCAN_TM_CK = 8


def scan_tm_supported(dim, dstate):
    """the limits of aum_scan_tm_fwd / _bwd (include/aum_hip.h); outside them callers use scan_fwd / scan_bwd"""
    return dstate == 16 and dim % 64 == 0


def _tm3(t, name, last):
    """(batch, len, X) tensor with unit stride along X -> (batch stride, token stride) in elements"""
    if t.dim() != 3 or t.shape[2] != last or (t.stride(2) != 1 and last != 1):
        raise RuntimeError(f"{name}: expected (batch, len, {last}) with the last axis contiguous (token-major)")
    ts = t.stride(1) if t.shape[1] > 1 else last                # the stride of a size-1 axis is arbitrary: normalise
    bs = t.stride(0) if t.shape[0] > 1 else ts * t.shape[1]
    return bs, ts


def _tm2(t, name, last):
    """(total, X) packed rows with unit stride along X -> row stride in elements"""
    if t.dim() != 2 or t.shape[1] != last or (t.stride(1) != 1 and last != 1):
        raise RuntimeError(f"{name}: expected (total, {last}) with the last axis contiguous (packed token-major rows)")
    return t.stride(0) if t.shape[0] > 1 else last


# the row operands of a token-major scan as _scan_rows took them: ops (u, delta, z, B, C); lead (batch, len), or (total,) for packed rows; es bytes
# per element; strides per operand in elements, (batch stride, row stride) or for packed rows the row stride alone, 0s for an absent z
_ScanRows = typing.NamedTuple("_ScanRows", [("ops", tuple), ("lead", tuple), ("dim", int), ("dstate", int), ("es", int), ("strides", list)])


def _scan_rows(u, delta, z, B, C, dstate, strict=False, pad=0, activated=False):
    """THE operand rule of the token-major scans, for (batch, len, X) and packed (total, X) rows -> (_ScanRows, None), or (None, (clause,
    operand, message)) where it refuses; callers raise the message, or one of their own for the clause.  Every binding: u of a dtype the
    kernels have, delta / z / B / C of that dtype ("dtype"); every operand of u's rank, dim (u, delta, z) or dstate (B, C) columns of unit
    stride ("shape").  strict (the kernels that move rows as 16-byte chunks; the chunk kernels read element by element and take the rest):
    u's leading shape ("shape"); dim-wide rows at 16-byte addresses and strides, 16-bit B / C rows at 4-byte addresses and even strides
    ("align"); (row stride + pad) * es * rows < 2^31 with rows = len at pad 0 (the C check of fixed rows) or total at pad dim (that of
    packed rows) ("bound"); an activated delta only with 16-bit rows and z ("activated")."""
    packed = u.dim() == 2
    dim, dt = u.shape[-1], u.dtype
    ops = (("u", u, dim), ("delta", delta, dim), ("z", z, dim), ("B", B, dstate), ("C", C, dstate))
    if dt not in _DT:
        return None, ("dtype", "u", "u must be fp32, bf16 or fp16")
    if delta.dtype != dt or B.dtype != dt or C.dtype != dt or (z is not None and z.dtype != dt):
        name, t, _ = next(o for o in ops if o[1] is not None and o[1].dtype != dt)
        return None, ("dtype", name, f"{name} must have u's dtype ({dt}), got {t.dtype}")
    es = 4 if dt == torch.float32 else 2
    tm, none = (_tm2, 0) if packed else (_tm3, (0, 0))
    try:                                # every streaming call of a host loop over the blocks comes through here: the plain path is kept short
        strides = [none if t is None else tm(t, name, last) for name, t, last in ops]
    except RuntimeError as e:           # _tm2 / _tm3: not token-major rows of this rank and width; their message begins with the operand's name
        return None, ("shape", str(e).split(":")[0], str(e))
    if strict:
        for (name, t, last), st in zip(ops, strides):
            if t is None:
                continue
            bs, ts = (0, st) if packed else st
            if t.shape[:-1] != u.shape[:-1]:
                return None, ("shape", name, f"{name}: expected {tuple(u.shape[:-1]) + (last,)}, got {tuple(t.shape)}")
            if last == dim and (t.data_ptr() % 16 or (ts * es) % 16 or (bs * es) % 16):
                return None, ("align", name, f"{name}: rows are moved as 16-byte chunks")
            if last != dim and es == 2 and (t.data_ptr() % 4 or ts % 2 or bs % 2):
                return None, ("align", name, f"{name}: 16-bit B / C rows are read as dwords")
            if ts < 0 or (ts + pad) * es * u.shape[-2] >= 2 ** 31:
                return None, ("bound", name, f"{name}: row offsets are 32-bit byte cursors")
    if strict and activated and (es == 4 or z is None):
        return None, ("activated", "delta", "an activated delta is taken with 16-bit rows and z only")
    return _ScanRows((u, delta, z, B, C), (u.shape[0],) if packed else (u.shape[0], u.shape[1]), dim, dstate, es, strides), None


def _scan_flags(softplus, reverse, activated):
    return (SCAN_SOFTPLUS if softplus else 0) | (SCAN_REVERSE if reverse else 0) | (SCAN_DELTA_ACTIVATED if activated else 0)


def _fill_scan(a, rows, A, A_b, D, delta_bias, out, flags):
    """Writes what the token-major scan Args structs share into `a` (a struct, or the `base` of one): the row operands' pointers and strides
    (batch strides and batch / len where the rows have them, else total), the parameters as fp32 contiguous tensors, out (None: the struct
    has none), dim / dstate / dtype / flags.  Returns the converted parameters: the caller holds them until its launch is enqueued."""
    u, delta, z, B, C = rows.ops
    held = A, A_b, D, delta_bias = _f32c(A), _f32c(A_b), _f32c(D), _f32c(delta_bias)
    a.u, a.delta, a.z, a.B, a.C = _ptr(u), _ptr(delta), _ptr(z), _ptr(B), _ptr(C)
    a.A, a.D, a.delta_bias = _ptr(A), _ptr(D), _ptr(delta_bias)
    if A_b is not None:
        a.A_b = _ptr(A_b)
    if len(rows.lead) == 1:
        a.u_ts, a.delta_ts, a.z_ts, a.B_ts, a.C_ts = rows.strides
        a.total, = rows.lead
        if out is not None:
            a.out, a.out_ts = _ptr(out), _tm2(out, "out", rows.dim)
    else:
        (a.u_bs, a.u_ts), (a.delta_bs, a.delta_ts), (a.z_bs, a.z_ts), (a.B_bs, a.B_ts), (a.C_bs, a.C_ts) = rows.strides
        a.batch, a.len = rows.lead
        if out is not None:
            (a.out_bs, a.out_ts), a.out = _tm3(out, "out", rows.dim), _ptr(out)
    a.dim, a.dstate, a.dtype, a.flags = rows.dim, rows.dstate, _DT[u.dtype], flags
    return held


def _fill_map(a, m, nrows, pooled=True):
    """the sessions of a packed call: where they are in the stream, and (pooled) which of the `nrows` cache rows each owns"""
    a.cu_seqlens, a.state_indices = _ptr(m.cu), _ptr(m.idx) if pooled else None
    a.nseq, a.nrows = len(m.lens), nrows


def _scan_tm_ckpt_shape(lib, batch, length, dim, dstate, bidir, dtype):
    """THE size of the state checkpoint of scan_tm_fwd / _bwd: (directions, batch, nck, rows, dim) dwords -- fp32 states (rows = dstate)
    for fp32 activations, pairs of states in the activations' own type (rows = dstate / 2) for 16-bit ones"""
    rows = int(lib.c.aum_scan_tm_ckpt_rows(_DT[dtype])) if dstate == 16 else dstate
    return (2 if bidir else 1, batch, max(int(lib.c.aum_scan_tm_nck(length)), 1), rows, dim)


def _check_scan_tm_ckpt(lib, ckpt, *launch):
    if ckpt is None or ckpt.dtype != torch.float32 or not ckpt.is_contiguous():
        raise RuntimeError("ckpt: the contiguous fp32 tensor scan_tm_fwd filled")
    if ckpt.numel() < math.prod(_scan_tm_ckpt_shape(lib, *launch)):
        raise RuntimeError("ckpt too small for this launch")


def scan_tm_ckpt(batch, length, dim, dstate, bidir, device, lib=None, dtype=torch.float32):
    """empty state checkpoint (directions, batch, nck, rows, dim) dwords for scan_tm_fwd to fill and scan_tm_bwd to read; dtype = the
    activations' dtype: fp32 states (rows = dstate) for fp32, pairs of states in the activations' own type (rows = dstate / 2) for 16-bit activations"""
    return torch.empty(_scan_tm_ckpt_shape(lib or get(), batch, length, dim, dstate, bidir, dtype), dtype=torch.float32, device=device)


SCAN_TM_MAX_SEGMENTS = 32


def scan_tm_segments(batch, dim, length, bidir, training=False, nsimd=None, device=None):
    """time segments a token-major launch of this shape is cut into (1: not cut).  One wave per (batch entry, 64 channels, direction)
    leaves most SIMDs idle at a small batch while every wave walks the whole row; segments multiply the waves at the price of one
    carry pass (the recurrence once more, without outputs).  Rows are cut only when they are long (>= 1024 steps) and the uncut launch is
    under one wave per two SIMDs, into as many ranges as give every SIMD three waves per launch (each direction of a Fo-Bi pair is a
    launch of its own), ranges no shorter than 128 steps.  Measured at B = 8, L = 4097, E = 1536 (profiles/r04_seg_time.json): 16
    ranges are the fastest cut for the forward (three resident waves per SIMD: one round) AND for the backward (two resident: 11 or
    12 ranges leave a tail round, 16 is 1.5 rounds of shorter waves) -- 0.68 / 1.39 ms against 1.29 / 5.03 ms uncut."""
    nsimd = 4 * cu_count(device) if nsimd is None else nsimd          # MI355X: 256 CUs x 4 SIMDs; `device`: the operands' (default: current)
    per_dir = batch * (dim // 64)
    waves = per_dir * (2 if bidir else 1)
    if per_dir <= 0 or waves * 2 > nsimd or length < 1024:
        return 1
    want = -(-nsimd * 3 // per_dir)
    seg = min(want, length // 128, SCAN_TM_MAX_SEGMENTS)
    return seg if seg >= 2 else 1


def scan_tm_fwd(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, reverse=False, A_b=None,
                want_out_pre=False, ckpt=None, out=None, lib=None, segments=1, delta_activated=False):
    """Selective scan forward on token-major tensors: u, delta, z (batch, len, dim) with channels contiguous (row strides free: z
    may be a slice of an xz tensor); B, C (batch, len, dstate) in u's dtype.  A_b != None: both directions (Fo-Bi).
    segments > 1: the rows are cut into that many time ranges that run as waves of their own (aum_scan_tm_seg_fwd).
    delta_activated: delta already holds softplus(raw + delta_bias) (AUM_SCAN_DELTA_ACTIVATED; 16-bit with z only): used as it is.
    Returns (out, out_pre|None), both (batch, len, dim) contiguous."""
    lib = lib or get()
    (batch, length, dim), dstate = u.shape, A.shape[1]
    for t in (u, delta, z, B, C):
        lib.check_tensor(t)
    rows, why = _scan_rows(u, delta, z, B, C, dstate)
    if why:
        raise RuntimeError(why[2] if why[0] != "dtype" else "B, C must have u's dtype" if why[1] in "BC" else
                           "u, delta, z must share one dtype in {fp32, bf16, fp16}")
    if out is None:
        out = torch.empty((batch, length, dim), dtype=u.dtype, device=u.device)
    out_pre = torch.empty((batch, length, dim), dtype=u.dtype, device=u.device) if want_out_pre else None
    a = ScanTmFwdArgs()
    _held = _fill_scan(a, rows, A, A_b, D, delta_bias, out, _scan_flags(delta_softplus, reverse, delta_activated))
    if out_pre is not None:
        (a.pre_bs, a.pre_ts), a.out_pre = _tm3(out_pre, "out_pre", dim), _ptr(out_pre)
    if ckpt is not None:
        _check_scan_tm_ckpt(lib, ckpt, batch, length, dim, dstate, A_b is not None, u.dtype)
        lib.check_tensor(ckpt)
        a.ckpt = _ptr(ckpt)
    if segments > 1:
        sa = ScanTmSegFwdArgs()
        sa.base, sa.segments = a, int(segments)
        sa.carry_bytes = int(lib.c.aum_scan_tm_seg_carry_bytes(batch, dim, length, dstate, int(A_b is not None), int(segments)))
        if sa.carry_bytes <= 0:
            raise RuntimeError(f"scan_tm_fwd: segments={segments} not supported for this shape")
        carry = torch.empty((sa.carry_bytes // 4,), dtype=torch.float32, device=u.device)
        sa.carry = _ptr(carry)
        _launch(lib.c.aum_scan_tm_seg_fwd, sa, u, lib, "scan_tm_seg_fwd_bidir" if A_b is not None else "scan_tm_seg_fwd",
                (batch, dim, length, dstate, u.element_size(), want_out_pre, int(segments)))
    else:
        _launch(lib.c.aum_scan_tm_fwd, a, u, lib, "scan_tm_fwd_bidir" if A_b is not None else "scan_tm_fwd",
                (batch, dim, length, dstate, u.element_size(), want_out_pre))
    return out, out_pre


def scan_state_supported(t, batch, dim, dstate):
    """a state of aum_scan_tm_fwd_state: None, or fp32 contiguous (batch, dim, dstate), 16-byte aligned"""
    return t is None or (t.dim() == 3 and tuple(t.shape) == (batch, dim, dstate) and t.dtype == torch.float32 and t.is_contiguous()
                         and t.data_ptr() % 16 == 0)


def scan_tm_fwd_state_supported(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False,
                                state_in=None, state_out=None, segments=1):
    """the limits of aum_scan_tm_fwd_state (include/aum_hip.h): those of scan_tm_fwd for one direction -- dstate == 16, dim % 64 == 0,
    (batch, len >= 1, dim) token-major rows of one dtype moved as 16-byte chunks, B / C rows 4-byte aligned, an activated delta only
    for 16-bit rows with z -- and the states fp32 contiguous (batch, dim, 16), 16-byte aligned.  Outside them callers use scan_stream."""
    if u.dim() != 3 or A.dim() != 2 or u.shape[1] < 1 or not scan_tm_supported(u.shape[2], A.shape[1]) or u.dtype not in _DT:
        return False
    (batch, length, dim), dstate = u.shape, A.shape[1]
    if (not (1 <= int(segments) <= SCAN_TM_MAX_SEGMENTS) or A.shape[0] != dim
            or _scan_rows(u, delta, z, B, C, dstate, strict=True, activated=delta_activated)[0] is None):
        return False
    return scan_state_supported(state_in, batch, dim, dstate) and scan_state_supported(state_out, batch, dim, dstate)


def scan_tm_fwd_state(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, state_in=None,
                      state_out=None, segments=1, out=None, lib=None):
    """scan_tm_fwd for one direction, entered with a carried state and leaving the state behind the last step (aum_scan_tm_fwd_state):
    the prefill of a streaming session at the speed of the offline forward, continued by scan_tm_chunk / stream_block on the same cache
    row.  Operands as scan_tm_fwd; state_in / state_out: fp32 contiguous (batch, dim, 16) or None (a zero entry state / the exit state
    is not wanted), and they may be ONE tensor (advance in place).  segments > 1: the rows cut into time ranges (scan_tm_segments
    chooses).  Uncut, the result does not depend on how a stream is cut into calls (bitwise); with state_in None `out` is bit for bit
    scan_tm_fwd's.  Inference only: no checkpoints, no backward.  Returns out (batch, len, dim) contiguous in u's dtype."""
    lib = lib or get()
    for t in (u, delta, z, B, C, state_in, state_out, out):
        lib.check_tensor(t)
    if not scan_tm_fwd_state_supported(u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, state_in, state_out, segments):
        raise RuntimeError(f"scan_tm_fwd_state: unsupported operands u {tuple(u.shape)} {u.dtype} strides {u.stride()}, A {tuple(A.shape)}, state_in "
                           f"{None if state_in is None else (tuple(state_in.shape), state_in.dtype)}, state_out "
                           f"{None if state_out is None else (tuple(state_out.shape), state_out.dtype)}, segments {segments} "
                           "(need token-major 16-byte rows of one dtype, dim % 64 == 0, dstate 16, fp32 contiguous (batch, dim, 16) states)")
    (batch, length, dim), dstate = u.shape, A.shape[1]
    if out is None:
        out = torch.empty((batch, length, dim), dtype=u.dtype, device=u.device)
    if out.dtype != u.dtype or tuple(out.shape) != (batch, length, dim):
        raise RuntimeError("scan_tm_fwd_state: out must have u's shape and dtype")
    sa = ScanTmFwdStateArgs()
    _held = _fill_scan(sa.base, _scan_rows(u, delta, z, B, C, dstate)[0], A, None, D, delta_bias, out, _scan_flags(delta_softplus, False, delta_activated))
    for t in _held:
        lib.check_tensor(t)
    sa.state_in, sa.state_out, sa.segments = _ptr(state_in), _ptr(state_out), int(segments)
    if segments > 1:
        sa.carry_bytes = int(lib.c.aum_scan_tm_seg_carry_bytes(batch, dim, length, dstate, 0, int(segments)))
        carry = torch.empty((sa.carry_bytes // 4,), dtype=torch.float32, device=u.device)
        sa.carry = _ptr(carry)
    _launch(lib.c.aum_scan_tm_fwd_state, sa, u, lib, "scan_tm_fwd_state", (batch, dim, length, dstate, u.element_size(), int(segments)))
    return out


def scan_tm_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out_pre, ckpt, delta_softplus=False, reverse=False, A_b=None, dz_out=None,
                lib=None, segments=1, want_dA_xA=False, param_out=None, delta_activated=False):
    """Backward of scan_tm_fwd (same tensor conventions; ckpt: the tensor scan_tm_fwd filled).  Returns dict(du, ddelta, dz (batch, len,
    dim) in u's dtype, dBC (batch, len, 2 * dstate) fp32 = dB | dC, dA, dA_b (dim, dstate), dD, ddelta_bias (dim) fp32).
    delta_activated: delta holds softplus(raw + delta_bias); ddelta and ddelta_bias are still the gradients with respect to raw and the
    bias (ddelta_bias whenever delta_bias is given)."""
    lib = lib or get()
    (batch, length, dim), dstate = u.shape, A.shape[1]
    dev = u.device
    for t in (u, delta, z, B, C, dout, out_pre, ckpt):
        lib.check_tensor(t)
    # the kernel is told ONE element type: a tensor of another one would be read past its end (e.g. a 16-bit dout under fp32 rows)
    rows, why = _scan_rows(u, delta, z, B, C, dstate)
    if why and why[0] == "dtype":
        raise RuntimeError(why[2])
    for name, t in (("dout", dout), ("out_pre", out_pre), ("dz_out", dz_out)):
        if t is not None and t.dtype != u.dtype:
            raise RuntimeError(f"{name} must have u's dtype ({u.dtype}), got {t.dtype}")
    for name, t in (("delta", delta), ("z", z), ("dout", dout), ("out_pre", out_pre), ("dz_out", dz_out)):
        if t is not None and tuple(t.shape) != (batch, length, dim):
            raise RuntimeError(f"{name}: expected shape {(batch, length, dim)}, got {tuple(t.shape)}")
    if z is not None and out_pre is None:
        raise RuntimeError("out_pre (the forward's pre-gate sum) is required when z is given")
    bidir = A_b is not None
    _check_scan_tm_ckpt(lib, ckpt, batch, length, dim, dstate, bidir, u.dtype)
    if why:
        raise RuntimeError(why[2])
    new = lambda: torch.empty((batch, length, dim), dtype=u.dtype, device=dev)
    du, ddelta = new(), new()
    dz = None if z is None else dz_out if dz_out is not None else new()
    f32 = dict(dtype=torch.float32, device=dev)
    dBC = torch.empty((batch, length, 2 * dstate), **f32)
    # param_out: {"dD" | "ddelta_bias" | "dA_xA" | "dA_b_xA": destination} -- where a parameter's gradient is wanted (its bucket view under
    # DistributedDataParallel); anything missing or unfit is a new tensor
    po = param_out or {}
    dA = torch.empty((dim, dstate), **f32)
    dA_b = torch.empty((dim, dstate), **f32) if bidir else None
    dD = _sum_out(po.get("dD"), (dim,), dev) if D is not None else None
    dbias = _sum_out(po.get("ddelta_bias"), (dim,), dev) if delta_bias is not None else None
    # want_dA_xA: dA .* A (and dA_b .* A_b) from the same partial-sum launch -- the gradient of A_log where A = -exp(A_log)
    dA_xA = _sum_out(po.get("dA_xA"), (dim, dstate), dev) if want_dA_xA else None
    dA_b_xA = _sum_out(po.get("dA_b_xA"), (dim, dstate), dev) if want_dA_xA and bidir else None
    if segments > 1:
        ws_bytes = int(lib.c.aum_scan_tm_seg_workspace_bytes(batch, dim, length, dstate, int(bidir), int(segments)))
        if ws_bytes <= 0:
            raise RuntimeError(f"scan_tm_bwd: segments={segments} not supported for this shape")
    else:
        ws_bytes = int(lib.c.aum_scan_tm_workspace_bytes(batch, dim, length, dstate, int(bidir)))
    ws = torch.empty((max(ws_bytes, 4) // 4,), **f32)
    a = ScanTmBwdArgs()
    _held = _fill_scan(a, rows, A, A_b, D, delta_bias, None, _scan_flags(delta_softplus, reverse, delta_activated))
    a.dout, a.out_pre, a.ckpt, a.du, a.ddelta, a.dz = map(_ptr, (dout, out_pre, ckpt, du, ddelta, dz))
    a.dA, a.dA_b, a.dBC, a.dD, a.ddelta_bias, a.dA_xA, a.dA_b_xA = map(_ptr, (dA, dA_b, dBC, dD, dbias, dA_xA, dA_b_xA))
    a.workspace, a.workspace_bytes = _ptr(ws), ws_bytes
    a.dout_bs, a.dout_ts = _tm3(dout, "dout", dim)
    a.du_bs, a.du_ts = _tm3(du, "du", dim)
    a.ddelta_bs, a.ddelta_ts = _tm3(ddelta, "ddelta", dim)
    if z is not None:
        a.pre_bs, a.pre_ts = _tm3(out_pre, "out_pre", dim)
        a.dz_bs, a.dz_ts = _tm3(dz, "dz", dim)
    if segments > 1:
        sa = ScanTmSegBwdArgs()
        sa.base, sa.segments = a, int(segments)
        _launch(lib.c.aum_scan_tm_seg_bwd, sa, u, lib, "scan_tm_seg_bwd_bidir" if bidir else "scan_tm_seg_bwd",
                (batch, dim, length, dstate, u.element_size(), True, int(segments)))
    else:
        _launch(lib.c.aum_scan_tm_bwd, a, u, lib, "scan_tm_bwd_bidir" if bidir else "scan_tm_bwd", (batch, dim, length, dstate, u.element_size(), True))
    return dict(du=du, ddelta=ddelta, dz=dz, dBC=dBC, dA=dA, dA_b=dA_b, dD=dD, ddelta_bias=dbias, dA_xA=dA_xA, dA_b_xA=dA_b_xA, _ws=ws)


GEMM_BN, GEMM_BK = 256, 64


_dev_cu = {}


def cu_count(device=None):
    """compute units of the device the kernels run on (MI355X: 256; a partitioned or different part reports its own) -- the host-side
    dispatch rules (time segments, token splits) are stated in CUs / SIMDs and must agree with what the library sees (csrc: cu_count())"""
    if not torch.cuda.is_available():
        return 256
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    n = _dev_cu.get(idx)
    if n is None:
        n = _dev_cu[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return n


def gemm_wgrad_splits(n, k, ncu=None, device=None):
    """token splits that give every CU one workgroup: (n / 256) (k / 256) output tiles x splits ~ the CU count"""
    ncu = cu_count(device) if ncu is None else ncu
    tiles = (n // 256) * max(1, k // 256)          # a skinny operand (k = 48 / 80, 24 / 56) is one column tile
    return max(1, min(64, ncu // max(tiles, 1)))


WGRAD_SKINNY_K = (48, 80, 24, 56)        # dt_rank and dt_rank + 2 d_state of AuM-Base and AuM-Small


def gemm_wgrad_supported(y, x, splits=None):
    """shapes aum_gemm_wgrad takes (include/aum_hip.h, ABI 10; the C side's gemm_wgrad_check, rule for rule): 16-bit 2-D token-major
    operands (rows = tokens, unit column stride), y's width a multiple of 256, x's a multiple of 256 or one of the skinny widths 48 / 80 (AuM-Base) and
    24 / 56 (AuM-Small), at most 64 token splits, and a split's rows within 32-bit byte offsets of both operands"""
    if not (y.dim() == 2 and x.dim() == 2 and y.dtype == x.dtype and y.dtype in (torch.bfloat16, torch.float16) and y.shape[0] == x.shape[0]
            and y.stride(1) == 1 and x.stride(1) == 1 and y.shape[1] % 256 == 0 and (x.shape[1] % 256 == 0 or x.shape[1] in WGRAD_SKINNY_K)
            and y.stride(0) % 8 == 0 and y.stride(0) >= y.shape[1] and x.stride(0) >= x.shape[1]
            and x.stride(0) % 8 == 0 and y.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and y.shape[0] > 0):
        return False
    splits = splits or gemm_wgrad_splits(y.shape[1], x.shape[1], device=y.device if y.is_cuda else None)
    if not 0 < splits <= 64:
        return False
    chunk = (-(-y.shape[0] // splits) + 63) // 64 * 64
    return chunk * y.stride(0) * 2 < (1 << 31) and chunk * x.stride(0) * 2 < (1 << 31)


def gemm_wgrad(y, x, splits=None, lib=None, partials=False, out=None):
    """dW (n, k) fp32 = y (t, n)^T @ x (t, k): the weight gradient of a projection from token-major operands (aum_gemm_wgrad: hand-written
    MFMA kernel with transposing LDS reads, fp32 partial tiles over `splits` token ranges summed in a fixed order by aum_sum_rows)."""
    lib = lib or get()
    t, n = y.shape
    k = x.shape[1]
    splits = splits or gemm_wgrad_splits(n, k, device=y.device if y.is_cuda else None)
    if not gemm_wgrad_supported(y, x, splits):
        raise RuntimeError("gemm_wgrad: operands outside the kernel's limits (see gemm_wgrad_supported)")
    lib.check_tensor(y)
    lib.check_tensor(x)
    part = torch.empty((splits, n, k), dtype=torch.float32, device=y.device)
    a = GemmWArgs()
    a.y, a.x, a.part = _ptr(y), _ptr(x), _ptr(part)
    a.t, a.ldy, a.ldx, a.n, a.k, a.splits, a.dtype = t, y.stride(0), x.stride(0), n, k, splits, _DT[y.dtype]
    _launch(lib.c.aum_gemm_wgrad, a, y, lib, "gemm_wgrad", (t, n, k, y.element_size()))
    if partials:
        return part
    if splits == 1:
        return part[0] if out is None else sum_rows(part, lib=lib, out=out)
    return sum_rows(part, lib=lib, out=out)


def gemm_tn_supported(a, b):
    """shapes aum_gemm_tn takes (include/aum_hip.h, ABI 9): 16-bit 2-D operands with contiguous K, n % 256 == 0, k % 64 == 0"""
    if a.dim() != 2 or b.dim() != 2 or a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        return False
    m, k = a.shape
    n = b.shape[0]
    return (b.shape[1] == k and m > 0 and n % GEMM_BN == 0 and k % GEMM_BK == 0 and a.stride(1) == 1 and b.stride(1) == 1
            and a.stride(0) % 8 == 0 and b.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
            and 512 * a.stride(0) < 2 ** 31 and 512 * b.stride(0) < 2 ** 31)


GEMM_LOCKSTEP, GEMM_PIPELINED, GEMM_PACED = 1, 32, 256


def gemm_tn(a, b, out=None, lib=None, flags=0):
    """out[m][n] = sum_k a[m][k] b[n][k]: the in_proj / out_proj GEMM and their data gradients on token-major activations (MS:185-189,
    SSI:517, 540).  a (m, k), b (n, k): 16-bit, K contiguous; out (m, n) rows contiguous (may be a column block of a wider tensor).
    flags: 0 (the library picks: the paced-store kernel from k = 448 on) or one of GEMM_LOCKSTEP / GEMM_PIPELINED / GEMM_PACED."""
    lib = lib or get()
    lib.check_tensor(a)
    lib.check_tensor(b)
    if not gemm_tn_supported(a, b):
        raise RuntimeError(f"gemm_tn: unsupported operands {tuple(a.shape)} {a.dtype} x {tuple(b.shape)} {b.dtype} (need 16-bit, contiguous K, "
                           "n % 256 == 0, k % 64 == 0, 16-byte aligned rows)")
    m, k = a.shape
    n = b.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    elif (out.shape != (m, n) or out.dtype != a.dtype or out.stride(1) != 1 or out.stride(0) % 8 or out.data_ptr() % 16
          or out.device != a.device):
        raise RuntimeError("gemm_tn: out must be an (m, n) tensor of the operands' dtype with contiguous, 16-byte aligned rows")
    g = GemmArgs()
    g.a, g.b, g.c = _ptr(a), _ptr(b), _ptr(out)
    g.m, g.n, g.k, g.lda, g.ldb, g.ldc, g.dtype = m, n, k, a.stride(0), b.stride(0), out.stride(0), _DT[a.dtype]
    g.flags = flags
    _launch(lib.c.aum_gemm_tn, g, a, lib, "gemm_tn", (m, n, k))
    return out


def conv1d_update(x, conv_state, weight, bias=None, silu=True, lib=None):
    """one token of the causal conv (aum_causal_conv1d_update): x (batch, dim); conv_state (batch, dim, width) fp32 contiguous, shifted and
    extended IN PLACE; weight (dim, width); returns act(<window, weight> + bias) (batch, dim) in x's dtype"""
    lib = lib or get()
    if x.dim() != 2 or conv_state.dim() != 3 or conv_state.shape[:2] != x.shape or conv_state.dtype != torch.float32 or not conv_state.is_contiguous():
        raise RuntimeError("conv1d_update: x (batch, dim), conv_state (batch, dim, width) fp32 contiguous")
    for t in (x, conv_state):
        lib.check_tensor(t)
    x = x.contiguous()
    weight, bias = _conv_weights(weight, bias, x.shape[1], False)
    out = torch.empty_like(x)
    a = ConvUpdateArgs()
    a.x, a.conv_state, a.weight, a.bias, a.out = _ptr(x), _ptr(conv_state), _ptr(weight), _ptr(bias), _ptr(out)
    a.batch, a.dim, a.width, a.dtype, a.flags = x.shape[0], x.shape[1], conv_state.shape[2], _DT[x.dtype], _conv_flags(silu)
    _launch(lib.c.aum_causal_conv1d_update, a, x, lib, "conv1d_update")
    return out


def state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, lib=None):
    """one token of the selective scan (aum_selective_state_update): state (batch, dim, dstate) fp32 contiguous, advanced IN PLACE;
    x, dt, z (batch, dim), B, C (batch, dstate) in one dtype; A (dim, dstate), D, dt_bias (dim); returns (batch, dim) in x's dtype"""
    lib = lib or get()
    if state.dim() != 3 or state.dtype != torch.float32 or not state.is_contiguous() or x.shape != state.shape[:2]:
        raise RuntimeError("state_update: state (batch, dim, dstate) fp32 contiguous, x (batch, dim)")
    for t in (state, x, dt, z, B, C):
        lib.check_tensor(t)
    dty = x.dtype
    x, dt, B, C = x.contiguous(), dt.to(dty).contiguous(), B.to(dty).contiguous(), C.to(dty).contiguous()
    z = None if z is None else z.to(dty).contiguous()
    if dt.shape != x.shape or B.shape != (x.shape[0], state.shape[2]) or C.shape != B.shape or (z is not None and z.shape != x.shape):
        raise RuntimeError("state_update: dt, z (batch, dim); B, C (batch, dstate)")
    A, D, dt_bias = _f32c(A), _f32c(D), _f32c(dt_bias)
    out = torch.empty_like(x)
    a = StateUpdateArgs()
    a.state, a.x, a.dt, a.z, a.B, a.C = _ptr(state), _ptr(x), _ptr(dt), _ptr(z), _ptr(B), _ptr(C)
    a.A, a.D, a.dt_bias, a.out = _ptr(A), _ptr(D), _ptr(dt_bias), _ptr(out)
    a.batch, a.dim, a.dstate, a.dtype, a.flags = x.shape[0], x.shape[1], state.shape[2], _DT[dty], _scan_flags(dt_softplus, False, False)
    _launch(lib.c.aum_selective_state_update, a, x, lib, "state_update")
    return out


# ---- streaming inference, T tokens per launch: fixed batch (aum_*_tm_chunk) or packed sessions (aum_*_tm_chunk_var), which differ in addressing
# only: one filler per operator (_fill_conv, _fill_scan) writes either struct, the packed forms add their map (_fill_map)
def _stream_ok(cache, x, scan):
    """x a token-major (batch, T >= 1, dim) view, cache fp32 contiguous (., dim, .), of a dim / dstate / width the operator's kernels take"""
    if not (cache.dim() == 3 and cache.dtype == torch.float32 and cache.is_contiguous() and x.dim() == 3 and x.shape[1] >= 1
            and cache.shape[1] == x.shape[2]):
        return False
    if scan:            # the state is read with 16-byte accesses
        return cache.data_ptr() % 16 == 0 and x.dtype in _DT and scan_tm_supported(x.shape[2], cache.shape[2])
    return conv1d_tm_supported(x, cache.shape[2])


def conv1d_tm_chunk_supported(x, conv_state):
    """the limits of aum_conv1d_tm_chunk (include/aum_hip.h): a token-major (batch, T, dim) view as conv1d_tm_fwd takes it, an fp32
    contiguous (batch, dim, width <= 4) cache; outside them callers use conv1d_update token by token"""
    return _stream_ok(conv_state, x, False) and conv_state.shape[0] == x.shape[0]


def scan_tm_chunk_supported(state, u):
    """the limits of aum_scan_tm_chunk (include/aum_hip.h): fp32 contiguous (batch, dim, 16) state, dim % 64 == 0, (batch, T, dim)
    activations; outside them callers use state_update token by token"""
    return _stream_ok(state, u, True) and state.shape[0] == u.shape[0]


def conv1d_tm_chunk_var_supported(x, conv_state):
    """the limits of aum_conv1d_tm_chunk_var (include/aum_hip.h): packed (total >= 1, dim) rows as conv1d_tm_chunk takes them at batch 1, an
    fp32 contiguous (nrows, dim, width <= 4) pool; outside them callers loop over the sessions through conv1d_tm_chunk / conv1d_update"""
    return x.dim() == 2 and _stream_ok(conv_state, x.unsqueeze(0), False) and conv_state.shape[0] >= 1


def scan_tm_chunk_var_supported(state, u):
    """the limits of aum_scan_tm_chunk_var (include/aum_hip.h): an fp32 contiguous (nrows, dim, 16) pool, dim % 64 == 0, packed
    (total >= 1, dim) activations; outside them callers loop over the sessions through scan_tm_chunk / state_update"""
    return u.dim() == 2 and _stream_ok(state, u.unsqueeze(0), True) and state.shape[0] >= 1


def _conv_chunk_operands(a, name, lib, x, conv_state, weight, bias, silu, out):
    """Fills what the conv's streaming Args structs share -- ConvTmChunkArgs (batch, T, dim) rows, the packed ConvTmChunkVarArgs and
    ConvTmPrefillVarArgs (total, dim) rows -- through _fill_conv; returns y (out, or allocated) and the converted operands."""
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device) if out is None else out
    if y.dtype != x.dtype or y.shape != x.shape:
        raise RuntimeError(f"{name}: out must have x's shape and dtype")
    held = _fill_conv(a, x, conv_state, weight, bias, y, _conv_flags(silu))
    if a.width != conv_state.shape[2]:
        raise RuntimeError(f"{name}: weight (dim, width) and conv_state (rows, dim, width) disagree on the width")
    for t in held:
        lib.check_tensor(t)
    return y, held                       # the converted operands: the caller holds them until its launch is enqueued


def _fill_conv(a, x, conv_state, weight, bias, y, flags):
    """The conv counterpart of _fill_scan: x / y pointers and strides (batch strides and batch / len, or total for packed rows), the cache,
    weight (dim, width) and bias as fp32 16-byte aligned tensors, dim / width / dtype / flags.  Returns the converted weight and bias."""
    dim = x.shape[-1]
    held = weight, bias = _conv_weights(weight, bias, dim, True)
    a.x, a.conv_state, a.weight, a.bias, a.y = _ptr(x), _ptr(conv_state), _ptr(weight), _ptr(bias), _ptr(y)
    if x.dim() == 2:
        a.x_ts, a.y_ts, a.total = _tm2(x, "x", dim), _tm2(y, "out", dim), x.shape[0]
    else:
        a.x_bs, a.x_ts = _tm3(x, "x", dim)
        a.y_bs, a.y_ts = _tm3(y, "y", dim)
        a.batch, a.len = x.shape[0], x.shape[1]
    a.dim, a.width, a.dtype, a.flags = dim, weight.shape[1], _DT[x.dtype], flags
    return held


def _scan_chunk_operands(a, name, lib, state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out):
    """Fills what the scan's streaming Args structs share -- ScanTmChunkArgs (batch, T, dim) rows, the packed ScanTmChunkVarArgs and
    ScanTmFwdStateVarArgs (total, dim) rows -- through _scan_rows and _fill_scan; returns out (given, or allocated) and the converted operands."""
    dim, dstate = u.shape[-1], state.shape[2]
    rows, why = _scan_rows(u, delta, z, B, C, dstate)
    if why and why[0] == "dtype":
        raise RuntimeError(f"{name}: u, delta, z, B, C must share one dtype")
    if A.shape != (dim, dstate):
        raise RuntimeError(f"{name}: A must be (dim, dstate)")
    if out is None:
        out = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    if out.dtype != u.dtype or out.shape != u.shape:
        raise RuntimeError(f"{name}: out must have u's shape and dtype")
    if why:
        raise RuntimeError(why[2])
    A, _, D, delta_bias = _fill_scan(a, rows, A, None, D, delta_bias, out, _scan_flags(delta_softplus, False, delta_activated))
    for t in (A, D, delta_bias):
        lib.check_tensor(t)
    a.state = _ptr(state)
    return out, (A, D, delta_bias)       # the converted operands: the caller holds them until its launch is enqueued


def conv1d_tm_chunk(x, conv_state, weight, bias=None, silu=True, lib=None):
    """T tokens of the causal conv in one launch (aum_conv1d_tm_chunk) = T conv1d_update calls: x (batch, T, dim) token-major view (may be
    the first half of in_proj output rows); conv_state (batch, dim, width) fp32 contiguous, advanced IN PLACE; weight (dim, width);
    returns y (batch, T, dim) contiguous in x's dtype.  The result does not depend on how a stream is cut into calls (bitwise)."""
    lib = lib or get()
    for t in (x, conv_state):
        lib.check_tensor(t)
    if not conv1d_tm_chunk_supported(x, conv_state):
        raise RuntimeError(f"conv1d_tm_chunk: unsupported operands x {tuple(x.shape)} {x.dtype} strides {x.stride()}, conv_state "
                           f"{tuple(conv_state.shape)} {conv_state.dtype} (need (batch, T, dim) token-major, 16-byte rows; fp32 contiguous (batch, dim, width <= 4))")
    batch, length, dim = x.shape
    a = ConvTmChunkArgs()
    y, _held = _conv_chunk_operands(a, "conv1d_tm_chunk", lib, x, conv_state, weight, bias, silu, None)
    _launch(lib.c.aum_conv1d_tm_chunk, a, x, lib, "conv_tm_chunk", (batch, dim, length, x.element_size()))
    return y


def scan_tm_chunk(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, out=None, lib=None):
    """T tokens of the selective scan in one launch (aum_scan_tm_chunk) = T state_update calls: state (batch, dim, dstate) fp32 contiguous,
    advanced IN PLACE; u, delta, z (batch, T, dim) token-major views (row strides free: u / z may be the halves of xz rows), B, C
    (batch, T, dstate) views (column blocks of the x_dbl rows) in u's dtype.  delta_activated: delta already holds
    softplus(raw + delta_bias) (xdt_tm_fwd(..., delta_softplus=True)).  Returns (batch, T, dim) contiguous in u's dtype.  The result does
    not depend on how a stream is cut into calls (bitwise)."""
    lib = lib or get()
    for t in (state, u, delta, z, B, C, out):
        lib.check_tensor(t)
    if not scan_tm_chunk_supported(state, u):
        raise RuntimeError(f"scan_tm_chunk: unsupported operands state {tuple(state.shape)} {state.dtype}, u {tuple(u.shape)} {u.dtype} "
                           "(need fp32 contiguous (batch, dim, 16), dim % 64 == 0, u (batch, T, dim))")
    batch, length, dim = u.shape
    a = ScanTmChunkArgs()
    out, _held = _scan_chunk_operands(a, "scan_tm_chunk", lib, state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out)
    _launch(lib.c.aum_scan_tm_chunk, a, u, lib, "scan_tm_chunk", (batch, dim, length, state.shape[2], u.element_size()))
    return out


class SeqMap(typing.NamedTuple):
    """Where the sessions of one packed call are (seq_map builds it): session i owns rows [sum(lens[:i]), sum(lens[:i + 1])) of the
    (total, dim) token stream and row rows[i] of the pool of caches.  lens, rows: host tuples; cu (nseq + 1) / idx (nseq, or None: session
    i owns row i) the same as int32 device tensors, what the kernels read."""
    lens: tuple
    rows: tuple
    total: int
    cu: torch.Tensor
    idx: typing.Optional[torch.Tensor]


def seq_map(seq_lens, state_indices=None, *, device):
    """Built once per push and handed to every layer: the per-session row counts (>= 0) and the cache row of each session (distinct, >= 0;
    None: session i owns row i) -- checked here, on the host, and sent to `device` in ONE pinned, non-blocking upload.  That the rows exist
    is checked where a cache is known (check_seq_map)."""
    lens = tuple(int(n) for n in seq_lens)
    if not lens or min(lens) < 0:
        raise ValueError(f"seq_map: one length >= 0 per session, got {lens}")
    rows = tuple(range(len(lens))) if state_indices is None else tuple(int(r) for r in state_indices)
    if len(rows) != len(lens) or min(rows) < 0 or len(set(rows)) != len(rows):
        raise ValueError(f"seq_map: one cache row per session, distinct and >= 0, got {rows} for {len(lens)} sessions")
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    if cu[-1] >= 1 << 31:
        raise ValueError("seq_map: too many rows")
    host = torch.tensor(cu + (list(rows) if state_indices is not None else []), dtype=torch.int32)
    device = torch.device(device)
    if device.type == "cuda":
        host = host.pin_memory()
    buf = host.to(device, non_blocking=True)
    n1 = len(lens) + 1
    return SeqMap(lens, rows, cu[-1], buf[:n1], buf[n1:] if state_indices is not None else None)


def check_seq_map(name, m, total, nrows, device):
    """The one check of a SeqMap against a call: it is of this stream (`total` packed rows) and of this device, its rows are in the pool
    (`nrows` cache rows).  Made ONCE per call, by the outermost public function the caller used (conv1d_tm_chunk_var / scan_tm_chunk_var,
    causal_conv1d_update / selective_scan_update, Mamba.step_chunk); what those call underneath trusts the map."""
    if not isinstance(m, SeqMap):
        raise TypeError(f"{name}: seq_map must come from aum_hip.seq_map()")
    if m.total != total:
        raise ValueError(f"{name}: seq_map describes {m.total} rows, the packed stream has {total}")
    if max(m.rows) >= nrows:
        raise ValueError(f"{name}: seq_map names cache row {max(m.rows)}, the pool has {nrows} rows")
    if m.cu.device != device or m.cu.dtype != torch.int32 or (m.idx is not None and (m.idx.device != device or m.idx.dtype != torch.int32)):
        raise RuntimeError(f"{name}: seq_map lives on {m.cu.device}, the packed stream on {device}")


def _packed_call(name, lib, tensors, lead, pool, seq_map, out, supported, refusal, run):
    """The front door of every public packed entry point, in this order: tensors of the library's kind; a pack of nothing but empty sessions is
    answered at once; `supported()` or the entry point's own `refusal()` text; the call's one check_seq_map; `run()`, the underscore form."""
    for t in tensors:
        lib.check_tensor(t)
    if lead.dim() == 2 and lead.shape[0] == 0 and isinstance(seq_map, SeqMap) and seq_map.total == 0:       # nothing but empty sessions
        return lead.new_empty(lead.shape) if out is None else out
    if not supported():
        raise RuntimeError(refusal())
    check_seq_map(name, seq_map, lead.shape[0], pool.shape[0], lead.device)
    return run()


def _conv_var_refusal(name, x, conv_state, rows="total"):
    return (f"{name}: unsupported operands x {tuple(x.shape)} {x.dtype} strides {x.stride()}, conv_state "
            f"{tuple(conv_state.shape)} {conv_state.dtype} (need ({rows}, dim) packed rows, 16-byte rows; fp32 contiguous (nrows, dim, width <= 4))")


def _scan_var_refusal(name, state, u):
    return (f"{name}: unsupported operands state {tuple(state.shape)} {state.dtype}, u {tuple(u.shape)} {u.dtype} "
            "(need fp32 contiguous (nrows, dim, 16), dim % 64 == 0, u (total, dim))")


def conv1d_tm_chunk_var(x, conv_state, weight, bias=None, silu=True, seq_map=None, out=None, lib=None, peek=False):
    """The causal conv on packed sessions in one launch (aum_conv1d_tm_chunk_var): x (total, dim) packed rows (row stride free: may be the
    first half of in_proj output rows), conv_state (nrows, dim, width) the pool of fp32 caches -- the rows seq_map names are advanced IN
    PLACE, the others are not touched.  Per session bit for bit conv1d_tm_chunk at batch 1.  Returns y (total, dim) in x's dtype.  No
    device synchronisation.  peek (AUM_CONV_PEEK_LAST): every session's last row is computed and the caches close one row early."""
    lib = lib or get()
    return _packed_call("conv1d_tm_chunk_var", lib, (x, conv_state, out), x, conv_state, seq_map, out,
                        lambda: conv1d_tm_chunk_var_supported(x, conv_state), lambda: _conv_var_refusal("conv1d_tm_chunk_var", x, conv_state),
                        lambda: _conv1d_tm_chunk_var(x, conv_state, weight, bias, silu, seq_map, out, lib, peek))


def _conv1d_tm_chunk_var(x, conv_state, weight, bias, silu, m, out, lib, peek=False, peek_every=None):
    """conv1d_tm_chunk_var behind its checks: operands conv1d_tm_chunk_var_supported takes, a map check_seq_map passed, total >= 1.
    peek_every: the same operands through aum_conv1d_tm_chunk_peeks"""
    total, dim = x.shape
    pa = ConvTmChunkPeeksArgs()
    a = pa.base                         # a view of pa's first field
    y, _held = _conv_chunk_operands(a, "conv1d_tm_chunk_var", lib, x, conv_state, weight, bias, silu, out)
    _fill_map(a, m, conv_state.shape[0])
    if peek_every is not None:
        pa.peek_every = peek_every
        _launch(lib.c.aum_conv1d_tm_chunk_peeks, pa, x, lib, "conv1d_tm_chunk_peeks", (len(m.lens), dim, total, x.element_size()))
        return y
    if peek:
        a.flags |= CONV_PEEK_LAST
    _launch(lib.c.aum_conv1d_tm_chunk_var, a, x, lib, "conv_tm_chunk_var", (len(m.lens), dim, total, x.element_size()))
    return y


def _peek_period(name, peek_every):
    if isinstance(peek_every, bool) or not isinstance(peek_every, int) or not 1 <= peek_every < 1 << 31:
        raise ValueError(f"{name}: peek_every is the number of committed rows before each peek row, an int >= 1, not {peek_every!r}")
    return peek_every


def conv1d_tm_chunk_peeks(x, conv_state, weight, bias=None, silu=True, seq_map=None, out=None, lib=None, peek_every=None):
    """conv1d_tm_chunk_var with a peek row behind every peek_every committed rows of each session (aum_conv1d_tm_chunk_peeks): row j of a
    session is a peek row iff (j + 1) % (peek_every + 1) == 0 -- computed and stored like any other, the window not moved.  Per session
    bit for bit conv1d_tm_chunk_var(peek=True) on one group of peek_every + 1 rows after the other, then a plain call on the rest."""
    lib = lib or get()
    peek_every = _peek_period("conv1d_tm_chunk_peeks", peek_every)
    return _packed_call("conv1d_tm_chunk_peeks", lib, (x, conv_state, out), x, conv_state, seq_map, out,
                        lambda: conv1d_tm_chunk_var_supported(x, conv_state), lambda: _conv_var_refusal("conv1d_tm_chunk_peeks", x, conv_state),
                        lambda: _conv1d_tm_chunk_var(x, conv_state, weight, bias, silu, seq_map, out, lib, False, peek_every))


def scan_tm_chunk_var(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None,
                      out=None, lib=None, peek=False):
    """The selective scan on packed sessions in one launch (aum_scan_tm_chunk_var): state (nrows, dim, dstate) the pool of fp32 caches --
    the rows seq_map names are advanced IN PLACE, the others are not touched; u, delta, z (total, dim) and B, C (total, dstate) packed
    rows in one dtype (row strides free).  Per session bit for bit scan_tm_chunk at batch 1.  Returns (total, dim) in u's dtype.  No
    device synchronisation.  peek (AUM_SCAN_PEEK_LAST): every session's last row is computed and the caches close one row early."""
    lib = lib or get()
    return _packed_call("scan_tm_chunk_var", lib, (state, u, delta, z, B, C, out), u, state, seq_map, out,
                        lambda: scan_tm_chunk_var_supported(state, u), lambda: _scan_var_refusal("scan_tm_chunk_var", state, u),
                        lambda: _scan_tm_chunk_var(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, seq_map, out, lib, peek))


def _scan_tm_chunk_var(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, m, out, lib, peek=False, peek_every=None):
    """scan_tm_chunk_var behind its checks: operands scan_tm_chunk_var_supported takes, a map check_seq_map passed, total >= 1.
    peek_every: the same operands through aum_scan_tm_chunk_peeks"""
    (total, dim), dstate = u.shape, state.shape[2]
    pa = ScanTmChunkPeeksArgs()
    a = pa.base                         # a view of pa's first field
    out, _held = _scan_chunk_operands(a, "scan_tm_chunk_var", lib, state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out)
    _fill_map(a, m, state.shape[0])
    if peek_every is not None:
        pa.peek_every = peek_every
        _launch(lib.c.aum_scan_tm_chunk_peeks, pa, u, lib, "scan_tm_chunk_peeks", (len(m.lens), dim, total, dstate, u.element_size()))
        return out
    if peek:
        a.flags |= SCAN_PEEK_LAST
    _launch(lib.c.aum_scan_tm_chunk_var, a, u, lib, "scan_tm_chunk_var", (len(m.lens), dim, total, dstate, u.element_size()))
    return out


def scan_tm_chunk_peeks(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None,
                        out=None, lib=None, peek_every=None):
    """scan_tm_chunk_var with a peek row behind every peek_every committed rows of each session (aum_scan_tm_chunk_peeks): row j of a
    session is a peek row iff (j + 1) % (peek_every + 1) == 0 -- one step from the current state and the gate, stored like any other
    row, the state not updated.  Per session bit for bit scan_tm_chunk_var(peek=True) on one group of peek_every + 1 rows after the
    other, then a plain call on the rest."""
    lib = lib or get()
    peek_every = _peek_period("scan_tm_chunk_peeks", peek_every)
    return _packed_call("scan_tm_chunk_peeks", lib, (state, u, delta, z, B, C, out), u, state, seq_map, out,
                        lambda: scan_tm_chunk_var_supported(state, u), lambda: _scan_var_refusal("scan_tm_chunk_peeks", state, u),
                        lambda: _scan_tm_chunk_var(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, seq_map, out, lib, False,
                                                   peek_every))


# ---- timeline training: the peek-row operators from the start of a clip, differentiable (aum_scan_tm_peeks_fwd_ckpt / _bwd, aum_conv1d_tm_peeks_bwd)
def peeks_rows(t, smap, name="peeks"):
    """Token-major operands of the peek-row training functions: packed (total, X) rows with a map from seq_map(), or (batch, T, X) with every batch
    entry one sequence -> ((rows, X) rows, the map, the leading shape to give the result back in or None)"""
    if smap is not None:
        if t.dim() != 2:
            raise ValueError(f"{name}: with seq_map the operands are packed (total, X) rows")
        return t, smap, None
    if t.dim() != 3:
        raise ValueError(f"{name}: operands are token-major (batch, T, X), or packed (total, X) with seq_map")
    return t.reshape(-1, t.shape[-1]), seq_map([t.shape[1]] * t.shape[0], device=t.device), t.shape[:2]


def _peeks_train_check(name, lib, u, seq_map, width=None):
    """operands of the training entry points: packed (total >= 1, dim) rows as the *_chunk_var kernels take them (width None: the scan's,
    dim % 64 == 0; else the conv's at that window width, 16-byte rows), and a map of this stream"""
    ok = u.dim() == 2 and u.shape[0] >= 1 and u.dtype in _DT
    if ok and width is None:
        ok = scan_tm_supported(u.shape[1], 16)
    elif ok:
        ok = 1 <= width <= 4 and conv1d_tm_chunk_var_supported(u, torch.empty((1, u.shape[1], width), dtype=torch.float32, device=u.device))
    if not ok:
        raise RuntimeError(f"{name}: unsupported operands {tuple(u.shape)} {u.dtype} strides {u.stride()} (need packed (total >= 1, dim) rows"
                           + (", dim % 64 == 0)" if width is None else f", 16-byte rows, window width {width} <= 4)"))
    check_seq_map(name, seq_map, u.shape[0], len(seq_map.lens) if isinstance(seq_map, SeqMap) else 0, u.device)


def _scan_peeks_base(a, name, lib, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out, m):
    state = u.new_empty((0, u.shape[1], 16), dtype=torch.float32)         # no pool: the shape alone is read
    out, held = _scan_chunk_operands(a, name, lib, state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out)
    a.state = None
    _fill_map(a, m, len(m.lens), pooled=False)
    return out, held


def scan_tm_peeks_fwd(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None, peek_every=None,
                      lib=None):
    """The training forward of the peek-row scan (aum_scan_tm_peeks_fwd_ckpt): packed sequences, each from a zero state, a peek row behind
    every peek_every committed rows.  Returns (out, ckpt): out (total, dim) bit for bit scan_tm_chunk_peeks on a zeroed pool; ckpt the
    fp32 states in front of every 8 rows, which scan_tm_peeks_bwd reads."""
    lib = lib or get()
    peek_every = _peek_period("scan_tm_peeks_fwd", peek_every)
    for t in (u, delta, z, B, C):
        lib.check_tensor(t)
    _peeks_train_check("scan_tm_peeks_fwd", lib, u, seq_map)
    pa = ScanTmPeeksFwdArgs()
    out, _held = _scan_peeks_base(pa.base, "scan_tm_peeks_fwd", lib, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, None, seq_map)
    total, dim = u.shape
    nbytes = int(lib.c.aum_scan_tm_peeks_ckpt_bytes(total, len(seq_map.lens), dim, 16))
    ckpt = torch.empty(nbytes // 4, dtype=torch.float32, device=u.device)
    pa.ckpt, pa.ckpt_bytes, pa.peek_every = _ptr(ckpt), nbytes, peek_every
    _launch(lib.c.aum_scan_tm_peeks_fwd_ckpt, pa, u, lib, "scan_tm_peeks_fwd", (len(seq_map.lens), dim, total, 16, u.element_size()))
    return out, ckpt


def scan_tm_peeks_bwd_parts(dout, ckpt, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None,
                            peek_every=None, lib=None, fill=None):
    """aum_scan_tm_peeks_bwd as it is: (du, ddelta, dz or None) in u's dtype and the fp32 partial rows (dBC_part (dim / 64, total, 32),
    dA_part (nseq, dim, 16), dD_part (nseq, dim), dbias_part (nseq, dim)) still to be added over their first axis.  fill: what the
    buffers hold before the launch (tests: a sentinel); None: the per-sequence parts are zeroed, the rest is left uninitialised."""
    lib = lib or get()
    peek_every = _peek_period("scan_tm_peeks_bwd", peek_every)
    for t in (dout, ckpt, u, delta, z, B, C):
        lib.check_tensor(t)
    _peeks_train_check("scan_tm_peeks_bwd", lib, u, seq_map)
    if dout.dtype != u.dtype or dout.shape != u.shape:
        raise RuntimeError("scan_tm_peeks_bwd: dout must have u's shape and dtype")
    total, dim = u.shape
    nseq, ngrp = len(seq_map.lens), dim // 64
    pa = ScanTmPeeksBwdArgs()
    _, _held = _scan_peeks_base(pa.base, "scan_tm_peeks_bwd", lib, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, dout, seq_map)
    new = (lambda shape, dt: torch.empty(shape, dtype=dt, device=u.device)) if fill is None else (
        lambda shape, dt: torch.full(shape, fill, dtype=dt, device=u.device))
    du, ddelta = new(u.shape, u.dtype), new(u.shape, u.dtype)
    dz = None if z is None else new(u.shape, u.dtype)
    nbytes = int(lib.c.aum_scan_tm_peeks_bwd_workspace_bytes(total, nseq, dim, 16))
    ws = new((nbytes // 4,), torch.float32)
    n_bc = ngrp * total * 32
    if fill is None:
        ws[n_bc:].zero_()
    pa.ckpt, pa.ckpt_bytes = _ptr(ckpt), ckpt.numel() * 4
    pa.du, pa.ddelta, pa.dz, pa.workspace, pa.workspace_bytes = _ptr(du), _ptr(ddelta), _ptr(dz), _ptr(ws), nbytes
    pa.du_ts, pa.ddelta_ts, pa.dz_ts, pa.peek_every = dim, dim, dim, peek_every
    _launch(lib.c.aum_scan_tm_peeks_bwd, pa, u, lib, "scan_tm_peeks_bwd", (nseq, dim, total, 16, u.element_size()))
    n_a = nseq * dim * 16
    parts = (ws[:n_bc].view(ngrp, total, 32), ws[n_bc:n_bc + n_a].view(nseq, dim, 16), ws[n_bc + n_a:n_bc + n_a + nseq * dim].view(nseq, dim),
             ws[n_bc + n_a + nseq * dim:].view(nseq, dim))
    return du, ddelta, dz, parts


def scan_tm_peeks_bwd(dout, ckpt, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None,
                      peek_every=None, lib=None):
    """The adjoint of scan_tm_peeks_fwd.  Returns (du, ddelta, dz or None, dA (dim, 16), dB (total, 16), dC (total, 16), dD (dim) or None,
    ddelta_bias (dim)): the first three in u's dtype, ddelta in raw space, the rest fp32 -- the kernel's partial rows added in a fixed
    order by aum_sum_rows (bitwise repeatable)."""
    lib = lib or get()
    du, ddelta, dz, (p_bc, p_a, p_d, p_b) = scan_tm_peeks_bwd_parts(dout, ckpt, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated,
                                                                    seq_map, peek_every, lib)
    dbc = sum_rows(p_bc, lib=lib)
    return (du, ddelta, dz, sum_rows(p_a, lib=lib), dbc[:, :16], dbc[:, 16:], None if D is None else sum_rows(p_d, lib=lib), sum_rows(p_b, lib=lib))


def conv1d_tm_peeks_fwd(x, weight, bias=None, silu=True, seq_map=None, peek_every=None, lib=None):
    """The training forward of the peek-row conv: conv1d_tm_chunk_peeks itself on a zeroed pool (every sequence starts a clip)."""
    lib = lib or get()
    pool = torch.zeros((len(seq_map.lens), x.shape[1], weight.reshape(x.shape[1], -1).shape[1]), dtype=torch.float32, device=x.device)
    return conv1d_tm_chunk_peeks(x, pool, weight, bias, silu, seq_map=seq_map, lib=lib, peek_every=peek_every)


def conv1d_tm_peeks_bwd_parts(dy, x, weight, bias=None, silu=True, seq_map=None, peek_every=None, lib=None, fill=None):
    """aum_conv1d_tm_peeks_bwd as it is: dx in x's dtype and the fp32 partial rows dw_part (nseq, dim, width), db_part (nseq, dim) (fill: see
    scan_tm_peeks_bwd_parts)"""
    lib = lib or get()
    peek_every = _peek_period("conv1d_tm_peeks_bwd", peek_every)
    for t in (dy, x):
        lib.check_tensor(t)
    _peeks_train_check("conv1d_tm_peeks_bwd", lib, x, seq_map, weight.reshape(x.shape[-1], -1).shape[1] if x.dim() == 2 else 0)
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise RuntimeError("conv1d_tm_peeks_bwd: dy must have x's shape and dtype")
    total, dim = x.shape
    nseq = len(seq_map.lens)
    weight = _al16(_f32c(weight.reshape(dim, -1)))
    bias = _al16(_f32c(bias))
    for t in (weight, bias):
        lib.check_tensor(t)
    width = weight.shape[1]
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if fill is None else torch.full(x.shape, fill, dtype=x.dtype, device=x.device)
    nbytes = int(lib.c.aum_conv1d_tm_peeks_bwd_workspace_bytes(nseq, dim, width))
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=x.device) if fill is None else torch.full((nbytes // 4,), fill, dtype=torch.float32,
                                                                                                        device=x.device)
    a = ConvTmPeeksBwdArgs()
    a.x, a.dy, a.weight, a.bias, a.dx, a.workspace, a.cu_seqlens = _ptr(x), _ptr(dy), _ptr(weight), _ptr(bias), _ptr(dx), _ptr(ws), _ptr(seq_map.cu)
    a.workspace_bytes, a.x_ts, a.dy_ts, a.dx_ts = nbytes, _tm2(x, "x", dim), _tm2(dy, "dy", dim), dim
    a.total, a.nseq, a.dim, a.width, a.dtype, a.flags, a.peek_every = total, nseq, dim, width, _DT[x.dtype], _conv_flags(silu), peek_every
    _launch(lib.c.aum_conv1d_tm_peeks_bwd, a, x, lib, "conv1d_tm_peeks_bwd", (nseq, dim, total, x.element_size()))
    n_w = nseq * dim * width
    return dx, (ws[:n_w].view(nseq, dim, width), ws[n_w:].view(nseq, dim))


def conv1d_tm_peeks_bwd(dy, x, weight, bias=None, silu=True, seq_map=None, peek_every=None, lib=None):
    """The adjoint of the peek-row conv from a zero window.  Returns (dx in x's dtype, dw (dim, width) fp32, db (dim) fp32 or None): the
    kernel's per-sequence partial rows added in a fixed order by aum_sum_rows."""
    lib = lib or get()
    dx, (p_w, p_b) = conv1d_tm_peeks_bwd_parts(dy, x, weight, bias, silu, seq_map, peek_every, lib)
    return dx, sum_rows(p_w, lib=lib), None if bias is None else sum_rows(p_b, lib=lib)


# ---- packed prefill: the backlogs of many sessions in one launch per operator (aum_conv1d_tm_prefill_var, aum_scan_tm_fwd_state_var)
def conv1d_tm_prefill_var_supported(x, conv_state):
    """the limits of aum_conv1d_tm_prefill_var (include/aum_hip.h): those of conv1d_tm_chunk_var -- packed (total >= 1, dim) rows with
    16-byte rows, an fp32 contiguous (nrows, dim, width <= 4) pool"""
    return conv1d_tm_chunk_var_supported(x, conv_state)


def conv1d_tm_prefill_var(x, conv_state, weight, bias=None, silu=True, seq_map=None, out=None, lib=None):
    """conv1d_tm_prefill on PACKED sessions in one launch (aum_conv1d_tm_prefill_var): x (total, dim) packed rows (row stride free: the x
    half of in_proj rows), conv_state (nrows, dim, width) the pool of fp32 windows -- each session's rows enter with the window of the
    row seq_map names for it, read as fp32 in place (no [window ; x] copy, no rounding), and that row then holds the session's last
    `width` inputs (fewer rows than `width`: the old entries shift); an empty session's row and the rows no session names are not
    touched.  Time-parallel: one wave per (session, 64 rows, channel block).  Per session, y and the window are bit for bit
    conv1d_tm_prefill's at batch 1 when the window's values are exact in x's dtype.  Returns y (total, dim) contiguous in x's dtype
    (out: written there).  Raises where the kernel does not take the operands.  No device synchronisation."""
    lib = lib or get()
    return _packed_call("conv1d_tm_prefill_var", lib, (x, conv_state, out), x, conv_state, seq_map, out,
                        lambda: x.dim() == 2 and x.shape[0] >= 1 and conv1d_tm_prefill_var_supported(x, conv_state),
                        lambda: _conv_var_refusal("conv1d_tm_prefill_var", x, conv_state, "total >= 1"),
                        lambda: _conv1d_tm_prefill_var(x, conv_state, weight, bias, silu, seq_map, out, lib))


def _conv1d_tm_prefill_var(x, conv_state, weight, bias, silu, m, out, lib):
    """conv1d_tm_prefill_var behind its checks: operands conv1d_tm_prefill_var_supported takes, a map check_seq_map passed, total >= 1"""
    total, dim = x.shape
    a = ConvTmPrefillVarArgs()
    y, _held = _conv_chunk_operands(a, "conv1d_tm_prefill_var", lib, x, conv_state, weight, bias, silu, out)
    if not y.is_contiguous():
        raise RuntimeError("conv1d_tm_prefill_var: out must be contiguous")
    _fill_map(a, m, conv_state.shape[0])
    a.max_len = max(m.lens)
    _launch(lib.c.aum_conv1d_tm_prefill_var, a, x, lib, "conv_tm_prefill_var", (len(m.lens), dim, total, x.element_size()))
    return y


def scan_tm_var_range(lens, dim, nsimd=None, device=None):
    """range_len of scan_tm_fwd_state_var for sessions of these lengths (0: not cut): the rule of scan_tm_segments with batch := the number
    of sessions and length := the longest session -- cut only when the longest has >= 1024 steps and the uncut launch is under one wave
    per two SIMDs, into as many ranges as give every SIMD three waves, ranges no shorter than 128 steps, at most SCAN_TM_MAX_SEGMENTS
    of them; the range is ceil(longest / ranges) rounded up to the 8-step block.  The rule is inherited from the B = 8, L = 4097
    measurement of the fixed-batch kernels (profiles/r04_seg_time.json) and is NOT measured for ragged packs: short sessions of a
    pack leave the ranges past their end empty, so the waves it counts on are fewer than at a fixed batch."""
    lens = [int(n) for n in lens]
    longest = max(lens) if lens else 0
    seg = scan_tm_segments(len(lens), dim, longest, False, nsimd=nsimd, device=device) if longest >= 1 else 1
    if seg < 2:
        return 0
    return -(-(-(-longest // seg)) // SCAN_TM_CK) * SCAN_TM_CK


def scan_tm_fwd_state_var_supported(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False,
                                    range_len=0, max_len=None):
    """the limits of aum_scan_tm_fwd_state_var (include/aum_hip.h): those of scan_tm_fwd_state on packed rows -- dstate == 16, dim % 64
    == 0, (total >= 1, dim) rows of one dtype moved as 16-byte chunks, B / C rows 4-byte aligned, an activated delta only for 16-bit
    rows with z -- the pool fp32 contiguous (nrows, dim, 16), 16-byte aligned, and range_len 0 or a multiple of 8 that cuts the longest
    session (max_len; None: not known here) into at most SCAN_TM_MAX_SEGMENTS ranges."""
    if u.dim() != 2 or A.dim() != 2 or u.shape[0] < 1 or not scan_tm_supported(u.shape[1], A.shape[1]) or u.dtype not in _DT:
        return False
    dim, dstate = u.shape[1], A.shape[1]
    if A.shape[0] != dim or _scan_rows(u, delta, z, B, C, dstate, strict=True, pad=dim, activated=delta_activated)[0] is None:
        return False
    range_len = int(range_len)
    if range_len < 0 or range_len % SCAN_TM_CK:
        return False
    if range_len and max_len is not None and -(-int(max_len) // range_len) > SCAN_TM_MAX_SEGMENTS:
        return False
    return (state.dim() == 3 and state.shape[0] >= 1 and tuple(state.shape[1:]) == (dim, dstate) and state.dtype == torch.float32
            and state.is_contiguous() and state.data_ptr() % 16 == 0)


def scan_tm_fwd_state_var(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None,
                          range_len=0, out=None, lib=None):
    """scan_tm_fwd_state on PACKED sessions (aum_scan_tm_fwd_state_var): state (nrows, dim, 16) the pool of fp32 states -- session i runs
    its rows of the packed u, delta, z (total, dim) and B, C (total, 16) from row seq_map.rows[i], which is advanced IN PLACE; an empty
    session's row and the rows no session names are not touched.  One direction, forward time, both delta forms, with and without z,
    fp32 / bf16 / fp16 (row strides free).
    range_len == 0: uncut, one wave per (session, 64 channels); per session bit for bit scan_tm_fwd_state(segments=1) at batch 1.
    range_len > 0, a multiple of 8 (scan_tm_var_range chooses): every session is cut into ranges of range_len steps -- at most
    SCAN_TM_MAX_SEGMENTS for the longest -- a carry launch and a main launch; the ranges past a session's end are empty.  COINCIDENCE:
    a session of n steps is bit for bit scan_tm_fwd_state(segments=s) at batch 1 with s = ceil(n / range_len) exactly when that call
    cuts the same ranges, i.e. when ceil(ceil(n / s) / 8) * 8 == range_len (n = 40, 24, 9, 1 at range_len 8: yes; n = 130 at 128: two
    ranges of 128 + 2 here, of 72 + 58 there -- no); elsewhere the two differ by the re-association at the range boundaries.
    A session's results do not depend on the other sessions of the call, on its place in the pack or on its pool row (bitwise).
    Returns out (total, dim) contiguous in u's dtype.  Raises where the kernel does not take the operands.  No device synchronisation."""
    lib = lib or get()
    max_len = max(seq_map.lens) if isinstance(seq_map, SeqMap) else None
    return _packed_call(
        "scan_tm_fwd_state_var", lib, (state, u, delta, z, B, C, out), u, state, seq_map, out,
        lambda: scan_tm_fwd_state_var_supported(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, range_len, max_len),
        lambda: (f"scan_tm_fwd_state_var: unsupported operands state {tuple(state.shape)} {state.dtype}, u {tuple(u.shape)} {u.dtype} strides "
                 f"{u.stride()}, A {tuple(A.shape)}, range_len {range_len} for a longest session of {max_len} (need packed 16-byte "
                 "rows of one dtype, dim % 64 == 0, dstate 16, an fp32 contiguous 16-byte aligned (nrows, dim, 16) pool, range_len a "
                 f"multiple of {SCAN_TM_CK} giving at most {SCAN_TM_MAX_SEGMENTS} ranges)"),
        lambda: _scan_tm_fwd_state_var(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, seq_map, int(range_len), out, lib))


def _scan_tm_fwd_state_var(state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, m, range_len, out, lib):
    """scan_tm_fwd_state_var behind its checks: operands scan_tm_fwd_state_var_supported takes, a map check_seq_map passed"""
    (total, dim), dstate = u.shape, state.shape[2]
    a = ScanTmFwdStateVarArgs()
    out, _held = _scan_chunk_operands(a, "scan_tm_fwd_state_var", lib, state, u, delta, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, out)
    if not out.is_contiguous():
        raise RuntimeError("scan_tm_fwd_state_var: out must be contiguous")
    _fill_map(a, m, state.shape[0])
    a.max_len, a.range_len = max(m.lens), range_len
    if range_len:
        nranges = -(-max(m.lens) // range_len)
        a.carry_bytes = int(lib.c.aum_scan_tm_fwd_state_var_carry_bytes(len(m.lens), dim, dstate, nranges))
        if a.carry_bytes <= 0:
            raise RuntimeError(f"scan_tm_fwd_state_var: range_len={range_len} ({nranges} ranges) not supported for this shape")
        carry = torch.empty((a.carry_bytes // 4,), dtype=torch.float32, device=u.device)
        a.carry = _ptr(carry)
    _launch(lib.c.aum_scan_tm_fwd_state_var, a, u, lib, "scan_tm_fwd_state_var", (len(m.lens), dim, total, dstate, u.element_size(), range_len))
    return out


def _unit_last(t):
    return t if t is None or t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


def _settled(ok, st, lead):
    """the leading operand as a launch takes it -- itself, or a contiguous copy where that is what turns ok() true -- or None"""
    lead = _unit_last(lead)
    if ok(st, lead):
        return lead
    c = lead.contiguous()
    return c if c is not lead and ok(st, c) else None


def _advance_batch(st, rows, chunk_ok, chunk, token):
    lead = _settled(chunk_ok, st, rows[0])
    if lead is not None:
        return chunk(st, lead, *[_unit_last(t) for t in rows[1:]])
    return torch.stack([token(st, *[None if t is None else t[:, i] for t in rows]) for i in range(rows[0].shape[1])], dim=1)


def _packed_rows(t):
    """(batch, T, X) rows as one (1, batch * T, X) pack: a view where batch and T share one stride, else a contiguous copy"""
    if t is None:
        return None
    batch, T, X = t.shape
    if batch == 1 or t.stride(0) == T * t.stride(1):
        return t.as_strided((1, batch * T, X), (0, t.stride(1), t.stride(2)))
    return t.contiguous().view(1, batch * T, X)


def _peek_cuts(n, peek, peek_every):
    """the n rows of one session as the host loop advances them: [(first, end, committed)] -- runs of committed rows, each peek row alone"""
    if peek_every is not None:
        cuts = []
        for g in range(0, n, peek_every + 1):
            cuts.append((g, min(g + peek_every, n), True))
            if g + peek_every < n:
                cuts.append((g + peek_every, g + peek_every + 1, False))
        return cuts
    keep = max(n - 1, 0) if peek else n
    return ([(0, keep, True)] if keep > 0 else []) + ([(keep, n, False)] if n > keep else [])


def _stream_advance(lib, cache, rows, m, var_ok, var, chunk_ok, chunk, token, peek=False, peek_every=None):
    """The one ladder under conv1d_stream and scan_stream: advance `cache` IN PLACE (through an fp32 copy, written back, if it is not fp32
    contiguous) by the token-major operands `rows` ((batch, T, .) views or None; rows[0] is what the *_ok predicates look at) with the
    first launch that takes them.  m (a SeqMap its caller checked; rows (1, total, .), cache a pool): var() on the packed rows, else a host
    loop over the sessions (host lengths: no synchronisation), each on its pool row as without m: chunk(), else token() token by token
    (a (batch, .) rows[0] is one token).  An operand is copied to contiguous rows only where that makes a launch take it.
    peek: every session's last row is computed and the cache closes one row early (the flag of the packed kernels -- a fixed batch goes
    through them with fixed_seq_map; in the host loop a session's last row is advanced on a copy of its cache row).
    peek_every (not with peek): a peek row behind every peek_every committed rows of each session -- var() is then the *_chunk_peeks
    launch; the host loop advances every peek row on a copy of the cache row, group by group."""
    if peek and peek_every is not None:
        raise ValueError("peek (the last row of every session) and peek_every (a peek row every so many rows) exclude each other")
    for t in (cache, *rows):
        lib.check_tensor(t)
    st = cache if cache.dtype == torch.float32 and cache.is_contiguous() else cache.float().contiguous()
    shape = None
    if (peek or peek_every is not None) and m is None:
        if rows[0].dim() != 3:
            raise ValueError("peek takes (batch, T >= 1, .) rows: the last of the T rows is the peek row" if peek else
                             "peek_every takes (batch, T >= 1, .) rows")
        shape = rows[0].shape
        m = fixed_seq_map(shape[0], shape[1], rows[0].device)
        rows = [_packed_rows(t) for t in rows]
    if m is None:
        out = token(st, *rows) if rows[0].dim() == 2 else _advance_batch(st, rows, chunk_ok, chunk, token)
    elif m.total == 0:
        out = rows[0].new_empty(rows[0].shape)
    else:
        rows2d = [None if t is None else t[0] for t in rows]
        lead = _settled(var_ok, st, rows2d[0])
        if lead is not None:
            out = var(st, lead, *[_unit_last(t) for t in rows2d[1:]]).unsqueeze(0)
        else:
            outs, o = [], 0
            cut = lambda a, b: [None if t is None else t[:, a:b] for t in rows]
            for n, r in zip(m.lens, m.rows):
                for a, b, keep in _peek_cuts(n, peek, peek_every):
                    outs.append(_advance_batch(st[r:r + 1] if keep else st[r:r + 1].clone(), cut(o + a, o + b), chunk_ok, chunk, token))
                o += n
            out = torch.cat(outs, dim=1)
    if st is not cache:
        cache.copy_(st)
    return out if shape is None else out.reshape(shape[0], shape[1], -1)


def conv1d_stream(x, conv_state, weight, bias=None, silu=True, seq_map=None, lib=None, peek=False, peek_every=None):
    """causal_conv1d.causal_conv1d_update on token-major rows, as Mamba.step_chunk has them: x (batch, T, dim) (a view is read in place),
    (batch, dim) one token, or with seq_map (trusted: check_seq_map is the caller's) (1, total, dim) over a pool; returns x's shape.
    peek: the last row of every session (of the T rows without seq_map) is computed, conv_state is advanced by the rows before it.
    peek_every (not with peek): a peek row behind every peek_every committed rows of each session (conv1d_tm_chunk_peeks)."""
    lib = lib or get()
    if peek_every is not None:
        peek_every = _peek_period("conv1d_stream", peek_every)
    if (peek or peek_every is not None) and seq_map is None and x.dim() == 3:
        seq_map_k = fixed_seq_map(x.shape[0], x.shape[1], x.device)
    else:
        seq_map_k = seq_map
    return _stream_advance(lib, conv_state, (x,), seq_map,
                           lambda st, x: conv1d_tm_chunk_var_supported(x, st),
                           lambda st, x: _conv1d_tm_chunk_var(x, st, weight, bias, silu, seq_map_k, None, lib, peek, peek_every),
                           lambda st, x: conv1d_tm_chunk_supported(x, st),
                           lambda st, x: conv1d_tm_chunk(x, st, weight, bias, silu, lib),
                           lambda st, x: conv1d_update(x, st, weight, bias, silu, lib), peek, peek_every)


def scan_stream(state, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, delta_activated=False, seq_map=None, lib=None,
                peek=False, peek_every=None):
    """selective_scan_update behind its argument normalisation (operands of one dtype), what Mamba.step_chunk calls: seq_map is trusted
    (check_seq_map is the caller's).  peek: the last row of every session (of the T rows without seq_map) is computed, state is advanced
    by the rows before it.  peek_every (not with peek): a peek row behind every peek_every committed rows of each session
    (scan_tm_chunk_peeks)."""
    lib = lib or get()
    if peek_every is not None:
        peek_every = _peek_period("scan_stream", peek_every)
    if delta_activated:                 # delta holds softplus(raw + delta_bias) already
        delta_bias, delta_softplus = None, False
    if (peek or peek_every is not None) and seq_map is None and u.dim() == 3:
        seq_map_k = fixed_seq_map(u.shape[0], u.shape[1], u.device)
    else:
        seq_map_k = seq_map
    return _stream_advance(lib, state, (u, delta, z, B, C), seq_map,
                           scan_tm_chunk_var_supported,
                           lambda st, u, dl, z, B, C: _scan_tm_chunk_var(st, u, dl, A, B, C, D, z, delta_bias, delta_softplus, delta_activated,
                                                                         seq_map_k, None, lib, peek, peek_every),
                           scan_tm_chunk_supported,
                           lambda st, u, dl, z, B, C: scan_tm_chunk(st, u, dl, A, B, C, D, z, delta_bias, delta_softplus, delta_activated, lib=lib),
                           lambda st, u, dl, z, B, C: state_update(st, u, dl, A, B, C, D, z, delta_bias, delta_softplus, lib=lib), peek, peek_every)


# ---- the block's recurrent middle in one launch (aum_stream_block_tm): conv -> x/dt projections -> scan on packed sessions
STREAM_NO_COMMIT = 1
STREAM_PEEK_LAST = 2            # the last row of every session is computed and stored, the caches close one row early
CONV_PEEK_LAST = 8              # the same for aum_conv1d_tm_chunk_var ...
SCAN_PEEK_LAST = 64             # ... and aum_scan_tm_chunk_var
STREAM_BLOCK_MAX_T = 128        # tokens per session and call (aum_stream_block_max_len)
_fixed_maps = {}


def fixed_seq_map(batch, length, device):
    """The SeqMap of a fixed batch -- `batch` sessions of `length` rows on cache rows 0 .. batch - 1 -- uploaded once per (batch, length, device)"""
    key = (int(batch), int(length), torch.device(device))
    m = _fixed_maps.get(key)
    if m is None:
        if len(_fixed_maps) > 64:
            _fixed_maps.clear()
        m = _fixed_maps[key] = seq_map([length] * batch, device=device)
    return m


def stream_block_supported(x, z, conv_state, state, plan, max_len=1):
    """the limits of aum_stream_block_tm (include/aum_hip.h): x, z (total >= 1, dim) packed 16-bit rows (the halves of the in_proj rows),
    fp32 contiguous pools (nrows, dim, 4) / (nrows, dim, 16), the shapes xdt_tm_supported takes, sessions of at most STREAM_BLOCK_MAX_T rows,
    a plan (Mamba.stream_params) in x's dtype; outside them callers use the three launches"""
    if not (x.dim() == 2 and z.dim() == 2 and x.shape == z.shape and x.shape[0] >= 1 and x.dtype == z.dtype and x.dtype in (torch.bfloat16, torch.float16)):
        return False
    dim = x.shape[1]
    if not (plan.w_x.dtype == x.dtype and plan.w_dt.dtype == x.dtype and 1 <= max_len <= STREAM_BLOCK_MAX_T):
        return False
    ok_t = lambda t: t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0
    rank = plan.w_dt.shape[1]
    return (ok_t(x) and ok_t(z) and xdt_tm_supported(x, plan.w_x, plan.w_dt) and rank + 32 <= plan.w_x.shape[0]
            and conv_state.dim() == 3 and conv_state.dtype == torch.float32 and conv_state.is_contiguous() and conv_state.shape[1:] == (dim, 4)
            and state.dim() == 3 and state.dtype == torch.float32 and state.is_contiguous() and state.shape[1:] == (dim, 16)
            and state.shape[0] == conv_state.shape[0] >= 1 and state.data_ptr() % 16 == 0 and conv_state.data_ptr() % 16 == 0
            and plan.conv_w.shape == (dim, 4) and plan.A.shape == (dim, 16))


def stream_block(xz_x, z, conv_state, state, plan, seq_map=None, commit=True, out=None, lib=None, peek=False):
    """Conv (SiLU) from the carried window -> x_proj, dt_proj (dt_bias and softplus once) -> selective scan (D, z gate) from the carried
    state, in ONE launch (aum_stream_block_tm): xz_x, z the two halves of the in_proj rows -- (total, dim) packed rows with seq_map
    (trusted: check_seq_map is the caller's), or (batch, T, dim) views of one (batch, T, 2 dim) tensor, session b on cache row b.
    conv_state (nrows, dim, 4) / state (nrows, dim, 16): fp32 pools advanced IN PLACE; commit=False: read and not written.  plan:
    Mamba.stream_params().  Bit for bit conv1d_tm_chunk_var -> xdt_tm_fwd(delta_softplus) -> scan_tm_chunk_var(delta_activated).
    peek (AUM_STREAM_PEEK_LAST): the last row of every session is a peek row -- computed like any other, the pools advanced by the rows
    before it (bit for bit a call on those rows, then a commit=False call on the last row).  The peek row counts towards the 128.
    Returns y in xz_x's shape and dtype.  No device synchronisation."""
    lib = lib or get()
    shape = xz_x.shape
    if xz_x.dim() == 3:
        batch, T, dim = shape
        if seq_map is None:
            seq_map = fixed_seq_map(batch, T, xz_x.device)
        x2 = xz_x.as_strided((batch * T, dim), (xz_x.stride(1), 1)) if batch == 1 or xz_x.stride(0) == T * xz_x.stride(1) else None
        z2 = z.as_strided((batch * T, dim), (z.stride(1), 1)) if batch == 1 or z.stride(0) == T * z.stride(1) else None
        if x2 is None or z2 is None:
            raise RuntimeError("stream_block: (batch, T, dim) operands must be uniformly strided over (batch, T)")
    else:
        x2, z2 = xz_x, z
        if seq_map is None:
            seq_map = fixed_seq_map(1, x2.shape[0], x2.device)
    for t in (x2, z2, conv_state, state, out, plan.conv_w, plan.w_x):
        lib.check_tensor(t)
    max_len = max(seq_map.lens)
    if not stream_block_supported(x2, z2, conv_state, state, plan, max_len):
        raise RuntimeError(f"stream_block: unsupported operands x {tuple(x2.shape)} {x2.dtype} strides {x2.stride()}, pools "
                           f"{tuple(conv_state.shape)} / {tuple(state.shape)}, longest session {max_len}")
    total, dim = x2.shape
    y = torch.empty((total, dim), dtype=x2.dtype, device=x2.device) if out is None else out.reshape(total, dim)
    if y.dtype != x2.dtype or y.stride(1) != 1 or (out is not None and y.data_ptr() != out.data_ptr()):
        raise RuntimeError("stream_block: out must have x's shape and dtype, rows contiguous")
    ncols = plan.w_x.shape[0]
    nbytes = int(lib.c.aum_stream_block_scratch_bytes(total, dim, ncols))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
    a = StreamBlockArgs()
    a.x, a.z, a.conv_state, a.state, a.y, a.scratch = _ptr(x2), _ptr(z2), _ptr(conv_state), _ptr(state), _ptr(y), _ptr(scratch)
    a.conv_weight, a.conv_bias, a.wx, a.wdt = _ptr(plan.conv_w), _ptr(plan.conv_b), _ptr(plan.w_x), _ptr(plan.w_dt)
    a.A, a.D, a.delta_bias = _ptr(plan.A), _ptr(plan.D), _ptr(plan.dt_bias)
    a.cu_seqlens, a.state_indices = _ptr(seq_map.cu), _ptr(seq_map.idx)
    a.x_ts, a.z_ts, a.y_ts, a.scratch_bytes = x2.stride(0), z2.stride(0), y.stride(0), nbytes
    a.total, a.nseq, a.nrows, a.max_len = total, len(seq_map.lens), conv_state.shape[0], max_len
    a.dim, a.width, a.dstate, a.rank, a.ncols = dim, 4, 16, plan.w_dt.shape[1], ncols
    a.ldwx, a.ldwdt, a.dtype = plan.w_x.stride(0), plan.w_dt.stride(0), _DT[x2.dtype]
    a.flags = (0 if commit else STREAM_NO_COMMIT) | (STREAM_PEEK_LAST if peek else 0)
    _launch(lib.c.aum_stream_block_tm, a, x2, lib, "stream_block", (len(seq_map.lens), dim, total))
    return y.view(shape)


# ---- parking sessions: the pool rows of many sessions to one record each of a byte blob, and back (aum_stream_park) ----
PARK_RECORD_ALIGN = 256     # a record is rounded up to this many bytes
PARK_CHUNK = 4096           # PARK_CHUNK of csrc/stream_park_kernels.h: the bytes of a row one workgroup moves


class ParkLayout(typing.NamedTuple):
    """Where the rows of a list of pool tensors sit inside a session's record (stream_park_layout): tensor t's row is the row_bytes[t]
    bytes at offsets[t]; `record` is the size of a record, the end of the last row rounded up to PARK_RECORD_ALIGN."""
    offsets: tuple
    row_bytes: tuple
    record: int


class RowMap(typing.NamedTuple):
    """the pool rows of the sessions of one park / resume call: host tuple (checked there) and the same as an int32 device tensor"""
    rows: tuple
    idx: torch.Tensor


def row_map(rows, *, device):
    """Built once per call (stream_park takes a list as well and builds it): distinct rows >= 0, sent to `device` in one pinned,
    non-blocking upload as seq_map does.  That the rows exist is checked where the pool is known (stream_park)."""
    rows = tuple(int(r) for r in rows)
    if not rows or min(rows) < 0 or len(set(rows)) != len(rows) or max(rows) >= 1 << 31:
        raise ValueError(f"row_map: at least one pool row, distinct and >= 0, got {rows}")
    host = torch.tensor(rows, dtype=torch.int32)
    device = torch.device(device)
    if device.type == "cuda":
        host = host.pin_memory()
    return RowMap(rows, host.to(device, non_blocking=True))


def stream_park_layout(tensors):
    """The record of a session over these pool tensors (each (nrows, ...), a session's row t[r]): the rows behind one another in the
    order given, every offset a multiple of 16, the record rounded up to 256 bytes -> ParkLayout(offsets, row_bytes, record)."""
    offs, sizes, at = [], [], 0
    for t in tensors:
        n = t[0].numel() * t.element_size()
        offs.append(at)
        sizes.append(n)
        at = (at + n + 15) // 16 * 16
    return ParkLayout(tuple(offs), tuple(sizes), (at + PARK_RECORD_ALIGN - 1) // PARK_RECORD_ALIGN * PARK_RECORD_ALIGN)


def stream_park_args_ok(a):
    """park_check of csrc/stream_park_kernels.h on a filled ParkArgs, rule for rule: what aum_stream_park takes (AUM_OK) and what it
    refuses (AUM_E_NULL / AUM_E_UNSUPPORTED)"""
    if not a.rows or not a.blob:
        return False
    if not 1 <= a.n_tensors <= PARK_MAX_TENSORS or a.n_sessions < 1 or (a.flags & ~PARK_RESTORE):
        return False
    if any(not a.base[t] for t in range(a.n_tensors)):
        return False
    restore = bool(a.flags & PARK_RESTORE)
    if (a.rows & 3) or (a.blob & 15) or (a.blob_stride & 15) or a.blob_stride < 0:
        return False
    end = chunks = 0
    for t in range(a.n_tensors):
        if (a.base[t] | a.row_stride[t] | a.row_bytes[t] | a.blob_off[t]) & 15:
            return False
        if a.row_bytes[t] < 16 or a.row_stride[t] < a.row_bytes[t] or a.blob_off[t] < end:
            return False
        if a.row_bytes[t] > 1 << 40:
            return False
        end = a.blob_off[t] + a.row_bytes[t]
        chunks += (a.row_bytes[t] + PARK_CHUNK - 1) // PARK_CHUNK
    if not (restore and a.blob_stride == 0) and end > a.blob_stride:
        return False
    return chunks * a.n_sessions <= 0x7fffffff


def stream_park(tensors, rows, blob=None, restore=False, lib=None):
    """ONE launch (aum_stream_park) for the rows `rows` of every pool tensor: restore=False copies them into one record per session of
    `blob` ((len(rows), record) uint8 on the tensors' device; None: allocated, zero-filled) and leaves the pools as they are;
    restore=True copies the records of `blob` into those rows (a blob expanded from one record -- row stride 0 -- restores every
    session from it).  tensors: at most 64, each (nrows, ...) with contiguous rows, all with the same nrows and device; the record is
    stream_park_layout(tensors).  rows: a list of distinct rows of the pools, or a row_map().  Returns the blob.
    Every operand is checked on the host before the launch, by the rules of the C side (stream_park_args_ok) and against the pools'
    row count, which the kernel does not know: a refused call raises and changes nothing.  No device synchronisation."""
    lib = lib or get()
    tensors = list(tensors)
    if not tensors or any(not torch.is_tensor(t) or t.dim() < 1 or t.shape[0] < 1 for t in tensors):
        raise RuntimeError("stream_park: at least one pool tensor, each (nrows >= 1, ...)")
    dev, nrows = tensors[0].device, tensors[0].shape[0]
    m = rows if isinstance(rows, RowMap) else row_map(rows, device=dev)
    if max(m.rows) >= nrows:
        raise ValueError(f"stream_park: pool row {max(m.rows)} named, the pools have {nrows} rows")
    if m.idx.device != dev or m.idx.dtype != torch.int32 or m.idx.numel() != len(m.rows):
        raise RuntimeError(f"stream_park: the row map lives on {m.idx.device}, the pools on {dev}")
    n, lay = len(m.rows), stream_park_layout(tensors)
    bad = [i for i, t in enumerate(tensors) if t.device != dev or t.shape[0] != nrows or t.numel() == 0 or not t[0].is_contiguous()]
    if bad or len(tensors) > PARK_MAX_TENSORS:
        raise RuntimeError(f"stream_park: unsupported operands: {len(tensors)} pool tensors (at most {PARK_MAX_TENSORS}), tensors {bad} are not "
                           f"({nrows}, ...) on {dev} with contiguous rows")
    if blob is None:
        if restore:
            raise RuntimeError("stream_park: restore=True needs the blob to restore from")
        blob = torch.zeros((n, lay.record), dtype=torch.uint8, device=dev)
    if (not torch.is_tensor(blob) or blob.dtype != torch.uint8 or blob.device != dev or tuple(blob.shape) != (n, lay.record)
            or blob.stride(1) != 1):
        got = f"{tuple(blob.shape)} {blob.dtype} on {blob.device}" if torch.is_tensor(blob) else type(blob).__name__
        raise RuntimeError(f"stream_park: unsupported operands: the blob must be ({n}, {lay.record}) uint8 on {dev}, got {got}")
    for t in tensors + [blob]:
        lib.check_tensor(t)
    a = ParkArgs()
    for i, t in enumerate(tensors):
        a.base[i], a.row_stride[i], a.row_bytes[i], a.blob_off[i] = t.data_ptr(), t.stride(0) * t.element_size(), lay.row_bytes[i], lay.offsets[i]
    a.rows, a.blob, a.blob_stride = m.idx.data_ptr(), blob.data_ptr(), blob.stride(0) if n > 1 or restore else lay.record
    a.n_tensors, a.n_sessions, a.flags = len(tensors), n, PARK_RESTORE if restore else 0
    if not stream_park_args_ok(a):
        raise RuntimeError(f"stream_park: unsupported operands: rows of {lay.row_bytes} bytes at strides {[int(a.row_stride[i]) for i in range(len(tensors))]}, "
                           f"blob row stride {blob.stride(0)} (16-byte multiples, rows inside their strides, records inside the blob's)")
    _launch(lib.c.aum_stream_park, a, blob, lib, "stream_park", (n, len(tensors), lay.record))
    return blob


# ---- a hop through all blocks in one library call (aum_stream_in_tm, aum_stream_out_tm, aum_stream_layers) ----
STREAM_STACK_WIDTHS = ((192, 384), (384, 768), (768, 1536))     # (d_model, d_inner) the two projection kernels are built for


def _al16p(*ptrs):
    return all(p is None or p % 16 == 0 for p in ptrs)


def stream_in_args_ok(a):
    """ss_in_check of csrc/stream_stack_kernels.h on a filled StreamInArgs, rule for rule"""
    if not (a.hidden and a.norm_weight and a.w_in and a.residual_out and a.xz):
        return False
    if a.total <= 0 or a.d_model <= 0 or a.dim <= 0:
        return False
    if a.dtype not in (AUM_BF16, AUM_F16):
        return False
    if (a.d_model, a.dim) not in STREAM_STACK_WIDTHS:
        return False
    if a.hidden_ts < a.d_model or a.xz_ts < 2 * a.dim or a.ldw < a.d_model or ((a.hidden_ts | a.xz_ts | a.ldw) & 7):
        return False
    if not _al16p(a.hidden, a.residual_in, a.norm_weight, a.w_in, a.residual_out, a.xz):
        return False
    if a.residual_in == a.residual_out:
        return False
    return a.total * max(a.hidden_ts, a.xz_ts) * 2 <= (1 << 31) - 1


def stream_out_args_ok(a):
    """ss_out_check of csrc/stream_stack_kernels.h on a filled StreamOutArgs, rule for rule"""
    if not (a.y and a.w_out and a.out):
        return False
    if a.total <= 0 or a.d_model <= 0 or a.dim <= 0:
        return False
    if a.dtype not in (AUM_BF16, AUM_F16):
        return False
    if (a.d_model, a.dim) not in STREAM_STACK_WIDTHS:
        return False
    if a.y_ts < a.dim or a.out_ts < a.d_model or a.ldw < a.dim or ((a.y_ts | a.out_ts | a.ldw) & 7):
        return False
    if not _al16p(a.y, a.w_out, a.out) or a.y == a.out:
        return False
    return a.total * max(a.y_ts, a.out_ts) * 2 <= (1 << 31) - 1


def _rows16(name, t, last, lib):
    lib.check_tensor(t)
    if t.dim() != 2 or t.shape[1] != last or t.stride(1) != 1 or t.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"{name}: expected 16-bit (total, {last}) rows with the last axis contiguous, got {tuple(t.shape)} {t.dtype}")
    return t.stride(0) if t.shape[0] > 1 else last


def stream_in(hidden, norm_weight, w_in, residual=None, eps=1e-5, lib=None):
    """Fused add + RMSNorm + in_proj of a streaming hop in ONE launch (aum_stream_in_tm): hidden (total, d_model) 16-bit rows, residual fp32
    (total, d_model) contiguous or None, norm_weight (d_model) fp32, w_in (2 dim, d_model) in hidden's dtype -> (xz (total, 2 dim),
    residual_out fp32 (total, d_model), a new tensor).  residual_out and the normed row behind xz are rmsnorm_fwd's bits; every xz element
    is one rounding of an fp32 sum of exact products; a row's bits do not depend on the other rows of the call."""
    lib = lib or get()
    d_model = hidden.shape[-1]
    a = StreamInArgs()
    a.hidden_ts = _rows16("stream_in", hidden, d_model, lib)
    for t in (norm_weight, w_in, residual):
        lib.check_tensor(t)
    total, n2 = hidden.shape[0], w_in.shape[0]
    if (w_in.dim() != 2 or w_in.dtype != hidden.dtype or w_in.shape[1] != d_model or w_in.stride(1) != 1 or norm_weight.dtype != torch.float32
            or norm_weight.shape != (d_model,) or not norm_weight.is_contiguous()
            or (residual is not None and (residual.dtype != torch.float32 or residual.shape != hidden.shape or not residual.is_contiguous()))):
        raise RuntimeError("stream_in: unsupported operands: w_in (2 dim, d_model) in hidden's dtype, norm_weight fp32 (d_model), residual fp32 contiguous")
    xz = torch.empty((total, n2), dtype=hidden.dtype, device=hidden.device)
    res_out = torch.empty((total, d_model), dtype=torch.float32, device=hidden.device)
    a.hidden, a.residual_in, a.norm_weight, a.w_in, a.residual_out, a.xz = _ptr(hidden), _ptr(residual), _ptr(norm_weight), _ptr(w_in), _ptr(res_out), _ptr(xz)
    a.xz_ts, a.total, a.d_model, a.dim, a.ldw, a.dtype, a.eps = n2, total, d_model, n2 // 2, w_in.stride(0), _DT[hidden.dtype], eps
    if n2 % 2 or not stream_in_args_ok(a):
        raise RuntimeError(f"stream_in: unsupported operands hidden {tuple(hidden.shape)} {hidden.dtype} strides {hidden.stride()}, w_in {tuple(w_in.shape)}")
    _launch(lib.c.aum_stream_in_tm, a, hidden, lib, "stream_in", (total, d_model, n2))
    return xz, res_out


def stream_out(y, w_out, lib=None):
    """out_proj of a streaming hop (aum_stream_out_tm): y (total, dim) 16-bit rows, w_out (d_model, dim) in y's dtype -> (total, d_model);
    the numeric contract of stream_in's projection."""
    lib = lib or get()
    dim = y.shape[-1]
    a = StreamOutArgs()
    a.y_ts = _rows16("stream_out", y, dim, lib)
    lib.check_tensor(w_out)
    if w_out.dim() != 2 or w_out.dtype != y.dtype or w_out.shape[1] != dim or w_out.stride(1) != 1:
        raise RuntimeError("stream_out: unsupported operands: w_out (d_model, dim) in y's dtype, rows contiguous")
    total, d_model = y.shape[0], w_out.shape[0]
    out = torch.empty((total, d_model), dtype=y.dtype, device=y.device)
    a.y, a.w_out, a.out = _ptr(y), _ptr(w_out), _ptr(out)
    a.out_ts, a.total, a.d_model, a.dim, a.ldw, a.dtype = d_model, total, d_model, dim, w_out.stride(0), _DT[y.dtype]
    if not stream_out_args_ok(a):
        raise RuntimeError(f"stream_out: unsupported operands y {tuple(y.shape)} {y.dtype} strides {y.stride()}, w_out {tuple(w_out.shape)}")
    _launch(lib.c.aum_stream_out_tm, a, y, lib, "stream_out", (total, dim, d_model))
    return out


def stream_layers_scratch_layout(total, d_model, dim, ncols):
    """ss_ws of csrc/stream_stack_kernels.h: byte offsets (xz, y, hid0, hid1, res0, res1, block), the block scratch's size and the total"""
    up = lambda n: (n + 15) // 16 * 16
    block_bytes = 2 * (2 * total * dim + total * ncols)         # aum_stream_block_scratch_bytes
    offs, at = [], 0
    for n in (total * 2 * dim * 2, total * dim * 2, total * d_model * 2, total * d_model * 2, total * d_model * 4, total * d_model * 4, block_bytes):
        offs.append(at)
        at += up(n)
    return offs, block_bytes, at


def stream_layers_table(layers):
    """the HOST table of aum_stream_layers: one StreamLayer record per block from dicts / objects naming STREAM_LAYER_POINTERS as tensors
    (None: NULL).  The caller keeps the tensors alive; the pool pointers may be rewritten per call."""
    table = (StreamLayer * len(layers))()
    for rec, L in zip(table, layers):
        for n in STREAM_LAYER_POINTERS:
            setattr(rec, n, _ptr(L[n]))
    return table


_STREAM_LAYER_PARAMS = tuple(n for n in STREAM_LAYER_POINTERS if n not in ("conv_state", "state"))


def stream_layers_records_ok(table, depth):
    """the rules of stream_layers_check for the PARAMETER pointers of the records (everything but the two pools): the required ones are
    there, all are 16-byte aligned.  They do not change between the calls of a StreamStack, which asks once and passes records_ok=True"""
    recs = [table[l] for l in range(depth)]
    return (all(getattr(L, n) for L in recs for n in _STREAM_LAYER_PARAMS if n not in ("conv_bias", "D", "delta_bias"))
            and all(_al16p(*(getattr(L, n) or None for n in _STREAM_LAYER_PARAMS)) for L in recs))


def stream_layers_supported(a, table=None, records_ok=False):
    """stream_layers_check of csrc/aum_api_tm.inc on a filled StreamLayersArgs (table: its StreamLayer array; None: read through a.layers),
    rule for rule and in its order: what aum_stream_layers takes, and what it refuses before its first launch.  records_ok=True: the
    parameter pointers of this table have passed stream_layers_records_ok; only the pool pointers are looked at"""
    if not (a.layers and a.hidden and a.hidden_out and a.residual_out and a.workspace and a.cu_seqlens):
        return False
    if min(a.depth, a.total, a.nseq, a.nrows, a.d_model, a.dim, a.ncols, a.rank) <= 0:
        return False
    if table is None:
        table = C.cast(a.layers, C.POINTER(StreamLayer))
    recs = [table[l] for l in range(a.depth)]
    names = ("conv_state", "state") if records_ok else STREAM_LAYER_POINTERS
    if any(not getattr(L, n) for L in recs for n in names if n not in ("conv_bias", "D", "delta_bias")):
        return False
    if a.dtype not in (AUM_BF16, AUM_F16):
        return False
    if (a.d_model, a.dim) not in STREAM_STACK_WIDTHS:
        return False
    if not _al16p(a.workspace, a.hidden_out, a.residual_out) or a.residual_in == a.residual_out:
        return False
    offs, block_bytes, need = stream_layers_scratch_layout(a.total, a.d_model, a.dim, a.ncols)
    if a.workspace_bytes < need:
        return False
    lim = (1 << 31) - 1
    # what ss_in_check / stream_block_check / ss_out_check see of layer l: the workspace offsets are multiples of 16, the pitches the widths
    if (a.cu_seqlens | (a.state_indices or 0)) & 3:
        return False
    if a.flags & ~(STREAM_NO_COMMIT | STREAM_PEEK_LAST) or not 1 <= a.max_len <= STREAM_BLOCK_MAX_T:
        return False
    if (not xdt_fwd_shape_ok(a.ncols, a.dim) or a.rank % 8 or a.rank > 64 or a.rank + 32 > a.ncols or a.ldwx < a.dim or a.ldwdt < a.rank
            or a.ldwx % 8 or a.ldwdt % 8):
        return False
    if a.hidden_ts < a.d_model or a.hidden_ts & 7 or not _al16p(a.hidden, a.residual_in):
        return False
    if a.total * max(a.hidden_ts, 2 * a.dim) * 2 > lim or (2 * a.dim + a.dim) * 2 * a.total > lim:
        return False
    return all(_al16p(*(getattr(L, n) or None for n in names)) for L in recs)


def stream_layers_args(hidden, table, depth, conv_state0, seq_map, workspace, hidden_out, residual_out, *, dim, rank, ncols, ldwx, ldwdt, eps,
                       commit=True, peek=False, residual=None):
    """the filled StreamLayersArgs of one hop (stream_layers makes it; tests alter it): hidden (total, d_model) rows, table from
    stream_layers_table, conv_state0 any layer's conv pool (for the row count)"""
    a = StreamLayersArgs()
    total, d_model = hidden.shape
    a.layers = C.cast(table, C.c_void_p)
    a.hidden, a.residual_in, a.hidden_out, a.residual_out, a.workspace = _ptr(hidden), _ptr(residual), _ptr(hidden_out), _ptr(residual_out), _ptr(workspace)
    a.cu_seqlens, a.state_indices = _ptr(seq_map.cu), _ptr(seq_map.idx)
    a.hidden_ts, a.workspace_bytes = (hidden.stride(0) if total > 1 else d_model), workspace.numel() * workspace.element_size()
    a.depth, a.total, a.nseq, a.nrows, a.max_len = depth, total, len(seq_map.lens), conv_state0.shape[0], max(seq_map.lens)
    a.d_model, a.dim, a.rank, a.ncols, a.ldwx, a.ldwdt, a.dtype = d_model, dim, rank, ncols, ldwx, ldwdt, _DT.get(hidden.dtype, -1)
    a.flags, a.eps = (0 if commit else STREAM_NO_COMMIT) | (STREAM_PEEK_LAST if peek else 0), eps
    return a


def stream_layers(hidden, table, depth, conv_state0, seq_map, *, dim, rank, ncols, ldwx, ldwdt, eps, commit=True, peek=False, residual=None,
                  workspace=None, lib=None, records_ok=False):
    """ALL blocks of a streaming hop in ONE library call (aum_stream_layers): per block stream_in -> stream_block -> stream_out, 3 * depth
    launches enqueued from a C loop.  hidden (total, d_model) 16-bit packed rows with seq_map (trusted: check_seq_map is the caller's);
    table: stream_layers_table of the blocks' parameters and pools (the pools advance in place; commit / peek as stream_block).
    workspace: a uint8 tensor of at least stream_layers_scratch_layout(...)[2] bytes, or None: allocated.
    Returns (hidden_out (total, d_model), residual_out fp32) of the last block.  Bit for bit the loop of the three calls."""
    lib = lib or get()
    for t in (hidden, conv_state0, workspace, residual):
        lib.check_tensor(t)
    if hidden.dim() != 2 or hidden.stride(1) != 1:
        raise RuntimeError("stream_layers: hidden must be (total, d_model) packed rows")
    total, d_model = hidden.shape
    if workspace is None:
        workspace = torch.empty(stream_layers_scratch_layout(total, d_model, dim, ncols)[2], dtype=torch.uint8, device=hidden.device)
    hidden_out = torch.empty((total, d_model), dtype=hidden.dtype, device=hidden.device)
    residual_out = torch.empty((total, d_model), dtype=torch.float32, device=hidden.device)
    a = stream_layers_args(hidden, table, depth, conv_state0, seq_map, workspace, hidden_out, residual_out, dim=dim, rank=rank, ncols=ncols,
                           ldwx=ldwx, ldwdt=ldwdt, eps=eps, commit=commit, peek=peek, residual=residual)
    if not stream_layers_supported(a, table, records_ok):
        raise RuntimeError(f"stream_layers: unsupported operands hidden {tuple(hidden.shape)} {hidden.dtype}, widths ({d_model}, {dim}), x_dbl "
                           f"{ncols} columns, rank {rank}, longest session {a.max_len}, workspace {a.workspace_bytes} bytes")
    _launch(lib.c.aum_stream_layers, a, hidden, lib, "stream_layers", (depth, total, d_model))
    return hidden_out, residual_out


def dtproj_tm_supported(x_dbl, rank, w):
    """shapes aum_dtproj_tm_fwd takes (include/aum_hip.h, ABI 9): 16-bit row-major x_dbl (ntok, >= rank) and dt_proj.weight (dim, rank)"""
    return (x_dbl.dim() == 2 and w.dim() == 2 and x_dbl.dtype == w.dtype and x_dbl.dtype in (torch.bfloat16, torch.float16)
            and w.shape[1] == rank and x_dbl.shape[1] >= rank and rank % 8 == 0 and rank <= 64 and w.shape[0] % 32 == 0
            and x_dbl.stride(1) == 1 and w.stride(1) == 1 and x_dbl.stride(0) % 8 == 0 and w.stride(0) % 8 == 0
            and x_dbl.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def dtproj_tm_fwd(x_dbl, rank, w, lib=None):
    """delta (ntok, dim) = x_dbl[:, :rank] @ w^T (SSI:468 on token-major rows): w = dt_proj.weight (dim, rank) in x_dbl's 16-bit dtype"""
    lib = lib or get()
    lib.check_tensor(x_dbl)
    lib.check_tensor(w)
    if not dtproj_tm_supported(x_dbl, rank, w):
        raise RuntimeError(f"dtproj_tm_fwd: unsupported operands {tuple(x_dbl.shape)} {x_dbl.dtype}, rank {rank}, weight {tuple(w.shape)} {w.dtype}")
    ntok, dim = x_dbl.shape[0], w.shape[0]
    out = torch.empty((ntok, dim), dtype=x_dbl.dtype, device=x_dbl.device)
    a = DtProjArgs()
    a.x, a.w, a.out = _ptr(x_dbl), _ptr(w), _ptr(out)
    a.ntok, a.dim, a.rank, a.ldx, a.ldw, a.ldo, a.dtype = ntok, dim, rank, x_dbl.stride(0), w.stride(0), dim, _DT[x_dbl.dtype]
    _launch(lib.c.aum_dtproj_tm_fwd, a, x_dbl, lib, "dtproj_tm_fwd", (ntok, dim, rank))
    return out


XDT_COLS, XDT_MAX_DIM = 80, 1536
XDT_COLS_FWD = (80, 56, 48)    # x_dbl widths aum_xdt_tm_fwd is built for (AuM-Base, AuM-Small, AuM-Tiny's 44 padded: Mamba.stream_params)
XDT_COLS_BWD = (80, 56)        # ... and aum_xdt_tm_bwd, each with its own dt_rank = width - 32 (48, 24) only


def xdt_fwd_shape_ok(ncols, dim):
    """the rule of csrc/xdt_args.h (xdt_fwd_shape_ok), shared by aum_xdt_tm_fwd and aum_stream_block_tm: a width the kernels are built for
    and W_x K-halves of whole 64-column steps"""
    return ncols in XDT_COLS_FWD and dim > 0 and dim % 128 == 0 and dim <= XDT_MAX_DIM


def xdt_tm_supported(u, wx, wdt):
    """shapes aum_xdt_tm_fwd takes (include/aum_hip.h, ABI 9): 16-bit row-major conv_out (ntok, dim), x_proj.weight (80 / 56 / 48, dim),
    dt_proj.weight (dim, rank)"""
    if not (u.dim() == 2 and wx.dim() == 2 and wdt.dim() == 2 and u.dtype == wx.dtype == wdt.dtype and u.dtype in (torch.bfloat16, torch.float16)):
        return False
    dim, rank = u.shape[1], wdt.shape[1]
    ok_t = lambda t: t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0
    return (xdt_fwd_shape_ok(wx.shape[0], dim) and wx.shape[1] == dim and wdt.shape[0] == dim and rank % 8 == 0
            and rank <= 64 and rank <= wx.shape[0]
            and ok_t(u) and ok_t(wx) and ok_t(wdt))


def xdt_tm_bwd_widths(dim, rank, dstate, dtype):
    """the widths aum_xdt_tm_bwd is built for: 16-bit rows of dx_dbl = [dt block (rank) | dB | dC (dstate each)] with rank + 2 * dstate in
    XDT_COLS_BWD.  What a caller asks before it prepares the transposed weights; xdt_tm_bwd_supported then checks the operands themselves"""
    return (rank + 2 * dstate in XDT_COLS_BWD and dstate == 16 and dim % 256 == 0 and dim <= XDT_MAX_DIM
            and dtype in (torch.bfloat16, torch.float16))


def xdt_tm_bwd_supported(ddelta, dbc, wdt_t, wx_t, du):
    """shapes aum_xdt_tm_bwd takes (include/aum_hip.h, ABI 10): 16-bit row-major ddelta / du (ntok, dim), fp32 dB | dC rows (ntok, 32),
    x_proj.weight^T (dim, ncols) and dt_proj.weight^T (ncols - 32, dim) with ncols = 80 (AuM-Base: rank 48) or 56 (AuM-Small: rank 24)"""
    if not (ddelta.dim() == 2 and du.shape == ddelta.shape and ddelta.dtype == du.dtype == wdt_t.dtype == wx_t.dtype
            and dbc.dtype == torch.float32 and dbc.dim() == 2):
        return False
    if wx_t.dim() != 2 or wdt_t.dim() != 2:
        return False
    ntok, dim = ddelta.shape
    ncols = wx_t.shape[1]
    ok_t = lambda t, m=8: t.stride(1) == 1 and t.stride(0) % m == 0 and t.data_ptr() % 16 == 0
    return (xdt_tm_bwd_widths(dim, ncols - 32, 16, ddelta.dtype) and wx_t.shape == (dim, ncols) and wdt_t.shape == (ncols - 32, dim)
            and dbc.shape == (ntok, 32) and ok_t(ddelta) and ok_t(du) and ok_t(wdt_t) and ok_t(wx_t) and ok_t(dbc, 4))


def xdt_tm_bwd(ddelta, dbc, wdt_t, wx_t, du, lib=None):
    """dx_dbl (ntok, ncols) = [ddelta @ wdt_t^T | dbc] in ddelta's dtype, and du += dx_dbl @ wx_t^T IN PLACE (SSI:570-574, 587, 590 on
    token-major rows: one pass over ddelta and du).  ncols = wx_t.shape[1]: 80 or 56, the dt block its first ncols - 32 columns.
    Returns dx_dbl."""
    lib = lib or get()
    for t in (ddelta, dbc, wdt_t, wx_t, du):
        lib.check_tensor(t)
    if not xdt_tm_bwd_supported(ddelta, dbc, wdt_t, wx_t, du):
        raise RuntimeError(f"xdt_tm_bwd: unsupported operands {tuple(ddelta.shape)} {ddelta.dtype}, {tuple(dbc.shape)}, {tuple(wdt_t.shape)}, {tuple(wx_t.shape)}")
    ntok, dim = ddelta.shape
    ncols = wx_t.shape[1]
    dx_dbl = torch.empty((ntok, ncols), dtype=ddelta.dtype, device=ddelta.device)
    a = XdtBwdArgs()
    a.ddelta, a.dbc, a.wdt_t, a.wx_t, a.du, a.dx_dbl = _ptr(ddelta), _ptr(dbc), _ptr(wdt_t), _ptr(wx_t), _ptr(du), _ptr(dx_dbl)
    a.ntok, a.dim, a.rank, a.ncols = ntok, dim, ncols - 32, ncols
    a.ldd, a.lddbc, a.ldwdt, a.ldwx, a.ldu, a.ldx = ddelta.stride(0), dbc.stride(0), wdt_t.stride(0), wx_t.stride(0), du.stride(0), ncols
    a.dtype = _DT[ddelta.dtype]
    _launch(lib.c.aum_xdt_tm_bwd, a, ddelta, lib, "xdt_tm_bwd", (ntok, dim))
    return dx_dbl


def xdt_tm_fwd(u, wx, wdt, lib=None, delta_bias=None, delta_softplus=False):
    """(x_dbl (ntok, ncols), delta (ntok, dim)) = (u @ wx^T, x_dbl[:, :rank] @ wdt^T) in one pass over u (SSI:467-468 on token-major rows).
    delta_softplus: delta = softplus(x_dbl[:, :rank] @ wdt^T + delta_bias) instead, rounded once -- the activated delta a token-major scan
    takes with delta_activated=True (delta_bias: (dim) fp32 or None)."""
    lib = lib or get()
    for t in (u, wx, wdt):
        lib.check_tensor(t)
    if not xdt_tm_supported(u, wx, wdt):
        raise RuntimeError(f"xdt_tm_fwd: unsupported operands {tuple(u.shape)} {u.dtype}, {tuple(wx.shape)}, {tuple(wdt.shape)}")
    if delta_bias is not None and not delta_softplus:
        raise RuntimeError("xdt_tm_fwd: delta_bias is only added together with the softplus (delta_softplus=True)")
    if delta_softplus and lib.host:
        # the lane-array build's aum_xdt_tm_fwd is a plain loop that ignores the activation fields: it would hand back the raw product
        raise RuntimeError("xdt_tm_fwd: delta_softplus needs the device library")
    if delta_bias is not None:
        delta_bias = _f32c(delta_bias)
        lib.check_tensor(delta_bias)
        if delta_bias.shape != (u.shape[1],) or delta_bias.data_ptr() % 16:
            raise RuntimeError(f"xdt_tm_fwd: delta_bias must be a 16-byte aligned ({u.shape[1]},) fp32 tensor")
    ntok, dim = u.shape
    rank = wdt.shape[1]
    ncols = wx.shape[0]
    x_dbl = torch.empty((ntok, ncols), dtype=u.dtype, device=u.device)
    delta = torch.empty((ntok, dim), dtype=u.dtype, device=u.device)
    a = XdtArgs()
    a.u, a.wx, a.wdt, a.x_dbl, a.delta = _ptr(u), _ptr(wx), _ptr(wdt), _ptr(x_dbl), _ptr(delta)
    a.ntok, a.dim, a.rank, a.ncols = ntok, dim, rank, ncols
    a.ldu, a.ldwx, a.ldwdt, a.ldx, a.ldd, a.dtype = u.stride(0), wx.stride(0), wdt.stride(0), ncols, dim, _DT[u.dtype]
    a.delta_bias, a.flags = _ptr(delta_bias), (XDT_DELTA_SOFTPLUS if delta_softplus else 0)
    _launch(lib.c.aum_xdt_tm_fwd, a, u, lib, "xdt_tm_fwd", (ntok, dim, rank))
    return x_dbl, delta


def conv1d_tm_supported(x, width):
    """the token-major conv takes (batch, len, dim) views with contiguous channels, 16-byte aligned rows and width <= 4"""
    if x.dim() != 3 or x.dtype not in _DT or width > 4 or (x.stride(2) != 1 and x.shape[2] != 1):
        return False
    es = x.element_size()
    bs, ts = _tm3(x, "x", x.shape[2])
    return x.shape[2] % (16 // es) == 0 and x.data_ptr() % 16 == 0 and (ts * es) % 16 == 0 and (bs * es) % 16 == 0


def _al16(t):
    """the kernels read weights with 16-byte accesses: a parameter that is a misaligned view gets its own storage"""
    return t if t is None or t.data_ptr() % 16 == 0 else t.detach().clone()


def _conv_weights(weight, bias, dim, align16):
    """weight (dim, width) / (dim, 1, width) and bias (dim) | None as the conv kernels read them: fp32 contiguous, and (align16: the
    token-major kernels) at 16-byte addresses.  The caller holds them until its launch is enqueued."""
    weight, bias = _f32c(weight.reshape(dim, -1)), _f32c(bias)
    return (_al16(weight), _al16(bias)) if align16 else (weight, bias)


def _conv_flags(silu, reverse=False, generic=False):
    return (CONV_SILU if silu else 0) | (CONV_REVERSE if reverse else 0) | (CONV_GENERIC if generic else 0)


def _check_conv_dy(lib, dy, x):
    lib.check_tensor(dy)
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise RuntimeError(f"dy: expected x's dtype and shape ({x.dtype}, {tuple(x.shape)}), got {dy.dtype}, {tuple(dy.shape)}")


def _fill_conv_tm(a, x, weight, bias, silu, reverse):
    """what the forward and backward of the token-major conv share in ConvTmArgs: x, the converted weight and bias, sizes, dtype, flags"""
    batch, length, dim = x.shape
    a.x, a.weight, a.bias = _ptr(x), _ptr(weight), _ptr(bias)
    a.x_bs, a.x_ts = _tm3(x, "x", dim)
    a.batch, a.dim, a.len, a.width, a.dtype = batch, dim, length, weight.shape[1], _DT[x.dtype]
    a.flags = _conv_flags(silu, reverse)


def _fill_conv_cm(a, x, weight, bias, silu, reverse, generic):
    """the same for the channel-major conv's ConvArgs"""
    batch, dim, length = x.shape
    a.x, a.weight, a.bias = _ptr(x), _ptr(weight), _ptr(bias)
    a.x_bs, a.x_ds = x.stride(0), x.stride(1)
    a.batch, a.dim, a.len, a.width, a.dtype = batch, dim, length, weight.shape[1], _DT[x.dtype]
    a.flags = _conv_flags(silu, reverse, generic)


def conv1d_tm_fwd(x, weight, bias=None, silu=True, reverse=False, lib=None):
    """causal_conv1d_fn on a token-major (batch, len, dim) view (x may be the first half of the in_proj output rows) -> y (batch, len,
    dim) contiguous.  weight (dim, width) / (dim, 1, width)."""
    lib = lib or get()
    lib.check_tensor(x)
    batch, length, dim = x.shape
    weight, bias = _conv_weights(weight, bias, dim, True)
    y = torch.empty((batch, length, dim), dtype=x.dtype, device=x.device)
    a = ConvTmArgs()
    _fill_conv_tm(a, x, weight, bias, silu, reverse)
    a.y = _ptr(y)
    a.y_bs, a.y_ts = _tm3(y, "y", dim)
    _launch(lib.c.aum_conv1d_tm_fwd, a, x, lib, "conv_tm_fwd", (batch, dim, length, x.element_size()))
    return y


def conv1d_tm_prefill(x, conv_state, weight, bias=None, silu=True, lib=None):
    """The causal conv of a BACKLOG entered with a carried window: x (batch, T >= 1, dim) token-major view, conv_state (batch, dim, width)
    fp32 contiguous, advanced IN PLACE by T tokens -- what conv1d_tm_chunk computes, on the time-parallel kernel of the offline forward
    and without a kernel of its own: the rows [last width - 1 carried inputs ; x] go through conv1d_tm_fwd and the first width - 1
    outputs are dropped; the last `width` inputs are then written back into conv_state (T < width: the old entries shift, as in
    k_convt_chunk).  A zero window gives the same result as the plain causal conv (conv1d_tm_fwd on x alone: its rows before the first
    are zero).  The carried inputs enter the rows in x's dtype: a window that was filled from activations of that dtype -- every
    window this library writes -- is carried exactly; conv_state itself only ever holds the inputs as they were (no rounding).
    Returns y (batch, T, dim) in x's dtype, a view with 16-byte aligned rows."""
    lib = lib or get()
    for t in (x, conv_state):
        lib.check_tensor(t)
    if not conv1d_tm_chunk_supported(x, conv_state):
        raise RuntimeError(f"conv1d_tm_prefill: unsupported operands x {tuple(x.shape)} {x.dtype} strides {x.stride()}, conv_state "
                           f"{tuple(conv_state.shape)} {conv_state.dtype} (need (batch, T, dim) token-major, 16-byte rows; fp32 contiguous (batch, dim, width <= 4))")
    batch, T, dim = x.shape
    width = conv_state.shape[2]
    if weight.reshape(dim, -1).shape[1] != width:
        raise RuntimeError("conv1d_tm_prefill: weight (dim, width) and conv_state (rows, dim, width) disagree on the width")
    rows = torch.empty((batch, width - 1 + T, dim), dtype=x.dtype, device=x.device)
    rows[:, :width - 1] = conv_state[:, :, 1:].transpose(1, 2)
    rows[:, width - 1:] = x
    y = conv1d_tm_fwd(rows, weight, bias, silu, lib=lib)[:, width - 1:]
    if T >= width:
        conv_state.copy_(x[:, T - width:].transpose(1, 2))
    else:
        conv_state[:, :, :width - T] = conv_state[:, :, T:].clone()
        conv_state[:, :, width - T:] = x.transpose(1, 2)
    return y


def conv1d_tm_bwd(x, weight, bias, dy, silu=True, reverse=False, dx_out=None, lib=None, partials=False):
    """-> (dx (batch, len, dim), dweight (dim, width) fp32, dbias (dim) fp32 | None); dx_out may be a strided token-major view (the
    first half of d(in_proj output)).  The per-wave partial sums of dweight / dbias are added in a fixed order (aum_sum_rows_multi);
    partials=True: -> (dx, dw_part (nparts, dim, width), db_part (nparts, dim) | None) for a caller that sums them with other sets."""
    lib = lib or get()
    lib.check_tensor(x)
    _check_conv_dy(lib, dy, x)
    batch, length, dim = x.shape
    weight, bias = _conv_weights(weight, bias, dim, True)
    dy = dy if dy.stride(2) == 1 else dy.contiguous()
    dx = dx_out if dx_out is not None else torch.empty((batch, length, dim), dtype=x.dtype, device=x.device)
    nparts = int(lib.c.aum_conv1d_tm_nparts(batch, length))
    f32 = dict(dtype=torch.float32, device=x.device)
    dw_part = torch.empty((nparts, dim, weight.shape[1]), **f32)
    db_part = torch.empty((nparts, dim), **f32) if bias is not None else None
    a = ConvTmArgs()
    _fill_conv_tm(a, x, weight, bias, silu, reverse)
    a.dy, a.dx, a.dw_part, a.db_part = _ptr(dy), _ptr(dx), _ptr(dw_part), _ptr(db_part)
    a.dy_bs, a.dy_ts = _tm3(dy, "dy", dim)
    a.dx_bs, a.dx_ts = _tm3(dx, "dx", dim)
    _launch(lib.c.aum_conv1d_tm_bwd, a, x, lib, "conv_tm_bwd", (batch, dim, length, x.element_size()))
    if partials:
        return dx, dw_part, db_part
    if db_part is None:
        return dx, sum_rows(dw_part, lib=lib), None           # (dim, width): the partial rows are in the weight's own layout
    dweight, dbias = sum_rows_multi([dw_part, db_part], lib=lib)      # both partial sets in one launch
    return dx, dweight, dbias


def conv1d_fwd(x, weight, bias=None, silu=True, reverse=False, dmajor=False, generic=False, lib=None):
    """causal_conv1d_cuda.causal_conv1d_fwd(x, weight(dim,width), bias, None, silu) -> y (batch, dim, len) contiguous."""
    lib = lib or get()
    _unit(x, "x")
    lib.check_tensor(x)
    batch, dim, length = x.shape
    weight, bias = _conv_weights(weight, bias, dim, False)
    y = _alloc(batch, dim, length, x.dtype, x.device, dmajor)
    a = ConvArgs()
    _fill_conv_cm(a, x, weight, bias, silu, reverse, generic)
    a.y, a.y_bs, a.y_ds = _ptr(y), y.stride(0), y.stride(1)
    _launch(lib.c.aum_causal_conv1d_fwd, a, x, lib, "conv_fwd", (batch, dim, length, x.element_size()))
    return y


def conv1d_bwd(x, weight, bias, dy, silu=True, reverse=False, dx_out=None, generic=False, lib=None):
    """causal_conv1d_cuda.causal_conv1d_bwd -> (dx, dweight(dim,width) fp32, dbias fp32|None); dx_out may be a
    preallocated strided view written in place (SSI:594-596)."""
    lib = lib or get()
    _unit(x, "x")
    _unit(dy, "dy")
    lib.check_tensor(x)
    _check_conv_dy(lib, dy, x)
    batch, dim, length = x.shape
    weight, bias = _conv_weights(weight, bias, dim, False)
    dx = dx_out if dx_out is not None else torch.empty((batch, dim, length), dtype=x.dtype, device=x.device)
    _unit(dx, "dx")
    # dweight / dbias accumulate (one fp32 atomic per wave and tap): one zero fill for both
    zb = torch.zeros((weight.numel() + (dim if bias is not None else 0),), dtype=torch.float32, device=x.device)
    dw = zb[:weight.numel()].view_as(weight)
    db = zb[weight.numel():] if bias is not None else None
    a = ConvArgs()
    _fill_conv_cm(a, x, weight, bias, silu, reverse, generic)
    a.dy, a.dx, a.dweight, a.dbias = _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db)
    a.dy_bs, a.dy_ds, a.dx_bs, a.dx_ds = dy.stride(0), dy.stride(1), dx.stride(0), dx.stride(1)
    _launch(lib.c.aum_causal_conv1d_bwd, a, x, lib, "conv_bwd", (batch, dim, length, x.element_size()))
    return dx, dw, db


def _norm_refuse(name, t, rows, cols, dt=None):
    raise RuntimeError(f"{name}: expected ({rows}, {cols}){f' {dt}' if dt else ''}, unit column stride, got {tuple(t.shape)} {t.dtype}, {t.stride()}")


def _norm_fwd(lib, entry, name, x, weight, residual, residual_dtype, eps, generic, scale=None):
    """The forward of the add + RMSNorm pair, plain (aum_rmsnorm_fwd, NormArgs) or with scale = (row_scale, rows_per_scale) behind stochastic
    depth (aum_rmsnorm_drop_fwd, NormDropArgs with the same NormArgs as its base).  -> (y, rstd, res_out | None)"""
    rows, cols = x.shape
    lib.check_tensor(x)
    if x.stride(1) != 1:
        _norm_refuse("x", x, rows, cols)
    if residual is not None:
        lib.check_tensor(residual)
        if residual.shape != x.shape or residual.stride(1) != 1:
            _norm_refuse("residual", residual, rows, cols)
        residual_dtype = residual.dtype
    need_res_out = residual is not None or (residual_dtype is not None and residual_dtype != x.dtype)
    d = a = NormArgs()
    if scale is not None:               # the same NormArgs as the base of a NormDropArgs; the drop pair always has a residual
        d = NormDropArgs()
        a, row_scale = d.base, _row_scale(*scale, rows, x, lib)
        d.row_scale, d.rows_per_scale = _ptr(row_scale), scale[1]
    weight = _f32c(weight)
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    res_out = torch.empty((rows, cols), dtype=residual_dtype, device=x.device) if need_res_out else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    a.x, a.residual, a.weight, a.y, a.residual_out, a.rstd_out = map(_ptr, (x, residual, weight, y, res_out, rstd))
    a.row_stride_x, a.row_stride_y = x.stride(0), y.stride(0)
    if residual is not None:
        a.row_stride_res = residual.stride(0)
    if res_out is not None:
        a.row_stride_res_out = res_out.stride(0)
    a.eps, a.rows, a.cols = eps, rows, cols
    a.x_dtype = a.y_dtype = _DT[x.dtype]
    a.res_dtype = _DT[residual_dtype] if need_res_out else _DT[x.dtype]
    a.flags = NORM_GENERIC if generic else 0
    _launch(entry, d, x, lib, name, (rows, cols, x.element_size()))
    return y, rstd, res_out


def _norm_bwd(lib, entry, name, dy, x_saved, weight, rstd, dresidual, own_dres_in, x_dtype, generic, dw_out, scale=None):
    """The backward of the pair, plain or scaled as _norm_fwd.  own_dres_in: dresidual_in is a buffer of its own.  -> (dx, dweight, dres_in | None)"""
    rows, cols = x_saved.shape
    x_dtype = x_dtype or x_saved.dtype
    lib.check_tensor(dy)
    if dy.shape != x_saved.shape or dy.stride(1) != 1 or dy.dtype != x_dtype:
        _norm_refuse("dy", dy, rows, cols, x_dtype)
    lib.check_tensor(x_saved)
    if x_saved.stride(1) != 1:
        _norm_refuse("x_saved", x_saved, rows, cols)
    if dresidual is not None:
        lib.check_tensor(dresidual)
        if dresidual.shape != x_saved.shape or dresidual.stride(1) != 1 or dresidual.dtype != x_saved.dtype:
            _norm_refuse("dresidual", dresidual, rows, cols, x_saved.dtype)
    lib.check_tensor(rstd)
    if rstd.shape != (rows,) or rstd.dtype != torch.float32 or not rstd.is_contiguous():
        raise RuntimeError(f"rstd: expected the contiguous fp32 ({rows},) tensor of the forward, got {tuple(rstd.shape)} {rstd.dtype}, strides {rstd.stride()}")
    d = a = NormArgs()
    if scale is not None:
        d = NormDropArgs()
        a, row_scale = d.base, _row_scale(*scale, rows, dy, lib)
        d.row_scale, d.rows_per_scale = _ptr(row_scale), scale[1]
    weight = _f32c(weight)
    dx = torch.empty((rows, cols), dtype=x_dtype, device=dy.device)
    dres_in = torch.empty_like(x_saved, memory_format=torch.contiguous_format) if own_dres_in else None
    flags = NORM_GENERIC if generic else 0
    # the rows the kernel leaves sums in, and the rows to allocate (include/aum_hip.h: aum_rmsnorm_bwd_partial_rows)
    dwp = torch.empty((int(lib.c.aum_rmsnorm_bwd_partial_rows(rows, cols, flags)), cols), dtype=torch.float32, device=dy.device)
    a.x, a.dy, a.dresidual_out, a.weight, a.rstd_in = map(_ptr, (x_saved, dy, dresidual, weight, rstd))
    a.dx, a.dresidual_in, a.dweight_partial = _ptr(dx), _ptr(dres_in), _ptr(dwp)
    a.row_stride_x, a.row_stride_dy, a.row_stride_dx = x_saved.stride(0), dy.stride(0), dx.stride(0)
    if dresidual is not None:
        a.row_stride_dres_out = dresidual.stride(0)
    if dres_in is not None:
        a.row_stride_dres_in = dres_in.stride(0)
    a.rows, a.cols = rows, cols
    a.x_dtype = a.y_dtype = _DT[x_dtype]
    a.res_dtype = _DT[x_saved.dtype]
    a.flags = flags
    _launch(entry, d, dy, lib, name, (rows, cols, dy.element_size()))
    return dx, sum_rows(dwp, lib, out=dw_out), dres_in


def rmsnorm_fwd(x, weight, residual=None, eps=1e-5, residual_dtype=None, generic=False, lib=None):
    """_layer_norm_fwd(is_rms_norm=True) (LN:123-177).  x: (rows, cols).  Returns (y, rstd, residual_out) where
    residual_out is x itself when no new residual tensor is needed (LN:176-177)."""
    lib = lib or get()
    y, rstd, res_out = _norm_fwd(lib, lib.c.aum_rmsnorm_fwd, "rmsnorm_fwd", x, weight, residual, residual_dtype, eps, generic)
    return y, rstd, (res_out if res_out is not None else x)


def rmsnorm_bwd(dy, x_saved, weight, rstd, dresidual=None, has_residual=False, x_dtype=None, generic=False, lib=None, dw_out=None):
    """_layer_norm_bwd(is_rms_norm=True) (LN:293-377).  x_saved = residual_out of the forward.  Returns
    (dx [x_dtype], dweight fp32, dresidual_in | None)."""
    lib = lib or get()
    own = has_residual and (x_dtype or x_saved.dtype) != x_saved.dtype
    dx, dw, dres_in = _norm_bwd(lib, lib.c.aum_rmsnorm_bwd, "rmsnorm_bwd", dy, x_saved, weight, rstd, dresidual, own, x_dtype, generic, dw_out)
    return dx, dw, (dx if has_residual and not own else dres_in)


def _row_scale(row_scale, rows_per_scale, rows, like, lib):
    """the (rows / rows_per_scale,) fp32 per-sample factors of the scaled add + norm, checked against the row count"""
    lib.check_tensor(row_scale)
    if rows_per_scale < 1 or rows % rows_per_scale:
        raise ValueError(f"rmsnorm_drop: {rows} rows are not whole samples of {rows_per_scale} rows")
    if row_scale.dtype != torch.float32 or row_scale.dim() != 1 or row_scale.numel() != rows // rows_per_scale or row_scale.device != like.device:
        raise ValueError(f"rmsnorm_drop: row_scale must be ({rows // rows_per_scale},) fp32 on {like.device}, not "
                         f"{tuple(row_scale.shape)} {row_scale.dtype} on {row_scale.device}")
    return row_scale.detach().contiguous()


def rmsnorm_drop_fwd(x, weight, residual, row_scale, rows_per_scale, eps=1e-5, generic=False, lib=None):
    """rmsnorm_fwd behind stochastic depth on x (aum_rmsnorm_drop_fwd): residual_out = fma(s, x, residual) in fp32 with
    s = row_scale[row // rows_per_scale]; a sample with s == 0 has its x rows not read.  x, residual: (rows, cols); the residual is
    required.  Returns (y, rstd, residual_out), residual_out a new tensor in the residual's dtype."""
    lib = lib or get()
    if residual is None:
        raise ValueError("rmsnorm_drop_fwd: the factor multiplies x on its way into the add: a residual is required")
    return _norm_fwd(lib, lib.c.aum_rmsnorm_drop_fwd, "rmsnorm_drop_fwd", x, weight, residual, None, eps, generic, (row_scale, rows_per_scale))


def rmsnorm_drop_bwd(dy, x_saved, weight, rstd, row_scale, rows_per_scale, dresidual=None, x_dtype=None, generic=False, lib=None,
                     dw_out=None):
    """rmsnorm_bwd of rmsnorm_drop_fwd (aum_rmsnorm_drop_bwd).  x_saved = residual_out of the forward.  Returns (dx [x_dtype] = s * g
    rounded once, +0 where s == 0; dweight fp32 (into dw_out where given); dresidual_in = g in x_saved's dtype) -- always two buffers."""
    lib = lib or get()
    return _norm_bwd(lib, lib.c.aum_rmsnorm_drop_bwd, "rmsnorm_drop_bwd", dy, x_saved, weight, rstd, dresidual, True, x_dtype, generic, dw_out,
                     (row_scale, rows_per_scale))


def _norm_pool_operands(lib, name, lead, weight, rows_per_sample, others):
    """THE operand rule of the add + RMSNorm + mean pair: `lead` (the forward's x, the backward's saved residual_out) is (rows, cols) with
    unit column stride, rows whole samples of rows_per_sample, cols what the vectorised norm kernels take; others = [(name, tensor, shape,
    dtype)] are on the library's side with that shape and dtype and unit last stride.  -> (rows, cols, samples, the weight as fp32)"""
    rows, cols = lead.shape
    if rows_per_sample < 1 or rows < 1 or rows % rows_per_sample:
        raise ValueError(f"{name}: {rows} rows are not whole samples of {rows_per_sample} rows")
    if cols % 8 or cols > 2048:
        raise RuntimeError(f"{name}: {cols} columns: the pooled norm takes cols % 8 == 0 and cols <= 2048")
    samples = rows // rows_per_sample
    for what, t, shape, dt in others:
        lib.check_tensor(t)
        want = tuple(samples if s == "samples" else s for s in shape)
        if tuple(t.shape) != want or t.dtype != dt or (t.dim() and t.stride(-1) != 1 and t.shape[-1] != 1) or (t.dim() == 1 and not t.is_contiguous()):
            raise RuntimeError(f"{name}: {what} must be {want} {dt} with unit last stride, got {tuple(t.shape)} {t.dtype}, strides {t.stride()}")
    if weight.shape != (cols,):
        raise RuntimeError(f"{name}: weight must be ({cols},), got {tuple(weight.shape)}")
    return rows, cols, samples, _f32c(weight)


def _fill_norm_pool(q, lead_dtype, weight, rows, cols, rows_per_sample, eps=0.0):
    """THE filler of NormPoolArgs: what both directions share"""
    a = q.base
    a.weight, a.eps, a.rows, a.cols = _ptr(weight), eps, rows, cols
    a.x_dtype = a.y_dtype = _DT[lead_dtype]
    a.res_dtype, a.flags = _DT[torch.float32], 0
    q.rows_per_sample, q.reserved = rows_per_sample, 0
    return a


def rmsnorm_pool_fwd(x, weight, residual, rows_per_sample, eps=1e-5, save=True, lib=None):
    """add + RMSNorm + mean over a sample's rows (aum_rmsnorm_pool_fwd).  x (rows, cols) bf16 / fp16, residual (rows, cols) fp32, rows =
    samples x rows_per_sample -> (pooled (samples, cols) in x's dtype, rstd (rows,) | None, residual_out (rows, cols) fp32 | None); the
    last two are aum_rmsnorm_fwd's (what the backward needs) and exist with save=True.  The normalised rows are not stored."""
    lib = lib or get()
    lib.check_tensor(x)
    if x.dim() != 2 or x.dtype not in (torch.bfloat16, torch.float16) or x.stride(1) != 1:
        raise RuntimeError(f"rmsnorm_pool_fwd: x must be (rows, cols) bf16 / fp16 with unit column stride, got {tuple(x.shape)} {x.dtype}, {x.stride()}")
    if residual is None:
        raise ValueError("rmsnorm_pool_fwd: the residual stream is required")
    rows, cols, samples, weight = _norm_pool_operands(lib, "rmsnorm_pool_fwd", x, weight, rows_per_sample,
                                                      [("residual", residual, x.shape, torch.float32)])
    pooled = torch.empty((samples, cols), dtype=x.dtype, device=x.device)
    res_out = torch.empty((rows, cols), dtype=torch.float32, device=x.device) if save else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if save else None
    nchunk = int(lib.c.aum_rmsnorm_pool_partial_rows(rows_per_sample))
    part = torch.empty((samples * nchunk, cols), dtype=torch.float32, device=x.device) if nchunk > 1 else None
    q = NormPoolArgs()
    a = _fill_norm_pool(q, x.dtype, weight, rows, cols, rows_per_sample, eps)
    a.x, a.residual, a.residual_out, a.rstd_out = map(_ptr, (x, residual, res_out, rstd))
    a.row_stride_x, a.row_stride_res, a.row_stride_res_out = x.stride(0), residual.stride(0), cols
    q.pooled, q.pool_partial, q.row_stride_pooled = _ptr(pooled), _ptr(part), cols
    _launch(lib.c.aum_rmsnorm_pool_fwd, q, x, lib, "rmsnorm_pool_fwd", (rows, cols, x.element_size()))
    return pooled, rstd, res_out


def rmsnorm_pool_bwd(dpooled, x_saved, weight, rstd, rows_per_sample, lib=None, dw_out=None):
    """The backward of rmsnorm_pool_fwd (aum_rmsnorm_pool_bwd).  dpooled (samples, cols) bf16 / fp16; x_saved, rstd: the forward's
    residual_out and rstd.  Every row of sample s gets what rmsnorm_bwd writes for dy = (dpooled[s] / rows_per_sample) rounded to dpooled's
    dtype.  -> (dx (rows, cols) in dpooled's dtype, dweight fp32 (into dw_out where given), dresidual_in (rows, cols) fp32)"""
    lib = lib or get()
    lib.check_tensor(x_saved)
    if x_saved.dim() != 2 or x_saved.dtype != torch.float32 or x_saved.stride(1) != 1:
        raise RuntimeError(f"rmsnorm_pool_bwd: x_saved must be the forward's (rows, cols) fp32 residual_out, got {tuple(x_saved.shape)} {x_saved.dtype}")
    if dpooled.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"rmsnorm_pool_bwd: dpooled must be bf16 / fp16, got {dpooled.dtype}")
    rows, cols, samples, weight = _norm_pool_operands(lib, "rmsnorm_pool_bwd", x_saved, weight, rows_per_sample,
                                                      [("dpooled", dpooled, ("samples", x_saved.shape[1]), dpooled.dtype),
                                                       ("rstd", rstd, (x_saved.shape[0],), torch.float32)])
    dx = torch.empty((rows, cols), dtype=dpooled.dtype, device=dpooled.device)
    dres_in = torch.empty((rows, cols), dtype=torch.float32, device=dpooled.device)
    dwp = torch.empty((int(lib.c.aum_rmsnorm_bwd_partial_rows(rows, cols, 0)), cols), dtype=torch.float32, device=dpooled.device)
    q = NormPoolArgs()
    a = _fill_norm_pool(q, dpooled.dtype, weight, rows, cols, rows_per_sample)
    a.x, a.rstd_in, a.dx, a.dresidual_in, a.dweight_partial = map(_ptr, (x_saved, rstd, dx, dres_in, dwp))
    a.row_stride_x, a.row_stride_dx, a.row_stride_dres_in = x_saved.stride(0), cols, cols
    q.dpooled, q.row_stride_dpooled = _ptr(dpooled), dpooled.stride(0)
    _launch(lib.c.aum_rmsnorm_pool_bwd, q, dpooled, lib, "rmsnorm_pool_bwd", (rows, cols, dpooled.element_size()))
    return dx, sum_rows(dwp, lib, out=dw_out), dres_in


FBANK_AUG = 8     # columns of the per-clip augmentation table (include/aum_hip.h AUM_FBANK_AUG)


def fbank_fwd(wave, tables, target_length, norm_mean, norm_std, preemph=0.97, aug=None, noise=None, lib=None):
    """Log-mel frontend.  wave: (batch, n_samples) fp32 mean-removed; tables: dict(window, twiddle, mel_start_f,
    mel_count_f, mel_w [num_mel, stride], win, shift, padded) of device tensors built by aum.frontend.FbankTables.
    aug: optional (batch, 8) fp32 per-clip table [frames, f_lo, f_hi, t_lo, t_hi, roll, noise_amp, 0] applied in the kernel's
    store (ragged padding, SpecAug bands, noise, roll); noise: (batch, target_length, num_mel) fp32 uniform numbers."""
    lib = lib or get()
    batch, num_mel = wave.shape[0], tables["mel_w"].shape[0]
    out = torch.empty((batch, target_length, num_mel), dtype=torch.float32, device=wave.device)
    a = FbankArgs()
    _fill_fbank(a, lib, wave, tables, target_length, norm_mean, norm_std, preemph, aug, noise)
    a.out, a.out_bs = _ptr(out), out.stride(0)
    _launch(lib.c.aum_fbank_fwd, a, wave, lib, "fbank_fwd", (batch, target_length, num_mel))
    return out


def _fill_fbank(a, lib, wave, tables, target_length, norm_mean, norm_std, preemph, aug, noise):
    lib.check_tensor(wave)
    assert wave.dtype == torch.float32 and wave.stride(1) == 1
    batch, n = wave.shape
    win, shift, padded = tables["win"], tables["shift"], tables["padded"]
    num_frames = 0 if n < win else min(target_length, 1 + (n - win) // shift)
    num_mel, stride = tables["mel_w"].shape
    a.wave = _ptr(wave)
    a.window, a.twiddle = _ptr(tables["window"]), _ptr(tables["twiddle"])
    a.mel_start_f, a.mel_count_f, a.mel_w = _ptr(tables["mel_start_f"]), _ptr(tables["mel_count_f"]), _ptr(tables["mel_w"])
    a.wave_bs = wave.stride(0)
    a.batch, a.n_samples, a.win, a.shift, a.padded = batch, n, win, shift, padded
    a.num_frames, a.target_length, a.num_mel, a.mel_wstride = num_frames, target_length, num_mel, stride
    a.preemph, a.norm_mean, a.norm_inv2std = preemph, norm_mean, 1.0 / (2.0 * norm_std)
    a.log_floor = 1.1920928955078125e-07
    if aug is not None:
        assert aug.dtype == torch.float32 and aug.is_contiguous() and aug.shape == (batch, FBANK_AUG)
        lib.check_tensor(aug)
        a.aug = _ptr(aug)
    if noise is not None:
        assert aug is not None and noise.dtype == torch.float32 and noise.is_contiguous()
        assert noise.shape == (batch, target_length, num_mel)
        lib.check_tensor(noise)
        a.noise = _ptr(noise)


FBANK_STREAM_MAX_CAP = 2816     # FBS_MAX_CAP of csrc/fbank_kernels.h: the longest tail row the tail launch holds in registers


class WaveMap(typing.NamedTuple):
    """Where the sessions of one fbank_stream call are (wave_map builds it): session i brings samples[i] new samples behind the
    tail_lens[i] it holds in pool row rows[i], gets frames[i] new frames from clip index first_frames[i] on (those with clip index >=
    n_real[i] >= 0 are padding rows) and holds new_tail_lens[i] samples afterwards.  The host tuples, and the int32 device tensors the
    kernels read (one buffer: cu_samples | cu_frames | tail_len | first_frame | n_real | idx)."""
    samples: tuple
    tail_lens: tuple
    frames: tuple
    first_frames: tuple
    n_real: tuple
    rows: tuple
    new_tail_lens: tuple
    cap: int
    total_samples: int
    total_frames: int
    cu_samples: torch.Tensor
    cu_frames: torch.Tensor
    tail_len: torch.Tensor
    first_frame: torch.Tensor
    n_real_t: torch.Tensor
    idx: typing.Optional[torch.Tensor]


def wave_map(sample_counts, tail_lens, frame_counts, first_frames, n_real, rows=None, *, device, win=400, shift=160):
    """Built once per push of raw audio: per session the new samples m_i >= 0, the samples its tail row holds (0 <= tail_len < cap =
    win + 15 shift), its new frames >= 0 with the clip index of the first, the clip's real frame count (n_real < 0: no limit) and its
    pool row (distinct, >= 0; None: session i owns row i) -- checked here, on the host: every real frame must lie inside the samples
    there are (frames_i shift + (win - shift) <= tail_len_i + m_i), and the tail that remains must fit its row.  The five int32 arrays
    the kernel reads (and the rows) go to `device` in ONE pinned, non-blocking upload, as seq_map's do."""
    ms, tls, frs = tuple(int(n) for n in sample_counts), tuple(int(n) for n in tail_lens), tuple(int(n) for n in frame_counts)
    ffs, nrs = tuple(int(n) for n in first_frames), tuple(int(n) for n in n_real)
    n = len(ms)
    cap = win + 15 * shift
    if not n or not (len(tls) == len(frs) == len(ffs) == len(nrs) == n):
        raise ValueError(f"wave_map: one entry per session in every list, got {len(ms)}, {len(tls)}, {len(frs)}, {len(ffs)}, {len(nrs)}")
    if min(ms) < 0 or min(frs) < 0 or min(ffs) < 0:
        raise ValueError(f"wave_map: sample counts, frame counts and first frames >= 0, got {ms}, {frs}, {ffs}")
    if min(tls) < 0 or max(tls) >= cap:
        raise ValueError(f"wave_map: a tail holds 0 <= tail_len < {cap} samples, got {tls}")
    rws = tuple(range(n)) if rows is None else tuple(int(r) for r in rows)
    if len(rws) != n or min(rws) < 0 or len(set(rws)) != n:
        raise ValueError(f"wave_map: one pool row per session, distinct and >= 0, got {rws} for {n} sessions")
    new_tls = []
    for i in range(n):
        have = tls[i] + ms[i]
        real = frs[i] if nrs[i] < 0 else max(0, min(frs[i], nrs[i] - ffs[i]))
        if real > 0 and real * shift + (win - shift) > have:
            raise ValueError(f"wave_map: session {i} asks for {real} frames of {win} samples every {shift}, its tail and hop hold {have} samples")
        keep = have - min(frs[i] * shift, have)
        if keep >= cap:
            raise ValueError(f"wave_map: session {i} would be left with {keep} samples, a tail row holds fewer than {cap}")
        new_tls.append(keep)
    cu_s, cu_f = [0], [0]
    for m, f in zip(ms, frs):
        cu_s.append(cu_s[-1] + m)
        cu_f.append(cu_f[-1] + f)
    if cu_s[-1] + cu_f[-1] >= 1 << 31:
        raise ValueError("wave_map: too many samples")
    host = torch.tensor(cu_s + cu_f + list(tls) + list(ffs) + list(nrs) + (list(rws) if rows is not None else []), dtype=torch.int32)
    device = torch.device(device)
    if device.type == "cuda":
        host = host.pin_memory()
    buf = host.to(device, non_blocking=True)
    o = [0, n + 1, 2 * n + 2, 3 * n + 2, 4 * n + 2, 5 * n + 2]
    return WaveMap(ms, tls, frs, ffs, nrs, rws, tuple(new_tls), cap, cu_s[-1], cu_f[-1], buf[o[0]:o[1]], buf[o[1]:o[2]], buf[o[2]:o[3]],
                   buf[o[3]:o[4]], buf[o[4]:o[5]], buf[o[5]:] if rows is not None else None)


def fbank_stream_supported(wave, tails, tables):
    """the limits of aum_fbank_stream_fwd (include/aum_hip.h): the padded == 512 tables (16 kHz / 25 ms), packed fp32 samples (total,),
    an fp32 contiguous (nrows >= 1, win + 15 shift <= 2816) pool of tails on the samples' device"""
    cap = tables["win"] + 15 * tables["shift"]
    return (tables["padded"] == 512 and wave.dim() == 1 and wave.dtype == torch.float32 and wave.is_contiguous()
            and tails.dim() == 2 and tails.dtype == torch.float32 and tails.is_contiguous() and tails.shape[0] >= 1
            and tails.shape[1] == cap <= FBANK_STREAM_MAX_CAP and tails.device == wave.device)


def fbank_stream(wave, wmap, tails, tables, norm_mean, norm_std, preemph=0.97, aug=None, noise=None, lib=None):
    """The new log-mel frames of several sessions from raw audio that arrives in hops of any size (aum_fbank_stream_fwd): wave
    (total_samples,) fp32, the sessions' new samples behind one another; wmap from wave_map; tails (nrows, win + 15 shift) fp32, the pool
    of carried samples -- the rows wmap names are rewritten IN PLACE (the last wmap.new_tail_lens[i] samples of [tail ; hop]), the
    others are not touched.  Returns (wmap.total_frames, num_mel) fp32: every frame is bit-identical to the same row of fbank_fwd on
    the whole waveform, however the stream was cut.  aug / noise: not in streams (refused)."""
    lib = lib or get()
    for t in (wave, tails):
        lib.check_tensor(t)
    if aug is not None or noise is not None or not fbank_stream_supported(wave, tails, tables):
        raise RuntimeError(f"fbank_stream: unsupported operands wave {tuple(wave.shape)} {wave.dtype}, tails {tuple(tails.shape)} {tails.dtype}, "
                           f"padded {tables['padded']}, aug {'set' if aug is not None else None}, noise {'set' if noise is not None else None} "
                           "(need (total,) fp32 samples, an fp32 contiguous (nrows, win + 15 shift <= 2816) pool on their device, the padded == 512 "
                           "tables, no aug, no noise)")
    if not isinstance(wmap, WaveMap):
        raise TypeError("fbank_stream: wmap must come from aum_hip.wave_map()")
    if wmap.total_samples != wave.shape[0] or wmap.cap != tails.shape[1]:
        raise ValueError(f"fbank_stream: wave_map describes {wmap.total_samples} samples and tails of {wmap.cap}, the call has {wave.shape[0]} and {tails.shape[1]}")
    if max(wmap.rows) >= tails.shape[0]:
        raise ValueError(f"fbank_stream: wave_map names pool row {max(wmap.rows)}, the pool has {tails.shape[0]} rows")
    if wmap.cu_samples.device != wave.device:
        raise RuntimeError(f"fbank_stream: wave_map lives on {wmap.cu_samples.device}, the samples on {wave.device}")
    num_mel, stride = tables["mel_w"].shape
    out = torch.empty((wmap.total_frames, num_mel), dtype=torch.float32, device=wave.device)
    if wmap.total_samples == 0 and wmap.total_frames == 0:          # nothing arrives, nothing is due: the tails stay as they are
        return out
    a = FbankStreamArgs()
    f = a.fbank
    f.wave, f.out = _ptr(wave) if wave.shape[0] else None, _ptr(out) if wmap.total_frames else None
    f.window, f.twiddle = _ptr(tables["window"]), _ptr(tables["twiddle"])
    f.mel_start_f, f.mel_count_f, f.mel_w = _ptr(tables["mel_start_f"]), _ptr(tables["mel_count_f"]), _ptr(tables["mel_w"])
    f.win, f.shift, f.padded, f.num_mel, f.mel_wstride = tables["win"], tables["shift"], tables["padded"], num_mel, stride
    f.preemph, f.norm_mean, f.norm_inv2std, f.log_floor = preemph, norm_mean, 1.0 / (2.0 * norm_std), 1.1920928955078125e-07
    a.cu_samples, a.cu_frames, a.tail_len = _ptr(wmap.cu_samples), _ptr(wmap.cu_frames), _ptr(wmap.tail_len)
    a.first_frame, a.n_real, a.idx, a.tails = _ptr(wmap.first_frame), _ptr(wmap.n_real_t), _ptr(wmap.idx), _ptr(tails)
    a.total_samples, a.total_frames, a.nseq, a.nrows, a.cap = wmap.total_samples, wmap.total_frames, len(wmap.samples), tails.shape[0], wmap.cap
    _launch(lib.c.aum_fbank_stream_fwd, a, tails, lib, "fbank_stream", (len(wmap.samples), wmap.total_samples, wmap.total_frames))
    return out


TIME_WARP_COLS = 8     # columns of the per-clip time-warp table (include/aum_hip.h AUM_TIME_WARP_COLS)


def stft_logmel_fwd(wave, n_valid, tables, target_length, eps=1e-6, lib=None):
    """EPIC-Sounds log-mel frontend (librosa stft -> |X| -> HTK mel -> log(x + eps) -> edge padding).  wave: (batch, n_samples) fp32;
    n_valid: (batch,) int32 valid samples per clip; tables: dict(window, twiddle, mel_start_f, mel_count_f, mel_w [num_mel, stride], win,
    hop, n_fft) of device tensors built by aum.epic.StftTables.  -> (batch, target_length, num_mel) fp32."""
    lib = lib or get()
    lib.check_tensor(wave)
    lib.check_tensor(n_valid)
    assert wave.dtype == torch.float32 and wave.dim() == 2 and wave.stride(1) == 1
    assert n_valid.dtype == torch.int32 and n_valid.is_contiguous() and n_valid.shape == (wave.shape[0],)
    batch, n = wave.shape
    num_mel, stride = tables["mel_w"].shape
    out = torch.empty((batch, target_length, num_mel), dtype=torch.float32, device=wave.device)
    a = StftArgs()
    a.wave, a.n_valid, a.out = _ptr(wave), _ptr(n_valid), _ptr(out)
    a.window, a.twiddle = _ptr(tables["window"]), _ptr(tables["twiddle"])
    a.mel_start_f, a.mel_count_f, a.mel_w = _ptr(tables["mel_start_f"]), _ptr(tables["mel_count_f"]), _ptr(tables["mel_w"])
    a.wave_bs, a.out_bs = wave.stride(0), out.stride(0)
    a.batch, a.n_samples, a.win, a.hop, a.n_fft = batch, n, tables["win"], tables["hop"], tables["n_fft"]
    a.num_mel, a.mel_wstride, a.target_length, a.eps = num_mel, stride, target_length, eps
    _launch(lib.c.aum_stft_logmel_fwd, a, wave, lib, "stft_logmel_fwd", (batch, target_length, num_mel))
    return out


def spec_time_warp(spec, table, lib=None):
    """SpecAugment time warp of the EPIC-Sounds recipe, out of place.  spec: (batch, frames, num_mel) fp32; table: (batch, 8) fp32 per clip
    [cy, cx, w, v0, v1, v2, xn, yn] (aum.epic.warp_table).  -> (batch, frames, num_mel) fp32."""
    lib = lib or get()
    lib.check_tensor(spec)
    lib.check_tensor(table)
    assert spec.dtype == torch.float32 and spec.dim() == 3 and spec.stride(2) == 1 and spec.stride(1) == spec.shape[2]
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape == (spec.shape[0], TIME_WARP_COLS)
    out = torch.empty_like(spec, memory_format=torch.contiguous_format)
    a = TimeWarpArgs()
    a.in_, a.table, a.out = _ptr(spec), _ptr(table), _ptr(out)
    a.in_bs, a.out_bs = spec.stride(0), out.stride(0)
    a.batch, a.frames, a.num_mel = spec.shape
    _launch(lib.c.aum_spec_time_warp, a, spec, lib, "spec_time_warp", tuple(spec.shape))
    return out


FRONTEND_TIME_MAJOR = 1


def frontend_tokens_supported(tables, target_length, dim, dtype):
    """the limits of aum_frontend_tokens_fwd (include/aum_hip.h); outside them callers run fbank_fwd and a GEMM"""
    return (dtype in (torch.bfloat16, torch.float16) and tables["padded"] == 512 and tables["mel_w"].shape[0] == 128
            and target_length % 64 == 0 and dim % 16 == 0)


def frontend_tokens(wave, tables, target_length, norm_mean, norm_std, weight, bias, pos, cls_row, cls_pos, out_dtype=torch.float32,
                    time_major=False, save_patches=False, preemph=0.97, aug=None, noise=None, lib=None):
    """Waveform -> token sequence in one launch (aum_frontend_tokens_fwd).  weight: (dim, 256) bf16/f16 (the flattened 16 x 16
    conv weight); bias (dim), pos (n_patches, dim), cls_row (dim) or None: fp32.  Returns (tokens (batch, n_patches [+1], dim)
    in out_dtype, patches (batch * n_patches, 256) in weight.dtype or None)."""
    lib = lib or get()
    batch = wave.shape[0]
    dim = weight.shape[0]
    n_patches = target_length // 16 * 8
    assert weight.shape == (dim, 256) and weight.is_contiguous() and weight.dtype in (torch.bfloat16, torch.float16)
    assert bias.shape == (dim,) and bias.dtype == torch.float32 and bias.is_contiguous()
    assert pos.shape == (n_patches, dim) and pos.dtype == torch.float32 and pos.is_contiguous()
    for t in (weight, bias, pos):
        lib.check_tensor(t)
    n_tok = n_patches + (cls_row is not None)
    tokens = torch.empty((batch, n_tok, dim), dtype=out_dtype, device=wave.device)
    patches = torch.empty((batch * n_patches, 256), dtype=weight.dtype, device=wave.device) if save_patches else None
    a = FrontendArgs()
    _fill_fbank(a.fbank, lib, wave, tables, target_length, norm_mean, norm_std, preemph, aug, noise)
    a.weight, a.bias, a.pos, a.tokens = _ptr(weight), _ptr(bias), _ptr(pos), _ptr(tokens)
    if cls_row is not None:
        assert cls_row.shape == (dim,) and cls_row.dtype == torch.float32 and cls_row.is_contiguous()
        lib.check_tensor(cls_row)
        a.cls_row, a.cls_pos = _ptr(cls_row), cls_pos
    if patches is not None:
        a.patches = _ptr(patches)
    a.tokens_bs, a.dim, a.dtype, a.out_dtype = tokens.stride(0), dim, _DT[weight.dtype], _DT[out_dtype]
    a.flags = FRONTEND_TIME_MAJOR if time_major else 0
    _launch(lib.c.aum_frontend_tokens_fwd, a, wave, lib, "frontend_tokens", (batch, target_length, dim))
    return tokens, patches


def proj_supported(dim, dt_rank, dstate, ntok, dtype):
    """the limits of include/aum_hip.h for the MFMA projection kernels; outside them callers use library GEMMs"""
    return (dtype in (torch.bfloat16, torch.float16) and dim % 64 == 0 and dt_rank <= 64 and dt_rank + 2 * dstate <= 80
            and ntok * 80 < 2 ** 31)


def _proj_common(a, ntok, dim, dt_rank, dstate, dtype):
    a.ntok, a.dim, a.dt_rank, a.dstate, a.dtype = ntok, dim, dt_rank, dstate, _DT[dtype]


def _pad_cols8(w):
    """[rows][cols] -> [rows][ceil8(cols)] zero-padded (the kernels read the short k dimension in groups of 8)"""
    pad = (-w.shape[1]) % 8
    return w.contiguous() if pad == 0 else torch.nn.functional.pad(w, (0, pad)).contiguous()


def _proj_operands(lib, names, *tensors):
    """the operands of the channel-major projections: on the library's side, contiguous, of the first one's 16-bit dtype"""
    for i, t in enumerate(tensors):
        lib.check_tensor(t)
        if not t.is_contiguous() or t.dtype != tensors[0].dtype:
            raise RuntimeError(f"{names[i]}: expected a contiguous {tensors[0].dtype} tensor, got {t.dtype}, {tuple(t.shape)}, strides {t.stride()}")


def proj_fwd(conv_out2d, w_x, w_dt, dstate, lib=None):
    """conv_out2d [dim][ntok], w_x [dt_rank+2*dstate][dim], w_dt [dim][dt_rank] (all one 16-bit dtype, contiguous)
    -> x_dbl [dt_rank+2*dstate][ntok] (rows dt | B | C) and delta [dim][ntok] = w_dt @ dt   (SSI:467-468)."""
    lib = lib or get()
    _proj_operands(lib, ("conv_out2d", "w_x", "w_dt"), conv_out2d, w_x, w_dt)
    dim, ntok = conv_out2d.shape
    rt, dt_rank = w_x.shape[0], w_dt.shape[1]
    if w_x.shape != (dt_rank + 2 * dstate, dim) or w_dt.shape != (dim, dt_rank):
        raise RuntimeError(f"proj_fwd: expected w_x ({dt_rank + 2 * dstate}, {dim}) and w_dt ({dim}, {dt_rank}), got {tuple(w_x.shape)}, {tuple(w_dt.shape)}")
    w_dt = _pad_cols8(w_dt)
    x_dbl = torch.empty((rt, ntok), dtype=conv_out2d.dtype, device=conv_out2d.device)
    delta = torch.empty_like(conv_out2d)
    a = ProjArgs()
    a.act, a.w_x, a.w_dt, a.x_dbl, a.out_act = _ptr(conv_out2d), _ptr(w_x), _ptr(w_dt), _ptr(x_dbl), _ptr(delta)
    _proj_common(a, ntok, dim, dt_rank, dstate, conv_out2d.dtype)
    a.len, a.w_ld = ntok, w_dt.shape[1]
    _launch(lib.c.aum_proj_fwd, a, conv_out2d, lib, "proj_fwd", (dim, ntok, rt))
    return x_dbl, delta


def proj_bwd_data(ddelta2d, w_dt_t, w_x_t, dB, dC, dconv2d, length, lib=None):
    """ddelta2d [dim][ntok], w_dt_t = W_dt^T [dt_rank][dim], w_x_t = W_x^T [dim][rt], dB/dC fp32 (batch, dstate, len)
    -> dx_dbl [rt][ntok]; dconv2d [dim][ntok] += W_x^T dx_dbl in place   (SSI:570-574, 587, 590)."""
    lib = lib or get()
    _proj_operands(lib, ("ddelta2d", "w_dt_t", "w_x_t", "dconv2d"), ddelta2d, w_dt_t, w_x_t, dconv2d)
    dim, ntok = ddelta2d.shape
    dt_rank, rt = w_dt_t.shape[0], w_x_t.shape[1]
    dstate = dB.shape[1]
    for name, t in (("dB", dB), ("dC", dC)):
        lib.check_tensor(t)
        if t.dtype != torch.float32 or t.stride(2) != 1:
            raise RuntimeError(f"{name}: expected fp32 (batch, dstate, len) with a unit time stride, got {t.dtype}, strides {t.stride()}")
    if rt != dt_rank + 2 * dstate or dB.shape[0] * length != ntok or dB.shape[2] != length:
        raise RuntimeError(f"proj_bwd_data: w_x_t: expected {dt_rank + 2 * dstate} columns, got {rt}; dB: expected ({ntok // length}, {dstate}, {length}), got {tuple(dB.shape)}")
    w_x_t = _pad_cols8(w_x_t)
    dx_dbl = torch.empty((rt, ntok), dtype=ddelta2d.dtype, device=ddelta2d.device)
    a = ProjArgs()
    a.act, a.w_x, a.w_dt, a.x_dbl, a.out_act = _ptr(ddelta2d), _ptr(w_x_t), _ptr(w_dt_t), _ptr(dx_dbl), _ptr(dconv2d)
    a.dB, a.dC = _ptr(dB), _ptr(dC)
    a.dB_bs, a.dB_ns, a.dC_bs, a.dC_ns = dB.stride(0), dB.stride(1), dC.stride(0), dC.stride(1)
    _proj_common(a, ntok, dim, dt_rank, dstate, ddelta2d.dtype)
    a.len, a.w_ld = length, w_x_t.shape[1]
    _launch(lib.c.aum_proj_bwd_data, a, ddelta2d, lib, "proj_bwd_data", (dim, ntok, rt))
    return dx_dbl


def proj_bwd_weight(x2d, y2d, transpose_out, lib=None):
    """sum_t x[e][t] * y[r][t] -> [dim][nrows] (or [nrows][dim] with transpose_out) fp32   (SSI:586, 589)."""
    lib = lib or get()
    _proj_operands(lib, ("x2d", "y2d"), x2d, y2d)
    if y2d.shape[1] != x2d.shape[1]:
        raise RuntimeError(f"y2d: expected (nrows, {x2d.shape[1]}) as x2d's tokens, got {tuple(y2d.shape)}")
    dim, ntok = x2d.shape
    nrows = y2d.shape[0]
    nsplit = debug.proj_splits or int(lib.c.aum_proj_bwd_weight_splits(dim, ntok))
    if nsplit <= 0:
        raise RuntimeError("aum_proj_bwd_weight: unsupported shape")
    part = torch.empty((nsplit, nrows, dim) if transpose_out else (nsplit, dim, nrows), dtype=torch.float32, device=x2d.device)
    a = ProjWArgs()
    a.x, a.y, a.out, a.ntok = _ptr(x2d), _ptr(y2d), _ptr(part), ntok
    a.dim, a.nrows, a.nsplit, a.transpose_out, a.dtype = dim, nrows, nsplit, int(transpose_out), _DT[x2d.dtype]
    _launch(lib.c.aum_proj_bwd_weight, a, x2d, lib, "proj_bwd_weight", (dim, ntok, nrows))
    return sum_rows(part, lib) if nsplit > 1 else part[0]


def selftest_wave_scan(P, S, rev=False, lib=None):
    lib = lib or get()
    inp = torch.cat([P.float().reshape(64), S.float().reshape(64)]).contiguous()
    out = torch.empty_like(inp)
    _chk(lib.c.aum_selftest_wave_scan(_ptr(inp), _ptr(out), int(rev), lib.stream(inp)), "aum_selftest_wave_scan")
    return out[:64], out[64:]


def selftest_wave_sum32(values, lib=None):
    """values: (32, 64) fp32 -> (2, 64): row 0 the totals in the lane order of wave_sum32 (lane l: value 2 * (l & 15) + ((l >> 4) & 1)),
    row 1 wave_sum16 of the first 16 values"""
    lib = lib or get()
    inp = values.float().contiguous()
    out = torch.empty((2, 64), dtype=torch.float32, device=inp.device)
    _chk(lib.c.aum_selftest_wave_sum32(_ptr(inp), _ptr(out), lib.stream(inp)), "aum_selftest_wave_sum32")
    return out


def _sum_out(out, shape, device):
    """the destination of a sum: `out` -- a contiguous fp32 tensor of exactly that shape on that device, at any float address (4-byte aligned is
    enough: the bucket view a parameter's gradient lives in under DistributedDataParallel may sit behind an odd-sized parameter, and every
    kernel that takes a destination stores to it with 4-byte aligned stores) -- or a new tensor.  Anything else passed as `out` is left alone"""
    if out is not None and out.dtype == torch.float32 and out.is_contiguous() and out.device == device and tuple(out.shape) == tuple(shape):
        return out
    return torch.empty(shape, dtype=torch.float32, device=device)


def sum_rows(t, lib=None, out=None):
    """t: (outer, ...) contiguous fp32 / bf16 / fp16 -> fp32 sum over dim 0, in a fixed order (aum_sum_rows): the partial results of
    rmsnorm_bwd / proj_bwd_weight and split-K GEMM partial products.  Tall and narrow inputs (the 4096 x 768 norm partials: too few
    columns for one pass to fill the chip) are summed in two stages, 32 slices first.  Shapes the kernel does not take go through torch.
    out: where to put the sum (see _sum_out); the result is returned either way."""
    lib = lib or get()
    inner = t[0].numel() if t.shape[0] > 0 else 0
    if debug.torch_sums or t.dtype not in _DT or not t.is_contiguous() or inner % 8 or inner == 0 or t.data_ptr() % 16:
        r = t.sum(0, dtype=torch.float32)
        return _sum_out(out, r.shape, r.device).copy_(r) if out is not None else r
    lib.check_tensor(t)
    outer, shape = t.shape[0], t.shape[1:]
    stream = lib.stream(t)
    if outer >= 1024 and inner < 8192 and outer % 32 == 0:
        mid = torch.empty((32, inner), dtype=torch.float32, device=t.device)
        _chk(lib.c.aum_sum_rows(_ptr(t), _ptr(mid), 32, outer // 32, inner, _DT[t.dtype], stream), "aum_sum_rows")
        t, outer = mid, 32
    out = _sum_out(out, shape, t.device)
    _chk(lib.c.aum_sum_rows(_ptr(t), _ptr(out), 1, outer, inner, _DT[t.dtype], stream), "aum_sum_rows")
    return out


def _two_stage(t):
    """sum_rows' rule for a tall and narrow partial set (two stages, 32 slices first)"""
    return t.shape[0] >= 1024 and t[0].numel() < 8192 and t.shape[0] % 32 == 0


def sum_rows_multi(parts, tr_cols=None, lib=None, outs=None):
    """parts: up to SUM_MAX_JOBS (outer, ...) contiguous fp32 tensors of partial results on one device -> their fp32 sums over dim 0 in ONE launch
    (aum_sum_rows_multi; bitwise the sums sum_rows gives one by one).  tr_cols[q] > 0: part q is (outer, rows, tr_cols) and its sum is
    returned transposed, (tr_cols, rows) contiguous.  Shapes the entry does not take go through sum_rows / torch one by one."""
    lib = lib or get()
    tr_cols = list(tr_cols or [0] * len(parts))
    outs = list(outs or [None] * len(parts))
    # (a set that sum_rows would add in two stages keeps that order: it goes through sum_rows, and so does every set of its call)
    ok = 0 < len(parts) <= SUM_MAX_JOBS and not debug.torch_sums and not debug.sums_one_by_one and all(
        t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] > 0 and t[0].numel() > 0 and t[0].numel() % 8 == 0 and t.data_ptr() % 16 == 0
        and not _two_stage(t) and (not tc or (t.dim() == 3 and t.shape[2] == tc)) for t, tc in zip(parts, tr_cols))
    if not ok:
        res = []
        for t, tc, o in zip(parts, tr_cols, outs):
            if tc:
                r = sum_rows(t, lib=lib).t()
                res.append(_sum_out(o, r.shape, r.device).copy_(r) if o is not None else r.contiguous())
            else:
                res.append(sum_rows(t, lib=lib, out=o))
        return res
    for t in parts:
        lib.check_tensor(t)
    outs = [_sum_out(o, (t.shape[2], t.shape[1]) if tc else tuple(t.shape[1:]), t.device) for t, tc, o in zip(parts, tr_cols, outs)]
    jobs = (SumJob * len(parts))()
    for j, t, o, tc in zip(jobs, parts, outs, tr_cols):
        j.src, j.dst, j.outer, j.inner, j.tr_cols = _ptr(t), _ptr(o), t.shape[0], t[0].numel(), tc
    _chk(lib.c.aum_sum_rows_multi(C.cast(jobs, C.c_void_p), len(parts), lib.stream(parts[0])), "aum_sum_rows_multi")
    return outs


_cast_tables = {}


def cast_bank(params, dtype, want_t=False, lib=None):
    """params: equally shaped 2-D fp32 contiguous matrices on one device -> (bank (n, rows, cols) in `dtype`, bank_t (n, cols, rows) or None):
    every matrix read once, both copies written by ONE launch (aum_cast_bank).  The device table of the n addresses is kept per address
    tuple (parameters are updated in place: their addresses are stable across steps)."""
    lib = lib or get()
    p0 = params[0]
    rows, cols = p0.shape
    key = (p0.device, tuple(p.data_ptr() for p in params))
    tab = _cast_tables.get(key)
    if tab is None:
        if len(_cast_tables) > 64:
            _cast_tables.clear()
        tab = _cast_tables[key] = torch.tensor(key[1], dtype=torch.int64, device=p0.device)
    for p in params:
        lib.check_tensor(p)
    bank = torch.empty((len(params), rows, cols), dtype=dtype, device=p0.device)
    bank_t = torch.empty((len(params), cols, rows), dtype=dtype, device=p0.device) if want_t else None
    _chk(lib.c.aum_cast_bank(_ptr(tab), len(params), rows, cols, _ptr(bank), _ptr(bank_t), _DT[dtype], lib.stream(p0)), "aum_cast_bank")
    return bank, bank_t


def cast_bank_supported(params, dtype):
    p0 = params[0]
    return (dtype in (torch.bfloat16, torch.float16) and p0.dim() == 2 and p0.shape[0] % 8 == 0 and p0.shape[1] % 4 == 0
            and all(p.dtype == torch.float32 and p.is_contiguous() and p.shape == p0.shape and p.device == p0.device and p.data_ptr() % 16 == 0
                    for p in params))


def hbm_copy(src, dst, lib=None):
    lib = lib or get()
    _chk(lib.c.aum_hbm_copy(_ptr(src), _ptr(dst), src.numel() * src.element_size(), lib.stream(src)), "aum_hbm_copy")
