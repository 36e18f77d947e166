"""ctypes binding of libl2s_hip.so (the C-ABI declared in include/l2s.h).

PyTorch is used here for what it is good at on the host side of this path - device
memory (caching allocator), streams, ``torch.distributed`` - and nothing else: every
function below hands raw device pointers and the current HIP stream to the native
library.  There is no fallback: if the library is missing or a call fails, a
``RuntimeError`` is raised.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading
from typing import Dict, Iterable, Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DIAG_LIB_PATH = os.path.join(_HERE, "csrc", "libl2s_diag.so")      # the diagnostic build (include/l2s_diag.h): tools/ and the operator tests only
# L2S_LIB: another build of the same ABI - tools/ point it at the diagnostic library ("diag" = DIAG_LIB_PATH), whose ABI is a superset
LIB_PATH = os.environ.get("L2S_LIB") or os.path.join(_HERE, "csrc", "libl2s_hip.so")
if LIB_PATH == "diag":
    LIB_PATH = DIAG_LIB_PATH

# every symbol include/l2s.h declares; tests check the built library exports all of them (and the product library nothing else)
ABI_SYMBOLS = (
    "l2s_abi_version", "l2s_last_error",
    "l2s_model_create", "l2s_model_set_tensor", "l2s_model_finalize", "l2s_model_destroy",
    "l2s_min_T", "l2s_workspace_bytes", "l2s_state_floats", "l2s_state_offset",
    "l2s_mel_frames", "l2s_mel_targets_workspace_bytes", "l2s_mel_targets",
    "l2s_resize_check", "l2s_resize_normalise", "l2s_align_check", "l2s_align_faces",
    "l2s_jpeg_plan", "l2s_jpeg_workspace_bytes", "l2s_jpeg_decode",
    "l2s_encoder_fwd", "l2s_normalise_pad_frames", "l2s_build_visual", "l2s_decoder_prologue", "l2s_decode_steps", "l2s_postnet",
    "l2s_workspace_bytes_masked", "l2s_masked_bilstm_plan", "l2s_inference_masked", "l2s_forward_eval_masked", "l2s_decoder_prologue_masked", "l2s_decode_steps_masked",
    "l2s_ragged_plan", "l2s_workspace_bytes_ragged", "l2s_inference_ragged",
    "l2s_forward_eval_ragged_plan", "l2s_workspace_bytes_eval_ragged", "l2s_forward_eval_ragged",
    "l2s_output_lengths", "l2s_inference", "l2s_inference_multi", "l2s_workspace_bytes_multi", "l2s_forward_eval", "l2s_forward_eval_multi", "l2s_model_set_option", "l2s_persist_available", "l2s_persist_timeouts", "l2s_set_thread_chains", "l2s_speaker_workspace_bytes", "l2s_speaker_encoder_fwd",
    "l2s_speaker_packed_plan", "l2s_speaker_workspace_bytes_packed", "l2s_speaker_encoder_packed",
    "l2s_face_workspace_bytes", "l2s_face_encoder_fwd",
    "l2s_inverse_mel_workspace_bytes", "l2s_inverse_mel", "l2s_griffin_lim_workspace_bytes", "l2s_griffin_lim", "l2s_estoi_workspace_bytes", "l2s_estoi_workspace_bytes_long", "l2s_estoi",
    "l2s_inverse_mel_ragged_check", "l2s_inverse_mel_ragged_workspace_bytes", "l2s_inverse_mel_ragged",
    "l2s_griffin_lim_ragged_check", "l2s_griffin_lim_ragged_workspace_bytes", "l2s_griffin_lim_ragged",
    "l2s_estoi_ragged_check", "l2s_estoi_ragged_workspace_bytes", "l2s_estoi_ragged",
    "l2s_set_option",
    "l2s_train_scratch_bytes", "l2s_loss", "l2s_grad_norm", "l2s_adamw_amsgrad_step",
    "l2s_train_steps_tape_floats", "l2s_train_steps_weights_floats", "l2s_train_steps_ws_bytes", "l2s_train_steps_pack_weights",
    "l2s_train_steps_fwd", "l2s_train_steps_bwd",
    "l2s_train_set_bn", "l2s_train_refresh_weights", "l2s_train_encoder_tape_floats", "l2s_train_encoder_ws_bytes", "l2s_train_encoder_fwd", "l2s_train_encoder_bwd",
    "l2s_train_prologue_tape_floats", "l2s_train_prologue_ws_bytes", "l2s_train_prologue_fwd", "l2s_train_prologue_bwd",
    "l2s_train_encoder_tape_floats_masked", "l2s_train_encoder_ws_bytes_masked", "l2s_train_prologue_tape_floats_masked", "l2s_train_prologue_ws_bytes_masked",
    "l2s_train_steps_tape_floats_masked", "l2s_train_encoder_masked_fwd", "l2s_train_encoder_masked_bwd", "l2s_train_prologue_masked_fwd",
    "l2s_train_prologue_masked_bwd", "l2s_train_steps_masked_fwd", "l2s_train_steps_masked_bwd",
    "l2s_loss_lengths_check", "l2s_train_scratch_bytes_lengths", "l2s_loss_lengths", "l2s_train_postnet_tape_floats_masked", "l2s_train_postnet_ws_bytes_masked",
    "l2s_train_postnet_masked_fwd", "l2s_train_postnet_masked_bwd",
    "l2s_train_bind", "l2s_train_postnet_tape_floats", "l2s_train_postnet_ws_bytes", "l2s_train_postnet_fwd", "l2s_train_postnet_bwd",
    "l2s_profile_enable", "l2s_profile_reset", "l2s_profile_count", "l2s_profile_get",
)
# what include/l2s_diag.h adds: exported by libl2s_diag.so only
DIAG_SYMBOLS = (
    "l2s_op_gemm", "l2s_op_conv1d", "l2s_op_gemm_ex", "l2s_op_conv1d_ex", "l2s_op_conv1d_bwd", "l2s_op_frontend", "l2s_op_launch_chain", "l2s_op_launch_chain2", "l2s_op_skinny_timeline", "l2s_op_attn_timeline", "l2s_op_flat_timeline", "l2s_op_pdecode_timeline", "l2s_op_gemm_x3_timeline", "l2s_op_fused_unit_timeline", "l2s_op_lstm_cell_chain", "l2s_op_step_attn_chain", "l2s_op_stamp_log", "l2s_op_skinny_form", "l2s_op_step_site", "l2s_op_skinny", "l2s_op_skinny_hoist",
    "l2s_op_face_conv2d", "l2s_op_face_taps", "l2s_op_speaker_taps", "l2s_op_speaker_taps_packed", "l2s_op_encoder_taps",
    "l2s_op_gemm_bwd", "l2s_op_gemm_bwd_recorder", "l2s_op_upload_table", "l2s_op_table_layout", "l2s_op_jpeg_entropy_host", "l2s_op_post_wino_matrices",
)

# run-time options only the diagnostic build accepts (block-form A/B switches of the same arithmetic, include/l2s_diag.h)
DIAG_OPTIONS = frozenset(("overlap_postnet", "fuse_trunk", "fuse_s2", "skinny_static", "skinny_sized", "skinny_split", "skinny_split8", "skinny_rc", "skinny_rc_jb",
                          "skinny_rc_multi", "skinny_flat", "hoist_vproj", "attn_lds", "flat_half", "half_min_mts", "gemm_x3_dma", "flat_xcd", "attn_skip0", "trunk_chain", "frontend_solo", "post_wino"))

ST_K, ST_V, ST_CKEY, ST_CVAL, ST_ECELL, ST_H, ST_C, ST_ENC, ST_STOPC, ST_VP, ST_CP = range(11)

_lib = None
_diag = None
_process_defaults: Dict[str, int] = {}
_vp, _i, _i64, _fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p


class ResizeJob(ctypes.Structure):
    """`l2s_resize_job` (include/l2s.h): an image of the packed buffer, a source rectangle inside it, a flip bit and an output slot"""
    _fields_ = [("offset", _i64)] + [(k, ctypes.c_int32) for k in ("H", "W", "y0", "x0", "h", "w", "flip", "slot")]


class AlignJob(ctypes.Structure):
    """`l2s_align_job` (include/l2s.h): an image of the packed buffer and the six float64 of its destination-to-source map"""
    _fields_ = [("offset", _i64), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("m", ctypes.c_double * 6)]


class JpegImage(ctypes.Structure):
    """`l2s_jpeg_image` (include/l2s.h): what `l2s_jpeg_plan` finds in one stream's headers"""
    _fields_ = [("scan_offset", _i64)] + [(k, ctypes.c_int32) for k in ("scan_bytes", "H", "W", "layout", "restart", "table_set", "eoi", "reserved")]


class JpegHuff(ctypes.Structure):
    """`l2s_jpeg_huff` (include/l2s.h): the derived lookup of one Huffman table"""
    _fields_ = [("lut", ctypes.c_uint16 * 256), ("maxcode", ctypes.c_int32 * 18), ("valoff", ctypes.c_int32 * 18), ("vals", ctypes.c_uint8 * 256)]


class JpegTables(ctypes.Structure):
    """`l2s_jpeg_tables` (include/l2s.h): a table set - per component its quantisers and table ids, and the four Huffman tables"""
    _fields_ = [("quant", (ctypes.c_uint16 * 64) * 3), ("dc", ctypes.c_uint8 * 4), ("ac", ctypes.c_uint8 * 4), ("huff", JpegHuff * 4)]


class SkinnyGroup(ctypes.Structure):
    """`l2s_skinny_group` (include/l2s_diag.h): one GEMM group of a batch-row launch of `l2s_op_skinny` - pointers, then 64-bit, then 32-bit integers"""
    _fields_ = ([("seg_a", _vp * 4)] + [(k, _vp) for k in ("a_sum", "W", "planes", "bias", "actw", "add", "addrow", "out", "pre", "c_in", "c_out", "h_out", "h_seq",
                                                            "h_plain", "mel", "stop", "stop_const", "yfrag")]
                + [(k, _i64) for k in ("ld_pre", "ld_hseq", "ld_mel_b", "ld_stop_b")] + [("nchunks", ctypes.c_int32 * 4)]
                + [(k, ctypes.c_int32) for k in ("ntiles", "epi", "N", "act", "ldo", "ld_add", "H", "h_out_K", "h_out_off", "ld_hplain")])


GEMM_BWD_INTS = ("mode", "M", "N", "K", "lda", "ldb", "ldc", "Tx", "Tz", "taps", "stride", "pad", "padp", "Nout", "Cin", "c_T", "accumulate")
BWD_DX, BWD_DW = 0, 1                     # BwdMode of l2s_common.h


class GemmBwdDesc(ctypes.Structure):
    """`l2s_gemm_bwd_desc` (include/l2s_diag.h): the integers of one backward-GEMM descriptor - the 64-bit field, the 32-bit integers, alpha"""
    _fields_ = [("c_seq_stride", _i64)] + [(k, ctypes.c_int32) for k in GEMM_BWD_INTS] + [("alpha", ctypes.c_float)]


class GemmBwdRecord(ctypes.Structure):
    """`l2s_gemm_bwd_record` (include/l2s_diag.h): what one call of a launch function of gemm_bwd.hip ran"""
    _fields_ = ([("d", GemmBwdDesc * 2)] + [(k, ctypes.c_int32) for k in ("entry", "splits_asked", "splits", "vec", "bf16", "pair")]
                + [("align", (ctypes.c_int32 * 3) * 2), ("name", ctypes.c_char * 40)])


RESIZE_MOUTH, RESIZE_FACE = 0, 1        # L2S_RESIZE_MOUTH / L2S_RESIZE_FACE
RESIZE_JOBS_PER_LAUNCH = 240              # L2S_RESIZE_JOBS_PER_LAUNCH: output slots whose table one launch carries in its kernel arguments
ALIGN_JOBS_PER_LAUNCH = 56                # L2S_ALIGN_JOBS_PER_LAUNCH: 64-byte align jobs whose table one launch carries in its kernel arguments
JPEG_GREY, JPEG_444, JPEG_420 = 0, 1, 2   # L2S_JPEG_*: an image's layout
JPEG_STATUS_CODE, JPEG_STATUS_END, JPEG_STATUS_RESTART, JPEG_STATUS_RUN, JPEG_STATUS_EXTRA = 1, 2, 4, 8, 16      # L2S_JPEG_STATUS_*


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(
            f"native library not built: {path} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C lip2speech_amd/csrc` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the Lip2Speech hot path.")
    L = ctypes.CDLL(path)
    _bind(L)
    if hasattr(L, "l2s_op_gemm"):
        _bind_diag(L)
    return L


def lib() -> ctypes.CDLL:
    """Load the native library (once).  Fails loudly - the HIP path is the only path."""
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def diag() -> ctypes.CDLL:
    """The diagnostic build (libl2s_diag.so, include/l2s_diag.h): the product ABI plus operator-level hooks, chain microbenches, stamped kernel builds
    and the block-form A/B options.  Loaded on demand by tools/ and the operator tests - never by the package's own callers."""
    global _diag
    if _diag is None:
        _diag = lib() if hasattr(lib(), "l2s_op_gemm") else _load(DIAG_LIB_PATH)
        if _diag is not _lib:
            for name, value in _process_defaults.items():      # the process defaults set so far hold for models of either library
                check(_diag.l2s_set_option(name.encode(), value), _diag)
            _replay_thread_chains(_diag)
    return _diag


def _bind(L: ctypes.CDLL) -> None:
    L.l2s_last_error.restype = ctypes.c_char_p
    L.l2s_abi_version.restype = _i
    L.l2s_model_create.argtypes = [ctypes.POINTER(_vp)]
    L.l2s_model_set_tensor.argtypes = [_vp, ctypes.c_char_p, _vp, _i64]
    L.l2s_model_finalize.argtypes = [_vp, _vp]
    L.l2s_model_destroy.argtypes = [_vp]
    L.l2s_min_T.argtypes = [_i]
    L.l2s_workspace_bytes.argtypes = [_i] * 5
    L.l2s_workspace_bytes.restype = _i64
    L.l2s_state_floats.argtypes = [_i, _i]
    L.l2s_state_floats.restype = _i64
    L.l2s_state_offset.argtypes = [_i, _i, _i]
    L.l2s_state_offset.restype = _i64
    L.l2s_encoder_fwd.argtypes = [_vp, _fp, _i, _i, _i, _i, _fp, _vp, _i64, _vp]
    L.l2s_normalise_pad_frames.argtypes = [_vp, ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int32), _i, _i, _i, _i, _fp, _vp]
    L.l2s_build_visual.argtypes = [_fp, _fp, _i, _i, _fp, _vp]
    L.l2s_decoder_prologue.argtypes = [_vp, _fp, _fp, _fp, _i, _i, _fp, _fp, _vp, _i64, _vp]
    L.l2s_decode_steps.argtypes = [_vp, _fp, _i, _i, _i, _fp, _vp, _fp, _fp, _fp, _i, _vp, _i64, _vp]
    L.l2s_postnet.argtypes = [_vp, _fp, _i, _i, _fp, _fp, _vp, _i64, _vp]
    L.l2s_output_lengths.argtypes = [_fp, _i, _i, _vp, _vp]
    L.l2s_speaker_workspace_bytes.argtypes = [_i, _i]
    L.l2s_speaker_workspace_bytes.restype = _i64
    L.l2s_speaker_encoder_fwd.argtypes = [_vp, _fp, _i, _i, _fp, _vp, _i64, _vp]
    L.l2s_face_workspace_bytes.argtypes = [_i, _i, _i]
    L.l2s_face_workspace_bytes.restype = _i64
    L.l2s_face_encoder_fwd.argtypes = [_vp, _fp, _i64, _i, _i, _i, _fp, _fp, _vp, _i64, _vp]
    L.l2s_inference.argtypes = [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _vp, _fp, _vp, _i64, _vp]
    L.l2s_workspace_bytes_multi.argtypes = [_i] * 6
    L.l2s_workspace_bytes_multi.restype = _i64
    L.l2s_inference_multi.argtypes = [_vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _i, _i, _i, _i, _i, _fp, _vp, _fp, _vp, _i64, _vp]
    L.l2s_forward_eval.argtypes = [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _vp, _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_forward_eval_multi.argtypes = [_vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp,
                                         _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_model_set_option.argtypes = [_vp, ctypes.c_char_p, _i]
    L.l2s_set_option.argtypes = [ctypes.c_char_p, _i]
    L.l2s_train_bind.argtypes = [_vp, ctypes.c_char_p, _fp, _fp]
    L.l2s_train_postnet_tape_floats.argtypes = [_i, _i]
    L.l2s_train_postnet_tape_floats.restype = _i64
    L.l2s_train_postnet_ws_bytes.argtypes = [_i, _i]
    L.l2s_train_postnet_ws_bytes.restype = _i64
    L.l2s_train_postnet_fwd.argtypes = [_vp, _fp, _i, _i, _fp, _fp, _fp, _vp]
    L.l2s_train_postnet_bwd.argtypes = [_vp, _fp, _fp, _i, _i, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_train_steps_tape_floats.argtypes = [_i, _i]
    L.l2s_train_steps_tape_floats.restype = _i64
    L.l2s_train_steps_weights_floats.restype = _i64
    L.l2s_train_steps_ws_bytes.argtypes = [_i, _i]
    L.l2s_train_steps_ws_bytes.restype = _i64
    L.l2s_train_steps_pack_weights.argtypes = [_vp, _fp, _vp]
    L.l2s_train_steps_fwd.argtypes = [_vp, _fp, _i, _i, _i, _fp, _vp, _vp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_train_steps_bwd.argtypes = [_vp, _fp, _i, _i, _i, _vp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_train_set_bn.argtypes = [_vp, _i, ctypes.c_float]
    L.l2s_train_refresh_weights.argtypes = [_vp, _vp]
    L.l2s_train_encoder_tape_floats.argtypes = [_i, _i, _i]
    L.l2s_train_encoder_tape_floats.restype = _i64
    L.l2s_train_encoder_ws_bytes.argtypes = [_i, _i, _i]
    L.l2s_train_encoder_ws_bytes.restype = _i64
    L.l2s_train_encoder_fwd.argtypes = [_vp, _fp, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _vp]
    L.l2s_train_encoder_bwd.argtypes = [_vp, _fp, _i, _i, _i, _i, _fp, _i, _fp, _vp, _i64, _vp]
    L.l2s_train_prologue_tape_floats.argtypes = [_i, _i]
    L.l2s_train_prologue_tape_floats.restype = _i64
    L.l2s_train_prologue_ws_bytes.argtypes = [_i, _i]
    L.l2s_train_prologue_ws_bytes.restype = _i64
    L.l2s_train_prologue_fwd.argtypes = [_vp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_train_prologue_bwd.argtypes = [_vp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_train_scratch_bytes.restype = _i64
    L.l2s_loss.argtypes = [_fp] * 6 + [_i, _i, _i] + [_fp] * 5 + [_vp, _vp]
    L.l2s_grad_norm.argtypes = [_fp, _i64, _vp, _fp, _vp]
    _f = ctypes.c_float
    L.l2s_adamw_amsgrad_step.argtypes = [_fp] * 5 + [_i64, _f, _f, _f, _f, _f, _i, _fp, _f, _f, _vp]
    L.l2s_inverse_mel_workspace_bytes.argtypes = [_i] * 6
    L.l2s_inverse_mel_workspace_bytes.restype = _i64
    L.l2s_inverse_mel.argtypes = [_fp, _i, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _vp, _vp, _i64, _vp]
    L.l2s_griffin_lim_workspace_bytes.argtypes = [_i, _i]
    L.l2s_griffin_lim_workspace_bytes.restype = _i64
    L.l2s_griffin_lim.argtypes = [_fp, _fp, _i, _i, _i, _i, _i, ctypes.c_float, _fp, _vp, _i64, _vp]
    L.l2s_estoi_workspace_bytes.argtypes = [_i]
    L.l2s_estoi_workspace_bytes.restype = _i64
    L.l2s_estoi.argtypes = [_fp, _fp, _i, _i, _fp, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int), _fp, _vp, _i64, _vp]
    # the long forms of the vocoder and the metric (include/l2s.h): the workspace query is absent from a library built before them
    if hasattr(L, "l2s_estoi_workspace_bytes_long"):
        L.l2s_estoi_workspace_bytes_long.argtypes = [_i, _i]
        L.l2s_estoi_workspace_bytes_long.restype = _i64
    # the ragged forms of the vocoder and the metric (include/l2s.h): likewise absent from a library built before them
    # (tools/vocoder_ragged/time_vocoder_ragged.py times one next to this build)
    if hasattr(L, "l2s_griffin_lim_ragged"):
        _ints, _offs = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_i64)
        L.l2s_inverse_mel_ragged_check.argtypes = [_ints, _offs, _offs, _i, _i64, _i, _i, _i, _i]
        L.l2s_inverse_mel_ragged_workspace_bytes.argtypes = [_ints, _i, _i, _i, _i]
        L.l2s_inverse_mel_ragged_workspace_bytes.restype = _i64
        L.l2s_inverse_mel_ragged.argtypes = [_fp, _i64, _offs, _offs, _ints, _i, _i, _fp, _i, _fp, _i, _i, _i, _fp, _fp, _vp, _vp, _i64, _vp]
        L.l2s_griffin_lim_ragged_check.argtypes = [_ints, _i, _i, _i, _i, _i64]
        L.l2s_griffin_lim_ragged_workspace_bytes.argtypes = [_ints, _i]
        L.l2s_griffin_lim_ragged_workspace_bytes.restype = _i64
        L.l2s_griffin_lim_ragged.argtypes = [_fp, _fp, _ints, _i, _i, _i, _i, ctypes.c_float, _fp, _i64, _vp, _i64, _vp]
        L.l2s_estoi_ragged_check.argtypes = [_ints, _ints, _ints, _i, _i64, _i, _i, _i, _i, _i]
        L.l2s_estoi_ragged_workspace_bytes.argtypes = [_ints, _i]
        L.l2s_estoi_ragged_workspace_bytes.restype = _i64
        L.l2s_estoi_ragged.argtypes = [_fp, _fp, _i64, _ints, _i, _fp, _i, _ints, _i, _i, _i, _ints, _ints, _fp, _vp, _i64, _vp]
    L.l2s_profile_enable.argtypes = [_i]
    L.l2s_profile_get.argtypes = [_i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_double)]
    # per-clip video lengths: the unmasked signature plus the host length array.  A library of the same ABI version built before these entry points
    # existed still binds (tools/masked_lengths/time_masked_lengths.py times one next to this build); lib() itself is checked against ABI_SYMBOLS by build()
    if hasattr(L, "l2s_inference_masked"):
        _lens = ctypes.POINTER(ctypes.c_int32)
        L.l2s_workspace_bytes_masked.argtypes = [_i] * 5
        L.l2s_workspace_bytes_masked.restype = _i64
        L.l2s_masked_bilstm_plan.argtypes = [_lens, _i, _i, _lens, _lens, ctypes.POINTER(_i), ctypes.POINTER(_i)]
        L.l2s_inference_masked.argtypes = L.l2s_inference.argtypes + [_lens]
        L.l2s_forward_eval_masked.argtypes = L.l2s_forward_eval.argtypes + [_lens]
        L.l2s_decoder_prologue_masked.argtypes = L.l2s_decoder_prologue.argtypes + [_lens]
        L.l2s_decode_steps_masked.argtypes = L.l2s_decode_steps.argtypes + [_lens]
    # training with per-clip video lengths (include/l2s.h): likewise absent from a library built before them (timing/masked_train times one next to this build)
    if hasattr(L, "l2s_train_steps_masked_fwd"):
        _lens = ctypes.POINTER(ctypes.c_int32)
        for name, n in (("l2s_train_encoder_tape_floats_masked", 3), ("l2s_train_encoder_ws_bytes_masked", 3), ("l2s_train_prologue_tape_floats_masked", 2),
                        ("l2s_train_prologue_ws_bytes_masked", 2), ("l2s_train_steps_tape_floats_masked", 2)):
            getattr(L, name).argtypes = [_i] * n
            getattr(L, name).restype = _i64
        for name in ("l2s_train_encoder_fwd", "l2s_train_encoder_bwd", "l2s_train_prologue_fwd", "l2s_train_prologue_bwd", "l2s_train_steps_fwd", "l2s_train_steps_bwd"):
            getattr(L, name[:-4] + "_masked" + name[-4:]).argtypes = getattr(L, name).argtypes + [_lens]      # l2s_train_<stage>_masked_fwd / _bwd
    # training with per-clip mel lengths (include/l2s.h): likewise absent from a library built before them (timing/masked_mel times one next to this build)
    if hasattr(L, "l2s_loss_lengths"):
        _lens = ctypes.POINTER(ctypes.c_int32)
        L.l2s_loss_lengths_check.argtypes = [_lens, _lens, _i, _i, _i]
        L.l2s_train_scratch_bytes_lengths.argtypes = [_i]
        L.l2s_train_scratch_bytes_lengths.restype = _i64
        L.l2s_loss_lengths.argtypes = L.l2s_loss.argtypes + [_lens, _lens, _i, _fp]
        for name in ("l2s_train_postnet_tape_floats_masked", "l2s_train_postnet_ws_bytes_masked"):
            getattr(L, name).argtypes = [_i, _i]
            getattr(L, name).restype = _i64
        L.l2s_train_postnet_masked_fwd.argtypes = L.l2s_train_postnet_fwd.argtypes + [_lens]
        L.l2s_train_postnet_masked_bwd.argtypes = L.l2s_train_postnet_bwd.argtypes + [_lens]
    # ragged groups (include/l2s.h): likewise absent from a library built before them (tools/ragged/time_ragged.py times one next to this build)
    if hasattr(L, "l2s_inference_ragged"):
        _lens = ctypes.POINTER(ctypes.c_int32)
        L.l2s_ragged_plan.argtypes = [_i, _lens, _lens, _lens, _lens, _lens, ctypes.POINTER(_i), ctypes.POINTER(_i)]
        L.l2s_workspace_bytes_ragged.argtypes = [_i, _lens, _lens, _i, _i, _i]
        L.l2s_workspace_bytes_ragged.restype = _i64
        L.l2s_inference_ragged.argtypes = [_vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _lens, _lens, _lens, _i, _i, _i, _fp, _vp, _fp,
                                           _vp, _i64, _vp]
    # the evaluate-shaped ragged group (include/l2s.h): likewise absent from a library built before it (tools/ragged/time_forward_ragged.py times one
    # next to this build)
    if hasattr(L, "l2s_forward_eval_ragged"):
        _lens, _offs = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i64)
        L.l2s_forward_eval_ragged_plan.argtypes = [_i, _lens, _lens, _lens, _offs, _offs, _offs, _offs, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i)]
        L.l2s_workspace_bytes_eval_ragged.argtypes = [_i, _lens, _lens, _lens, _i, _i]
        L.l2s_workspace_bytes_eval_ragged.restype = _i64
        L.l2s_forward_eval_ragged.argtypes = [_vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _lens, _lens, _lens, _lens, _i, _i,
                                              _fp, _fp, _fp, _fp, _fp, _vp, _i64, _vp]
    # device-side mel targets (include/l2s.h): likewise absent from a library built before them
    if hasattr(L, "l2s_mel_targets"):
        L.l2s_mel_frames.argtypes = [_i64]
        L.l2s_mel_frames.restype = _i
        L.l2s_mel_targets_workspace_bytes.argtypes = [_i, _i]
        L.l2s_mel_targets_workspace_bytes.restype = _i64
        L.l2s_mel_targets.argtypes = [_fp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i, _fp, _i, _i, _i, _i, _i, ctypes.c_float, _i, _i64, _fp, _fp, _fp, _vp,
                                      _vp, _i64, _vp]
    # device-side face crops (include/l2s.h): likewise absent from a library built before them (tools/frame_resize/time_frame_resize.py times one next to this build)
    if hasattr(L, "l2s_resize_normalise"):
        _jobs = ctypes.POINTER(ResizeJob)
        L.l2s_resize_check.argtypes = [_jobs, _i, _i64, _i, _i, _i, _i, _i]
        L.l2s_resize_normalise.argtypes = [_vp, _i64, _jobs, _i, _i, _i, _i, _i, _i, _fp, _vp]
    # device-side face alignment (include/l2s.h): likewise absent from a library built before it
    if hasattr(L, "l2s_align_faces"):
        _ajobs = ctypes.POINTER(AlignJob)
        L.l2s_align_check.argtypes = [_ajobs, _i, _i64]
        L.l2s_align_faces.argtypes = [_vp, _i64, _ajobs, _i, _vp, _vp]
    # device-side JPEG decode (include/l2s.h): likewise absent from a library built before it
    if hasattr(L, "l2s_jpeg_decode"):
        _imgs, _sets = ctypes.POINTER(JpegImage), ctypes.POINTER(JpegTables)
        L.l2s_jpeg_plan.argtypes = [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i, _imgs, _sets, _i, ctypes.POINTER(_i)]
        L.l2s_jpeg_workspace_bytes.argtypes = [_imgs, _i, _i]
        L.l2s_jpeg_workspace_bytes.restype = _i64
        L.l2s_jpeg_decode.argtypes = [_vp, _i64, _imgs, _i, _sets, _i, ctypes.POINTER(_i64), _vp, _i64, _vp, _vp, _i64, _vp]
    # the voice tower over clips of unequal length (include/l2s.h): likewise absent from a library built before it
    # (tools/speaker_packed/time_speaker_packed.py times one next to this build)
    if hasattr(L, "l2s_speaker_encoder_packed"):
        _lens, _ns = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i64)
        L.l2s_speaker_packed_plan.argtypes = [_ns, _i, _lens, _lens, _lens, ctypes.POINTER(_i), ctypes.POINTER(_i64)]
        L.l2s_speaker_workspace_bytes_packed.argtypes = [_ns, _i]
        L.l2s_speaker_workspace_bytes_packed.restype = _i64
        L.l2s_speaker_encoder_packed.argtypes = [_vp, _fp, _ns, _ns, _i, _fp, _vp, _i64, _vp]


def _bind_diag(L: ctypes.CDLL) -> None:
    L.l2s_op_gemm.argtypes = [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _vp]
    L.l2s_op_conv1d.argtypes = [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]
    L.l2s_op_gemm_ex.argtypes = [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _vp]
    L.l2s_op_conv1d_ex.argtypes = [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]
    L.l2s_op_conv1d_bwd.argtypes = [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]
    L.l2s_op_frontend.argtypes = [_vp, _fp, _i, _i, _i, _i, _fp, _vp]
    L.l2s_op_launch_chain.argtypes = [_i, _i, _i, _i, _fp, _fp, _vp]
    L.l2s_op_skinny_timeline.argtypes = [_vp]
    L.l2s_op_attn_timeline.argtypes = [_vp]
    L.l2s_op_flat_timeline.argtypes = [_vp]
    L.l2s_op_pdecode_timeline.argtypes = [_vp, ctypes.c_int]
    L.l2s_op_gemm_x3_timeline.argtypes = [_vp, ctypes.c_int]
    L.l2s_op_fused_unit_timeline.argtypes = [_vp, _i]
    L.l2s_op_launch_chain2.argtypes = [_i, _i, _i, _i, _fp, _fp, _vp, _vp]
    L.l2s_op_step_attn_chain.argtypes = [_vp, _fp, _i, _i, _i, _vp, _i64, _vp]
    L.l2s_op_lstm_cell_chain.argtypes = [_vp, _i, _i, _vp, _i64, _vp, ctypes.POINTER(ctypes.c_double)]
    L.l2s_op_stamp_log.argtypes = [_vp, _i64]
    L.l2s_op_skinny_form.argtypes = [_vp, _i, ctypes.POINTER(ctypes.c_int), _i, _i, _i, _i, ctypes.c_char_p, _i]
    L.l2s_op_step_site.argtypes = [_vp, ctypes.c_char_p, _i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.l2s_op_skinny.argtypes = [_vp, _i, ctypes.POINTER(SkinnyGroup), _i, _vp, _i, _vp]
    L.l2s_op_skinny_hoist.argtypes = [_vp, ctypes.POINTER(SkinnyGroup), _vp, _vp, _i, _i, _vp]
    L.l2s_op_face_conv2d.argtypes = [_fp, _i64, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, _vp]
    L.l2s_op_face_taps.argtypes = [_vp, _fp, _i64, _i, _vp, _fp, _fp, _vp, _i64, _vp]
    L.l2s_op_speaker_taps.argtypes = [_vp, _fp, _i, _i, _vp, _fp, _vp, _i64, _vp]
    L.l2s_op_speaker_taps_packed.argtypes = [_vp, _fp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), _i, _vp, _fp, _vp, _i64, _vp]
    L.l2s_op_encoder_taps.argtypes = [_vp, _fp, _i, _i, _i, _i, _vp, _fp, _vp, _i64, _vp]
    L.l2s_op_gemm_bwd.argtypes = [ctypes.POINTER(GemmBwdDesc), _fp, _fp, _fp, ctypes.POINTER(GemmBwdDesc), _fp, _fp, _fp, _i, _fp, _i, ctypes.POINTER(GemmBwdRecord), _vp]
    L.l2s_op_gemm_bwd_recorder.argtypes = [_i, ctypes.POINTER(GemmBwdRecord), _i, ctypes.POINTER(_i)]
    if hasattr(L, "l2s_op_upload_table"):
        L.l2s_op_upload_table.argtypes = [_vp, _i64, _vp, _vp]
        L.l2s_op_table_layout.argtypes = [_vp, _i64, _vp, _i64, _i, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64), _vp]
    if hasattr(L, "l2s_op_jpeg_entropy_host"):
        L.l2s_op_jpeg_entropy_host.argtypes = [_vp, _i64, ctypes.POINTER(JpegImage), _i, ctypes.POINTER(JpegTables), _i, _vp, _i64, _vp]
    if hasattr(L, "l2s_op_post_wino_matrices"):
        L.l2s_op_post_wino_matrices.argtypes = [_vp, _vp, _vp]


def check(rc: int, L: Optional[ctypes.CDLL] = None) -> None:
    if rc != 0:
        raise RuntimeError("libl2s_hip: " + (L or lib()).l2s_last_error().decode("utf-8", "replace"))


def _dcheck(rc: int) -> None:
    check(rc, diag())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return t.data_ptr()


def _f32(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("the Lip2Speech hot path runs on the GPU: move inputs to cuda (no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def min_T(T: int) -> int:
    return int(lib().l2s_min_T(T))


def video_lengths_array(video_lengths, B: int, T: int):
    """The `video_lengths` argument of the `*_masked` entry points (include/l2s.h "per-clip video lengths"), checked BEFORE the native call: a
    1-D sequence / integer tensor of B lengths in [7, T] -> a host `int32[B]` ctypes array.  A device tensor is copied to the host (the library
    plans its launches from the lengths).  Raises `TypeError` for a non-integer dtype, `ValueError` for a wrong shape or a length out of range."""
    if isinstance(video_lengths, torch.Tensor):
        if video_lengths.is_floating_point() or video_lengths.is_complex() or video_lengths.dtype == torch.bool:
            raise TypeError(f"video_lengths must hold integers, got {video_lengths.dtype}")
        arr = video_lengths.detach().cpu().numpy()
    else:
        arr = np.asarray(video_lengths)
        if arr.dtype.kind not in "iu":
            raise TypeError(f"video_lengths must hold integers, got {arr.dtype}")
    if arr.shape != (B,):
        raise ValueError(f"video_lengths must have shape ({B},) - one length per clip - got {tuple(arr.shape)}")
    bad = [(b, int(v)) for b, v in enumerate(arr) if v < 7 or v > T]
    if bad:
        raise ValueError(f"video_lengths outside [7, T = {T}]: " + ", ".join(f"clip {b}: {v}" for b, v in bad))
    return (ctypes.c_int32 * B)(*[int(v) for v in arr])


def mel_lengths_array(mel_lengths, B: int, S: int):
    """The `mel_lengths` argument of `l2s_loss_lengths` and the `l2s_train_postnet_masked_*` entry points (include/l2s.h "training with per-clip mel
    lengths"), checked BEFORE the native call: B integers in [1, S] -> a host `int32[B]` ctypes array.  Same errors as `video_lengths_array`."""
    if mel_lengths is None:
        raise ValueError("mel_lengths is None: one length per clip is needed")
    if isinstance(mel_lengths, torch.Tensor):
        if mel_lengths.is_floating_point() or mel_lengths.is_complex() or mel_lengths.dtype == torch.bool:
            raise TypeError(f"mel_lengths must hold integers, got {mel_lengths.dtype}")
        arr = mel_lengths.detach().cpu().numpy()
    else:
        arr = np.asarray(mel_lengths)
        if arr.dtype.kind not in "iu":
            raise TypeError(f"mel_lengths must hold integers, got {arr.dtype}")
    if arr.shape != (B,):
        raise ValueError(f"mel_lengths must have shape ({B},) - one length per clip - got {tuple(arr.shape)}")
    bad = [(b, int(v)) for b, v in enumerate(arr) if v < 1 or v > S]
    if bad:
        raise ValueError(f"mel_lengths outside [1, S = {S}]: " + ", ".join(f"clip {b}: {v}" for b, v in bad))
    return (ctypes.c_int32 * B)(*[int(v) for v in arr])


def masked_bilstm_plan(video_lengths, T: int):
    """`l2s_masked_bilstm_plan`: (capture_steps, reset_steps) of the BiLSTM recurrence for these lengths - a pure host function of the library."""
    B = len(video_lengths)
    lens = (ctypes.c_int32 * B)(*[int(v) for v in video_lengths])
    cap, rst = (ctypes.c_int32 * B)(), (ctypes.c_int32 * B)()
    nc, nr = _i(), _i()
    check(lib().l2s_masked_bilstm_plan(lens, B, int(T), cap, rst, ctypes.byref(nc), ctypes.byref(nr)))
    return list(cap[:nc.value]), list(rst[:nr.value])


def workspace_bytes_ragged(batch_B, batch_T, H: int = 96, W: int = 96, S: int = 300) -> int:
    """`l2s_workspace_bytes_ragged`: the workspace of a ragged group of these batch shapes, every frame real."""
    G, i32 = len(batch_B), ctypes.c_int32
    need = int(lib().l2s_workspace_bytes_ragged(G, (i32 * G)(*[int(b) for b in batch_B]), (i32 * G)(*[int(t) for t in batch_T]), H, W, S))
    if need < 0:
        check(1)
    return need


MAX_GROUP = 8             # L2S_MAX_GROUP
MAX_RAGGED_CLIPS = 256    # L2S_MAX_RAGGED_CLIPS


def ragged_plan(batch_B, batch_T, video_lengths):
    """`l2s_ragged_plan`: the compact layout of a ragged group, a pure host function of the library.  `batch_B` / `batch_T`: clips and padded length of
    every batch; `video_lengths`: one list per batch, or the flat list of all N lengths in batch order.  Returns `(frame0, pair0, N, Tmax)`: the prefix
    sums (N + 1 entries each) of the lengths and of ceil(len / 2).  Raises `RuntimeError` with the library's message for shapes outside the limits."""
    G = len(batch_B)
    flat = [int(v) for v in video_lengths] if not (len(video_lengths) and hasattr(video_lengths[0], "__len__")) else [int(v) for b in video_lengths for v in b]
    n = sum(int(b) for b in batch_B)
    if len(flat) != n:
        raise ValueError(f"video_lengths must hold {n} lengths (sum of batch_B), got {len(flat)}")
    i32 = ctypes.c_int32
    f0, p0 = (i32 * (n + 1))(), (i32 * (n + 1))()
    N, Tmax = _i(), _i()
    check(lib().l2s_ragged_plan(G, (i32 * G)(*[int(b) for b in batch_B]), (i32 * G)(*[int(t) for t in batch_T]), (i32 * max(n, 1))(*flat), f0, p0,
                                ctypes.byref(N), ctypes.byref(Tmax)))
    return list(f0[:N.value + 1]), list(p0[:N.value + 1]), N.value, Tmax.value


def _i32s(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int32 * max(len(vals), 1))(*vals)


def forward_eval_ragged_plan(batch_B, batch_T, batch_S):
    """`l2s_forward_eval_ragged_plan`: where the packed outputs of an evaluate-shaped ragged group start, a pure host function of the library.  `batch_B` /
    `batch_T` / `batch_S`: clips, padded length and decode steps of every batch.  Returns `(mel_off, stop_off, attn_off, dis_off, N, Tmax, Smax)`: four
    lists of G + 1 float offsets - batch g's block is `[off[g], off[g + 1])` - and the clips, the longest padding and the most steps of the group.
    Raises `RuntimeError` with the library's message for shapes outside the limits."""
    G = len(batch_B)
    if len(batch_T) != G or len(batch_S) != G:
        raise ValueError(f"batch_B, batch_T and batch_S hold one entry per batch ({G}), got {len(batch_T)} and {len(batch_S)}")
    offs = [(_i64 * (G + 1))() for _ in range(4)]
    N, Tmax, Smax = _i(), _i(), _i()
    check(lib().l2s_forward_eval_ragged_plan(G, _i32s(batch_B), _i32s(batch_T), _i32s(batch_S), *offs, ctypes.byref(N), ctypes.byref(Tmax), ctypes.byref(Smax)))
    return tuple(list(o) for o in offs) + (N.value, Tmax.value, Smax.value)


def workspace_bytes_eval_ragged(batch_B, batch_T, batch_S, H: int = 96, W: int = 96) -> int:
    """`l2s_workspace_bytes_eval_ragged`: the workspace of an evaluate-shaped ragged group of these batch shapes, every frame real."""
    G = len(batch_B)
    if len(batch_T) != G or len(batch_S) != G:
        raise ValueError(f"batch_B, batch_T and batch_S hold one entry per batch ({G}), got {len(batch_T)} and {len(batch_S)}")
    need = int(lib().l2s_workspace_bytes_eval_ragged(G, _i32s(batch_B), _i32s(batch_T), _i32s(batch_S), H, W))
    if need < 0:
        check(1)
    return need


def speaker_packed_plan(samples):
    """`l2s_speaker_packed_plan`: the time-major compact layout of the voice tower over clips of these sample counts, a pure host function of the
    library.  Returns `(order, step_rows, step_row0, L_max, R)`: the clips by frame count L_b = n_b // 160 + 1 descending (ties in call order), the
    clips still running at step t (L_max entries), its prefix sum (L_max + 1 entries) and R = sum L_b.  Frame l of the clip of rank r is row
    `step_row0[l] + r`.  Raises `RuntimeError` with the library's message for lengths outside the limits."""
    ns = [int(v) for v in samples]
    B = len(ns)
    lmax = max([n // 160 + 1 for n in ns if n > 0] or [1])
    i32 = ctypes.c_int32
    order, rows, row0 = (i32 * max(B, 1))(), (i32 * lmax)(), (i32 * (lmax + 1))()
    L_max, R = _i(), _i64()
    check(lib().l2s_speaker_packed_plan((_i64 * max(B, 1))(*ns), B, order, rows, row0, ctypes.byref(L_max), ctypes.byref(R)))
    return list(order[:B]), list(rows[:L_max.value]), list(row0[:L_max.value + 1]), L_max.value, R.value


def _host_ints(v, name: str):
    """offsets / samples of a packed call: a host list, or an integer tensor that is already on the host (a device tensor would cost a sync)."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise ValueError(f"{name} must stay on the host (the library plans its launches from it): got a device tensor")
        if v.is_floating_point() or v.dtype == torch.bool:
            raise TypeError(f"{name} must hold integers, got {v.dtype}")
        v = v.tolist()
    out = []
    for x in v:
        if isinstance(x, float) or isinstance(x, bool):
            raise TypeError(f"{name} must hold integers, got {type(x).__name__}")
        out.append(int(x))
    return out


def encoder_tap_shapes(NF: int, H: int):
    """Shapes of the 18 taps of l2s_op_encoder_taps (include/l2s_diag.h) for NF frames of H x H pixels.  Diagnostic only: encoder_fwd(taps=...) sizes
    its tap tensors with it.  The widths and unit counts restate STAGE_CH = {24, 116, 232, 464}, LAST_CH = 768 and the 4 / 8 / 4 units per stage of
    lip2speech_amd/csrc/l2s_model.h; the map halves, rounded up, at the first (stride-2) unit of each stage, as in encoder_run."""
    h = H // 4
    shapes = [(NF, h, h, 24)]
    for cout, n in ((116, 4), (232, 8), (464, 4)):
        h = (h + 1) // 2
        shapes += [(NF, h, h, cout)] * n
    return shapes + [(NF * h * h, 768)]


class NativeModel:
    """Owns an ``l2s_model`` (the packed device weight blob)."""

    def __init__(self, library: Optional[ctypes.CDLL] = None):
        self._L = library or lib()        # every call of this model goes to ONE library: the product, or the diagnostic build (tests of the A/B options, tools)
        self._h = _vp()
        self._check(self._L.l2s_model_create(ctypes.byref(self._h)))
        self._tls = threading.local()      # the workspace is per host thread: several threads may run batches on ONE model (one weight blob)
        self.calls = collections.Counter()  # whole-path entry points used, by C-ABI name (tests assert which route a caller took)

    def _check(self, rc: int) -> None:
        check(rc, self._L)

    def set_option(self, name: str, value: int) -> None:
        """Run-time option of THIS model (include/l2s.h "run-time options"); `native.set_option` changes the defaults of models created later."""
        self._check(self._L.l2s_model_set_option(self._h, name.encode(), int(value)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.l2s_model_destroy(self._h)
        except Exception:
            pass

    def load(self, tensors: Dict[str, torch.Tensor], keys: Iterable[str]) -> None:
        """Hand the checkpoint tensors named ``keys`` (reference key names) to the library and pack them."""
        L = self._L
        for key in keys:
            t = tensors[key]
            if not t.is_floating_point():
                continue                                   # num_batches_tracked: not used in eval arithmetic
            a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
            self._check(L.l2s_model_set_tensor(self._h, key.encode(), a.ctypes.data_as(_vp), a.size))
        self._check(L.l2s_model_finalize(self._h, _stream()))

    # ------------------------------------------------------------------ workspace (caller-owned, cached)
    def workspace(self, B: int, T: int, H: int, W: int, S: int, device, G: int = 0, masked: bool = False) -> torch.Tensor:
        need = int(self._L.l2s_workspace_bytes_multi(G, B, T, H, W, S)) if G else int(self._L.l2s_workspace_bytes(B, T, H, W, S))
        if masked:
            need = int(self._L.l2s_workspace_bytes_masked(B, T, H, W, S))
        return self._workspace(need, device)

    def _workspace(self, need: int, device) -> torch.Tensor:
        ws = getattr(self._tls, "ws", None)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = self._tls.ws = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    # ------------------------------------------------------------------ stages
    def encoder_fwd(self, video: torch.Tensor, taps=None):
        """VideoExtractor.forward: video (B,3,T,H,W) -> feat (B,T,768).  taps = an iterable of tap indices (diagnostic library only): also the stage
        outputs of l2s_op_encoder_taps, as (feat, {index: tensor}) - 0 the front-end map, 1 + u the output of ShuffleNet unit u (channels last, shuffled
        order), 17 the conv_last output.  A unit interior to a stage-chain launch raises with the library's message."""
        video = _f32(video)
        B, C, T, H, W = video.shape
        assert C == 3, "frames are (B,3,T,H,W) RGB"
        feat = torch.empty(B, T, 768, dtype=torch.float32, device=video.device)
        ws = self.workspace(B, T, H, W, 1, video.device)
        if taps is not None:
            shapes = encoder_tap_shapes(B * T, H)
            outs = {int(i): torch.empty(shapes[int(i)], dtype=torch.float32, device=video.device) for i in taps}
            arr = (_vp * len(shapes))(*[outs[i].data_ptr() if i in outs else None for i in range(len(shapes))])
            _dcheck(diag().l2s_op_encoder_taps(self._h, _ptr(video), B, T, H, W, arr, _ptr(feat), _ptr(ws), ws.numel(), _stream()))
            return feat, outs
        self._check(self._L.l2s_encoder_fwd(self._h, _ptr(video), B, T, H, W, _ptr(feat), _ptr(ws), ws.numel(), _stream()))
        return feat

    def decoder_prologue(self, vis: torch.Tensor, emb: torch.Tensor, gumbel: torch.Tensor, want_dis: bool = True, video_lengths=None):
        """`video_lengths` (B integers in [7, T]): `l2s_decoder_prologue_masked` - hand the same lengths to `decode_steps`."""
        vis, emb, gumbel = _f32(vis), _f32(emb), _f32(gumbel)
        B, T, C = vis.shape
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None
        assert C == 1024 and emb.shape == (B, 256)
        m = min_T(T)
        assert m == 0 or gumbel.shape == (B * m, 501), f"gumbel noise must be {(B * m, 501)}"
        state = torch.zeros(int(self._L.l2s_state_floats(B, T)), dtype=torch.float32, device=vis.device)
        dis = torch.empty(B * m, 501, dtype=torch.float32, device=vis.device) if want_dis else None
        ws = self.workspace(B, T, 96, 96, 1, vis.device, masked=lens is not None)
        if lens is not None:
            self._check(self._L.l2s_decoder_prologue_masked(self._h, _ptr(vis), _ptr(emb), _ptr(gumbel), B, T, _ptr(state), _ptr(dis),
                                                            _ptr(ws), ws.numel(), _stream(), lens))
            return state, dis
        self._check(self._L.l2s_decoder_prologue(self._h, _ptr(vis), _ptr(emb), _ptr(gumbel), B, T, _ptr(state), _ptr(dis),
                                         _ptr(ws), ws.numel(), _stream()))
        return state, dis

    def decode_steps(self, state: torch.Tensor, B: int, T: int, S: int, teacher: Optional[torch.Tensor] = None,
                     teacher_mask=None, want_attn: bool = True, attn_logits: bool = False, video_lengths=None):
        dev = state.device
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None
        mel = torch.empty(B, S, 80, dtype=torch.float32, device=dev)
        stop = torch.empty(B, S, dtype=torch.float32, device=dev)
        attn = torch.empty(B, S, T, dtype=torch.float32, device=dev) if want_attn else None
        mask_buf = None
        if teacher is not None and teacher_mask is not None:
            teacher = _f32(teacher)
            assert teacher.shape == (B, S, 80)
            mask_np = np.ascontiguousarray(np.asarray(teacher_mask, dtype=np.uint8))
            assert mask_np.shape == (S,)
            mask_buf = mask_np.ctypes.data_as(_vp)
        else:
            teacher = None
        ws = self.workspace(B, T, 96, 96, S, dev, masked=lens is not None)
        if lens is not None:
            self._check(self._L.l2s_decode_steps_masked(self._h, _ptr(state), B, T, S, _ptr(teacher), mask_buf, _ptr(mel), _ptr(stop),
                                                        _ptr(attn), 1 if attn_logits else 0, _ptr(ws), ws.numel(), _stream(), lens))
            return mel, stop, attn
        self._check(self._L.l2s_decode_steps(self._h, _ptr(state), B, T, S, _ptr(teacher), mask_buf, _ptr(mel), _ptr(stop),
                                     _ptr(attn), 1 if attn_logits else 0, _ptr(ws), ws.numel(), _stream()))
        return mel, stop, attn

    def postnet(self, mel: torch.Tensor, want_cf: bool = False):
        mel = _f32(mel)
        B, S, C = mel.shape
        assert C == 80
        out = torch.empty(B, 80, S, dtype=torch.float32, device=mel.device)
        cf = torch.empty(B, 80, S, dtype=torch.float32, device=mel.device) if want_cf else None
        ws = self.workspace(B, 29, 96, 96, S, mel.device)
        self._check(self._L.l2s_postnet(self._h, _ptr(mel), B, S, _ptr(out), _ptr(cf), _ptr(ws), ws.numel(), _stream()))
        return out, cf

    def forward_eval(self, video: torch.Tensor, emb: torch.Tensor, gumbel: torch.Tensor, S: int, teacher: Optional[torch.Tensor] = None,
                     teacher_mask=None, video_lengths=None):
        """`Lip2Speech.forward(..., tf_ratio)` in eval mode as ONE native call (`l2s_forward_eval`; what evaluate.py runs, evaluate.py:38):
        S = mels.shape[2] steps, free-running unless `teacher` (B,S,80) = cat(BOS, mels)[:, :S] and the per-step `teacher_mask` are given.
        Returns (mel (B,80,S), mel_post (B,80,S), stop (B,S), attention LOGITS (B,S,T), content_dis).
        `video_lengths` (B integers in [7, T]; the clips ZERO-padded to T): `l2s_forward_eval_masked` - row b is what clip b alone at T = len_b
        gives; logits of the columns t >= len_b are -inf, content_dis rows past a clip's min_T(len_b) slots are zeros."""
        if video_lengths is None:
            return self.forward_eval_multi([(video, emb, gumbel, teacher)], S, teacher_mask=teacher_mask)[0]
        video, emb, gumbel = _f32(video), _f32(emb), _f32(gumbel)
        B, _, T, H, W = video.shape
        m = min_T(T)
        if emb.shape != (B, 256) or gumbel.shape != (B * m, 501):
            raise ValueError(f"emb must be {(B, 256)} and the gumbel noise {(B * m, 501)}, got {tuple(emb.shape)} and {tuple(gumbel.shape)}")
        lens = video_lengths_array(video_lengths, B, T)
        mask_buf = mask_np = None
        if teacher_mask is not None and any(teacher_mask):
            mask_np = np.ascontiguousarray(np.asarray(teacher_mask, dtype=np.uint8))
            assert mask_np.shape == (S,)
            mask_buf = mask_np.ctypes.data_as(_vp)
            teacher = _f32(teacher)
            assert teacher.shape == (B, S, 80), "teacher frames are (B,S,80) = cat(BOS, mels)[:, :S]"
        else:
            teacher = None
        dev = video.device
        mel_cf = torch.empty(B, 80, S, dtype=torch.float32, device=dev)
        mel_post = torch.empty(B, 80, S, dtype=torch.float32, device=dev)
        stop = torch.empty(B, S, dtype=torch.float32, device=dev)
        attn = torch.empty(B, S, T, dtype=torch.float32, device=dev)
        dis = torch.empty(B * m, 501, dtype=torch.float32, device=dev)
        self.calls["l2s_forward_eval_masked"] += 1
        ws = self.workspace(B, T, H, W, S, dev, masked=True)
        self._check(self._L.l2s_forward_eval_masked(self._h, _ptr(video), _ptr(emb), _ptr(gumbel), B, T, H, W, S, _ptr(teacher), mask_buf, _ptr(mel_cf),
                                                    _ptr(mel_post), _ptr(stop), _ptr(attn), _ptr(dis), _ptr(ws), ws.numel(), _stream(), lens))
        return mel_cf, mel_post, stop, attn, dis

    def forward_eval_multi(self, batches, S: int, teacher_mask=None):
        """Grouped `forward_eval` (`l2s_forward_eval_multi`): up to 8 (video, emb, gumbel[, teacher]) tuples of one shape through ONE launch
        chain; the batches share S and the scheduled-sampling mask.  Returns per batch (mel, mel_post, stop, attn_logits, content_dis) -
        views of one allocation, each bit-identical to `forward_eval` on that batch alone."""
        G = len(batches)
        assert 1 <= G <= 8, "1..8 batches per group"
        vids = [_f32(b[0]) for b in batches]
        embs = [_f32(b[1]) for b in batches]
        gums = [_f32(b[2]) for b in batches]
        B, _, T, H, W = vids[0].shape
        m = min_T(T)
        assert all(v.shape == vids[0].shape for v in vids) and all(e.shape == (B, 256) for e in embs), "the batches of a group share one shape"
        assert all(g.shape == (B * m, 501) for g in gums), f"gumbel noise must be {(B * m, 501)}"
        teach = mask_buf = mask_np = None
        if teacher_mask is not None and any(teacher_mask):
            mask_np = np.ascontiguousarray(np.asarray(teacher_mask, dtype=np.uint8))
            assert mask_np.shape == (S,)
            mask_buf = mask_np.ctypes.data_as(_vp)
            teach = [_f32(b[3]) for b in batches]
            assert all(t.shape == (B, S, 80) for t in teach), "teacher frames are (B,S,80) = cat(BOS, mels)[:, :S]"
        dev = vids[0].device
        mel_cf = torch.empty(G * B, 80, S, dtype=torch.float32, device=dev)
        mel_post = torch.empty(G * B, 80, S, dtype=torch.float32, device=dev)
        stop = torch.empty(G * B, S, dtype=torch.float32, device=dev)
        attn = torch.empty(G * B, S, T, dtype=torch.float32, device=dev)
        dis = torch.empty(G * B * m, 501, dtype=torch.float32, device=dev)
        arr = lambda ts: (_vp * G)(*[t.data_ptr() for t in ts])      # noqa: E731
        self.calls["l2s_forward_eval" if G == 1 else "l2s_forward_eval_multi"] += 1
        if G == 1:
            ws = self.workspace(B, T, H, W, S, dev)
            self._check(self._L.l2s_forward_eval(self._h, _ptr(vids[0]), _ptr(embs[0]), _ptr(gums[0]), B, T, H, W, S, _ptr(teach[0]) if teach else None, mask_buf,
                                         _ptr(mel_cf), _ptr(mel_post), _ptr(stop), _ptr(attn), _ptr(dis), _ptr(ws), ws.numel(), _stream()))
        else:
            ws = self.workspace(B, T, H, W, S, dev, G=G)
            self._check(self._L.l2s_forward_eval_multi(self._h, G, arr(vids), arr(embs), arr(gums), arr(teach) if teach else None, mask_buf, B, T, H, W, S,
                                               _ptr(mel_cf), _ptr(mel_post), _ptr(stop), _ptr(attn), _ptr(dis), _ptr(ws), ws.numel(), _stream()))
        return [(mel_cf[g * B:(g + 1) * B], mel_post[g * B:(g + 1) * B], stop[g * B:(g + 1) * B], attn[g * B:(g + 1) * B],
                 dis[g * B * m:(g + 1) * B * m]) for g in range(G)]

    def forward_eval_staged(self, video: torch.Tensor, emb: torch.Tensor, gumbel: torch.Tensor, S: int):
        """The same pass as five staged C-ABI calls (encoder, visual cat, prologue, loop, post-net) - the route `net.encoder` / `net.decoder`
        take when a caller uses them separately; the tests hold it bit-identical to `forward_eval`."""
        B, _, T, _, _ = video.shape
        feat = self.encoder_fwd(video)
        vis = build_visual(feat, emb)
        state, dis = self.decoder_prologue(vis, emb, gumbel)
        mel, stop, attn = self.decode_steps(state, B, T, S, want_attn=True, attn_logits=True)
        mel_post, mel_cf = self.postnet(mel, want_cf=True)
        return mel_cf, mel_post, stop, attn, dis

    def inference(self, video: torch.Tensor, emb: torch.Tensor, gumbel: torch.Tensor, S: int = 300, want_attn: bool = False, video_lengths=None):
        """`video_lengths` (B integers in [7, T]; the clips ZERO-padded to T): `l2s_inference_masked` - row b is what clip b alone at T = len_b
        gives, attention columns t >= len_b are zeros; clip b uses the first min_T(len_b) of its min_T(T) Gumbel rows."""
        video, emb, gumbel = _f32(video), _f32(emb), _f32(gumbel)
        B, _, T, H, W = video.shape
        lens = None
        if video_lengths is not None:
            if emb.shape != (B, 256) or gumbel.shape != (B * min_T(T), 501):
                raise ValueError(f"emb must be {(B, 256)} and the gumbel noise {(B * min_T(T), 501)}, got {tuple(emb.shape)} and {tuple(gumbel.shape)}")
            lens = video_lengths_array(video_lengths, B, T)
        mel_post = torch.empty(B, 80, S, dtype=torch.float32, device=video.device)
        lengths = torch.empty(B, dtype=torch.int64, device=video.device)
        attn = torch.empty(B, S, T, dtype=torch.float32, device=video.device) if want_attn else None
        if lens is not None:
            self.calls["l2s_inference_masked"] += 1
            ws = self.workspace(B, T, H, W, S, video.device, masked=True)
            self._check(self._L.l2s_inference_masked(self._h, _ptr(video), _ptr(emb), _ptr(gumbel), B, T, H, W, S, _ptr(mel_post),
                                                     _ptr(lengths), _ptr(attn), _ptr(ws), ws.numel(), _stream(), lens))
            return mel_post, lengths, attn
        self.calls["l2s_inference"] += 1
        ws = self.workspace(B, T, H, W, S, video.device)
        self._check(self._L.l2s_inference(self._h, _ptr(video), _ptr(emb), _ptr(gumbel), B, T, H, W, S, _ptr(mel_post),
                                  _ptr(lengths), _ptr(attn), _ptr(ws), ws.numel(), _stream()))
        return mel_post, lengths, attn

    def inference_multi(self, batches, S: int = 300, want_attn: bool = False, video_lengths=None):
        """Grouped inference (`l2s_inference_multi`): `batches` = up to 8 (video, emb, gumbel) tuples of the same shape, advanced through ONE
        launch chain.  Returns [(mel_post (B,80,S), lengths (B,), attn (B,S,T) or None)] - views of one allocation, each bit-identical to
        `inference` on that batch."""
        if video_lengths is not None:
            raise NotImplementedError("the grouped entry points have no length-masked form (include/l2s.h): call inference(..., video_lengths=) per batch")
        G = len(batches)
        assert 1 <= G <= 8, "1..8 batches per group"
        vids = [_f32(b[0]) for b in batches]
        embs = [_f32(b[1]) for b in batches]
        gums = [_f32(b[2]) for b in batches]
        B, _, T, H, W = vids[0].shape
        assert all(v.shape == vids[0].shape for v in vids) and all(e.shape == (B, 256) for e in embs), "the batches of a group share one shape"
        dev = vids[0].device
        mel_post = torch.empty(G * B, 80, S, dtype=torch.float32, device=dev)
        lengths = torch.empty(G * B, dtype=torch.int64, device=dev)
        attn = torch.empty(G * B, S, T, dtype=torch.float32, device=dev) if want_attn else None
        self.calls["l2s_inference_multi"] += 1
        ws = self.workspace(B, T, H, W, S, dev, G=G)
        arr = lambda ts: (_vp * G)(*[t.data_ptr() for t in ts])      # noqa: E731
        self._check(self._L.l2s_inference_multi(self._h, G, arr(vids), arr(embs), arr(gums), B, T, H, W, S, _ptr(mel_post), _ptr(lengths), _ptr(attn),
                                        _ptr(ws), ws.numel(), _stream()))
        return [(mel_post[g * B:(g + 1) * B], lengths[g * B:(g + 1) * B], attn[g * B:(g + 1) * B] if want_attn else None) for g in range(G)]

    def inference_ragged(self, batches, video_lengths, S: int = 300, want_attn: bool = False):
        """A ragged group (`l2s_inference_ragged`): `batches` = up to 8 (video, emb, gumbel) tuples, each batch with its own B and T (padded to its own
        longest clip, or further), at most 256 clips in all; `video_lengths` = one sequence of B_g lengths in [7, T_g] per batch.  All clips run as rows
        of ONE launch chain, each decoded as it would be alone, the encoder on the real frames only (frames past a clip's length are never read).
        Returns, per batch, `(mel_post (B_g,80,S), lengths (B_g,), attn (B_g,S,T_g) or None)` - slices of the group's tensors; row b is what
        `inference(batch, video_lengths=)` gives for it."""
        G = len(batches)
        shapes, lens, N = self._ragged_check(batches, video_lengths)
        vids = [_f32(b[0]) for b in batches]
        embs = [_f32(b[1]) for b in batches]
        gums = [_f32(b[2]) for b in batches]
        H, W = shapes[0][3:]
        Tmax = max(sh[2] for sh in shapes)
        i32 = ctypes.c_int32
        bB, bT = (i32 * G)(*[sh[0] for sh in shapes]), (i32 * G)(*[sh[2] for sh in shapes])
        flat = (i32 * N)(*[v for l in lens for v in l])
        dev = vids[0].device
        need = int(self._L.l2s_workspace_bytes_ragged(G, bB, bT, H, W, S))
        if need < 0:
            self._check(1)
        ws = self._workspace(need, dev)
        mel_post = torch.empty(N, 80, S, dtype=torch.float32, device=dev)
        lengths = torch.empty(N, dtype=torch.int64, device=dev)
        attn = torch.empty(N, S, Tmax, dtype=torch.float32, device=dev) if want_attn else None
        self.calls["l2s_inference_ragged"] += 1
        arr = lambda ts: (_vp * G)(*[t.data_ptr() for t in ts])      # noqa: E731
        self._check(self._L.l2s_inference_ragged(self._h, G, arr(vids), arr(embs), arr(gums), bB, bT, flat, H, W, S, _ptr(mel_post), _ptr(lengths), _ptr(attn),
                                                 _ptr(ws), ws.numel(), _stream()))
        out, c = [], 0
        for sh in shapes:
            out.append((mel_post[c:c + sh[0]], lengths[c:c + sh[0]], attn[c:c + sh[0], :, :sh[2]] if want_attn else None))
            c += sh[0]
        return out

    @staticmethod
    def _ragged_check(batches, video_lengths):
        """What the ragged entry points check before anything reaches the device: the group's limits, the shapes of every batch's operands and its
        lengths (`ValueError` / `TypeError`).  Returns (video shapes, one int32 length array per batch, N)."""
        G = len(batches)
        if not 1 <= G <= MAX_GROUP:
            raise ValueError(f"a ragged group holds 1..{MAX_GROUP} batches (L2S_MAX_GROUP), got {G}")
        if len(video_lengths) != G:
            raise ValueError(f"video_lengths must hold one sequence of lengths per batch ({G}), got {len(video_lengths)}")
        shapes = [tuple(b[0].shape) for b in batches]
        if any(len(sh) != 5 or sh[1] != 3 for sh in shapes) or any(sh[3:] != shapes[0][3:] for sh in shapes):
            raise ValueError(f"the batches of a ragged group are (B,3,T,H,W) videos of one H x W, got {shapes}")
        lens = [video_lengths_array(vl, sh[0], sh[2]) for vl, sh in zip(video_lengths, shapes)]      # ValueError / TypeError before anything reaches the device
        N = sum(sh[0] for sh in shapes)
        if N > MAX_RAGGED_CLIPS:
            raise ValueError(f"a ragged group holds at most {MAX_RAGGED_CLIPS} clips (L2S_MAX_RAGGED_CLIPS), got {N}")
        for b, sh in zip(batches, shapes):
            m = sh[2] // 7      # l2s_min_T(T_g) for T_g >= 7 (the stride-7 branch of Content.agg)
            if tuple(b[1].shape) != (sh[0], 256) or tuple(b[2].shape) != (sh[0] * m, 501):
                raise ValueError(f"emb must be {(sh[0], 256)} and the gumbel noise {(sh[0] * m, 501)}, got {tuple(b[1].shape)} and {tuple(b[2].shape)}")
        return shapes, lens, N

    def forward_eval_ragged(self, batches, video_lengths, S):
        """An evaluate-shaped ragged group (`l2s_forward_eval_ragged`): eval-mode `forward` at tf_ratio = 1 over up to 8 (video, emb, gumbel) batches that
        differ in B, T and step count, at most 256 clips in all, as rows of ONE launch chain.  `video_lengths` = one sequence of B_g lengths in [7, T_g]
        per batch, `S` = one step count in [1, 300] per batch (its `melspecs.shape[2]`).  Free-running: a teacher-forced batch keeps
        `forward_eval(..., video_lengths=)`.  The chain decodes every row for max(S) steps; a shorter batch's extra steps reach no output.
        Returns, per batch, `(mel (B_g,80,S_g), mel_post (B_g,80,S_g), stop (B_g,S_g), attention LOGITS (B_g,S_g,T_g), content_dis (B_g*min_T(T_g),501))` -
        contiguous views of the group's five packed tensors, each what `forward_eval(batch, S_g, video_lengths=)` gives."""
        G = len(batches)
        shapes, lens, N = self._ragged_check(batches, video_lengths)
        steps = S.detach().cpu().numpy() if isinstance(S, torch.Tensor) else np.asarray(S)
        if steps.shape != (G,):
            raise ValueError(f"S must hold one step count per batch - shape ({G},) - got {tuple(steps.shape)}")
        if steps.dtype.kind not in "iu":
            raise TypeError(f"S must hold integers, got {steps.dtype}")
        bad = [(g, int(v)) for g, v in enumerate(steps) if v < 1 or v > 300]
        if bad:
            raise ValueError("S outside [1, 300]: " + ", ".join(f"batch {g}: {v}" for g, v in bad))
        vids = [_f32(b[0]) for b in batches]
        embs = [_f32(b[1]) for b in batches]
        gums = [_f32(b[2]) for b in batches]
        H, W = shapes[0][3:]
        i32 = ctypes.c_int32
        bB, bT, bS = (i32 * G)(*[sh[0] for sh in shapes]), (i32 * G)(*[sh[2] for sh in shapes]), (i32 * G)(*[int(v) for v in steps])
        flat = (i32 * N)(*[v for l in lens for v in l])
        offs = [(_i64 * (G + 1))() for _ in range(4)]
        n_, t_, s_ = _i(), _i(), _i()
        self._check(self._L.l2s_forward_eval_ragged_plan(G, bB, bT, bS, *offs, ctypes.byref(n_), ctypes.byref(t_), ctypes.byref(s_)))
        mel_off, stop_off, attn_off, dis_off = (list(o) for o in offs)
        need = int(self._L.l2s_workspace_bytes_eval_ragged(G, bB, bT, bS, H, W))
        if need < 0:
            self._check(1)
        dev = vids[0].device
        ws = self._workspace(need, dev)
        new = lambda n: torch.empty(n, dtype=torch.float32, device=dev)      # noqa: E731
        mel_cf, mel_post, stop, attn, dis = new(mel_off[G]), new(mel_off[G]), new(stop_off[G]), new(attn_off[G]), new(dis_off[G])
        self.calls["l2s_forward_eval_ragged"] += 1
        arr = lambda ts: (_vp * G)(*[t.data_ptr() for t in ts])      # noqa: E731
        self._check(self._L.l2s_forward_eval_ragged(self._h, G, arr(vids), arr(embs), arr(gums), bB, bT, bS, flat, H, W, _ptr(mel_cf), _ptr(mel_post), _ptr(stop),
                                                    _ptr(attn), _ptr(dis), _ptr(ws), ws.numel(), _stream()))
        out = []
        for g, sh in enumerate(shapes):
            B, T, Sg = sh[0], sh[2], int(steps[g])
            out.append((mel_cf[mel_off[g]:mel_off[g + 1]].view(B, 80, Sg), mel_post[mel_off[g]:mel_off[g + 1]].view(B, 80, Sg),
                        stop[stop_off[g]:stop_off[g + 1]].view(B, Sg), attn[attn_off[g]:attn_off[g + 1]].view(B, Sg, T),
                        dis[dis_off[g]:dis_off[g + 1]].view(B * (T // 7), 501)))
        return out

    def speaker_encoder_fwd(self, audio: torch.Tensor, taps: bool = False):
        """SpeakerEncoder.inference (audio.py:131-150): audio (B,N) -> emb (B,256).  taps=True (diagnostic library only): also the stage outputs of
        l2s_op_speaker_taps as a list of 7 tensors - spec (B*L,402), power (B*L,204), mel (B*L,40), the three hidden sequences (B,L,256), linear (B,256)."""
        audio = _f32(audio)
        B, N = audio.shape
        emb = torch.empty(B, 256, dtype=torch.float32, device=audio.device)
        ws = torch.empty(int(self._L.l2s_speaker_workspace_bytes(B, N)), dtype=torch.uint8, device=audio.device)
        if taps:
            L = N // 160 + 1
            shapes = [(B * L, 402), (B * L, 204), (B * L, 40)] + [(B, L, 256)] * 3 + [(B, 256)]
            outs = [torch.empty(s, dtype=torch.float32, device=audio.device) for s in shapes]
            arr = (_vp * 7)(*[t.data_ptr() for t in outs])
            _dcheck(diag().l2s_op_speaker_taps(self._h, _ptr(audio), B, N, arr, _ptr(emb), _ptr(ws), ws.numel(), _stream()))
            return emb, outs
        self._check(self._L.l2s_speaker_encoder_fwd(self._h, _ptr(audio), B, N, _ptr(emb), _ptr(ws), ws.numel(), _stream()))
        return emb

    def speaker_encoder_packed(self, audio_packed: torch.Tensor, offsets, samples, taps: bool = False):
        """`l2s_speaker_encoder_packed`: the voice tower over B clips of unequal length, each embedding what `speaker_encoder_fwd` gives for that clip
        alone.  `audio_packed`: a device fp32 buffer of any shape; clip b is `samples[b]` floats at float offset `offsets[b]` of it (a padded (B, N)
        tensor: offsets b * N).  `offsets` / `samples`: host lists or host integer tensors.  -> emb (B,256) in call order.  taps=True (diagnostic
        library only): also the seven stage outputs of `l2s_op_speaker_taps_packed` in the compact layout of `speaker_packed_plan` - spec (R,402),
        power (R,204), mel (R,40), the three hidden sequences (R,256), linear (B,256)."""
        audio_packed = _f32(audio_packed)
        off, ns = _host_ints(offsets, "offsets"), _host_ints(samples, "samples")
        B = len(ns)
        if B < 1 or len(off) != B:
            raise ValueError(f"offsets and samples must hold one entry per clip (at least one): got {len(off)} and {B}")
        last = max(o + n for o, n in zip(off, ns))
        if last > audio_packed.numel():
            raise ValueError(f"a clip ends at float {last} of a buffer of {audio_packed.numel()}")
        L, dev = (diag() if taps else self._L), audio_packed.device
        c_off, c_ns = (_i64 * B)(*off), (_i64 * B)(*ns)
        need = int(L.l2s_speaker_workspace_bytes_packed(c_ns, B))
        if need < 0:
            check(1, L)
        emb = torch.empty(B, 256, dtype=torch.float32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if taps:
            R = sum(n // 160 + 1 for n in ns)
            shapes = [(R, 402), (R, 204), (R, 40)] + [(R, 256)] * 3 + [(B, 256)]
            outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
            arr = (_vp * 7)(*[t.data_ptr() for t in outs])
            _dcheck(L.l2s_op_speaker_taps_packed(self._h, _ptr(audio_packed), c_off, c_ns, B, arr, _ptr(emb), _ptr(ws), ws.numel(), _stream()))
            return emb, outs
        self._check(L.l2s_speaker_encoder_packed(self._h, _ptr(audio_packed), c_off, c_ns, B, _ptr(emb), _ptr(ws), ws.numel(), _stream()))
        return emb

    def _faces(self, faces: torch.Tensor):
        """(B,3,160,160) fp32 on the device, each image contiguous; the batch stride may be anything (face_frames[:, 0] is used as it is)."""
        if not faces.is_cuda:
            raise RuntimeError("the face tower runs on the GPU: move face_frames to cuda (no CPU fallback)")
        if faces.dim() != 4 or faces.shape[1] != 3:
            raise ValueError(f"faces must be (B, 3, H, W), got {tuple(faces.shape)}")
        B, _, H, W = faces.shape
        if faces.dtype != torch.float32 or faces.stride()[1:] != (H * W, W, 1) or faces.stride(0) < 3 * H * W:
            faces = faces.detach().to(torch.float32).contiguous()
        need = int(self._L.l2s_face_workspace_bytes(B, H, W))
        if need < 0:
            self._check(1)
        return faces, B, H, W, need

    def face_encoder_fwd(self, faces: torch.Tensor, want_proj: bool = False, taps: bool = False):
        """FaceRecognizer (vgg_face.py:28-60): faces (B,3,160,160) -> emb (B,256) = normalize(relu(proj)), and proj (B,256) with want_proj.
        taps=True (diagnostic library only): also the stage outputs of l2s_op_face_taps as a list of 8 tensors."""
        faces, B, H, W, need = self._faces(faces)
        dev = faces.device
        emb = torch.empty(B, 256, dtype=torch.float32, device=dev)
        proj = torch.empty(B, 256, dtype=torch.float32, device=dev) if want_proj else None
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if taps:
            shapes = [(B, 17, 17, 256)] * 2 + [(B, 8, 8, 896)] * 2 + [(B, 3, 3, 1792)] * 2 + [(B, 1792), (B, 512)]
            outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
            arr = (_vp * 8)(*[t.data_ptr() for t in outs])
            _dcheck(diag().l2s_op_face_taps(self._h, faces.data_ptr(), faces.stride(0), B, arr, _ptr(proj), _ptr(emb), _ptr(ws), ws.numel(), _stream()))
            return emb, proj, outs
        self._check(self._L.l2s_face_encoder_fwd(self._h, faces.data_ptr(), faces.stride(0), B, H, W, _ptr(proj), _ptr(emb), _ptr(ws), ws.numel(), _stream()))
        return (emb, proj) if want_proj else emb

    # ------------------------------------------------------------------ training (forward with tapes + backward)
    def train_bind(self, params: Dict[str, torch.Tensor], grads: Dict[str, torch.Tensor]) -> None:
        """Bind canonical-layout device parameters and their gradient slots by checkpoint key."""
        self._bound = (params, grads)                       # keep the tensors alive
        for key, p in params.items():
            if not p.is_floating_point():
                continue
            g = grads.get(key)
            self._check(self._L.l2s_train_bind(self._h, key.encode(), _ptr(p), _ptr(g) if g is not None else None))

    def train_set_bn(self, batch_stats: bool, momentum: float = 0.1) -> None:
        """BatchNorm of the training entry points: batch statistics + running-stat updates (nn.Module.train()) or running statistics."""
        self._check(self._L.l2s_train_set_bn(self._h, 1 if batch_stats else 0, float(momentum)))

    def train_refresh_weights(self) -> None:
        """Device-side re-pack of the weight blob from the bound tensors (needs self.set_option('refresh_map', 1) before load())."""
        self._check(self._L.l2s_train_refresh_weights(self._h, _stream()))

    def train_postnet_fwd(self, mel: torch.Tensor, drop: Optional[torch.Tensor] = None, mel_lengths=None):
        """Post-net forward with a tape: mel (B,S,80) -> (mel_post (B,80,S), tape).  drop: packed dropout multipliers (postnet_drop_pack).
        `mel_lengths` (B integers in [1, S]): `l2s_train_postnet_masked_fwd` - rows s >= S_b of `mel` are ZEROED IN PLACE (when `mel` is fp32 and contiguous,
        as the loop returns it), the post-net sees zeros past every clip's end and mel_post[b, :, S_b:] is exact zeros; hand the same lengths (and this tape)
        to `train_postnet_bwd`."""
        B, S, _ = mel.shape
        lens = mel_lengths_array(mel_lengths, B, S) if mel_lengths is not None else None      # checked on the host, before anything else
        mel = _f32(mel)
        L = self._L
        out = torch.empty(B, 80, S, dtype=torch.float32, device=mel.device)
        if lens is not None:
            tape = torch.zeros(int(L.l2s_train_postnet_tape_floats_masked(B, S)), dtype=torch.float32, device=mel.device)
            self.calls["l2s_train_postnet_masked_fwd"] += 1
            self._check(L.l2s_train_postnet_masked_fwd(self._h, _ptr(mel), B, S, _ptr(tape), _ptr(out), _ptr(drop), _stream(), lens))
            return out, tape
        tape = torch.zeros(int(L.l2s_train_postnet_tape_floats(B, S)), dtype=torch.float32, device=mel.device)
        self._check(L.l2s_train_postnet_fwd(self._h, _ptr(mel), B, S, _ptr(tape), _ptr(out), _ptr(drop), _stream()))
        return out, tape

    def train_postnet_bwd(self, mel: torch.Tensor, dmel_post: torch.Tensor, tape: torch.Tensor, drop: Optional[torch.Tensor] = None, mel_lengths=None) -> torch.Tensor:
        """Post-net backward: dmel_post (B,80,S) -> dmel (B,S,80) (residual path included); parameter gradients into the bound slots.
        `mel_lengths`: the lengths of the masked forward that wrote `tape` (`l2s_train_postnet_masked_bwd`): pad positions of dmel_post are never used,
        rows s >= S_b of dmel come back as exact zeros."""
        B, S, _ = mel.shape
        lens = mel_lengths_array(mel_lengths, B, S) if mel_lengths is not None else None
        mel, dmel_post = _f32(mel), _f32(dmel_post)
        L = self._L
        dmel = torch.zeros_like(mel)
        if lens is not None:
            ws = torch.empty(int(L.l2s_train_postnet_ws_bytes_masked(B, S)), dtype=torch.uint8, device=mel.device)
            self.calls["l2s_train_postnet_masked_bwd"] += 1
            self._check(L.l2s_train_postnet_masked_bwd(self._h, _ptr(mel), _ptr(dmel_post), B, S, _ptr(tape), _ptr(dmel), _ptr(drop), _ptr(ws), ws.numel(),
                                                       _stream(), lens))
            return dmel
        ws = torch.empty(int(L.l2s_train_postnet_ws_bytes(B, S)), dtype=torch.uint8, device=mel.device)
        self._check(L.l2s_train_postnet_bwd(self._h, _ptr(mel), _ptr(dmel_post), B, S, _ptr(tape), _ptr(dmel), _ptr(drop), _ptr(ws), ws.numel(), _stream()))
        return dmel

    def train_postnet(self, mel: torch.Tensor, dmel_post: torch.Tensor, drop: Optional[torch.Tensor] = None):
        """Post-net forward + backward (stage 1 of the training path): returns mel_post (B,80,S) and dmel (B,S,80)."""
        out, tape = self.train_postnet_fwd(mel, drop)
        return out, self.train_postnet_bwd(mel, dmel_post, tape, drop)

    def train_pack_weights(self, device) -> torch.Tensor:
        """Transposed step / prologue weights for the backward GEMMs, packed on the device from the bound parameters."""
        L = self._L
        wbuf = torch.empty(int(L.l2s_train_steps_weights_floats()), dtype=torch.float32, device=device)
        self._check(L.l2s_train_steps_pack_weights(self._h, _ptr(wbuf), _stream()))
        return wbuf

    def train_steps_fwd(self, state, B, T, S, teacher=None, teacher_mask=None, drop=None, video_lengths=None):
        """Loop forward with a tape.  Returns (mel (B,S,80), stop (B,S), attn_logits (B,S,T)) and the context for train_steps_bwd.
        drop: dict of dropout multipliers (any subset): 'prenet' (S,B,256), 'attn' (S,B,T), 'rnn' (S,B,512).
        `video_lengths` (B integers in [7, T]; a state of `train_prologue_fwd(..., video_lengths=)`): `l2s_train_steps_masked_fwd` - row b attends to its
        own frames and content slots, attn_logits at t >= len_b are -inf; the context carries the lengths to `train_steps_bwd`."""
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None
        drop = {k: _f32(v) for k, v in (drop or {}).items() if k in ("prenet", "attn", "rnn") and v is not None}
        dp, da, dr = drop.get("prenet"), drop.get("attn"), drop.get("rnn")
        assert dp is None or tuple(dp.shape) == (S, B, 256)
        assert da is None or tuple(da.shape) == (S, B, T)
        assert dr is None or tuple(dr.shape) == (S, B, 512)
        L, dev = self._L, state.device
        tape = torch.zeros(int((L.l2s_train_steps_tape_floats_masked if lens is not None else L.l2s_train_steps_tape_floats)(B, S)), dtype=torch.float32, device=dev)
        ws = torch.empty(int(L.l2s_train_steps_ws_bytes(B, S)), dtype=torch.uint8, device=dev)
        mel = torch.empty(B, S, 80, dtype=torch.float32, device=dev)
        stop = torch.empty(B, S, dtype=torch.float32, device=dev)
        logits = torch.empty(B, S, T, dtype=torch.float32, device=dev)
        mask_np = mask_dev = mask_ptr = None
        if teacher is not None:
            teacher = _f32(teacher)
            mask_np = np.ascontiguousarray(np.asarray(teacher_mask, dtype=np.uint8))
            mask_dev = torch.from_numpy(mask_np).to(dev)
            mask_ptr = mask_np.ctypes.data_as(_vp)
        args = (self._h, _ptr(state), B, T, S, _ptr(teacher), mask_ptr, _ptr(mask_dev) if mask_dev is not None else None,
                _ptr(tape), _ptr(mel), _ptr(stop), _ptr(logits), _ptr(dp), _ptr(da), _ptr(dr), _ptr(ws), ws.numel(), _stream())
        if lens is not None:
            self.calls["l2s_train_steps_masked_fwd"] += 1
            self._check(L.l2s_train_steps_masked_fwd(*args, lens))
        else:
            self._check(L.l2s_train_steps_fwd(*args))
        ctx = dict(state=state, B=B, T=T, S=S, tape=tape, ws=ws, logits=logits, mask_np=mask_np, mask_ptr=mask_ptr, teacher=teacher, mask_dev=mask_dev,
                   drop=(dp, da, dr), lens=lens)
        return (mel, stop, logits), ctx

    def train_steps_bwd(self, ctx, dmel, dstop, wbuf=None):
        """BPTT through the loop: dmel (B,S,80), dstop (B,S) -> gradients of the prologue state; parameter gradients into the bound slots."""
        L, state = self._L, ctx["state"]
        B, T, S, dev = ctx["B"], ctx["T"], ctx["S"], state.device
        m = min_T(T)
        out = {"dk": torch.empty(B, T, 512, device=dev), "dv": torch.empty(B, T, 512, device=dev), "dckey": torch.empty(B, m, 256, device=dev),
               "dcval": torch.empty(B, m, 256, device=dev), "dh_init": torch.empty(2, B, 512, device=dev), "de_c": torch.empty(B, 512, device=dev)}
        if wbuf is None:
            wbuf = self.train_pack_weights(dev)
        ws = ctx["ws"]
        args = (self._h, _ptr(state), B, T, S, ctx["mask_ptr"], _ptr(ctx["tape"]), _ptr(ctx["logits"]), _ptr(_f32(dmel)), _ptr(_f32(dstop)),
                _ptr(wbuf), _ptr(out["dk"]), _ptr(out["dv"]), _ptr(out["dckey"]), _ptr(out["dcval"]), _ptr(out["dh_init"]), _ptr(out["de_c"]),
                _ptr(ctx["drop"][0]), _ptr(ctx["drop"][1]), _ptr(ctx["drop"][2]), _ptr(ws), ws.numel(), _stream())
        if ctx.get("lens") is not None:      # a masked forward: dk / dv rows t >= len_b and the content gradients of slots >= m_b come back as exact zeros
            self.calls["l2s_train_steps_masked_bwd"] += 1
            self._check(L.l2s_train_steps_masked_bwd(*args, ctx["lens"]))
        else:
            self._check(L.l2s_train_steps_bwd(*args))
        return out

    def train_steps(self, state, B, T, S, dmel, dstop, teacher=None, teacher_mask=None, drop=None, video_lengths=None):
        """Loop forward-with-tape + BPTT (stage 2 of the training path).  Returns (mel, stop, attn_logits) and the state gradients."""
        outs, ctx = self.train_steps_fwd(state, B, T, S, teacher, teacher_mask, drop=drop, video_lengths=video_lengths)
        return outs, self.train_steps_bwd(ctx, dmel, dstop)

    def train_encoder_fwd(self, video, emb=None, video_lengths=None):
        """Encoder forward with a tape.  Returns (vis (B,T,1024) or None, feat (B,T,768), tape).
        `video_lengths` (B integers in [7, T]; the clips ZERO-padded to T): `l2s_train_encoder_masked_fwd` - the trunk runs on the real frames only, the
        feature columns of rows t >= len_b are zeros; hand the same lengths (and this tape) to `train_encoder_bwd`."""
        B, _, T, H, W = video.shape
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None      # checked on the host, before anything else
        video = _f32(video)
        L, dev = self._L, video.device
        tape = torch.empty(int((L.l2s_train_encoder_tape_floats_masked if lens is not None else L.l2s_train_encoder_tape_floats)(B, T, H)), dtype=torch.float32, device=dev)
        feat = torch.empty(B, T, 768, dtype=torch.float32, device=dev)
        vis = torch.empty(B, T, 1024, dtype=torch.float32, device=dev) if emb is not None else None
        args = (self._h, _ptr(video), B, T, H, W, _ptr(_f32(emb)) if emb is not None else None, _ptr(vis), _ptr(feat), _ptr(tape), _stream())
        if lens is not None:
            self.calls["l2s_train_encoder_masked_fwd"] += 1
            self._check(L.l2s_train_encoder_masked_fwd(*args, lens))
        else:
            self._check(L.l2s_train_encoder_fwd(*args))
        return vis, feat, tape

    def train_encoder_bwd(self, video, dfeat, tape, video_lengths=None) -> None:
        """Encoder backward: dfeat (B,T,>=768) (e.g. dvis, row stride 1024); parameter gradients land in the bound slots.
        `video_lengths`: the lengths of the masked forward that wrote `tape` (`l2s_train_encoder_masked_bwd`; dfeat rows t >= len_b are never read)."""
        B, _, T, H, W = video.shape
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None
        video = _f32(video)
        L = self._L
        assert dfeat.is_cuda and dfeat.dtype == torch.float32 and dfeat.stride(-1) == 1 and dfeat.stride(0) == T * dfeat.stride(1)
        ws = torch.empty(int((L.l2s_train_encoder_ws_bytes_masked if lens is not None else L.l2s_train_encoder_ws_bytes)(B, T, H)), dtype=torch.uint8, device=video.device)
        args = (self._h, _ptr(video), B, T, H, W, dfeat.data_ptr(), int(dfeat.stride(1)), _ptr(tape), _ptr(ws), ws.numel(), _stream())
        if lens is not None:
            self.calls["l2s_train_encoder_masked_bwd"] += 1
            self._check(L.l2s_train_encoder_masked_bwd(*args, lens))
        else:
            self._check(L.l2s_train_encoder_bwd(*args))

    def train_prologue_fwd(self, vis, emb, gumbel, video_lengths=None):
        """Prologue forward with a tape (stage 3).  Returns (state, content_dis, tape).
        `video_lengths` (B integers in [7, T]): `l2s_train_prologue_masked_fwd` - hand the same lengths to `train_steps_fwd` and `train_prologue_bwd`."""
        B, T, _ = vis.shape
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None      # checked on the host, before anything else
        vis, emb, gumbel = _f32(vis), _f32(emb), _f32(gumbel)
        L, dev = self._L, vis.device
        state = torch.zeros(int(L.l2s_state_floats(B, T)), dtype=torch.float32, device=dev)
        dis = torch.empty(B * min_T(T), 501, dtype=torch.float32, device=dev)
        masked = lens is not None
        tape = torch.zeros(int((L.l2s_train_prologue_tape_floats_masked if masked else L.l2s_train_prologue_tape_floats)(B, T)), dtype=torch.float32, device=dev)
        ws = torch.empty(int((L.l2s_train_prologue_ws_bytes_masked if masked else L.l2s_train_prologue_ws_bytes)(B, T)), dtype=torch.uint8, device=dev)
        args = (self._h, _ptr(vis), _ptr(emb), _ptr(gumbel), B, T, _ptr(state), _ptr(dis), _ptr(tape), _ptr(ws), ws.numel(), _stream())
        if masked:
            self.calls["l2s_train_prologue_masked_fwd"] += 1
            self._check(L.l2s_train_prologue_masked_fwd(*args, lens))
        else:
            self._check(L.l2s_train_prologue_fwd(*args))
        return state, dis, tape

    def train_prologue_bwd(self, vis, emb, state, tape, g, dcontent_dis=None, wbuf=None, video_lengths=None):
        """Prologue backward: g = the state gradients of train_steps (dk, dv, dckey, dcval, dh_init, de_c).  Returns dvis (B,T,1024);
        parameter gradients land in the bound slots.  `video_lengths`: the lengths of the masked forward that wrote `tape`
        (`l2s_train_prologue_masked_bwd`; dvis rows t >= len_b come back as exact zeros)."""
        B, T, _ = vis.shape
        lens = video_lengths_array(video_lengths, B, T) if video_lengths is not None else None
        vis, emb = _f32(vis), _f32(emb)
        L, dev = self._L, vis.device
        if wbuf is None:
            wbuf = self.train_pack_weights(dev)
        ws = torch.empty(int((L.l2s_train_prologue_ws_bytes_masked if lens is not None else L.l2s_train_prologue_ws_bytes)(B, T)), dtype=torch.uint8, device=dev)
        dvis = torch.empty(B, T, 1024, dtype=torch.float32, device=dev)
        gg = {k: _f32(v) for k, v in g.items()}
        dd = _f32(dcontent_dis) if dcontent_dis is not None else None
        args = (self._h, _ptr(vis), _ptr(emb), B, T, _ptr(state), _ptr(tape), _ptr(wbuf), _ptr(gg["dk"]), _ptr(gg["dv"]),
                _ptr(gg["dckey"]), _ptr(gg["dcval"]), _ptr(gg["dh_init"]), _ptr(gg["de_c"]), _ptr(dd), _ptr(dvis), _ptr(ws), ws.numel(), _stream())
        if lens is not None:
            self.calls["l2s_train_prologue_masked_bwd"] += 1
            self._check(L.l2s_train_prologue_masked_bwd(*args, lens))
        else:
            self._check(L.l2s_train_prologue_bwd(*args))
        return dvis

    def lstm_cell_chain_us(self, B: int, n_pairs: int = 300) -> float:
        """Average duration of the decoder LSTM-cell kernel, one HIP-event pair around 2*n_pairs chained launches."""
        ws = self.workspace(B, 29, 96, 96, 300, torch.device("cuda", torch.cuda.current_device()))
        out = ctypes.c_double()
        D = diag()                          # diagnostic library; the model handle may come from either library
        _replay_thread_chains(D)            # the chain launches the block forms of this thread's hint: the ones the caller's timed region launches
        check(D.l2s_op_lstm_cell_chain(self._h, B, n_pairs, _ptr(ws), ws.numel(), _stream(), ctypes.byref(out)), D)
        return float(out.value)

    def step_site(self, site: str, B: int = 1) -> list:
        """The batch the library builds at a call site of the batch-row launches (csrc/decode_step.h), as the groups of l2s_op_skinny_form:
        [nchunks x 4, ntiles, epi, W3 set, a_sum set] each.  Nothing is launched."""
        groups, count = (ctypes.c_int * 32)(), ctypes.c_int()
        D = diag()
        check(D.l2s_op_step_site(self._h, site.encode(), B, groups, ctypes.byref(count)), D)
        return [list(groups[8 * g:8 * g + 8]) for g in range(count.value)]

    def op_frontend(self, video: torch.Tensor) -> torch.Tensor:
        video = _f32(video)
        B, _, T, H, W = video.shape
        out = torch.empty(B * T, H // 4, W // 4, 24, dtype=torch.float32, device=video.device)
        D = diag()
        check(D.l2s_op_frontend(self._h, _ptr(video), B, T, H, W, _ptr(out), _stream()), D)
        return out


def postnet_drop_pack(masks) -> torch.Tensor:
    """Five post-net dropout multipliers in the reference's layout - (B,512,S) x4 and (B,80,S) - packed channel-last, back to back
    (the layout l2s_train_postnet_fwd/_bwd read)."""
    assert len(masks) == 5
    B, _, S = masks[0].shape
    out = torch.zeros(4 * B * S * 512 + B * S * 80, dtype=torch.float32, device=masks[0].device)
    for l, mk in enumerate(masks):
        C = 512 if l < 4 else 80
        assert tuple(mk.shape) == (B, C, S)
        out[l * B * S * 512: l * B * S * 512 + B * S * C] = mk.to(torch.float32).permute(0, 2, 1).reshape(-1)
    return out


def normalise_pad_frames(packed_u8: torch.Tensor, offsets, frames, H: int = 96, W: int = 96, T: Optional[int] = None) -> torch.Tensor:
    """Packed uint8 RGB clips on the device -> the model's (B,3,T,H,W) fp32 input (`l2s_normalise_pad_frames`): /255, ImageNet mean/std,
    zero padding to T (default: the longest clip).  `offsets` / `frames`: per-clip byte offsets into `packed_u8` and frame counts."""
    assert packed_u8.is_cuda and packed_u8.dtype == torch.uint8 and packed_u8.is_contiguous()
    B = len(frames)
    T = int(max(frames)) if T is None else int(T)
    video = torch.empty(B, 3, T, H, W, dtype=torch.float32, device=packed_u8.device)
    off = (_i64 * B)(*[int(o) for o in offsets])
    fr = (ctypes.c_int32 * B)(*[int(f) for f in frames])
    check(lib().l2s_normalise_pad_frames(packed_u8.data_ptr(), off, fr, B, T, H, W, _ptr(video), _stream()))
    return video


_RESIZE_JOB_DTYPE = np.dtype([("offset", "<i8")] + [(k, "<i4") for k in ("H", "W", "y0", "x0", "h", "w", "flip", "slot")])


def _resize_jobs(jobs):
    """rows `(offset, H, W, y0, x0, h, w, flip, slot)` -> a pointer to as many `ResizeJob` (numpy holds the memory: the pointer keeps it alive)"""
    rows = np.asarray(jobs, dtype=np.int64).reshape(-1, 9)
    assert rows.size == 0 or (int(np.abs(rows[:, 1:]).max()) < 2 ** 31), "a job field other than the offset is a 32-bit integer"
    arr = np.zeros(max(len(rows), 1), dtype=_RESIZE_JOB_DTYPE)
    for k, name in enumerate(_RESIZE_JOB_DTYPE.names):
        arr[name][:len(rows)] = rows[:, k]
    ptr = arr.ctypes.data_as(ctypes.POINTER(ResizeJob))
    ptr._rows = arr
    return ptr


def resize_check(jobs, packed_bytes: int, mode: int, B: int, T: int, size: int) -> None:
    """`l2s_resize_check`: the pure host check of a job table (no device needed); raises with the job and the limit it breaks."""
    check(lib().l2s_resize_check(_resize_jobs(jobs), len(jobs), int(packed_bytes), int(mode), int(B), int(T), int(size), int(size)))


def resize_normalise(packed_u8: torch.Tensor, jobs, mode: int, B: int, T: int = 2, size: Optional[int] = None) -> torch.Tensor:
    """`l2s_resize_normalise`: uint8 RGB images `(H_i,W_i,3)` of any size packed back to back on the device (each on a 4-byte boundary) ->
    `mode = RESIZE_MOUTH`: the model's `(B,3,T,size,size)` input, size 96 (default) or 88, slot `b * T + t`, `/255` and ImageNet mean / std;
    `mode = RESIZE_FACE`: the face tower's `(B,2,3,160,160)` input, slot `2 * b + k`, `(x - 127.5) / 128`.  `jobs`: rows
    `(offset, H, W, y0, x0, h, w, flip, slot)` - image, source rectangle, mirror bit, output slot; slots that no job names come back as zeros."""
    assert packed_u8.is_cuda and packed_u8.dtype == torch.uint8 and packed_u8.is_contiguous() and packed_u8.dim() == 1
    face = int(mode) == RESIZE_FACE
    size = (160 if face else 96) if size is None else int(size)
    T = 2 if face else int(T)
    resize_check(jobs, packed_u8.numel(), mode, B, T, size)       # before the output is allocated: its shape comes from the arguments under check
    out = torch.empty((B, 2, 3, size, size) if face else (B, 3, T, size, size), dtype=torch.float32, device=packed_u8.device)
    check(lib().l2s_resize_normalise(packed_u8.data_ptr(), packed_u8.numel(), _resize_jobs(jobs), len(jobs), int(mode), int(B), T, size, size, _ptr(out), _stream()))
    return out


_ALIGN_JOB_DTYPE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("m", "<f8", (6,))])


def _align_jobs(jobs):
    """rows `(offset, H, W, m0, .., m5)` (or `AlignJob`s) -> a pointer to as many `AlignJob` (numpy holds the memory: the pointer keeps it alive)"""
    rows = [(j.offset, j.H, j.W) + tuple(j.m) if isinstance(j, AlignJob) else tuple(j) for j in jobs]
    assert all(len(r) == 9 for r in rows), "an align job is (offset, H, W, m0, m1, m2, m3, m4, m5)"
    ints = np.asarray([r[:3] for r in rows], dtype=np.int64).reshape(-1, 3)
    assert ints.size == 0 or int(np.abs(ints[:, 1:]).max()) < 2 ** 31, "H and W are 32-bit integers"
    arr = np.zeros(max(len(rows), 1), dtype=_ALIGN_JOB_DTYPE)
    arr["offset"][:len(rows)], arr["H"][:len(rows)], arr["W"][:len(rows)] = ints[:, 0], ints[:, 1], ints[:, 2]
    arr["m"][:len(rows)] = np.asarray([r[3:] for r in rows], dtype=np.float64).reshape(-1, 6)
    ptr = arr.ctypes.data_as(ctypes.POINTER(AlignJob))
    ptr._rows = arr
    return ptr


def align_check(jobs, packed_bytes: int) -> None:
    """`l2s_align_check`: the pure host check of an align job table (no device needed); raises with the job and the limit it breaks."""
    check(lib().l2s_align_check(_align_jobs(jobs), len(jobs), int(packed_bytes)))


def align_faces(packed_u8: torch.Tensor, jobs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`l2s_align_faces`: uint8 RGB images `(H_i,W_i,3)` packed back to back on the device (each on a 4-byte boundary) -> a packed buffer of the same
    size and layout in which every image a job names is warped by the job's destination-to-source map (`warpAffine`, bilinear, border 0 - the rotation of
    `datasets.face_utils.align_and_crop_face` with `rotation_inverse_map`).  `jobs`: rows `(offset, H, W, m0, .., m5)` or `AlignJob`s.  Bytes outside every
    named image's span rounded up to 4 bytes keep what `out` held; without `out` they are uninitialised."""
    assert packed_u8.is_cuda and packed_u8.dtype == torch.uint8 and packed_u8.is_contiguous() and packed_u8.dim() == 1
    align_check(jobs, packed_u8.numel())
    if out is None:
        out = torch.empty_like(packed_u8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == packed_u8.shape and out.device == packed_u8.device
    check(lib().l2s_align_faces(packed_u8.data_ptr(), packed_u8.numel(), _align_jobs(jobs), len(jobs), out.data_ptr(), _stream()))
    return out


class JpegPlan:
    """What `l2s_jpeg_plan` found in n streams of one host buffer: `images` (a ctypes array of n `JpegImage`), `sets` (of `n_sets` `JpegTables`), and the
    buffer's size.  `sizes`: `(H, W)` per image; `blocks`: 8 x 8 blocks per image, whole MCUs of every component."""

    def __init__(self, images, sets, n_sets: int, stream_bytes: int):
        self.images, self.sets, self.n, self.n_sets, self.stream_bytes = images, sets, len(images), int(n_sets), int(stream_bytes)

    @property
    def sizes(self):
        return [(int(r.H), int(r.W)) for r in self.images]

    @property
    def blocks(self):
        out = []
        for r in self.images:
            m = 16 if r.layout == JPEG_420 else 8
            out.append(((r.H + m - 1) // m) * ((r.W + m - 1) // m) * {JPEG_GREY: 1, JPEG_444: 3, JPEG_420: 6}[int(r.layout)])
        return out

    def workspace_bytes(self) -> int:
        nb = lib().l2s_jpeg_workspace_bytes(self.images, self.n, self.n_sets)
        check(0 if nb >= 0 else 1)
        return int(nb)


def jpeg_plan(streams, offsets, sizes) -> JpegPlan:
    """`l2s_jpeg_plan` (pure host): `streams`, a uint8 host buffer (numpy array or CPU tensor) that holds n JPEG streams, stream i the `sizes[i]` bytes at
    `offsets[i]` -> their records and deduplicated table sets.  Raises with the image and the reason for a stream outside the supported subset."""
    buf = streams.numpy() if isinstance(streams, torch.Tensor) else np.asarray(streams)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags.c_contiguous, "the stream buffer is a contiguous 1-D uint8 array"
    n = len(offsets)
    assert len(sizes) == n and all(0 <= int(o) and 0 <= int(z) and int(o) + int(z) <= buf.size for o, z in zip(offsets, sizes)), "streams inside the buffer"
    images, sets, n_sets = (JpegImage * n)(), np.empty(max(n, 1) * ctypes.sizeof(JpegTables), dtype=np.uint8), _i(0)
    check(lib().l2s_jpeg_plan(buf.ctypes.data, _int64s(offsets), _int64s(sizes), n, images, sets.ctypes.data_as(ctypes.POINTER(JpegTables)), n, ctypes.byref(n_sets)))
    kept = (JpegTables * max(n_sets.value, 1)).from_buffer_copy(sets[:max(n_sets.value, 1) * ctypes.sizeof(JpegTables)].tobytes())
    return JpegPlan(images, kept, n_sets.value, buf.size)


def jpeg_decode(streams_u8: torch.Tensor, plan: JpegPlan, out_offsets, out: Optional[torch.Tensor] = None, packed_bytes: Optional[int] = None,
                status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`l2s_jpeg_decode`: the planned streams, uploaded as they are, -> image i as interleaved uint8 `(H_i, W_i, 3)` at byte `out_offsets[i]` (a multiple
    of 4) of the packed buffer `out` (default: a new one of `packed_bytes`, default the last image's end rounded up to 4; bytes outside the images' spans
    then are uninitialised) - the layout `normalise_pad_frames`, `resize_normalise` and `align_faces` read.  `status`: int32 `(n)` on the device, 0 per
    stream that decoded cleanly."""
    assert streams_u8.is_cuda and streams_u8.dtype == torch.uint8 and streams_u8.is_contiguous() and streams_u8.dim() == 1 and streams_u8.numel() == plan.stream_bytes
    assert len(out_offsets) == plan.n
    if out is None:
        if packed_bytes is None:
            packed_bytes = max([(int(o) + H * W * 3 + 3) // 4 * 4 for o, (H, W) in zip(out_offsets, plan.sizes)] or [0])
        out = torch.empty(int(packed_bytes), dtype=torch.uint8, device=streams_u8.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1 and out.device == streams_u8.device
    assert status is None or (status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == plan.n)
    ws_bytes = plan.workspace_bytes()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=streams_u8.device)
    check(lib().l2s_jpeg_decode(streams_u8.data_ptr(), streams_u8.numel(), plan.images, plan.n, plan.sets, plan.n_sets, _int64s(out_offsets), out.data_ptr(),
                                out.numel(), _ptr(status), ws.data_ptr(), ws_bytes, _stream()))
    return out


def op_jpeg_entropy_host(streams, plan: JpegPlan, sentinel_words: int = 0):
    """`l2s_op_jpeg_entropy_host` (diagnostic library, no device): the entropy decoder's host instantiation over the plan's records -> `(coefs, status)`, numpy:
    int16 `(sum of blocks, 64)` image after image, int32 `(n)`.  With `sentinel_words` also the int16 words placed after the coefficient buffer, as they are after
    the call (written as 0x5A5A before it)."""
    buf = streams.numpy() if isinstance(streams, torch.Tensor) else np.asarray(streams)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags.c_contiguous and buf.size == plan.stream_bytes and buf.ctypes.data % 4 == 0
    count = sum(plan.blocks) * 64
    raw = np.zeros(count * 2 + sentinel_words * 2 + 64, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 64                     # the coefficient buffer starts on a 64-byte boundary
    coefs = raw[skip:skip + (count + sentinel_words) * 2].view(np.int16)
    coefs[count:] = 0x5A5A
    status = np.zeros(max(plan.n, 1), dtype=np.int32)
    _dcheck(diag().l2s_op_jpeg_entropy_host(buf.ctypes.data, buf.size, plan.images, plan.n, plan.sets, plan.n_sets, coefs.ctypes.data, count, status.ctypes.data))
    out = (coefs[:count].reshape(-1, 64).copy(), status[:plan.n])
    return out + (coefs[count:].copy(),) if sentinel_words else out


MEL_PAD = -11.5129      # ln(1e-5) as the collates write it (datasets.MEL_PAD)
_mel_tls = threading.local()


def mel_frames(n: int) -> int:
    """`l2s_mel_frames`: the frames `torch.stft(center=True)` makes of n samples at hop 256 (n // 256 + 1); raises below 513 samples."""
    m = int(lib().l2s_mel_frames(int(n)))
    if m == 0:
        check(1)
    return m


def mel_targets(audio_packed: torch.Tensor, offsets, n_samples, fb: torch.Tensor, fb_nnz: int, *, log: bool = True, mel_pad: float = MEL_PAD,
                M: Optional[int] = None, A: Optional[int] = None, want_audio: bool = True):
    """`l2s_mel_targets`: B waveforms packed back to back on the device (clip b = `n_samples[b]` floats at float offset `offsets[b]` of
    `audio_packed`) -> (mels (B, n_mels, M) log-mel (power-mel when not `log`) padded with `mel_pad`, gate (B, M), audio (B, A) zero-padded or
    None, mel_lengths (B,) int64 on the device).  M / A default to the longest clip's frames / samples; fb (513, n_mels) with `fb_nnz` non-zeros."""
    assert audio_packed.is_cuda and audio_packed.dtype == torch.float32 and audio_packed.is_contiguous() and audio_packed.dim() == 1
    fb = _f32(fb)
    B, n_mels = len(n_samples), int(fb.shape[1])
    assert len(offsets) == B and fb.shape[0] == 513, (len(offsets), B, fb.shape)
    ns = [int(n) for n in n_samples]
    off = [int(o) for o in offsets]
    assert all(0 <= o and o + n <= audio_packed.numel() for o, n in zip(off, ns)), "a clip lies outside the packed buffer"
    L = lib()
    dev = audio_packed.device
    M = (max(ns) // 256 + 1 if ns else 0) if M is None else int(M)
    A = (max(ns) if ns else 0) if A is None else int(A)
    need = int(L.l2s_mel_targets_workspace_bytes(B, n_mels))
    cache = _mel_tls.__dict__.setdefault("ws", {})             # one workspace per device (and host thread): the band tables are rebuilt by every call
    ws = cache.get(dev)
    if ws is None or ws.numel() < need:
        ws = cache[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    mels = torch.empty(B, n_mels, M, dtype=torch.float32, device=dev)
    gate = torch.empty(B, M, dtype=torch.float32, device=dev)
    audio = torch.empty(B, A, dtype=torch.float32, device=dev) if want_audio else None
    lengths = torch.empty(B, dtype=torch.int64, device=dev)
    check(L.l2s_mel_targets(audio_packed.data_ptr(), (_i64 * B)(*off), (_i64 * B)(*ns), B, fb.data_ptr(), int(fb_nnz), n_mels, 1024, 256, int(bool(log)),
                            float(mel_pad), M, A, mels.data_ptr(), gate.data_ptr(), _ptr(audio), lengths.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return mels, gate, audio, lengths


def build_visual(feat: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    feat, emb = _f32(feat), _f32(emb)
    B, T, _ = feat.shape
    vis = torch.empty(B, T, 1024, dtype=torch.float32, device=feat.device)
    check(lib().l2s_build_visual(_ptr(feat), _ptr(emb), B, T, _ptr(vis), _stream()))
    return vis


def output_lengths(stop: torch.Tensor) -> torch.Tensor:
    stop = _f32(stop)
    B, S = stop.shape
    out = torch.empty(B, dtype=torch.int64, device=stop.device)
    check(lib().l2s_output_lengths(_ptr(stop), B, S, _ptr(out), _stream()))
    return out


def state_field(state: torch.Tensor, B: int, T: int, field: int, shape) -> torch.Tensor:
    off = int(lib().l2s_state_offset(B, T, field))
    n = int(np.prod(shape))
    return state[off:off + n].view(*shape)


def op_gemm(A, Wt, scale=None, shift=None, actw=None, act: int = 0, x3: bool = False, bf16: bool = False, x3_narrow: bool = False,
            x3_dma: bool = False) -> torch.Tensor:
    A, Wt = _f32(A), _f32(Wt)
    M, K = A.shape
    N = Wt.shape[0]
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    _dcheck(diag().l2s_op_gemm_ex(_ptr(A), _ptr(Wt), _ptr(scale), _ptr(shift), _ptr(actw), _ptr(C), M, N, K, act, (1 if x3 else 0) | (2 if bf16 else 0) | (4 if x3_narrow else 0) | (8 if x3_dma else 0), _stream()))
    return C


def op_conv1d(X, Wp, scale=None, shift=None, actw=None, taps=1, stride=1, pad=0, act: int = 0, x3: bool = False, bf16: bool = False, x3_narrow: bool = False,
              x3_dma: bool = False) -> torch.Tensor:
    """X (B,Tin,Cin) channel-last, Wp (Cout, taps*Cin) tap-major."""
    X, Wp = _f32(X), _f32(Wp)
    B, Tin, Cin = X.shape
    Cout = Wp.shape[0]
    Tout = (Tin + 2 * pad - taps) // stride + 1
    out = torch.empty(B, Tout, Cout, dtype=torch.float32, device=X.device)
    _dcheck(diag().l2s_op_conv1d_ex(_ptr(X), _ptr(Wp), _ptr(scale), _ptr(shift), _ptr(actw), _ptr(out), B, Tin, Cin, Cout,
                                 taps, stride, pad, act, (1 if x3 else 0) | (2 if bf16 else 0) | (4 if x3_narrow else 0) | (8 if x3_dma else 0), _stream()))
    return out


SK_PLAIN, SK_FRAG, SK_LSTM, SK_MEL = range(4)      # SkinnyEpi (l2s_common.h)
SKINNY_SENTINEL = -7777.0                          # what op_skinny fills every output buffer with before the launch


def frag16_index(row, k, K):
    """`frag16_index` of l2s_common.h, on ints or integer tensors: where element [row][k] of a row-major [R][K] matrix sits in its frag16 buffer"""
    return (((row >> 4) * (K >> 4) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (row & 15)) * 4 + (k & 3)


def _frag16_map(R: int, K: int, device) -> torch.Tensor:
    assert K % 16 == 0, "frag16: K is a multiple of 16"
    return frag16_index(torch.arange(R, device=device).view(-1, 1), torch.arange(K, device=device).view(1, -1), K)


def frag16_pack(X: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
    """Row-major X [R][K] -> the flat frag16 buffer of pad16(max(R, rows)) rows; the padded rows are zero"""
    R, K = X.shape
    Rp = (max(R, rows or 0) + 15) // 16 * 16
    out = X.new_zeros(Rp * K)
    out[_frag16_map(R, K, X.device).reshape(-1)] = X.reshape(-1)
    return out


def frag16_unpack(F: torch.Tensor, R: int, K: int) -> torch.Tensor:
    """The row-major [R][K] view of a flat frag16 buffer (R may include the padded rows)"""
    return F[_frag16_map(R, K, F.device)]


def lstm_perm_rows(H: int, device=None) -> torch.Tensor:
    """`lstm_perm_row` of l2s_pack.hip for every packed row: entry np = 4 * unit + gate holds the PyTorch row gate * H + unit"""
    n = torch.arange(4 * H, device=device)
    return (n & 3) * H + (n >> 2)


def op_skinny_prepare(groups, B: int):
    """The device-side inputs of `op_skinny` for these groups, packed once (a caller that launches the same batch in several kernel forms passes the
    result as `prepared`).  Activations and the previous cell go to frag16 with rows padded to 16 (zero), weights to frag16 with their rows - the output
    columns - zero-padded to 16 * ntiles, SK_LSTM weights and bias permuted from PyTorch's gate * H + unit to 4 * unit + gate."""
    Bp = (B + 15) // 16 * 16
    prepared = []
    for d in groups:
        W = _f32(d["W"])
        N, K = W.shape
        Np = 16 * d["ntiles"]
        assert N <= Np and len(d["a"]) <= 4 and sum(a.shape[1] for a in d["a"]) == K and all(a.shape[0] == B for a in d["a"])
        bias = None if d.get("bias") is None else _f32(d["bias"])
        if d["epi"] == SK_LSTM:
            assert N == 4 * d["H"] == Np
            perm = lstm_perm_rows(d["H"], W.device)
            W, bias = W[perm], (None if bias is None else bias[perm])
        Wp = W.new_zeros(Np, K)
        Wp[:N] = W
        p = {"a": [frag16_pack(_f32(a), Bp) for a in d["a"]], "W": frag16_pack(Wp), "bias": None}
        if bias is not None:
            p["bias"] = W.new_zeros(Np)
            p["bias"][:N] = bias
        for k in ("actw", "add", "addrow", "pre", "stop_const"):
            p[k] = None if d.get(k) is None else _f32(d[k])
        p["a_sum"] = None if d.get("a_sum") is None else frag16_pack(_f32(d["a_sum"]), Bp)
        p["c_in"] = None if d.get("c_prev") is None else frag16_pack(_f32(d["c_prev"]), Bp)
        p["planes"] = torch.empty(d["ntiles"] * K * 16 * 6, dtype=torch.uint8, device=W.device) if d.get("planes") else None
        prepared.append(p)
    return prepared


def op_skinny(model, groups, B: int, es=None, refused: Optional[list] = None, prepared=None):
    """One batch-row launch through `l2s_op_skinny` (diagnostic library) from plain row-major tensors.  `model`: the handle of a diag model whose options
    choose the kernel form (the chains come from `set_thread_chains`).  `groups`: one dict per GEMM group -
      "epi" (SK_*), "ntiles", "a": the K segments as [B][K_j] tensors, "W": [N][K] (SK_LSTM: [4H][K] in PyTorch's gate order i, f, g, o), optional "bias" [N],
      "a_sum" [B][K_1], "planes" (True: the launch gets the bf16 planes of W), "act" (0 none, 1 ReLU, 2 SiLU, 3 sin(v) * actw), "actw" [N], "add" [B][N],
      "addrow" [N], "ldo" (row pitch of the output, default N for SK_PLAIN and 16 * ntiles for SK_FRAG);
      SK_LSTM: "H", "c_prev" [B][H], optional "pre" [B][4H], "h_out_K" / "h_out_off" (default H / 0), "h_seq" / "h_plain" (True: also the plain copies);
      SK_MEL: "stop_const" [B], "yfrag" (True: also the frag16 copy of the frame).
    `es` = (end, step): the early-stop twin of the kernel with *es_end = end and es_step = step.
    A single SK_LSTM group with "hoist_p" [B][4H][pitch] (rows in PyTorch's gate order, permuted here like W) and "hoist_alpha" [B][8] goes through
    `l2s_op_skinny_hoist`: the K = 768 layout of the decode step ("a": [B][0], [B][256], [B][512] with "a_sum") with the hoisted content term.
    Every output buffer is filled with SKINNY_SENTINEL first and returned WHOLE, unpacked to row-major with its padded rows and columns, so that a caller
    sees unwritten elements and stray writes: per group a dict of "out" [pad16(B)][ldo]; "c_out" [pad16(B)][H], "h_out" [pad16(B)][h_out_K], "h_seq"
    [pad16(B)][H + 8], "h_plain" [pad16(B)][H + 4]; "mel" [pad16(B)][88], "stop" [pad16(B)][2], "yfrag" [pad16(B)][80].
    A refused launch raises RuntimeError with the library's text - or, with `refused` a list, appends the text to it and returns the untouched buffers."""
    D = diag()
    dev = torch.device("cuda")
    Bp = (B + 15) // 16 * 16
    prepared = prepared or op_skinny_prepare(groups, B)
    arr = (SkinnyGroup * len(groups))()
    bufs = []

    def fill(*shape):
        return torch.full(shape, SKINNY_SENTINEL, dtype=torch.float32, device=dev)

    for g, d, p in zip(arr, groups, prepared):
        N, H = d["W"].shape[0], d.get("H", 0)
        for j, a in enumerate(p["a"]):
            g.seg_a[j], g.nchunks[j] = a.data_ptr(), d["a"][j].shape[1] // 16
        for k in ("a_sum", "W", "planes", "bias", "actw", "add", "addrow", "pre", "c_in", "stop_const"):
            setattr(g, k, _ptr(p[k]))
        g.ntiles, g.epi, g.N, g.act, g.H, g.ld_add, g.ld_pre = d["ntiles"], d["epi"], N, d.get("act", 0), H, N, 4 * H
        b = {}
        if d["epi"] == SK_PLAIN:
            g.ldo = d.get("ldo", N)
            b["out"] = fill(Bp, g.ldo)
            g.out = b["out"].data_ptr()
        elif d["epi"] == SK_FRAG:
            g.ldo = d.get("ldo", 16 * d["ntiles"])
            b["out"] = fill(Bp * g.ldo)
            g.out = b["out"].data_ptr()
        elif d["epi"] == SK_LSTM:
            g.h_out_K, g.h_out_off = d.get("h_out_K", H), d.get("h_out_off", 0)
            b["c_out"], b["h_out"] = fill(Bp * H), fill(Bp * g.h_out_K)
            g.c_out, g.h_out = b["c_out"].data_ptr(), b["h_out"].data_ptr()
            if d.get("h_seq"):
                b["h_seq"], g.ld_hseq = fill(Bp, H + 8), H + 8
                g.h_seq = b["h_seq"].data_ptr()
            if d.get("h_plain"):
                b["h_plain"], g.ld_hplain = fill(Bp, H + 4), H + 4
                g.h_plain = b["h_plain"].data_ptr()
        else:
            b["mel"], b["stop"], g.ld_mel_b, g.ld_stop_b = fill(Bp, 88), fill(Bp, 2), 88, 2
            g.mel, g.stop = b["mel"].data_ptr(), b["stop"].data_ptr()
            if d.get("yfrag"):
                b["yfrag"] = fill(Bp * 80)
                g.yfrag = b["yfrag"].data_ptr()
        bufs.append(b)
    es_end = None if es is None else torch.tensor([es[0]], dtype=torch.int32, device=dev)
    if groups[0].get("hoist_p") is not None:
        assert len(groups) == 1 and es is None and groups[0]["epi"] == SK_LSTM
        hp = _f32(groups[0]["hoist_p"])[:, lstm_perm_rows(groups[0]["H"], dev)].contiguous()
        ha = _f32(groups[0]["hoist_alpha"])
        assert ha.shape == (B, 8) and hp.shape[:2] == (B, 4 * groups[0]["H"]) and hp.shape[2] in (4, 8)
        rc = D.l2s_op_skinny_hoist(model, arr, _ptr(hp), _ptr(ha), hp.shape[2], B, _stream())
    else:
        rc = D.l2s_op_skinny(model, len(groups), arr, B, _ptr(es_end), 0 if es is None else es[1], _stream())
    if rc != 0:
        text = D.l2s_last_error().decode("utf-8", "replace")
        if refused is None:
            raise RuntimeError("libl2s_diag: " + text)
        refused.append(text)
    frag_K = {"c_out": lambda g: g.H, "h_out": lambda g: g.h_out_K, "yfrag": lambda g: 80}
    outs = []
    for g, d, b in zip(arr, groups, bufs):
        o = dict(b)
        if d["epi"] == SK_FRAG:
            o["out"] = frag16_unpack(b["out"], Bp, g.ldo)
        for k, K_of in frag_K.items():
            if k in b:
                o[k] = frag16_unpack(b[k], Bp, K_of(g))
        outs.append(o)
    return outs


def op_face_conv2d(x, w, scale, shift, stride=1, pad=(0, 0), res=None, relu=True, nchw=False) -> torch.Tensor:
    """One Conv2d of the face tower's kernel: x NHWC (B,H,W,Cin), or with nchw=True a (B,Cin,H,W) view whose images are contiguous (any
    batch stride); w (Cout,Cin,kh,kw) as torch stores it (re-laid here as [Cout][kh][kw][Cin]); -> NHWC (B,Ho,Wo,Cout)."""
    if not x.is_cuda:
        raise RuntimeError("device tensors only")
    Cout, Cin, kh, kw = w.shape
    if nchw:
        B, _, H, W = x.shape
        assert x.stride()[1:] == (H * W, W, 1)
        bstride = x.stride(0)
    else:
        x = _f32(x)
        B, H, W, _ = x.shape
        bstride = 0
    wp = _f32(w.permute(0, 2, 3, 1))
    ph, pw = pad
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    res = _f32(res) if res is not None else None
    _dcheck(diag().l2s_op_face_conv2d(x.data_ptr(), bstride, B, H, W, Cin, _ptr(wp), _ptr(_f32(scale)), _ptr(_f32(shift)), _ptr(res), 1 if relu else 0,
                                      _ptr(y), Cout, kh, kw, stride, ph, pw, _stream()))
    return y


def set_option(name: str, value: int) -> None:
    """Process DEFAULT of a run-time option: copied into models created afterwards (`NativeModel.set_option` changes one model)."""
    if name in DIAG_OPTIONS:
        _dcheck(diag().l2s_set_option(name.encode(), int(value)))      # a diagnostic switch: a default of diagnostic-library models only
        return
    check(lib().l2s_set_option(name.encode(), int(value)))
    _process_defaults[name] = int(value)
    if _diag is not None and _diag is not _lib:
        check(_diag.l2s_set_option(name.encode(), int(value)), _diag)


def set_thread_chains(n: int) -> None:
    """Tell the library how many launch chains the caller keeps in flight, for the calling host thread (include/l2s.h l2s_set_thread_chains): with
    two or more the step kernels take half-CU block forms so that chains overlap on the CUs.  A scheduling hint - results are the same bits."""
    _chains_tls.n = int(n)
    check(lib().l2s_set_thread_chains(int(n)))
    if _diag is not None and _diag is not _lib:      # the hint is thread-local state of each library
        check(_diag.l2s_set_thread_chains(int(n)), _diag)


_chains_tls = threading.local()      # the calling thread's hint, kept here so that it reaches a diagnostic library that loads after it was given


def _replay_thread_chains(D: ctypes.CDLL) -> None:
    """Hand the calling thread's chains hint to the diagnostic library `D`: the hint is thread-local state of each library, and `D` may have been
    loaded - by this thread or by another - after `set_thread_chains` ran here, so what `D` launches for this thread would be the forms of one chain."""
    n = getattr(_chains_tls, "n", None)
    if n is not None and D is not _lib:
        check(D.l2s_set_thread_chains(n), D)


def persist_available() -> bool:
    """True where the persistent forms (option "persist_decode") can be taken on the current device: every workgroup resident at once (include/l2s.h)."""
    return bool(lib().l2s_persist_available())


def persist_timeouts() -> int:
    """Persistent launches of this process that gave up (their outputs are NaN).  Pinned host memory: meaningful after a synchronize."""
    return int(lib().l2s_persist_timeouts())


_timeouts_reported = 0


def check_persist_timeouts() -> None:
    """For a host that has just synchronized with the stream: raise if a persistent launch timed out since the last check (instead of handing its
    NaNs on).  Later persistent-eligible calls take the launch path (l2s_persist_available() is 0 from then on), so the error is raised once."""
    global _timeouts_reported
    n = persist_timeouts()
    if n > _timeouts_reported:
        new, _timeouts_reported = n - _timeouts_reported, n
        raise RuntimeError(f"{new} persistent decode launch(es) gave up after 2 s without progress (shared or CU-masked device): their outputs are NaN; "
                           f"later calls take the launch-per-phase path (or set option persist_decode=0)")


def op_conv1d_bwd(dZ, X, Wp, taps=1, stride=1, pad=0, want_dx=True):
    """Gradients of op_conv1d wrt its input (stride 1) and its tap-major weight."""
    dZ, X, Wp = _f32(dZ), _f32(X), _f32(Wp)
    B, Tin, Cin = X.shape
    Cout = Wp.shape[0]
    dX = torch.empty_like(X) if want_dx else None
    dW = torch.empty_like(Wp)
    _dcheck(diag().l2s_op_conv1d_bwd(_ptr(dZ), _ptr(X), _ptr(Wp), _ptr(dX), _ptr(dW), B, Tin, Cin, Cout, taps, stride, pad, _stream()))
    return dX, dW


def gemm_bwd_desc(**fields) -> GemmBwdDesc:
    """A `GemmBwdDesc` from keyword integers (GEMM_BWD_INTS, c_seq_stride, alpha); alpha defaults to 1, every integer to 0"""
    d = GemmBwdDesc()
    d.alpha = 1.0
    for k, v in fields.items():
        assert k in GEMM_BWD_INTS or k in ("c_seq_stride", "alpha"), k
        setattr(d, k, v)
    return d


def gemm_bwd_record_dict(r: GemmBwdRecord) -> dict:
    """One launch record as plain Python: "d" (and, for a pair, "d2"): {field: value} of the descriptors, "align" / "align2": (A, B, C) addresses modulo
    16 bytes, "entry" (0 launch_gemm_bwd, 1 launch_gemm_bwd_splitk, 2 launch_gemm_bwd_dw_dx), "splits_asked", "splits", "vec", "bf16", "pair" and "name" (the launch's profile name)"""
    def desc(d):
        out = {k: int(getattr(d, k)) for k in GEMM_BWD_INTS + ("c_seq_stride",)}
        out["alpha"] = float(d.alpha)
        return out
    out = {k: int(getattr(r, k)) for k in ("entry", "splits_asked", "splits", "vec", "bf16", "pair")}
    out.update(d=desc(r.d[0]), align=tuple(int(a) for a in r.align[0]), name=r.name.decode("utf-8", "replace"))
    if out["pair"]:
        out.update(d2=desc(r.d[1]), align2=tuple(int(a) for a in r.align[1]))
    return out


def _addr(t) -> Optional[int]:
    return t if t is None or isinstance(t, int) else _ptr(t)


def op_gemm_bwd(d: GemmBwdDesc, A, B, C, splits: int = 0, partials=None, bf16: bool = False, pair=None, refused: Optional[list] = None) -> dict:
    """One backward GEMM through `l2s_op_gemm_bwd` (diagnostic library): descriptor `d` on the device operands A, B, C - tensors, or integer device
    addresses where an operand starts inside a larger buffer.  splits = 0: launch_gemm_bwd; splits >= 1: launch_gemm_bwd_splitk with `partials`
    (splits * M * N floats); pair = (d2, A2, B2, C2): launch_gemm_bwd_dw_dx with d the DW half and the pair the DX half.  Returns the record of what ran
    (`gemm_bwd_record_dict`).  A refused launch raises RuntimeError with the library's text - or, with `refused` a list, appends the text to it."""
    D = diag()
    ran = GemmBwdRecord()
    d2, A2, B2, C2 = pair if pair is not None else (None, None, None, None)
    rc = D.l2s_op_gemm_bwd(ctypes.byref(d), _addr(A), _addr(B), _addr(C), ctypes.byref(d2) if d2 is not None else None, _addr(A2), _addr(B2), _addr(C2),
                           int(splits), _addr(partials), 1 if bf16 else 0, ctypes.byref(ran), _stream())
    if rc != 0:
        text = D.l2s_last_error().decode("utf-8", "replace")
        if refused is None:
            raise RuntimeError("libl2s_diag: " + text)
        refused.append(text)
    return gemm_bwd_record_dict(ran)


def gemm_bwd_recorder_arm() -> None:
    """Forget the recorded backward-GEMM launches and record from now on: every call of launch_gemm_bwd / _splitk / _dw_dx made through the diagnostic
    library, by any entry point (a model bound to `diag()` included)"""
    _dcheck(diag().l2s_op_gemm_bwd_recorder(1, None, 0, None))


def gemm_bwd_recorder_read(disarm: bool = True) -> list:
    """The records since `gemm_bwd_recorder_arm`, in launch order, as `gemm_bwd_record_dict` dicts; disarms the recorder first unless told not to"""
    D = diag()
    n = _i(0)
    _dcheck(D.l2s_op_gemm_bwd_recorder(0 if disarm else 2, None, 0, ctypes.byref(n)))
    arr = (GemmBwdRecord * max(1, n.value))()
    _dcheck(D.l2s_op_gemm_bwd_recorder(2, arr, n.value, ctypes.byref(n)))
    return [gemm_bwd_record_dict(arr[i]) for i in range(min(n.value, len(arr)))]


TABLE_CHUNK = 960                         # L2S_TABLE_CHUNK (include/l2s_diag.h): words of a per-clip table that one launch carries in its kernel arguments


def op_upload_table(host_words: ctypes.Array, n: int, dst: torch.Tensor, offset: int = 0) -> None:
    """`l2s_op_upload_table`: dst (int32, device).flatten()[offset : offset + n] = host_words[:n] (a ctypes int32 array) on the current stream"""
    assert dst.dtype == torch.int32 and dst.is_contiguous() and 0 <= offset and offset + n <= dst.numel() and n <= len(host_words)
    _dcheck(diag().l2s_op_upload_table(ctypes.addressof(host_words), int(n), dst.data_ptr() + 4 * offset, _stream()))


def op_table_layout(a, b, fill: bool = True, dst: Optional[torch.Tensor] = None):
    """`l2s_op_table_layout`: the builder's (offset of the int32 segment, offset of the int64 segment, total words) for len(a) int32 words followed by
    len(b) int64 values; fill=False: sizes only; with dst (int32, device, 8-byte aligned) the table is uploaded to its front"""
    off_a, off_b, words = _i64(), _i64(), _i64()
    ha, hb = (ctypes.c_int32 * max(1, len(a)))(*[int(v) for v in a]), (_i64 * max(1, len(b)))(*[int(v) for v in b])
    for d in (None, dst) if dst is not None else (None,):      # sizes first: the upload only once the table is known to fit dst
        assert d is None or (fill and d.dtype == torch.int32 and d.data_ptr() % 8 == 0 and words.value <= d.numel())
        _dcheck(diag().l2s_op_table_layout(ctypes.addressof(ha) if fill else None, len(a), ctypes.addressof(hb) if fill else None, len(b), 1 if fill else 0,
                                           _ptr(d), ctypes.byref(off_a), ctypes.byref(off_b), ctypes.byref(words), _stream() if d is not None else None))
    return off_a.value, off_b.value, words.value


def op_post_wino_matrices():
    """`l2s_op_post_wino_matrices` (diagnostic library, no device): the matrices of the post-net's Winograd F(4,5) route as float64 numpy arrays
    `(AT (4, 8), G (8, 5), BT (8, 8))` - AT ((G g) * (BT d)) is the 4-output correlation of 5 taps g with an 8-frame tile d."""
    AT, G, BT = np.zeros((4, 8)), np.zeros((8, 5)), np.zeros((8, 8))
    _dcheck(diag().l2s_op_post_wino_matrices(AT.ctypes.data, G.ctypes.data, BT.ctypes.data))
    return AT, G, BT


# ---------------------------------------------------------------------------------------------- profiling
def profile_enable(on: bool) -> None:
    check(lib().l2s_profile_enable(1 if on else 0))


def profile_reset() -> None:
    check(lib().l2s_profile_reset())


def profile_read():
    """[(kernel name, launches, total ms)] measured with HIP events on the launch stream."""
    L = lib()
    out = []
    for i in range(L.l2s_profile_count()):
        name, n, ms = ctypes.c_char_p(), _i64(), ctypes.c_double()
        check(L.l2s_profile_get(i, ctypes.byref(name), ctypes.byref(n), ctypes.byref(ms)))
        out.append((name.value.decode(), int(n.value), float(ms.value)))
    return out


# ---------------------------------------------------------------------------------------------------------------- vocoder + metric (evaluate.py)
def inverse_mel(mel: torch.Tensor, fb: torch.Tensor, fb_nnz: int, init: torch.Tensor, iters: int, rows_per_call: Optional[int] = None,
                log_input: bool = False, want_loss: bool = False):
    """`l2s_inverse_mel`: mel (N, n_mels, L), fb (n_freqs, n_mels), init (N*L, n_freqs) -> spec (N, n_freqs, L)
    [, loss (calls, iters), iterations run per call (calls,) int32]."""
    mel, fb, init = _f32(mel), _f32(fb), _f32(init)
    N, M, Lf = mel.shape
    F = fb.shape[0]
    assert fb.shape[1] == M and tuple(init.shape) == (N * Lf, F), (fb.shape, init.shape)
    R = rows_per_call or N
    L = lib()
    ws = torch.empty(int(L.l2s_inverse_mel_workspace_bytes(N, Lf, M, F, R, iters)), dtype=torch.uint8, device=mel.device)
    spec = torch.empty(N, F, Lf, dtype=torch.float32, device=mel.device)
    loss = torch.empty(N // R, max(iters, 1), dtype=torch.float32, device=mel.device) if want_loss else None
    ran = torch.empty(N // R, dtype=torch.int32, device=mel.device) if want_loss else None
    check(L.l2s_inverse_mel(mel.data_ptr(), int(log_input), fb.data_ptr(), int(fb_nnz), init.data_ptr(), N, Lf, M, F, R, iters, spec.data_ptr(),
                            _ptr(loss), _ptr(ran), ws.data_ptr(), ws.numel(), _stream()))
    return (spec, loss, ran) if want_loss else spec


GRIFFIN_LIM_SHORT_FRAMES = 121     # l2s_griffin_lim: up to here one launch with the waveform in LDS; above, one launch per iteration over tiles of
GRIFFIN_LIM_TILE_FRAMES = 24       # this many frames (GLT_F in csrc/vocoder.hip)
ESTOI_SHORT_SAMPLES = 16512        # l2s_estoi at 10 kHz: up to here both signals in LDS; above, up to
ESTOI_MAX_SAMPLES = 48256          # this many, in the workspace (ESL_MAXLEN in csrc/vocoder.hip)


def griffin_lim(power_spec: torch.Tensor, init_angles: torch.Tensor, iters: int, n_fft: int = 1024, hop: int = 256, momentum: float = 0.99) -> torch.Tensor:
    """`l2s_griffin_lim`: power_spec (N, n_fft/2+1, L), init_angles complex (N, n_fft/2+1, L) or float (..., 2) -> wave (N, hop*(L-1))."""
    power_spec = _f32(power_spec)
    ang = torch.view_as_real(init_angles) if init_angles.is_complex() else init_angles
    ang = _f32(ang)
    N, F, Lf = power_spec.shape
    assert tuple(ang.shape) == (N, F, Lf, 2), ang.shape
    L = lib()
    ws = torch.empty(int(L.l2s_griffin_lim_workspace_bytes(N, Lf)), dtype=torch.uint8, device=power_spec.device)
    wave = torch.empty(N, hop * (Lf - 1), dtype=torch.float32, device=power_spec.device)
    check(L.l2s_griffin_lim(power_spec.data_ptr(), ang.data_ptr(), N, Lf, n_fft, hop, iters, momentum, wave.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return wave


def estoi(clean: torch.Tensor, pred: torch.Tensor, fir: Optional[torch.Tensor], up: int, down: int, n_pre_remove: int, n_resampled: int,
          band_lo_hi) -> torch.Tensor:
    """`l2s_estoi`: clean / pred (N, n_samples) on the device -> ESTOI per clip (N,).  `fir`: the padded polyphase filter (device) or None."""
    clean, pred = _f32(clean), _f32(pred)
    N, n = clean.shape
    assert pred.shape == clean.shape
    L = lib()
    bands = (ctypes.c_int * 30)(*[int(v) for v in band_lo_hi])
    ws_bytes = L.l2s_estoi_workspace_bytes_long(N, n_resampled) if hasattr(L, "l2s_estoi_workspace_bytes_long") else L.l2s_estoi_workspace_bytes(N)
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=clean.device)
    score = torch.empty(N, dtype=torch.float32, device=clean.device)
    check(L.l2s_estoi(clean.data_ptr(), pred.data_ptr(), N, n, _ptr(fir), 0 if fir is None else fir.numel(), up, down, n_pre_remove, n_resampled,
                      bands, score.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return score


# ------------------------------------------------------------------------------------- the same three stages over clips of unequal length (include/l2s.h)
def _ints(values) -> Optional[ctypes.Array]:
    """A host int table for the *_ragged entry points (None stays a null pointer: the host checks refuse it)."""
    return None if values is None else (ctypes.c_int * len(values))(*[int(v) for v in values])


def _int64s(values) -> Optional[ctypes.Array]:
    return None if values is None else (_i64 * len(values))(*[int(v) for v in values])


def padded_mel_layout(N: int, n_mels: int, L_pad: int):
    """(offsets, pitches) of a contiguous padded (N, n_mels, L_pad) mel tensor, as `inverse_mel_ragged` takes them."""
    return [b * n_mels * L_pad for b in range(N)], [L_pad] * N


def inverse_mel_ragged_check(lengths, offsets, pitches, mel_floats: int, n_mels: int, n_freqs: int, fb_nnz: int, iters: int, N: Optional[int] = None) -> None:
    """`l2s_inverse_mel_ragged_check`: the pure host check (no device needed); raises with the clip and the limit it breaks."""
    check(lib().l2s_inverse_mel_ragged_check(_ints(lengths), _int64s(offsets), _int64s(pitches), len(lengths) if N is None else N, int(mel_floats), n_mels, n_freqs,
                                             int(fb_nnz), iters))


def inverse_mel_ragged_workspace_bytes(lengths, n_mels: int, n_freqs: int, iters: int) -> int:
    return int(lib().l2s_inverse_mel_ragged_workspace_bytes(_ints(lengths), len(lengths), n_mels, n_freqs, iters))


def inverse_mel_ragged(mel: torch.Tensor, lengths, fb: torch.Tensor, fb_nnz: int, init: torch.Tensor, iters: int, offsets=None, pitches=None,
                       log_input: bool = False, want_loss: bool = False):
    """`l2s_inverse_mel_ragged`: clip b = lengths[b] frames read at mel.flatten()[offsets[b] + m * pitches[b] + l] (default: mel is a padded
    (N, n_mels, L_pad) tensor, whatever its pad frames hold); init (sum L_b, n_freqs), clips back to back -> spec, flat: clip b's (n_freqs, L_b) block at
    float n_freqs * sum_{c<b} L_c [, loss (N, iters), iterations run per clip (N,) int32].  Every clip as `inverse_mel` computes it alone."""
    mel, fb, init = _f32(mel), _f32(fb), _f32(init)
    lengths = [int(v) for v in lengths]
    N, (F, M) = len(lengths), fb.shape
    if offsets is None:
        assert mel.dim() == 3 and mel.shape[0] == N and mel.shape[1] == M, mel.shape
        offsets, pitches = padded_mel_layout(N, M, mel.shape[2])
    inverse_mel_ragged_check(lengths, offsets, pitches, mel.numel(), M, F, fb_nnz, iters)
    R = sum(lengths)
    assert tuple(init.shape) == (R, F), (init.shape, R, F)
    L = lib()
    ws = torch.empty(int(L.l2s_inverse_mel_ragged_workspace_bytes(_ints(lengths), N, M, F, iters)), dtype=torch.uint8, device=mel.device)
    spec = torch.empty(R * F, dtype=torch.float32, device=mel.device)
    loss = torch.empty(N, max(iters, 1), dtype=torch.float32, device=mel.device) if want_loss else None
    ran = torch.empty(N, dtype=torch.int32, device=mel.device) if want_loss else None
    check(L.l2s_inverse_mel_ragged(mel.data_ptr(), mel.numel(), _int64s(offsets), _int64s(pitches), _ints(lengths), N, int(log_input), fb.data_ptr(), int(fb_nnz),
                                   init.data_ptr(), M, F, iters, spec.data_ptr(), _ptr(loss), _ptr(ran), ws.data_ptr(), ws.numel(), _stream()))
    return (spec, loss, ran) if want_loss else spec


def griffin_lim_ragged_check(lengths, iters: int, wave_pitch: int, n_fft: int = 1024, hop: int = 256, N: Optional[int] = None) -> None:
    """`l2s_griffin_lim_ragged_check`: the pure host check; raises with the clip and the limit it breaks."""
    check(lib().l2s_griffin_lim_ragged_check(_ints(lengths), len(lengths) if N is None else N, n_fft, hop, iters, int(wave_pitch)))


def griffin_lim_ragged_workspace_bytes(lengths) -> int:
    return int(lib().l2s_griffin_lim_ragged_workspace_bytes(_ints(lengths), len(lengths)))


def griffin_lim_ragged(power_spec: torch.Tensor, init_angles: torch.Tensor, lengths, iters: int, wave_pitch: Optional[int] = None, n_fft: int = 1024,
                       hop: int = 256, momentum: float = 0.99, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`l2s_griffin_lim_ragged`: power_spec flat, clip b's (n_fft/2+1, L_b) block at float 513 * sum_{c<b} L_c (what `inverse_mel_ragged` returns);
    init_angles flat float, clip b's (513, L_b, 2) block likewise -> wave (N, wave_pitch), default pitch hop * (max L_b - 1): clip b's hop * (L_b - 1)
    samples, then exact zeros.  Every clip as `griffin_lim` computes it alone.  `out`: a contiguous (N, wave_pitch) tensor to write instead."""
    power_spec, ang = _f32(power_spec), _f32(torch.view_as_real(init_angles) if init_angles.is_complex() else init_angles)
    lengths = [int(v) for v in lengths]
    N, R = len(lengths), sum(lengths)
    pitch = int(wave_pitch) if wave_pitch is not None else (out.shape[1] if out is not None else hop * (max(lengths) - 1))
    griffin_lim_ragged_check(lengths, iters, pitch, n_fft, hop)
    assert power_spec.numel() == R * (n_fft // 2 + 1) and ang.numel() == 2 * power_spec.numel(), (power_spec.shape, ang.shape, R)
    L = lib()
    ws = torch.empty(int(L.l2s_griffin_lim_ragged_workspace_bytes(_ints(lengths), N)), dtype=torch.uint8, device=power_spec.device)
    wave = out if out is not None else torch.empty(N, pitch, dtype=torch.float32, device=power_spec.device)
    assert tuple(wave.shape) == (N, pitch) and wave.dtype == torch.float32
    check(L.l2s_griffin_lim_ragged(power_spec.data_ptr(), ang.data_ptr(), _ints(lengths), N, n_fft, hop, iters, momentum, _ptr(wave), pitch, ws.data_ptr(),
                                   ws.numel(), _stream()))
    return wave


def estoi_ragged_check(n_samples, n_fir, n_resampled, pitch: int, has_fir: bool, n_fir_max: int, up: int, down: int, n_pre_remove: int,
                       N: Optional[int] = None) -> None:
    """`l2s_estoi_ragged_check`: the pure host check; raises with the clip and the limit it breaks."""
    check(lib().l2s_estoi_ragged_check(_ints(n_samples), _ints(n_fir), _ints(n_resampled), (len(n_samples) if n_samples is not None else 0) if N is None else N,
                                       int(pitch), int(has_fir), int(n_fir_max), up, down, n_pre_remove))


def estoi_ragged_workspace_bytes(n_resampled) -> int:
    return int(lib().l2s_estoi_ragged_workspace_bytes(_ints(n_resampled), len(n_resampled)))


def estoi_ragged(clean: torch.Tensor, pred: torch.Tensor, n_samples, fir: Optional[torch.Tensor], n_fir, up: int, down: int, n_pre_remove: int, n_resampled,
                 band_lo_hi) -> torch.Tensor:
    """`l2s_estoi_ragged`: clean / pred (N, pitch) on the device, clip b its first n_samples[b] samples -> ESTOI per clip (N,), each as `estoi` scores the clip
    alone.  `fir`: the longest clip's padded polyphase filter (device) or None; clip b uses its first n_fir[b] taps and resamples to n_resampled[b]."""
    clean, pred = _f32(clean), _f32(pred)
    N, pitch = clean.shape
    assert pred.shape == clean.shape and len(n_samples) == N
    n_fir_max = 0 if fir is None else fir.numel()
    estoi_ragged_check(n_samples, n_fir, n_resampled, pitch, fir is not None, n_fir_max, up, down, n_pre_remove)
    L = lib()
    bands = (ctypes.c_int * 30)(*[int(v) for v in band_lo_hi])
    ws = torch.empty(int(L.l2s_estoi_ragged_workspace_bytes(_ints(n_resampled), N)), dtype=torch.uint8, device=clean.device)
    score = torch.empty(N, dtype=torch.float32, device=clean.device)
    check(L.l2s_estoi_ragged(clean.data_ptr(), pred.data_ptr(), pitch, _ints(n_samples), N, _ptr(fir), n_fir_max, _ints(n_fir), up, down, n_pre_remove,
                             _ints(n_resampled), bands, score.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return score
