"""ctypes binding of ``libpce.so`` (C ABI: ``include/pce.h``).

:class:`ProsodyEngine` owns one ``pce_ctx`` (one process, one GPU).  A batch of clips is
uploaded once and stays resident in HBM; every measurement the reference takes by
re-decoding the file (Code/audioPipeline.py:314-361) becomes a slice of that batch.
There is no CPU path: without the built library or without a GPU, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libpce.so")


class PceError(RuntimeError):
    pass


PITCH_MAX_CANDIDATES = 16    # PI_MAXC of csrc/pce_pitch_plan.h: the row width of the pitch candidate arrays of the two test hooks
PYIN_MAX_TROUGHS = 512       # PCE_PYIN_MAX_TROUGHS of include/pce.h: the row width of pYIN's observation lists


def native_library_path() -> str:
    """The library this process binds: ``libpce.so`` beside this file, or the file ``PCE_LIBRARY`` names (laboratory builds are
    selected this way -- ``tools/ab_*.sh`` -- instead of being copied over the product's library)."""
    return os.environ.get("PCE_LIBRARY") or _LIB_PATH


def build_native(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into ``libpce.so`` (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j4"], stdout=subprocess.DEVNULL)
    if not os.path.exists(_LIB_PATH):
        raise PceError("build did not produce libpce.so")
    return _LIB_PATH


class Slice(C.Structure):
    _fields_ = [("clip", C.c_int32), ("flags", C.c_int32), ("begin", C.c_int64), ("end", C.c_int64), ("x1", C.c_double)]


class Energy(C.Structure):
    _fields_ = [("n", C.c_int64), ("sum_sq", C.c_int64), ("sum_sq_wrap16", C.c_int64), ("n_loud", C.c_int64),
                ("peak_abs", C.c_int32), ("reserved", C.c_int32)]


class PitchParams(C.Structure):
    _fields_ = [("time_step", C.c_double), ("pitch_floor", C.c_double), ("periods_per_window", C.c_double),
                ("max_candidates", C.c_int32), ("reserved", C.c_int32), ("silence_threshold", C.c_double),
                ("voicing_threshold", C.c_double), ("octave_cost", C.c_double), ("octave_jump_cost", C.c_double),
                ("voiced_unvoiced_cost", C.c_double), ("pitch_ceiling", C.c_double)]

    @classmethod
    def praat(cls, pitch_floor=75.0, pitch_ceiling=600.0, time_step=0.0):
        """parselmouth ``Sound.to_pitch(time_step, pitch_floor, pitch_ceiling)`` defaults."""
        return cls(time_step or 0.0, float(pitch_floor), 3.0, 15, 0, 0.03, 0.45, 0.01, 0.35, 0.14, float(pitch_ceiling))


class PitchSummary(C.Structure):
    _fields_ = [("n_frames", C.c_int64), ("n_voiced", C.c_int64), ("median_f0", C.c_double), ("mean_log_f0", C.c_double),
                ("t1", C.c_double), ("status", C.c_int32), ("reserved", C.c_int32)]


class IntensityParams(C.Structure):
    _fields_ = [("pitch_floor", C.c_double), ("time_step", C.c_double), ("subtract_mean", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def praat(cls, pitch_floor=100.0, time_step=0.0, subtract_mean=True):
        """parselmouth ``Sound.to_intensity(minimum_pitch, time_step, subtract_mean)`` defaults."""
        return cls(float(pitch_floor), time_step or 0.0, 1 if subtract_mean else 0, 0)


class IntensitySummary(C.Structure):
    _fields_ = [("n_frames", C.c_int64), ("n_positive", C.c_int64), ("mean_positive", C.c_double), ("t1", C.c_double),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class SilenceParams(C.Structure):
    _fields_ = [("min_silence_len", C.c_int32), ("seek_step", C.c_int32), ("channels", C.c_int32), ("reserved", C.c_int32)]


class WhisperDims(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("n_ctx", C.c_int32), ("n_state", C.c_int32), ("n_head", C.c_int32), ("n_layer", C.c_int32)]


class WhisperTextDims(C.Structure):
    _fields_ = [("n_vocab", C.c_int32), ("n_text_ctx", C.c_int32), ("n_state", C.c_int32), ("n_head", C.c_int32), ("n_layer", C.c_int32)]


class WhisperDecodeRules(C.Structure):
    _fields_ = [("eot", C.c_int32), ("timestamp_begin", C.c_int32), ("max_initial_timestamp_index", C.c_int32), ("reserved", C.c_int32)]


class WhisperDecodeOpts(C.Structure):
    _fields_ = [("sample_begin", C.c_void_p), ("sample_begin_all", C.c_int32), ("temperature", C.c_float), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32), ("probe_token", C.c_int32), ("flags", C.c_int32)]


class BertDims(C.Structure):
    _fields_ = [("n_vocab", C.c_int32), ("n_pos", C.c_int32), ("n_type", C.c_int32), ("n_state", C.c_int32), ("n_head", C.c_int32),
                ("n_layer", C.c_int32), ("n_labels", C.c_int32)]


class W2vDims(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * 8), ("conv_kernel", C.c_int32 * 8), ("conv_stride", C.c_int32 * 8),
                ("feat_norm", C.c_int32), ("conv_bias", C.c_int32), ("n_state", C.c_int32), ("n_head", C.c_int32), ("n_inter", C.c_int32),
                ("n_layer", C.c_int32), ("stable_ln", C.c_int32), ("pos_taps", C.c_int32), ("pos_groups", C.c_int32), ("n_vocab", C.c_int32),
                ("ln_eps", C.c_float)]

    @classmethod
    def of(cls, dims: dict):
        """``w2v_weights.dims(config)`` -> the struct (at most eight feature-encoder layers fit; the loader takes seven)."""
        if not 1 <= len(dims["conv_dim"]) <= 8 or not len(dims["conv_dim"]) == len(dims["conv_kernel"]) == len(dims["conv_stride"]) == dims["n_conv"]:
            raise ValueError("conv_dim / conv_kernel / conv_stride: n_conv entries each, at most eight")
        pad = lambda v: (C.c_int32 * 8)(*(list(v) + [0] * (8 - len(v))))
        return cls(dims["n_conv"], pad(dims["conv_dim"]), pad(dims["conv_kernel"]), pad(dims["conv_stride"]), dims["feat_norm"], dims["conv_bias"],
                   dims["n_state"], dims["n_head"], dims["n_inter"], dims["n_layer"], dims["stable_ln"], dims["pos_taps"], dims["pos_groups"],
                   dims["n_vocab"], dims["ln_eps"])


class W2vPlan(C.Structure):
    _fields_ = [("window_samples", C.c_int32), ("context_samples", C.c_int32), ("windows_per_chunk", C.c_int32), ("star", C.c_int32)]


class W2vSegment(C.Structure):
    _fields_ = [("clip", C.c_int32), ("reserved", C.c_int32), ("begin", C.c_int64), ("end", C.c_int64)]


class W2vSegPlan(C.Structure):
    _fields_ = [("min_samples", C.c_int32), ("segments_per_chunk", C.c_int32), ("star", C.c_int32)]


class DeviceEmissions:
    """The packed emissions of ``ProsodyEngine.w2v_emissions`` / ``w2v_segment_emissions``: device memory ``[sum n_frames][n_cols]`` float32 of
    the engine that made them (valid until its next ``w2v_emissions`` / ``w2v_segment_emissions`` / ``w2v_load``, which may free or overwrite
    the memory), clip (or segment) ``q`` in rows ``row_start[q] .. row_start[q] + n_frames[q]``.  ``ProsodyEngine.ctc_align`` and ``wx_align``
    read it in place.  ``epoch`` is the engine's count of those calls when it was made: an object from before the engine's latest call is
    refused (``check``), not read."""

    def __init__(self, engine, pointer: int, row_start: np.ndarray, n_frames: np.ndarray, n_cols: int, epoch: int):
        self.engine, self.pointer, self.row_start, self.n_frames, self.n_cols = engine, int(pointer), row_start, n_frames, int(n_cols)
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.n_frames)

    def check(self):
        if self.epoch != self.engine._w2v_epoch:
            raise ValueError("these emissions are stale: the engine has run w2v_emissions / w2v_segment_emissions / w2v_load since they were made")

    def numpy(self):
        """-> one float32 array ``[n_frames][n_cols]`` per clip (fetched to the host)."""
        self.check()
        return [self.engine.w2v_fetch(q) for q in range(len(self.n_frames))]


class CtcParams(C.Structure):
    _fields_ = [("blank", C.c_int32), ("form", C.c_int32), ("reserved", C.c_int32 * 2)]


class WxParams(C.Structure):
    _fields_ = [("blank", C.c_int32), ("beam_width", C.c_int32), ("reserved", C.c_int32 * 2)]


class CrepeDims(C.Structure):
    _fields_ = [("c_out", C.c_int32 * 6), ("reserved", C.c_int32 * 2)]


class CrepePlan(C.Structure):
    _fields_ = [("hop", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("decoder", C.c_int32), ("frames_per_chunk", C.c_int32),
                ("reserved", C.c_int32)]


SLICE_DTYPE = np.dtype([("clip", "<i4"), ("flags", "<i4"), ("begin", "<i8"), ("end", "<i8"), ("x1", "<f8")])
ENERGY_DTYPE = np.dtype([("n", "<i8"), ("sum_sq", "<i8"), ("sum_sq_wrap16", "<i8"), ("n_loud", "<i8"),
                         ("peak_abs", "<i4"), ("reserved", "<i4")])
SUMMARY_DTYPE = np.dtype([("n_frames", "<i8"), ("n_voiced", "<i8"), ("median_f0", "<f8"), ("mean_log_f0", "<f8"),
                          ("t1", "<f8"), ("status", "<i4"), ("reserved", "<i4")])
assert SLICE_DTYPE.itemsize == C.sizeof(Slice) and ENERGY_DTYPE.itemsize == C.sizeof(Energy)
assert SUMMARY_DTYPE.itemsize == C.sizeof(PitchSummary)
INTENSITY_SUMMARY_DTYPE = np.dtype([("n_frames", "<i8"), ("n_positive", "<i8"), ("mean_positive", "<f8"), ("t1", "<f8"),
                                    ("status", "<i4"), ("reserved", "<i4")])
assert INTENSITY_SUMMARY_DTYPE.itemsize == C.sizeof(IntensitySummary) == 40 and C.sizeof(IntensityParams) == 24

# the records of pce_lufs_fetch_stages
LUFS_CHUNK_DTYPE = np.dtype([("rel", "<i8"), ("len", "<i4"), ("slice", "<i4"), ("state_end", "<f8", (4,)), ("state_init", "<f8", (4,)), ("energy", "<f8")])
LUFS_SLICE_DTYPE = np.dtype([("first_chunk", "<i4"), ("n_chunks", "<i4"), ("first_block", "<i4"), ("n_blocks", "<i4"), ("status", "<i4"), ("peak", "<i4")])
LUFS_BLOCK_DTYPE = np.dtype([("c0", "<i4"), ("c1", "<i4"), ("z", "<f8")])
assert (LUFS_CHUNK_DTYPE.itemsize, LUFS_SLICE_DTYPE.itemsize, LUFS_BLOCK_DTYPE.itemsize) == (88, 24, 16)
LUFS_MAX_CHUNK = 256                                          # LU_LMAX of csrc/pce_lufs.hip: the longest chunk, the last power of the table

SLICE_OK, SLICE_TOO_SHORT, SLICE_EMPTY = 0, 1, 2
DTW_OK, DTW_EMPTY, DTW_NO_PATH = 0, 1, 2                      # enum pce_dtw_status
CTC_OK, CTC_EMPTY, CTC_TOO_SHORT, CTC_NO_PATH = 0, 1, 2, 3     # enum pce_ctc_status
CTC_REG_STATES = 4096                                         # PCE_CTC_REG_STATES of include/pce.h: the states (2 L + 1) the register form of k_ctc holds
CTC_FORMS = {"auto": 0, "register": 1, "general": 2}
WX_OK, WX_EMPTY, WX_NO_PATH = 0, 1, 2                         # enum pce_wx_status
WX_MAX_TOKENS, WX_MAX_BEAM = 4096, 8                          # PCE_WX_MAX_TOKENS / PCE_WX_MAX_BEAM of include/pce.h: the tokens k_wx_trellis sweeps, the beams k_wx_backtrack keeps
DTW_SERIES_ROWS, DTW_SERIES_COLS = 1024, 2048                 # PCE_DTW_SERIES_ROWS / _COLS of include/pce.h: the tile of k_dtw_series

KERNEL_IDS = ["k_energy", "k_lufs_pass1", "k_lufs_scan", "k_lufs_pass2", "k_lufs_gate",
              "k_pitch_refine", "k_pitch_frames", "k_pitch_path", "k_pitch_median", "k_pitch_delta", "k_stft_max", "k_stft_db", "k_logmel_frames", "whisper_encoder", "k_resample", "k_dtw", "whisper_align", "k_nw", "k_stft_norm", "k_frame_energy", "bert_forward", "k_pyin_frames", "k_pyin_viterbi", "whisper_decode_step",
              "k_gemm_bf16", "k_gemm_wide", "k_attention", "k_layernorm", "k_gemm_flat",
              "k_add_layernorm", "k_stft_raw", "k_logmel_norm", "k_attention_lean",
              "k_gemm_flat:qkv", "k_gemm_flat:out", "k_gemm_flat:fc1", "k_gemm_flat:fc2", "k_gemm_flat:xkv",
              "whisper_decode_loop", "k_cross_attn1", "k_gemm_skinny", "k_levenshtein", "k_dtw_series", "k_dtw_series_trace",
              "k_intensity", "k_intensity_summary", "k_ms_energy", "k_silence_scan", "k_silence_ranges",
              "k_crepe_frames", "k_crepe_conv1", "k_crepe_conv:block2", "k_crepe_conv", "k_crepe_classifier", "k_crepe_decode", "k_crepe_viterbi",
              "k_ivl_classes", "k_ivl_claim",
              "w2v_forward", "k_w2v_wave", "k_w2v_posconv", "k_w2v_tail",
              "k_wx_rowmax", "k_wx_trellis", "k_wx_backtrack",
              "k_ctc", "k_ctc_general", "k_ctc_trace", "k_seqmatch", "k_seqmatch_align"]     # = pce_kernel_name(id) for every id (tests/test_abi_and_shard.py)

# every symbol include/pce.h declares (tests/test_abi_and_shard.py), in the header's order and under its section titles: name -> argtypes, or
# (argtypes, restype) where the function does not return int
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
SIGNATURES = {
    # context
    "pce_create": ([C.c_int, _vp, C.c_char_p, C.c_size_t], _vp),
    "pce_destroy": ([_vp], None),
    "pce_last_error": ([_vp], C.c_char_p),
    "pce_sync": [_vp],
    "pce_api_version": [],
    "pce_api_minor": [],
    "pce_device_info": [_vp, C.c_char_p, C.c_size_t, C.POINTER(_i32), C.POINTER(_i64)],
    # batch residency
    "pce_upload_pcm_s16": [_vp, _vp, _vp, _i32, _i32],
    "pce_bind_pcm_s16_device": [_vp, _vp, _vp, _i32, _i32],
    "pce_num_clips": [_vp],
    # sample-rate conversion of the resident batch
    "pce_resample_run": [_vp, _i32, _i32, _vp, _i32, _i64],
    "pce_download_pcm_s16": [_vp, _vp, _vp, C.POINTER(_i32)],
    # frame-level short-time energy
    "pce_frame_energy_run": [_vp, _i32, _i32, _i32],
    "pce_frame_energy_shape": [_vp, _i32, C.POINTER(_i64)],
    "pce_frame_energy_fetch": [_vp, _i32, _vp, _vp],
    # R3 / R7: short-time energy, peak, silence gate
    "pce_energy_run": [_vp, _vp, _i32, _i32],
    "pce_energy_fetch": [_vp, _vp],
    # R4: BS.1770 integrated loudness
    "pce_lufs_set_meter_rate": [_vp, _i32],
    "pce_lufs_run": [_vp, _vp, _i32],
    "pce_lufs_fetch": [_vp, _vp, _vp],
    "pce_lufs_stage_sizes": [_vp, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)],
    "pce_lufs_fetch_stages": [_vp, _vp, _vp, _vp, _vp, _vp],
    # R1 / R2: Praat autocorrelation pitch
    "pce_pitch_plan": [_vp, C.POINTER(PitchParams), _vp, _i32, _vp, _vp],
    "pce_pitch_run": [_vp, C.POINTER(PitchParams), _vp, _i32],
    "pce_pitch_set_refine": [_vp, _i32],
    "pce_pitch_fetch": [_vp, _vp, _vp, _vp],
    "pce_pitch_fetch_candidates": [_vp, _vp, _vp, _vp, _vp],
    "pce_selftest_pitch_path": [_vp, C.POINTER(PitchParams), C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # Praat intensity
    "pce_intensity_plan": [_vp, C.POINTER(IntensityParams), _vp, _i32, _vp, _vp],
    "pce_intensity_run": [_vp, C.POINTER(IntensityParams), _vp, _i32, _vp, _i32],
    "pce_intensity_fetch": [_vp, _vp, _vp],
    # silence detection
    "pce_silence_run": [_vp, C.POINTER(SilenceParams), _vp, _vp, _i32],
    "pce_silence_shape": [_vp, _vp, _vp, _vp],
    "pce_silence_fetch": [_vp, _vp],
    # R10: STFT magnitude in dB
    "pce_stft_db_run": [_vp, _i32, _i32],
    "pce_stft_db_shape": [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32)],
    "pce_stft_db_fetch": [_vp, _i32, _vp],
    "pce_stft_db_device": [_vp, C.POINTER(_vp), C.POINTER(_i64)],
    # R10: probabilistic YIN
    "pce_pyin_run": [_vp, _vp, _vp, _i64],
    "pce_pyin_shape": [_vp, _i32, C.POINTER(_i64)],
    "pce_pyin_fetch": [_vp, _i32, _vp, _vp, C.POINTER(_i32)],
    "pce_pyin_fetch_observations": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "pce_selftest_pyin_viterbi": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    # CREPE pitch tracking
    "pce_crepe_load": [_vp, C.POINTER(CrepeDims), _vp, _i64],
    "pce_crepe_run": [_vp, C.POINTER(CrepePlan)],
    "pce_crepe_shape": [_vp, _i32, C.POINTER(_i64)],
    "pce_crepe_fetch": [_vp, _i32, _vp, _vp, _vp, _vp],
    "pce_selftest_crepe_layer": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "pce_selftest_crepe_decode": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    # R8: log-mel spectrogram + Whisper audio encoder
    "pce_logmel_run": [_vp, _i32],
    "pce_logmel_run_at": [_vp, _i32, _vp],
    "pce_logmel_fetch": [_vp, _i32, _vp],
    "pce_selftest_logmel_image": [_vp, _i32, _vp],
    "pce_whisper_load": [_vp, C.POINTER(WhisperDims), _vp, _i64],
    "pce_whisper_encode_run": [_vp],
    "pce_selftest_gemm": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "pce_selftest_gemm_resid": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32],
    "pce_selftest_attention": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "pce_selftest_attention_ragged": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i64, _vp],
    "pce_selftest_attn1": [_vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64],
    "pce_selftest_align_matrix": [_vp, _i32, _i32, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_float, _vp, _i64, _vp, _i64, _vp, _i64],
    "pce_selftest_xattn": [_vp] * 11 + [_i32] * 5 + [_vp],
    "pce_selftest_xattn_stages": [_vp] * 10 + [_i64, _vp, _vp] + [_i32] * 5 + [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp],
    "pce_selftest_gemm_tiled": [_vp, _i32, _i32, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp],
    "pce_selftest_layernorm": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _vp, _vp, _vp],
    "pce_selftest_encoder_walk": [_vp] + [_i32] * 10 + [_vp, C.c_float, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp],
    "pce_whisper_encode_fetch": [_vp, _i32, _vp],
    # R8: forced alignment of known text tokens
    "pce_whisper_decoder_load": [_vp, C.POINTER(WhisperTextDims), _vp, _i64],
    "pce_whisper_align_run": [_vp, _vp, _vp, _vp, _i32, _vp, _i32, C.c_float],
    "pce_whisper_align_shape": [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32)],
    "pce_whisper_align_fetch": [_vp, _i32, _vp, _vp, C.POINTER(_i32), _vp],
    "pce_whisper_align_paths_enqueue": [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32)],
    "pce_whisper_align_paths_wait": [_vp, _i32, _vp, _vp, _vp],
    # R8: free-running decoding, one step
    "pce_whisper_decode_step": [_vp, _vp, _vp, _i32, C.POINTER(WhisperDecodeRules), _vp, _vp, _vp],
    "pce_whisper_decode_step_ex": [_vp, _vp, _vp, C.POINTER(WhisperDecodeRules), _vp, C.POINTER(WhisperDecodeOpts), _vp, _vp, _vp],
    "pce_whisper_sample_keys": [_vp, _vp, _i32],
    "pce_selftest_decode_rules": [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _vp, _i32, C.POINTER(WhisperDecodeRules), _vp, _i64, C.c_float, C.c_uint32, C.c_uint32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64],
    "pce_whisper_set_operands": [_vp, _i32],
    "pce_whisper_get_operands": [_vp],
    "pce_whisper_decode_loop": [_vp, _vp, _vp, C.POINTER(WhisperDecodeRules), _vp, C.POINTER(WhisperDecodeOpts), _i32, _i32, _vp, _vp, _vp, _vp],
    "pce_whisper_detect_language": [_vp, _i32, _i32, _i32, _vp, _vp],
    # R8: dynamic time warping
    "pce_dtw": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    # DTW of pairs of series
    "pce_dtw_series": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    # CTC forced alignment
    "pce_ctc_align": [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # whisperX forced alignment
    "pce_wx_align": [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    # batched Needleman-Wunsch word alignment
    "pce_nw_align": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    # batched Levenshtein distance
    "pce_levenshtein": [_vp, _vp, _vp, _vp, _vp, _i32, _vp],
    # batched difflib.SequenceMatcher and the fuzzy alignment of "Compare Breaks"
    "pce_seqmatch": [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _vp],
    "pce_seqmatch_align": [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, C.POINTER(_i32)],
    # the text matching of the aligner evaluation
    "pce_ivl_match": [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
    # break-prediction token classifier
    "pce_bert_load": [_vp, C.POINTER(BertDims), _vp, _i64],
    "pce_bert_run": [_vp, _vp, _vp, _i32],
    "pce_bert_fetch": [_vp, _i32, _vp, _vp],
    # wav2vec2 / MMS CTC acoustic model: the emissions of the forced alignment
    "pce_w2v_load": [_vp, C.POINTER(W2vDims), _vp, _i64],
    "pce_w2v_check": [C.POINTER(W2vDims), _i64, C.c_char_p, C.c_size_t],
    "pce_w2v_run": [_vp, C.POINTER(W2vPlan)],
    "pce_w2v_shape": [_vp, _i32, C.POINTER(_i64), C.POINTER(_i32)],
    "pce_w2v_fetch": [_vp, _i32, _vp],
    "pce_w2v_device": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32)],
    "pce_w2v_window_plan": [_i64, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)],
    "pce_w2v_run_segments": [_vp, C.POINTER(W2vSegment), _i32, C.POINTER(W2vSegPlan)],
    "pce_w2v_segment_frames": [C.POINTER(W2vDims), _i64, _i32, C.POINTER(_i64)],
    "pce_w2v_segments_plan": [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)],
    "pce_selftest_w2v_wave": [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "pce_selftest_w2v_lngelu": [_vp, _vp, _i32, _i32, _vp, _vp, C.c_float, _i32, _vp],
    "pce_selftest_w2v_posconv": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "pce_selftest_w2v_wave_segments": [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "pce_selftest_w2v_posconv_segments": [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    # asynchronous statistics fetch
    "pce_stats_enqueue": [_vp, _i32],
    "pce_stats_wait": [_vp, _i32, _vp, _vp, _vp, _vp],
    # measurement
    "pce_profile_enable": [_vp, C.c_int],
    "pce_profile_reset": [_vp],
    "pce_profile_get": [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(_i64)],
    "pce_profile_get_work": [_vp, C.c_int, C.POINTER(C.c_double)],
    "pce_kernel_name": ([C.c_int], C.c_char_p),
}
EXPORTS = list(SIGNATURES)


def load_library() -> C.CDLL:
    path = native_library_path()
    if not os.path.exists(path):
        raise PceError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                       "this engine has no CPU fallback")
    lib = C.CDLL(path)
    for name, sig in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
    return lib


def w2v_check(dims: dict, n_floats: int, lib=None):
    """-> (status, message) ``pce_w2v_load`` would give for these dims (``w2v_weights.dims``) and a blob of ``n_floats``: ``pce_w2v_check``, no device."""
    lib = lib or load_library()
    msg = C.create_string_buffer(320)
    rc = lib.pce_w2v_check(C.byref(W2vDims.of(dims)), int(n_floats), msg, len(msg))
    return rc, msg.value.decode(errors="replace")


def w2v_window_plan(n_samples: int, window_s=30, context_s=2, lib=None):
    """-> (windows, frames kept) of one 16 kHz clip as ``pce_w2v_run`` counts them: ``pce_w2v_window_plan``, host arithmetic that needs no device."""
    lib = lib or load_library()
    nw, nf = C.c_int64(), C.c_int64()
    rc = lib.pce_w2v_window_plan(int(n_samples), int(window_s * 16000), int(context_s * 16000), C.byref(nw), C.byref(nf))
    if rc:
        raise PceError(f"pce_w2v_window_plan: status {rc}")
    return nw.value, nf.value


def w2v_segment_frames(dims: dict, n_samples: int, min_samples: int = 400, lib=None) -> int:
    """-> frames the model of ``dims`` (``w2v_weights.dims``) gives for a segment of ``n_samples`` run on ``max(n_samples, min_samples)``, as
    ``pce_w2v_run_segments`` counts them: ``pce_w2v_segment_frames``, host arithmetic that needs no device."""
    lib = lib or load_library()
    nf = C.c_int64()
    rc = lib.pce_w2v_segment_frames(C.byref(W2vDims.of(dims)), int(n_samples), int(min_samples), C.byref(nf))
    if rc:
        raise PceError(f"pce_w2v_segment_frames: status {rc}")
    return nf.value


def make_slices(clips, begins, ends, x1=None) -> np.ndarray:
    """Pack parallel arrays into the ``pce_slice`` layout."""
    n = len(clips)
    s = np.zeros(n, dtype=SLICE_DTYPE)
    s["clip"] = clips; s["begin"] = begins; s["end"] = ends
    if x1 is not None:
        s["x1"] = x1
    return s


class ProsodyEngine:
    """One GPU context.  ``device``: HIP device index; ``stream``: optional ``hipStream_t`` handle
    (e.g. ``torch.cuda.current_stream().cuda_stream``) to enqueue on."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._lib = load_library()
        err = C.create_string_buffer(512)
        self._ctx = self._lib.pce_create(int(device), C.c_void_p(stream) if stream else None, err, len(err))
        if not self._ctx:
            raise PceError(f"pce_create failed: {err.value.decode(errors='replace')}")
        self.device = int(device)
        self.rate = 0
        self.clip_lengths = np.zeros(0, dtype=np.int64)
        self._keep = []
        self._w2v_epoch = 0                  # w2v_load / w2v_emissions calls so far (DeviceEmissions.check)
        self._w2v_held = None                # (weak reference to the model object of the latest w2v_load, operand mode)

    # ---------------------------------------------------------------- plumbing
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.pce_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise PceError(f"libpce status {rc}: {self._lib.pce_last_error(self._ctx).decode(errors='replace')}")

    def sync(self):
        self._check(self._lib.pce_sync(self._ctx))

    def device_info(self):
        name = C.create_string_buffer(256); cus = C.c_int32(); hbm = C.c_int64()
        self._check(self._lib.pce_device_info(self._ctx, name, len(name), C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    # ---------------------------------------------------------------- residency
    def upload(self, clips, rate: int):
        """Upload a batch: ``clips`` is a list of int16 1-D arrays (one per utterance)."""
        clips = [np.ascontiguousarray(c, dtype=np.int16).reshape(-1) for c in clips]
        lens = np.array([len(c) for c in clips], dtype=np.int64)
        offsets = np.zeros(len(clips) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        pcm = np.concatenate(clips) if clips else np.zeros(0, dtype=np.int16)
        if pcm.size == 0:
            pcm = np.zeros(1, dtype=np.int16)
        self._check(self._lib.pce_upload_pcm_s16(self._ctx, pcm.ctypes.data, offsets.ctypes.data, len(clips), int(rate)))
        self.rate = int(rate); self.clip_lengths = lens; self.offsets = offsets
        return self

    def bind_device(self, device_ptr: int, offsets, rate: int, keepalive=None):
        """Zero-copy: adopt int16 PCM already resident in HBM (e.g. a torch tensor's ``data_ptr()``)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self._check(self._lib.pce_bind_pcm_s16_device(self._ctx, C.c_void_p(device_ptr), offsets.ctypes.data,
                                                       len(offsets) - 1, int(rate)))
        self.rate = int(rate); self.clip_lengths = np.diff(offsets); self.offsets = offsets
        self._keep = [keepalive]
        return self

    def whole_clip_slices(self) -> np.ndarray:
        n = len(self.clip_lengths)
        return make_slices(np.arange(n), np.zeros(n, dtype=np.int64), self.clip_lengths, np.full(n, 0.5 / self.rate))

    # ---------------------------------------------------------------- ops
    @staticmethod
    def _slices(s) -> np.ndarray:
        s = np.ascontiguousarray(s, dtype=SLICE_DTYPE)
        return s

    def energy_run(self, slices, loud_threshold: int = 500):
        s = self._slices(slices); self._en_n = len(s)
        self._check(self._lib.pce_energy_run(self._ctx, s.ctypes.data, len(s), int(loud_threshold)))

    def energy_fetch(self) -> np.ndarray:
        out = np.zeros(self._en_n, dtype=ENERGY_DTYPE)
        self._check(self._lib.pce_energy_fetch(self._ctx, out.ctypes.data))
        return out

    def energy(self, slices, loud_threshold: int = 500) -> np.ndarray:
        self.energy_run(slices, loud_threshold)
        return self.energy_fetch()

    def lufs_set_meter_rate(self, rate: int = 0):
        """``pyln.Meter(rate)`` of the following ``lufs`` calls (0: the batch's own rate)."""
        self._check(self._lib.pce_lufs_set_meter_rate(self._ctx, int(rate)))

    def pitch_set_refine(self, mode: str = "seeded"):
        """How candidate maxima are refined (``pce_pitch_set_refine``): ``"seeded"`` (default: parabolic search seeded with the samples
        around the peak, Praat's own iterates only where the two could differ) or ``"praat"`` (NUMminimize_brent's iterates for every
        candidate).  Additive config key of ``AudioPipeline``: ``pitch_refine``."""
        self._check(self._lib.pce_pitch_set_refine(self._ctx, {"seeded": 0, "praat": 1}[str(mode).lower()]))

    def lufs_run(self, slices):
        s = self._slices(slices); self._lu_n = len(s)
        self._check(self._lib.pce_lufs_run(self._ctx, s.ctypes.data, len(s)))

    def lufs_fetch(self):
        out = np.zeros(self._lu_n, dtype=np.float64); st = np.zeros(self._lu_n, dtype=np.int32)
        self._check(self._lib.pce_lufs_fetch(self._ctx, out.ctypes.data, st.ctypes.data))
        return out, st

    def lufs(self, slices):
        self.lufs_run(slices)
        return self.lufs_fetch()

    def lufs_fetch_stages(self):
        """``pce_lufs_fetch_stages`` (test hook): what the plan and the four kernels of the last ``lufs_run`` left -> dict of ``coef`` float64 [13]
        (b, a, c, d, 1 / (0.4 rate)), ``apow`` float64 [257, 4, 4], and three record arrays: ``chunks`` (``LUFS_CHUNK_DTYPE``), ``slices``
        (``LUFS_SLICE_DTYPE``; ``peak`` is the integer the run divided by) and ``blocks`` (``LUFS_BLOCK_DTYPE``).  Read only."""
        n = _i32(); nch = _i64(); nbl = _i64()
        self._check(self._lib.pce_lufs_stage_sizes(self._ctx, C.byref(n), C.byref(nch), C.byref(nbl)))
        o = {"coef": np.zeros(13), "apow": np.zeros((LUFS_MAX_CHUNK + 1, 4, 4)), "chunks": np.zeros(nch.value, LUFS_CHUNK_DTYPE),
             "slices": np.zeros(n.value, LUFS_SLICE_DTYPE), "blocks": np.zeros(nbl.value, LUFS_BLOCK_DTYPE)}
        self._check(self._lib.pce_lufs_fetch_stages(self._ctx, *(o[k].ctypes.data for k in ("coef", "apow", "chunks", "slices", "blocks"))))
        return o

    def pitch_plan(self, slices, params: PitchParams):
        s = self._slices(slices)
        off = np.zeros(len(s) + 1, dtype=np.int64); st = np.zeros(len(s), dtype=np.int32)
        self._check(self._lib.pce_pitch_plan(self._ctx, C.byref(params), s.ctypes.data, len(s), off.ctypes.data, st.ctypes.data))
        return off, st

    def pitch_run(self, slices, params: PitchParams):
        s = self._slices(slices); self._pi_slices = s; self._pi_params = params
        self._check(self._lib.pce_pitch_run(self._ctx, C.byref(params), s.ctypes.data, len(s)))

    def pitch_fetch(self, want_f0=True, want_strength=False):
        s = self._pi_slices
        off, _ = self.pitch_plan(s, self._pi_params)
        total = int(off[-1])
        f0 = np.zeros(total, dtype=np.float64) if want_f0 else None
        sg = np.zeros(total, dtype=np.float64) if want_strength else None
        summ = np.zeros(len(s), dtype=SUMMARY_DTYPE)
        self._check(self._lib.pce_pitch_fetch(self._ctx, f0.ctypes.data if want_f0 else None,
                                              sg.ctypes.data if want_strength else None, summ.ctypes.data))
        return {"frame_offsets": off, "f0": f0, "strength": sg, "summary": summ}

    def pitch(self, slices, params: PitchParams, want_f0=True, want_strength=False):
        self.pitch_run(slices, params)
        return self.pitch_fetch(want_f0, want_strength)

    def pitch_fetch_candidates(self, fill=np.nan):
        """``pce_pitch_fetch_candidates`` (test hook): what ``k_pitch_frames`` and ``k_pitch_refine`` left for every frame of the last ``pitch_run`` ->
        dict of ``frame_offsets``, ``ncand`` int32 [frames], ``intensity`` float64 [frames], ``cand_f`` / ``cand_s`` float64 [frames, 16] (slot 0: 0 / 0;
        slots at or beyond ``ncand``: ``fill``, the device never wrote them)."""
        off, _ = self.pitch_plan(self._pi_slices, self._pi_params)
        total = int(off[-1])
        o = {"frame_offsets": off, "ncand": np.zeros(total, np.int32), "intensity": np.zeros(total), "cand_f": np.full((total, PITCH_MAX_CANDIDATES), fill, np.float64),
             "cand_s": np.full((total, PITCH_MAX_CANDIDATES), fill, np.float64)}
        self._check(self._lib.pce_pitch_fetch_candidates(self._ctx, *(o[k].ctypes.data for k in ("ncand", "intensity", "cand_f", "cand_s"))))
        return o

    def selftest_pitch_path(self, params: PitchParams, dt, frame_off, ncand, intensity, cand_f, cand_s):
        """``pce_selftest_pitch_path`` (test hook): ``k_pitch_delta``, ``k_pitch_path`` and the median kernels on given candidates (rows of 16, the
        first ``ncand`` count, slot 0 the voiceless one) of slices ``frame_off[i] .. frame_off[i + 1]``, through the launches of ``pitch_run`` ->
        dict of ``f0``, ``strength`` float64 [frames], ``psi`` uint8 [frames, 16], ``summary`` [slices].  The ceiling of ``params`` is taken as given.
        Uses the pitch buffers: ``pitch_fetch`` is refused afterwards until the next ``pitch_run``."""
        off = np.ascontiguousarray(frame_off, dtype=np.int64); n = np.ascontiguousarray(ncand, dtype=np.int32)
        it = np.ascontiguousarray(intensity, dtype=np.float64)
        cf = np.ascontiguousarray(cand_f, dtype=np.float64); cs = np.ascontiguousarray(cand_s, dtype=np.float64)
        total = int(off[-1]) if off.size else 0
        if off.ndim != 1 or off.size < 2 or n.shape != (total,) or it.shape != (total,) or cf.shape != (total, PITCH_MAX_CANDIDATES) or cs.shape != cf.shape:
            raise ValueError("frame_off [slices + 1]; ncand, intensity [frames]; cand_f, cand_s [frames, 16]")
        o = {"f0": np.zeros(total), "strength": np.zeros(total), "psi": np.zeros((total, PITCH_MAX_CANDIDATES), np.uint8),
             "summary": np.zeros(off.size - 1, dtype=SUMMARY_DTYPE)}
        self._check(self._lib.pce_selftest_pitch_path(self._ctx, C.byref(params), float(dt), off.size - 1, off.ctypes.data, n.ctypes.data, it.ctypes.data,
                                                      cf.ctypes.data, cs.ctypes.data, o["f0"].ctypes.data, o["strength"].ctypes.data, o["psi"].ctypes.data,
                                                      o["summary"].ctypes.data))
        return o

    def intensity_plan(self, slices, params: IntensityParams):
        """Host-only sizing of a Praat intensity analysis -> (frame_offsets int64 [n + 1], status int32 [n])."""
        s = self._slices(slices)
        off = np.zeros(len(s) + 1, dtype=np.int64); st = np.zeros(len(s), dtype=np.int32)
        self._check(self._lib.pce_intensity_plan(self._ctx, C.byref(params), s.ctypes.data, len(s), off.ctypes.data, st.ctypes.data))
        return off, st

    def intensity_run(self, slices, params: IntensityParams):
        """Enqueue Praat's ``Sound_to_Intensity`` over ``slices`` (``pce_intensity_run``); the window's tap table is built here
        (``hostrules.intensity_window``, kept per (rate, pitch floor)) and travels with the call.  A repeated call with the same slices,
        parameters and table skips the host plan."""
        from .hostrules import intensity_window
        key = (self.rate, float(params.pitch_floor))
        cache = self.__dict__.setdefault("_in_windows", {})
        if key not in cache:
            cache.clear()
            cache[key] = np.ascontiguousarray(intensity_window(self.rate, float(params.pitch_floor))[1], dtype=np.float64)
        taps = cache[key]
        s = self._slices(slices); self._in_slices = s; self._in_params = params
        self._check(self._lib.pce_intensity_run(self._ctx, C.byref(params), taps.ctypes.data, len(taps), s.ctypes.data, len(s)))

    def intensity_fetch(self, want_contour=True):
        """-> {"values": ragged float64 dB contour or None, "frame_offsets", "summary": INTENSITY_SUMMARY_DTYPE [n]}; without the
        contour a slice costs 40 bytes of download."""
        s = self._in_slices
        off, _ = self.intensity_plan(s, self._in_params)
        vals = np.zeros(int(off[-1]), dtype=np.float64) if want_contour else None
        summ = np.zeros(len(s), dtype=INTENSITY_SUMMARY_DTYPE)
        self._check(self._lib.pce_intensity_fetch(self._ctx, vals.ctypes.data if want_contour and vals.size else None, summ.ctypes.data))
        return {"values": vals, "frame_offsets": off, "summary": summ}

    def intensity(self, slices, params: IntensityParams = None, want_contour=True):
        """parselmouth ``Sound.to_intensity()`` of every slice: ``values[frame_offsets[i]:frame_offsets[i + 1]]`` is slice i's contour."""
        self.intensity_run(slices, params if params is not None else IntensityParams.praat())
        return self.intensity_fetch(want_contour)

    # ---------------------------------------------------------------- pydub.silence
    def silence_run(self, slices, rms_max, min_silence_len: int = 1000, seek_step: int = 1, channels: int = 1):
        """Enqueue pydub's ``detect_silence`` over ``slices`` (``pce_silence_run``).  ``rms_max``: the integer threshold ``T`` of every slice
        (``hostrules.silence_rms_max``), a scalar or one value per slice.  With ``channels`` > 1 the uploaded clips are interleaved streams,
        the upload's rate is the frame rate and slice bounds are in interleaved samples."""
        s = self._slices(slices)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(rms_max, dtype=np.int32), (len(s),)))
        self._si_n = len(s)
        params = SilenceParams(int(min_silence_len), int(seek_step), int(channels), 0)
        self._check(self._lib.pce_silence_run(self._ctx, C.byref(params), s.ctypes.data, t.ctypes.data, len(s)))

    def silence_fetch(self):
        """-> {"range_offsets": int64 [n + 1], "ranges": int32 [total, 2] (start_ms, end_ms), "len_ms": int32 [n], "status": int32 [n]}."""
        n = self._si_n
        off = np.zeros(n + 1, dtype=np.int64); len_ms = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.int32)
        self._check(self._lib.pce_silence_shape(self._ctx, off.ctypes.data, len_ms.ctypes.data, st.ctypes.data))
        ranges = np.zeros((int(off[-1]), 2), dtype=np.int32)
        self._check(self._lib.pce_silence_fetch(self._ctx, ranges.ctypes.data if ranges.size else None))
        return {"range_offsets": off, "ranges": ranges, "len_ms": len_ms, "status": st}

    def _silence(self, slices, min_silence_len, silence_thresh, seek_step, channels):
        from .hostrules import silence_rms_max
        thr = np.broadcast_to(np.asarray(silence_thresh, dtype=np.float64), (len(slices),))
        self.silence_run(slices, [silence_rms_max(t) for t in thr], min_silence_len, seek_step, channels)
        res = self.silence_fetch()
        off = res["range_offsets"]
        return [res["ranges"][off[i]:off[i + 1]].tolist() for i in range(len(slices))], res["len_ms"].tolist()

    def detect_silence(self, slices, min_silence_len=1000, silence_thresh=-16, seek_step=1, channels=1):
        """``pydub.silence.detect_silence`` of every slice -> per slice, the list of ``[start_ms, end_ms]`` silent ranges.
        ``silence_thresh`` (dBFS): a scalar or one value per slice."""
        return self._silence(slices, min_silence_len, silence_thresh, seek_step, channels)[0]

    def detect_nonsilent(self, slices, min_silence_len=1000, silence_thresh=-16, seek_step=1, channels=1):
        """``pydub.silence.detect_nonsilent`` of every slice -> per slice, the list of ``[start_ms, end_ms]`` nonsilent ranges."""
        from .hostrules import nonsilent_from_silent
        silent, len_ms = self._silence(slices, min_silence_len, silence_thresh, seek_step, channels)
        return [nonsilent_from_silent(r, n) for r, n in zip(silent, len_ms)]

    def split_on_silence(self, slices, min_silence_len=1000, silence_thresh=-16, seek_step=1, keep_silence=100, channels=1):
        """``pydub.silence.split_on_silence`` of every slice -> (per slice, the ``[start_ms, end_ms]`` of its chunks; per slice, their
        ``(begin, end)`` frame ranges relative to the slice, ``hostrules.pydub_slice_frames``: frames at or beyond the slice's length are
        pydub's silence padding)."""
        from .hostrules import nonsilent_from_silent, pydub_slice_frames, split_ranges
        s = self._slices(slices)
        silent, lens = self._silence(s, min_silence_len, silence_thresh, seek_step, channels)
        ms, frames = [], []
        for i, len_ms in enumerate(lens):
            n_frames = int(s["end"][i] - s["begin"][i]) // int(channels)
            cut = split_ranges(nonsilent_from_silent(silent[i], len_ms), keep_silence, len_ms)
            ms.append(cut)
            frames.append([pydub_slice_frames(n_frames, self.rate, a, b) for a, b in cut])
        return ms, frames

    def stats_enqueue(self, slot: int = 0):
        """Queue the device-to-host copies of the last energy / LUFS / pitch-summary results behind their
        runs and return at once; ``stats_wait(slot)`` collects them.  Two slots: the next batch can be
        launched before this one's numbers are read."""
        self._stat_n = getattr(self, "_stat_n", {})
        self._stat_n[slot] = (getattr(self, "_en_n", None), getattr(self, "_lu_n", None),
                              len(self._pi_slices) if getattr(self, "_pi_slices", None) is not None else None)
        self._check(self._lib.pce_stats_enqueue(self._ctx, int(slot)))

    def stats_wait(self, slot: int = 0):
        """-> dict(energy=ENERGY_DTYPE[n] | None, lufs=(values, status) | None, pitch=SUMMARY_DTYPE[n] | None)."""
        en_n, lu_n, pi_n = self._stat_n[slot]
        en = np.zeros(en_n, dtype=ENERGY_DTYPE) if en_n is not None else None
        lu = np.zeros(lu_n, dtype=np.float64) if lu_n is not None else None
        st = np.zeros(lu_n, dtype=np.int32) if lu_n is not None else None
        pi = np.zeros(pi_n, dtype=SUMMARY_DTYPE) if pi_n is not None else None
        self._check(self._lib.pce_stats_wait(self._ctx, int(slot), en.ctypes.data if en is not None else None,
                                             lu.ctypes.data if lu is not None else None, st.ctypes.data if st is not None else None,
                                             pi.ctypes.data if pi is not None else None))
        return {"energy": en, "lufs": (lu, st) if lu is not None else None, "pitch": pi}

    def stft_db_run(self, n_fft: int = 1024, hop: int = 256):
        self._check(self._lib.pce_stft_db_run(self._ctx, int(n_fft), int(hop)))

    def stft_db_fetch(self, clip: int) -> np.ndarray:
        nb = C.c_int32(); nf = C.c_int32()
        self._check(self._lib.pce_stft_db_shape(self._ctx, int(clip), C.byref(nb), C.byref(nf)))
        out = np.zeros((nb.value, nf.value), dtype=np.float32)
        self._check(self._lib.pce_stft_db_fetch(self._ctx, int(clip), out.ctypes.data))
        return out

    def stft_db_device(self):
        p = C.c_void_p(); n = C.c_int64()
        self._check(self._lib.pce_stft_db_device(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---------------------------------------------------------------- sample-rate conversion
    def resample(self, target_rate: int, filter=None):
        """Resample the resident batch to ``target_rate`` (polyphase, scipy.signal.resample_poly's filter design).  ``filter``: a caller-made
        ``(up, down, taps, n_pre_remove)`` for ``pce_resample_run`` in place of that design (``target_rate`` must be rate * up / down)."""
        from .hostrules import resample_filter
        if filter is None and target_rate == self.rate:
            return self
        up, down, taps, n_pre_remove = filter if filter is not None else resample_filter(self.rate, target_rate)
        if self.rate * up != target_rate * down:
            raise ValueError(f"{self.rate} Hz * {up} / {down} is not {target_rate} Hz")
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        self._check(self._lib.pce_resample_run(self._ctx, up, down, taps.ctypes.data, len(taps), n_pre_remove))
        off = np.zeros(len(self.clip_lengths) + 1, dtype=np.int64); rate = C.c_int32()
        self._check(self._lib.pce_download_pcm_s16(self._ctx, None, off.ctypes.data, C.byref(rate)))
        self.rate, self.offsets, self.clip_lengths = rate.value, off, np.diff(off)
        return self

    def download(self):
        """The resident batch as a list of int16 arrays."""
        pcm = np.zeros(max(int(self.offsets[-1]), 1), dtype=np.int16)
        self._check(self._lib.pce_download_pcm_s16(self._ctx, pcm.ctypes.data, None, None))
        return [pcm[self.offsets[i]:self.offsets[i + 1]].copy() for i in range(len(self.clip_lengths))]

    # ---------------------------------------------------------------- whisper front end
    def logmel_run(self, n_mels: int = 80):
        self._n_mels = int(n_mels)
        self._check(self._lib.pce_logmel_run(self._ctx, int(n_mels)))

    def logmel_run_at(self, n_mels: int, start_frames):
        """The 30 s window that starts ``start_frames[clip]`` frames (10 ms each) into every clip, as ``whisper.transcribe``
        slices the log-mel of the whole recording at its seek position."""
        sf = np.ascontiguousarray(start_frames, dtype=np.int64)
        self._check(self._lib.pce_logmel_run_at(self._ctx, int(n_mels), sf.ctypes.data))
        self._n_mels = int(n_mels)

    def logmel_fetch(self, clip: int) -> np.ndarray:
        out = np.zeros((self._n_mels, 3000), dtype=np.float32)
        self._check(self._lib.pce_logmel_fetch(self._ctx, int(clip), out.ctypes.data))
        return out

    def selftest_logmel_image(self, clip: int) -> np.ndarray:
        """The 16-bit time-major image ``[3002][n_mels]`` the conv stem reads, as the last ``logmel_run`` / ``logmel_run_at`` left it
        (bit patterns of the context's operand type; rows 0 and 3001 are the stem's zero padding).  Read-only."""
        out = np.zeros((3002, getattr(self, "_n_mels", 128)), dtype=np.uint16)
        self._check(self._lib.pce_selftest_logmel_image(self._ctx, int(clip), out.ctypes.data))
        return out

    # ---------------------------------------------------------------- operand type of the Whisper / BERT products
    def whisper_set_operands(self, kind: str):
        """``"fp16"`` (default: the reference's own arithmetic, openai-whisper's fp16=True) or ``"bf16"``.  The two builds keep
        separate state: select BEFORE loading weights / running the log-mel, and load again after switching."""
        code = {"bf16": 0, "fp16": 1, "fp16-resid16": 2}[str(kind).lower()]       # fp16-resid16: fp16 operands AND an fp16 residual stream in the batched encoder
        self._check(self._lib.pce_whisper_set_operands(self._ctx, code))

    @property
    def whisper_operands(self) -> str:
        code = self._lib.pce_whisper_get_operands(self._ctx)
        if code < 0:
            self._check(code)
        return {0: "bf16", 1: "fp16", 2: "fp16-resid16"}.get(code, f"mode-{code}")

    def _op_dtype(self):
        import torch
        return torch.bfloat16 if self.whisper_operands == "bf16" else torch.float16

    def whisper_load(self, dims: dict, weights: np.ndarray):
        """``dims``: n_mels, n_ctx, n_state, n_head, n_layer; ``weights``: float32 blob in the order of include/pce.h."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        self._wdims = WhisperDims(dims["n_mels"], dims["n_ctx"], dims["n_state"], dims["n_head"], dims["n_layer"])
        self._check(self._lib.pce_whisper_load(self._ctx, C.byref(self._wdims), w.ctypes.data, w.size))

    def whisper_encode_run(self):
        self._check(self._lib.pce_whisper_encode_run(self._ctx))
        self._n_encoded = len(self.clip_lengths)

    def whisper_num_encoded(self) -> int:
        return getattr(self, "_n_encoded", 0)

    def whisper_sample_keys(self, keys=None):
        """``pce_whisper_sample_keys``: the ids temperature sampling keys its noise by, one per clip of the encoded batch (None: back to
        batch positions).  They last until the next :meth:`whisper_encode_run`."""
        if keys is None or len(keys) == 0:
            self._check(self._lib.pce_whisper_sample_keys(self._ctx, None, 0)); return
        k = np.ascontiguousarray(np.asarray(keys, dtype=np.int64) & 0x7FFFFFFF, dtype=np.int32)
        self._check(self._lib.pce_whisper_sample_keys(self._ctx, k.ctypes.data, int(k.size)))

    def selftest_gemm(self, A, B, bias=None, epilogue: int = 0, rows_per_clip: int = 1, vt_sp: int = 0):
        """C = epilogue(A B^T + bias) on the persistent 256 x 256 GEMM kernel; A [M][K], B [N][K] float arrays (rounded to bf16 here) ->
        float32 result decoded from bf16 ([M][N], or [clips][N][vt_sp] for the transposed epilogue 2).  ``epilogue`` >= 256 (a multiple of 256, < N)
        is the split launch: returns (row-major [M][epilogue], transposed image [clips][N - epilogue][vt_sp])."""
        import torch
        a = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(self._op_dtype()).contiguous()
        b = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32)).to(self._op_dtype()).contiguous()
        M, K = a.shape; N = b.shape[0]
        if 16 <= epilogue <= 19:                                    # the tiled / few-row kernels behind launch_gemm (see pce_selftest_gemm)
            f32 = epilogue == 19
            outb = np.zeros(M * N, dtype=np.float32) if f32 else torch.zeros(M * N, dtype=self._op_dtype())
            bvv = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
            self._check(self._lib.pce_selftest_gemm(self._ctx, a.view(torch.int16).numpy().ctypes.data, b.view(torch.int16).numpy().ctypes.data,
                                                    bvv.ctypes.data if bvv is not None else None, M, N, K, int(epilogue), 1, 0,
                                                    outb.ctypes.data if f32 else outb.view(torch.int16).numpy().ctypes.data))
            return outb.reshape(M, N) if f32 else outb.float().numpy().reshape(M, N)
        split = epilogue if epilogue >= 256 else 0
        n_out = (M // rows_per_clip) * N * vt_sp if epilogue == 2 else M * split + (M // rows_per_clip) * (N - split) * vt_sp if split else M * N
        out = torch.zeros(n_out, dtype=self._op_dtype())
        bv = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        self._check(self._lib.pce_selftest_gemm(self._ctx, a.view(torch.int16).numpy().ctypes.data, b.view(torch.int16).numpy().ctypes.data,
                                                bv.ctypes.data if bv is not None else None, M, N, K, int(epilogue), int(rows_per_clip), int(vt_sp),
                                                out.view(torch.int16).numpy().ctypes.data))
        res = out.float().numpy()
        if split:
            return res[:M * split].reshape(M, split), res[M * split:].reshape(M // rows_per_clip, N - split, vt_sp)
        return res.reshape(M // rows_per_clip, N, vt_sp) if epilogue == 2 else res.reshape(M, N)

    def selftest_gemm_resid(self, A, B, bias, resid):
        """``pce_selftest_gemm_resid``: the persistent 256 x 256 GEMM with its residual epilogue, in place as the encoder runs it.  A [M][K], B [N][K]
        float arrays (rounded to the operand type here), resid [M][N] uint16 bit patterns of the operand type -> uint16 bit patterns of
        r16(resid + r16(A B^T + bias))."""
        import torch
        a = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(self._op_dtype()).contiguous()
        b = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32)).to(self._op_dtype()).contiguous()
        M, K = a.shape; N = b.shape[0]
        out = np.array(resid, dtype=np.uint16, order="C", copy=True)
        if out.shape != (M, N):
            raise ValueError("resid must be [M][N]")
        bv = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        self._check(self._lib.pce_selftest_gemm_resid(self._ctx, a.view(torch.int16).numpy().ctypes.data, b.view(torch.int16).numpy().ctypes.data,
                                                      bv.ctypes.data if bv is not None else None, out.ctypes.data, M, N, K))
        return out

    def selftest_attention(self, q, k, v, causal: bool = False, mode: int = 0):
        """softmax(q k^T / 8) v per (clip, head) on the attention kernel; q [clips][q_len][heads*64], k / v [clips][k_len][heads*64] float
        arrays (rounded to bf16 here).  mode 0: as the engine runs it, 1: exact path only.  Returns (out float32 decoded
        from bf16, number of workgroups that fell back to the exact path)."""
        import torch
        tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self._op_dtype()).contiguous() for x in (q, k, v))
        clips, q_len, hd = tq.shape
        k_len = tk.shape[1]
        assert hd % 64 == 0 and tk.shape == tv.shape == (clips, k_len, hd)
        out = torch.zeros_like(tq)
        fb = C.c_int32(0)
        self._check(self._lib.pce_selftest_attention(self._ctx, tq.view(torch.int16).numpy().ctypes.data, tk.view(torch.int16).numpy().ctypes.data,
                                                     tv.view(torch.int16).numpy().ctypes.data, clips, hd // 64, q_len, k_len, int(bool(causal)), int(mode),
                                                     out.view(torch.int16).numpy().ctypes.data, C.addressof(fb)))
        return out.float().numpy(), int(fb.value)

    def selftest_attention_ragged(self, q, k, v, q_len, k_len, out, causal: bool = False, mode: int = 0) -> int:
        """``pce_selftest_attention_ragged``: the attention kernel through the product's launch with per-clip lengths.  q [sum q_len][heads * 64],
        k / v [sum k_len][heads * 64] and out [rows >= sum q_len][heads * 64] are uint16 bit patterns of the context's operand type; out is read and
        updated in place.  Returns the number of workgroups that fell back to the exact path."""
        u = lambda x: self._u16(x)
        q, k, v, out = u(q), u(k), u(v), u(out)
        ql, kl = np.ascontiguousarray(q_len, dtype=np.int32), np.ascontiguousarray(k_len, dtype=np.int32)
        hd = q.shape[1]
        assert hd % 64 == 0 and k.shape == v.shape == (int(kl.sum()), hd) and q.shape[0] == int(ql.sum()) and out.shape[1] == hd and ql.size == kl.size
        fb = C.c_int32(0)
        self._check(self._lib.pce_selftest_attention_ragged(self._ctx, q.ctypes.data, k.ctypes.data, v.ctypes.data, int(ql.size), hd // 64, ql.ctypes.data,
                                                            kl.ctypes.data, int(bool(causal)), int(mode), out.ctypes.data, int(out.shape[0]), C.addressof(fb)))
        return int(fb.value)

    @staticmethod
    def _u16(x):
        assert isinstance(x, np.ndarray) and x.dtype == np.uint16 and x.flags["C_CONTIGUOUS"], getattr(x, "dtype", None)
        return x

    def selftest_attn1(self, form: int, heads: int, q, k, v, length, out, k_row0=None, skip=None, span: int = 0):
        """``pce_selftest_attn1``: one launch of the single-query attention kernels as a decoding step makes it.  form 0: k_cross_attn1w over given
        keys (q [n][d], k key rows, v the whole V^T image [n][d][span], length = keys per clip, k_row0 = first key row per clip); form 1: the same
        kernel appending (q = q | k | v [n][3 d], k cache [n][span][d], v = V^T cache [n][d][512], length = position); form 2: k_self_attn1w (as
        form 1, v = row-major cache [n][span][d]).  All arrays are uint16 bit patterns of the context's operand type; out [n][d], and in forms 1 / 2
        k and v, are read and updated in place."""
        q, k, v, out = self._u16(q), self._u16(k), self._u16(v), self._u16(out)
        i32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32)
        ln, r0, sk = i32(length), i32(k_row0), i32(skip)
        n = ln.size
        assert (r0 is None or r0.size == n) and (sk is None or sk.size == n)
        ptr = lambda x: None if x is None else x.ctypes.data
        self._check(self._lib.pce_selftest_attn1(self._ctx, int(form), int(n), int(heads), q.ctypes.data, q.size, k.ctypes.data, k.size, v.ctypes.data,
                                                 v.size, ptr(r0), ln.ctypes.data, ptr(sk), int(span), out.ctypes.data, out.size))

    def selftest_align_matrix(self, heads: int, q, k, t_len, f_len, heads_sel, w_soft, w_norm, cost, split: int = 0, sot_len: int = 3,
                              medfilt_width: int = 7, qk_scale: float = 1.0, k_rows=None):
        """``pce_selftest_align_matrix``: the forced alignment's k_align_scores -> k_align_colnorm -> k_align_cost through the launches
        ``pce_whisper_align_run`` makes.  q [n][T_pad][heads * 64] and k [n][k_rows][heads * 64] are uint16 bit patterns of the context's operand type
        (T_pad: the longest t_len rounded up to 16); heads_sel lists the selected heads, launched in one go (split 0 or len(heads_sel)) or as two
        layers (the first ``split``, then the rest).  w_soft / w_norm (float32, [n][n_sel][T_pad][F_pad], F_pad: the longest f_len rounded up to 64)
        and cost (float64, [n][max t_len - sot_len - 1][F_pad]) are read and updated in place.  The kernel scales its scores by
        float32(0.125) * float32(qk_scale).  k_rows: the key rows per clip where k is not given as [n][k_rows][.]."""
        q, k = self._u16(q), self._u16(k)
        for x, dt in ((w_soft, np.float32), (w_norm, np.float32), (cost, np.float64)):
            assert isinstance(x, np.ndarray) and x.dtype == dt and x.flags["C_CONTIGUOUS"], getattr(x, "dtype", None)
        tl, fl, hs = (np.ascontiguousarray(x, dtype=np.int32) for x in (t_len, f_len, heads_sel))
        n = tl.size
        if k_rows is None:
            assert k.ndim == 3 and k.shape[0] == n
            k_rows = k.shape[1]
        assert fl.size == n
        self._check(self._lib.pce_selftest_align_matrix(self._ctx, int(n), int(heads), q.ctypes.data, q.size, k.ctypes.data, k.size, int(k_rows),
                                                        tl.ctypes.data, fl.ctypes.data, hs.ctypes.data, int(hs.size), int(split), int(sot_len),
                                                        int(medfilt_width), float(qk_scale), w_soft.ctypes.data, w_soft.size, w_norm.ctypes.data,
                                                        w_norm.size, cost.ctypes.data, cost.size))

    def selftest_decode_rules(self, form: int, n_vocab: int, logits, token_lists, sample_begin, eot: int, timestamp_begin: int, vocab_mask, out_tok, out_lp,
                              probe_prob=None, max_initial_timestamp_index=None, temperature: float = 0.0, seed: int = 0, probe_token: int = -1,
                              sample_keys=None, pad_token: int = 0, t_cap: int = 448, max_new: int = 0, table=None, loop_state=None):
        """``pce_selftest_decode_rules``: k_decode_rules (and, form 1, k_step_advance) on host arrays through the decoding calls' own launches.
        logits: float32 [steps][n][ld], ld = n_vocab rounded up to 128; ``sample_begin``: int or one per sequence.  form 0: one step over the
        sequences padded with ``pad_token``; out_tok (int32) / out_lp / probe_prob (float32) [>= n] are read and updated in place.  form 1: ``steps``
        loop steps at pitch ``t_cap``; out_tok / out_lp [n][max_new], table int32 [n][t_cap] and loop_state int32 [10 n + max_new + 1]
        (len | ended | ct [8][n] | n_ended | step counter) are read and updated in place."""
        for x, dt in ((logits, np.float32), (out_tok, np.int32), (out_lp, np.float32), (probe_prob, np.float32), (table, np.int32), (loop_state, np.int32)):
            assert x is None or (isinstance(x, np.ndarray) and x.dtype == dt and x.flags["C_CONTIGUOUS"]), getattr(x, "dtype", None)
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists] + [np.zeros(0, np.int32)]), dtype=np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        n = len(token_lists)
        rules = WhisperDecodeRules(int(eot), int(timestamp_begin), -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), 0)
        vm = np.ascontiguousarray(vocab_mask, dtype=np.uint8)
        sb = None if np.isscalar(sample_begin) else np.ascontiguousarray(sample_begin, dtype=np.int32)
        keys = None if sample_keys is None else np.ascontiguousarray(sample_keys, dtype=np.int32)
        assert (sb is None or sb.size == n) and (keys is None or keys.size == n) and out_tok.size == out_lp.size and (probe_prob is None or probe_prob.size == out_tok.size)
        steps = logits.shape[0] if logits.ndim == 3 else 1
        ptr = lambda x: None if x is None else x.ctypes.data
        size = lambda x: 0 if x is None else x.size
        self._check(self._lib.pce_selftest_decode_rules(self._ctx, int(form), n, int(n_vocab), int(steps), logits.ctypes.data, logits.size, toks.ctypes.data,
                                                        off.ctypes.data, int(pad_token), int(t_cap), ptr(sb), int(sample_begin) if sb is None else 0, C.byref(rules),
                                                        vm.ctypes.data, vm.size, float(temperature), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF,
                                                        int(probe_token), ptr(keys), int(max_new), out_tok.ctypes.data, out_lp.ctypes.data, ptr(probe_prob),
                                                        out_tok.size, ptr(table), size(table), ptr(loop_state), size(loop_state)))

    def selftest_xattn(self, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, k_len, heads: int, workgroups_per_clip: int = 0):
        """One layer of the encoder-output cross-attention of a decoding step (``pce_selftest_xattn``): resid [n][d], E [n][k_cap][d], weights [d][d]
        float arrays (weights and E rounded to the context's operand type here) -> (out [n][d] float32 decoded from the 16-bit result, and the
        ROUNDED wq / wk / wv / E as float32: what the kernels really multiplied, for an exact restatement)."""
        import torch
        dt = self._op_dtype()
        r16 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).contiguous()
        tq, tk, tv, tE = r16(wq), r16(wk), r16(wv), r16(E)
        n, k_cap, d = tE.shape
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        res, lw, lb, vq, vv = f32(resid), f32(ln_w), f32(ln_b), f32(bq), f32(bv)
        kl = np.ascontiguousarray(k_len, dtype=np.int32)
        out = torch.zeros((n, d), dtype=dt)
        ptr = lambda t: t.view(torch.int16).numpy().ctypes.data
        self._check(self._lib.pce_selftest_xattn(self._ctx, res.ctypes.data, lw.ctypes.data, lb.ctypes.data, ptr(tq), vq.ctypes.data, ptr(tk), ptr(tv), vv.ctypes.data,
                                                 ptr(tE), kl.ctypes.data, int(n), int(k_cap), int(d), int(heads), int(workgroups_per_clip), ptr(out)))
        return out.float().numpy(), tq.float().numpy(), tk.float().numpy(), tv.float().numpy(), tE.float().numpy()

    def selftest_xattn_stages(self, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, k_len, heads: int, out, qp_hi, qp_lo, u_part, ml_part, skip=None,
                              workgroups_per_clip: int = 0) -> int:
        """``pce_selftest_xattn_stages``: one layer of the encoder-output cross-attention through the product's launch, with what lies between its three
        kernels.  wq / wk / wv [d][d], E [n][k_cap][d], out [n][d] and qp_hi / qp_lo [n][R][d] (R = heads rounded up to 16) are uint16 bit patterns of the
        context's operand type; resid [n][d], ln_w / ln_b / bq / bv [d], u_part [n][4][R][d] and ml_part [n][4][R][2] float32.  out, qp_hi, qp_lo, u_part
        and ml_part are read and updated in place.  Returns nodes (2: pair nodes, 4: leaves): the first n * nodes * R * d elements of u_part (n * nodes * R * 2
        of ml_part) are [n][nodes][R][.], the rest keeps the caller's values."""
        wq, wk, wv, E, out, qp_hi, qp_lo = (self._u16(x) for x in (wq, wk, wv, E, out, qp_hi, qp_lo))
        for x in (resid, ln_w, ln_b, bq, bv, u_part, ml_part):
            assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"], getattr(x, "dtype", None)
        n, k_cap, d = E.shape
        kl = np.ascontiguousarray(k_len, dtype=np.int32)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
        assert kl.size == n and (sk is None or sk.size == n) and resid.shape == (n, d) and wq.shape == wk.shape == wv.shape == (d, d)
        assert ln_w.size == ln_b.size == bq.size == bv.size == d and qp_hi.size == qp_lo.size
        nodes = C.c_int32(0)
        self._check(self._lib.pce_selftest_xattn_stages(self._ctx, resid.ctypes.data, ln_w.ctypes.data, ln_b.ctypes.data, wq.ctypes.data, bq.ctypes.data,
                                                        wk.ctypes.data, wv.ctypes.data, bv.ctypes.data, E.ctypes.data, E.size, kl.ctypes.data,
                                                        None if sk is None else sk.ctypes.data, int(n), int(k_cap), int(d), int(heads),
                                                        int(workgroups_per_clip), out.ctypes.data, out.size, qp_hi.ctypes.data, qp_lo.ctypes.data, qp_hi.size,
                                                        u_part.ctypes.data, u_part.size, ml_part.ctypes.data, ml_part.size, C.addressof(nodes)))
        return int(nodes.value)

    def selftest_gemm_tiled(self, epilogue: int, A, B, bias, M: int, N: int, K: int, C, lda: int, ldc: int, kernel: int = 0, a_batch: int = 0,
                            batch: int = 1, c_batch: int = 0, pos=None, v_col0: int = 0, rows_per_clip: int = 0, vt=None, vt_sp: int = 0) -> int:
        """``pce_selftest_gemm_tiled``: one launch of the tiled / few-row GEMM kernels as the product makes it.  A (flat) and B [N][K] are uint16 bit
        patterns of the context's operand type, bias [N] / pos [pos_T][N] float32; C (flat: uint16 for epilogues 0, 1, 4, else float32) and vt
        (flat uint16, epilogue 4) are read and updated in place.  Returns the kernel that ran (1 few-row, 2 128 x 256, 3 / 4 128 x 128)."""
        def arr(x, dt):
            assert isinstance(x, np.ndarray) and x.dtype == dt and x.flags["C_CONTIGUOUS"], (None if x is None else x.dtype, dt)
            return x
        f32 = epilogue in (2, 3, 5)
        A, B, C = arr(A, np.uint16), arr(B, np.uint16), arr(C, np.float32 if f32 else np.uint16)
        assert B.size == N * K
        bv = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        assert bv is None or bv.size == N
        pv = None if pos is None else np.ascontiguousarray(pos, dtype=np.float32)
        assert pv is None or pv.size % N == 0
        if vt is not None:
            arr(vt, np.uint16)
        used = np.zeros(1, dtype=np.int32)
        self._check(self._lib.pce_selftest_gemm_tiled(self._ctx, int(kernel), int(epilogue), A.ctypes.data, A.size, int(lda), int(a_batch), int(batch),
                                                      B.ctypes.data, None if bv is None else bv.ctypes.data, int(M), int(N), int(K), C.ctypes.data, C.size,
                                                      int(ldc), int(c_batch), None if pv is None else pv.ctypes.data, 0 if pv is None else pv.size // N,
                                                      int(v_col0), int(rows_per_clip), int(vt_sp), None if vt is None else vt.ctypes.data,
                                                      0 if vt is None else vt.size, used.ctypes.data))
        return int(used[0])

    def selftest_layernorm(self, form: int, x, w, b, eps: float = 1e-5, flags: int = 0, delta=None, delta2=None, want_copy: bool = False):
        """``pce_selftest_layernorm``: form 0 / 1 = k_layernorm to fp32 / 16-bit, form 2 + 3 o + s = k_add_layernorm (o: 16-bit output; s = 0 fp32
        stream, 1 fp32 in / 16-bit stream out, 2 16-bit stream).  x [rows][d]: float32, or uint16 bit patterns where the stream comes in 16-bit
        (s = 2); delta / delta2 uint16 bit patterns.  Returns (out, stream after the call or None, 16-bit copy or None); 16-bit arrays as uint16."""
        x = np.ascontiguousarray(x)
        rows, d = x.shape
        o, st = (form - 2) // 3, (form - 2) % 3
        assert x.dtype == (np.uint16 if form >= 2 and st == 2 else np.float32)
        out = np.zeros((rows, d), dtype=np.uint16 if form == 1 or (form >= 2 and o == 1) else np.float32)
        if form <= 1:
            resid = np.zeros((rows, d), dtype=np.float32) if flags & 2 else None
        else:
            resid = np.zeros((rows, d), dtype=np.float32 if st == 0 else np.uint16)
        cp = np.zeros((rows, d), dtype=np.uint16) if want_copy else None
        f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
        u = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.uint16)
        w, b, delta, delta2 = f(w), f(b), u(delta), u(delta2)
        ptr = lambda v: None if v is None else v.ctypes.data
        self._check(self._lib.pce_selftest_layernorm(self._ctx, int(form), rows, d, x.ctypes.data, ptr(delta), ptr(delta2), w.ctypes.data, b.ctypes.data,
                                                     float(eps), int(flags), out.ctypes.data, ptr(resid), ptr(cp)))
        return out, resid, cp

    def selftest_encoder_walk(self, pre_ln: bool, gemm_rule: int, key_bias: bool, heads: int, inner: int, n_layers: int, rows_per_item: int, vt_sp: int,
                              lens, eps: float, weights, stream, stages: dict, ln_in=None, d: int = None) -> bool:
        """``pce_selftest_encoder_walk``: the shared encoder layer walk on host arrays.  stream [M][d] float32 (M = len(lens) x rows_per_item), weights
        the layers' fp32 blob in the form's tensor order, ln_in [M][d] uint16 (post-LN).  ``stages``: the capture arrays of include/pce.h by name -- ln16
        [L][3][M][d], qk [L][M][2 d], vt [L][items][d][vt_sp], attn [L][M][d], hidden [L][M][inner] (uint16) and x32 [L][4][M][d] (float32) -- read and
        updated in place: what no launch writes keeps its values.  Returns whether every product was launched."""
        def arr(x, dt):
            assert isinstance(x, np.ndarray) and x.dtype == dt and x.flags["C_CONTIGUOUS"], (None if x is None else x.dtype, dt)
            return x
        stream, w = arr(stream, np.float32), arr(weights, np.float32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        d = stream.shape[-1] if d is None else d
        if ln_in is not None:
            assert arr(ln_in, np.uint16).size >= stream.size
        s = {k: arr(stages[k], np.float32 if k == "x32" else np.uint16) for k in ("ln16", "qk", "vt", "attn", "hidden", "x32")}
        fit = C.c_int32(-1)
        self._check(self._lib.pce_selftest_encoder_walk(self._ctx, int(bool(pre_ln)), int(gemm_rule), int(bool(key_bias)), int(d), int(heads), int(inner), int(n_layers),
                                                        int(lens.size), int(rows_per_item), int(vt_sp), lens.ctypes.data, float(eps), w.ctypes.data, w.size,
                                                        stream.ctypes.data, stream.size, None if ln_in is None else ln_in.ctypes.data, s["ln16"].ctypes.data,
                                                        s["ln16"].size, s["qk"].ctypes.data, s["qk"].size, s["vt"].ctypes.data, s["vt"].size, s["attn"].ctypes.data,
                                                        s["attn"].size, s["hidden"].ctypes.data, s["hidden"].size, s["x32"].ctypes.data, s["x32"].size,
                                                        C.addressof(fit)))
        return bool(fit.value)

    def whisper_encode_fetch(self, clip: int) -> np.ndarray:
        out = np.zeros((1500, self._wdims.n_state), dtype=np.float32)
        self._check(self._lib.pce_whisper_encode_fetch(self._ctx, int(clip), out.ctypes.data))
        return out

    def whisper_decoder_load(self, dims: dict, weights: np.ndarray):
        w = np.ascontiguousarray(weights, dtype=np.float32)
        self._tdims = WhisperTextDims(dims["n_vocab"], dims["n_text_ctx"], dims["n_state"], dims["n_head"], dims["n_layer"])
        self._check(self._lib.pce_whisper_decoder_load(self._ctx, C.byref(self._tdims), w.ctypes.data, w.size))

    def whisper_align_run(self, token_lists, num_frames, sot_len: int, head_mask=None, medfilt_width: int = 7, qk_scale: float = 1.0):
        """Enqueue the forced alignment (decoder, cross-attention weights, DTW) without fetching anything."""
        toks = np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]).astype(np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        hm = None if head_mask is None else np.ascontiguousarray(head_mask, dtype=np.uint8)
        self._check(self._lib.pce_whisper_align_run(self._ctx, toks.ctypes.data, off.ctypes.data, nf.ctypes.data, int(sot_len),
                                                    hm.ctypes.data if hm is not None else None, int(medfilt_width), float(qk_scale)))

    def whisper_align_paths_enqueue(self, slot: int = 0):
        """Queue the device-to-host copies of every clip's DTW path of the last ``whisper_align_run`` (pinned staging, returns at once)."""
        n = C.c_int32(); stride = C.c_int32()
        self._check(self._lib.pce_whisper_align_paths_enqueue(self._ctx, int(slot), C.byref(n), C.byref(stride)))
        self._al_slot = getattr(self, "_al_slot", {}); self._al_slot[int(slot)] = (n.value, stride.value)

    def whisper_align_paths_wait(self, slot: int = 0):
        """-> (path_len[n], text_idx[n][stride], time_idx[n][stride]); row i holds path_len[i] steps."""
        n, stride = self._al_slot[int(slot)]
        pl = np.zeros(n, dtype=np.int32); ti = np.zeros((n, stride), dtype=np.int32); tj = np.zeros((n, stride), dtype=np.int32)
        self._check(self._lib.pce_whisper_align_paths_wait(self._ctx, int(slot), pl.ctypes.data, ti.ctypes.data, tj.ctypes.data))
        return pl, ti, tj

    def whisper_align(self, token_lists, num_frames, sot_len: int, head_mask=None, medfilt_width: int = 7, qk_scale: float = 1.0,
                      want_cost: bool = False):
        """Forced alignment of the given token sequences (one per clip, specials included) against the encoded audio.
        Returns per clip a dict(text_indices, time_indices[, cost]) -- openai-whisper ``find_alignment`` up to the DTW."""
        toks = np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]).astype(np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        hm = None if head_mask is None else np.ascontiguousarray(head_mask, dtype=np.uint8)
        self._check(self._lib.pce_whisper_align_run(self._ctx, toks.ctypes.data, off.ctypes.data, nf.ctypes.data, int(sot_len),
                                                    hm.ctypes.data if hm is not None else None, int(medfilt_width), float(qk_scale)))
        out = []
        for i in range(len(token_lists)):
            nr = C.c_int32(); nc = C.c_int32()
            self._check(self._lib.pce_whisper_align_shape(self._ctx, i, C.byref(nr), C.byref(nc)))
            ti = np.zeros(nr.value + nc.value, dtype=np.int32); tj = np.zeros(nr.value + nc.value, dtype=np.int32); pl = C.c_int32()
            cost = np.zeros((nr.value, nc.value), dtype=np.float64) if want_cost else None
            self._check(self._lib.pce_whisper_align_fetch(self._ctx, i, ti.ctypes.data, tj.ctypes.data, C.byref(pl),
                                                          cost.ctypes.data if want_cost else None))
            r = {"text_indices": ti[:pl.value].copy(), "time_indices": tj[:pl.value].copy()}
            if want_cost:
                r["cost"] = cost
            out.append(r)
        return out

    def dtw(self, cost: np.ndarray):
        """DTW paths of a batch of [n_rows, n_cols] fp64 cost matrices -> list of (text_indices, time_indices)."""
        x = np.ascontiguousarray(cost, dtype=np.float64)
        if x.ndim == 2:
            x = x[None]
        b, n, m = x.shape
        pi = np.zeros((b, n + m), dtype=np.int32); pj = np.zeros((b, n + m), dtype=np.int32); pl = np.zeros(b, dtype=np.int32)
        self._check(self._lib.pce_dtw(self._ctx, x.ctypes.data, n, m, b, pi.ctypes.data, pj.ctypes.data, pl.ctypes.data))
        return [(pi[k, :pl[k]].copy(), pj[k, :pl[k]].copy()) for k in range(b)]

    def dtw_series(self, pairs, windows=None):
        """DTW of a batch of pairs of 1-D float64 series with the cost ``|a_i - b_j|`` formed on the device (``pce_dtw_series``: the
        dynamic programme of ``fastdtw``, candidates up / left / diagonal, first minimum).  ``pairs`` = [(a, b), ...]; ``windows`` = None
        or one entry per pair, each None or ``(lo, hi)``: int arrays giving every row of ``a`` its columns ``[lo, hi)``.
        -> [(path int32 [k, 2], dist float, status), ...]; status ``DTW_EMPTY``: a side is empty (no path, dist NaN), ``DTW_NO_PATH``:
        the window admits no path (dist inf)."""
        nb = len(pairs)
        if not nb:
            return []
        xs = [np.ascontiguousarray(p[0], dtype=np.float64).reshape(-1) for p in pairs]
        ys = [np.ascontiguousarray(p[1], dtype=np.float64).reshape(-1) for p in pairs]
        ao = np.zeros(nb + 1, dtype=np.int64); bo = np.zeros(nb + 1, dtype=np.int64)
        np.cumsum([len(x) for x in xs], out=ao[1:]); np.cumsum([len(y) for y in ys], out=bo[1:])
        a = np.concatenate(xs + [np.zeros(1)]); b = np.concatenate(ys + [np.zeros(1)])
        lo = hi = None
        if windows is not None and any(w is not None for w in windows):
            if len(windows) != nb:
                raise ValueError("windows: one entry (or None) per pair")
            lo = np.zeros(int(ao[-1]) + 1, dtype=np.int32); hi = np.zeros(int(ao[-1]) + 1, dtype=np.int32)
            for k, w in enumerate(windows):
                if w is None:
                    hi[ao[k]:ao[k + 1]] = len(ys[k])
                    continue
                wl = np.asarray(w[0]); wh = np.asarray(w[1])
                if wl.shape != (len(xs[k]),) or wh.shape != (len(xs[k]),):
                    raise ValueError(f"windows[{k}]: one [lo, hi) per row of the pair's first series")
                lo[ao[k]:ao[k + 1]] = wl; hi[ao[k]:ao[k + 1]] = wh
        oo = ao + bo
        pi = np.zeros(int(oo[-1]) + 1, dtype=np.int32); pj = np.zeros_like(pi)
        pl = np.zeros(nb, dtype=np.int32); dist = np.zeros(nb, dtype=np.float64); st = np.zeros(nb, dtype=np.int32)
        self._check(self._lib.pce_dtw_series(self._ctx, a.ctypes.data, ao.ctypes.data, b.ctypes.data, bo.ctypes.data,
                                             lo.ctypes.data if lo is not None else None, hi.ctypes.data if hi is not None else None, nb,
                                             pi.ctypes.data, pj.ctypes.data, pl.ctypes.data, dist.ctypes.data, st.ctypes.data))
        return [(np.stack([pi[oo[k]:oo[k] + pl[k]], pj[oo[k]:oo[k] + pl[k]]], axis=1), float(dist[k]), int(st[k])) for k in range(nb)]

    def _emission_args(self, emissions, n_frames):
        """The three ways ``ctc_align`` and ``wx_align`` take emissions (a list of ``[T, V]`` arrays, a ``DeviceEmissions``, one torch tensor
        ``[B, T_max, V]`` with ``n_frames``) -> ``(n, V, n_frames int32, row_start int64, pointer, on_device, keepalive)``."""
        keep = None
        if isinstance(emissions, DeviceEmissions):
            if n_frames is not None:
                raise ValueError("n_frames goes with a tensor of emissions; DeviceEmissions carries its own lengths")
            if emissions.engine is not self:
                raise ValueError("these emissions live in another engine's memory")
            emissions.check()
            n, V = len(emissions), emissions.n_cols
            nfr = np.ascontiguousarray(emissions.n_frames, dtype=np.int32); row_start = np.ascontiguousarray(emissions.row_start, dtype=np.int64)
            ptr, on_device = emissions.pointer, 1
        elif isinstance(emissions, (list, tuple)):
            if n_frames is not None:
                raise ValueError("n_frames goes with a tensor of emissions; a list carries its own lengths")
            rows = [np.ascontiguousarray(e, dtype=np.float32) for e in emissions]
            n = len(rows)
            if n and any(r.ndim != 2 or r.shape[1] != rows[0].shape[1] for r in rows):
                raise ValueError("emissions: [T, V] arrays with one vocabulary size")
            V = rows[0].shape[1] if n else 0
            nfr = np.array([r.shape[0] for r in rows], dtype=np.int32)
            row_start = np.zeros(n, dtype=np.int64)
            if n:
                row_start[1:] = np.cumsum(nfr[:-1], dtype=np.int64)
            keep = np.concatenate(rows + [np.zeros((1, V), dtype=np.float32)]) if n else None
            ptr, on_device = (keep.ctypes.data if n else None), 0
        else:
            e = emissions
            if not hasattr(e, "data_ptr") or e.dim() != 3 or str(e.dtype) != "torch.float32" or not e.is_contiguous():
                raise ValueError("emissions: a list of [T, V] float32 arrays or one contiguous float32 torch tensor [B, T_max, V]")
            n, t_max, V = (int(x) for x in e.shape)
            nfr = np.full(n, t_max, dtype=np.int32) if n_frames is None else np.ascontiguousarray(
                n_frames.cpu().numpy() if hasattr(n_frames, "cpu") else n_frames, dtype=np.int32).reshape(-1)
            if nfr.shape != (n,) or (n and (nfr.min() < 0 or nfr.max() > t_max)):
                raise ValueError("n_frames: one count in [0, T_max] per clip")
            if e.is_cuda and e.device.index not in (None, self.device):
                raise ValueError(f"emissions live on {e.device}, this engine on device {self.device}")
            row_start = np.arange(n, dtype=np.int64) * t_max
            keep = e
            ptr, on_device = e.data_ptr(), 1 if e.is_cuda else 0
            if on_device:
                import torch
                torch.cuda.current_stream(e.device).synchronize()      # the tensor's producer has finished before this engine's stream reads it
        return n, V, nfr, row_start, ptr, on_device, keep

    def _sequence_args(self, what, seqs, emissions, n_frames):
        """``_emission_args`` plus the label sequences of ``ctc_align`` / ``wx_align`` (``what`` names them in the error) ->
        ``(n, V, nfr, row_start, ptr, on_device, keep, labels int32 packed (+ 1 slack), toff int64 [n + 1], foff int64 [n + 1])``: a clip's labels
        are ``[toff[k], toff[k + 1])`` and its frames ``[foff[k], foff[k + 1])`` of the packed per-label and per-frame results."""
        sq = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in seqs]
        n, V, nfr, row_start, ptr, on_device, keep = self._emission_args(emissions, n_frames)
        if len(sq) != n:
            raise ValueError(f"{what}: one sequence per clip")
        toff = np.zeros(n + 1, dtype=np.int64); np.cumsum([len(t) for t in sq], out=toff[1:])
        foff = np.zeros(n + 1, dtype=np.int64); np.cumsum(nfr, out=foff[1:])
        return n, V, nfr, row_start, ptr, on_device, keep, np.concatenate(sq + [np.zeros(1, dtype=np.int32)]), toff, foff

    def ctc_align(self, emissions, targets, blank=0, n_frames=None, form="auto", return_path=True):
        """CTC forced alignment of a batch of clips (``pce_ctc_align``: the Viterbi pass of ``torchaudio.functional.forced_align`` over the
        ``2 L + 1`` blank-interleaved states of each transcript, bit-identical to its CPU restatement).  ``emissions``: a list of
        ``[T_c, V]`` float32 arrays of log-probabilities (packed and uploaded by the call), a ``DeviceEmissions`` of this engine's
        ``w2v_emissions`` (read in place), or ONE float32 contiguous torch tensor
        ``[B, T_max, V]`` with ``n_frames`` (valid frames per clip; default ``T_max`` for all): a ROCm tensor is read in place through its
        pointer, a CPU tensor is handed over as host memory (a process that uses ROCm tensors imports torch BEFORE it creates its first engine:
        torch ships its own copy of the HIP runtime, and the copy loaded first serves both).  ``targets``: one sequence of vocabulary indices per clip (none may be ``blank``).
        ``form``: ``"auto"`` | ``"register"`` | ``"general"`` (the register form holds ``CTC_REG_STATES`` states; asking it for more raises).
        -> one dict per clip: ``path`` int32 [T] (the label of every frame) and ``frame_score`` float32 [T] (``emissions[t, path[t]]``) unless
        ``return_path`` is false, ``tok_first`` / ``tok_last`` int32 [L] (first and last frame, inclusive, of every target), ``score``
        (numpy float32: the final alpha) and ``status`` (``CTC_OK``; ``CTC_EMPTY``: no targets or no frames; ``CTC_TOO_SHORT``: fewer frames
        than targets + adjacent repeats; ``CTC_NO_PATH``: the best score is -inf or NaN).  A clip without a path has ``path`` -1,
        ``frame_score`` NaN and token frames -1."""
        if form not in CTC_FORMS:
            raise ValueError(f"form: one of {sorted(CTC_FORMS)}")
        n, V, nfr, row_start, ptr, on_device, keep, tgt, toff, foff = self._sequence_args("targets", targets, emissions, n_frames)
        if not n:
            return []
        path = np.zeros(int(foff[-1]) + 1, dtype=np.int32) if return_path else None
        fsc = np.zeros(int(foff[-1]) + 1, dtype=np.float32) if return_path else None
        first = np.zeros(int(toff[-1]) + 1, dtype=np.int32); last = np.zeros_like(first)
        score = np.zeros(n, dtype=np.float32); status = np.zeros(n, dtype=np.int32)
        prm = CtcParams(int(blank), CTC_FORMS[form])
        self._check(self._lib.pce_ctc_align(self._ctx, C.c_void_p(ptr), on_device, row_start.ctypes.data, nfr.ctypes.data, V, tgt.ctypes.data,
                                            toff.ctypes.data, n, C.byref(prm), path.ctypes.data if return_path else None,
                                            fsc.ctypes.data if return_path else None, first.ctypes.data, last.ctypes.data,
                                            score.ctypes.data, status.ctypes.data))
        del keep
        out = []
        for k in range(n):
            d = {"tok_first": first[toff[k]:toff[k + 1]].copy(), "tok_last": last[toff[k]:toff[k + 1]].copy(),
                 "score": score[k], "status": int(status[k])}
            if return_path:
                d["path"] = path[foff[k]:foff[k + 1]].copy(); d["frame_score"] = fsc[foff[k]:foff[k + 1]].copy()
            out.append(d)
        return out

    def wx_align(self, emissions, tokens, blank=0, beam_width=2, n_frames=None, return_path=True, return_trellis=False):
        """whisperX's forced alignment of a batch of transcript segments (``pce_wx_align``: its trellis over the ``J`` characters of a segment with
        no interleaved blanks, the wildcard emission, the ``inf`` wedge and the beam-search back-track; the specification stands above
        ``pce_wx_align`` in ``include/pce.h``).  ``emissions``: as ``ctc_align`` takes them (a list of ``[T_c, V]`` float32 arrays, a
        ``DeviceEmissions`` read in place, or one contiguous float32 torch tensor ``[B, T_max, V]`` with ``n_frames``).  ``tokens``: one
        sequence of vocabulary indices per clip, ``-1`` for a wildcard (a character the dictionary lacks); at most ``WX_MAX_TOKENS``.
        ``beam_width``: 1 .. ``WX_MAX_BEAM`` (whisperx's default is 2; the width changes paths).
        -> one dict per clip: ``path_tok`` int32 [T] (the token INDEX of every frame) and ``path_lp`` float32 [T] (the log-probability the
        step consumed) unless ``return_path`` is false, ``score`` (numpy float32: the final trellis cell), ``status`` (``WX_OK``;
        ``WX_EMPTY``: no tokens or no frames; ``WX_NO_PATH``: the beams died out, e.g. more tokens than frames) and, if ``return_trellis``,
        ``trellis`` float32 [T, J].  A clip without a path has ``path_tok`` -1 and ``path_lp`` NaN."""
        n, V, nfr, row_start, ptr, on_device, keep, tok, toff, foff = self._sequence_args("tokens", tokens, emissions, n_frames)
        if not n:
            return []
        coff = np.zeros(n + 1, dtype=np.int64); np.cumsum(nfr.astype(np.int64) * np.diff(toff), out=coff[1:])
        path = np.zeros(int(foff[-1]) + 1, dtype=np.int32) if return_path else None
        plp = np.zeros(int(foff[-1]) + 1, dtype=np.float32) if return_path else None
        tre = np.zeros(int(coff[-1]) + 1, dtype=np.float32) if return_trellis else None
        score = np.zeros(n, dtype=np.float32); status = np.zeros(n, dtype=np.int32)
        prm = WxParams(int(blank), int(beam_width))
        self._check(self._lib.pce_wx_align(self._ctx, C.c_void_p(ptr), on_device, row_start.ctypes.data, nfr.ctypes.data, V, tok.ctypes.data,
                                           toff.ctypes.data, n, C.byref(prm), path.ctypes.data if return_path else None,
                                           plp.ctypes.data if return_path else None, tre.ctypes.data if return_trellis else None,
                                           score.ctypes.data, status.ctypes.data))
        del keep
        out = []
        for k in range(n):
            d = {"score": score[k], "status": int(status[k])}
            if return_path:
                d["path_tok"] = path[foff[k]:foff[k + 1]].copy(); d["path_lp"] = plp[foff[k]:foff[k + 1]].copy()
            if return_trellis:
                d["trellis"] = tre[coff[k]:coff[k + 1]].reshape(int(nfr[k]), int(toff[k + 1] - toff[k])).copy()
            out.append(d)
        return out

    def frame_energy_run(self, window: int, hop: int = None, requantize: bool = False):
        """Exact integer energy of every analysis window of every clip (k_frame_energy): frame k covers
        [k*hop, min(k*hop + window, n)); hop defaults to window (auditok's blocks)."""
        self._check(self._lib.pce_frame_energy_run(self._ctx, int(window), int(window if hop is None else hop), 1 if requantize else 0))

    def frame_energy_fetch(self, clip: int):
        """-> (sum_sq int64[n_frames], count int32[n_frames]) of one clip."""
        nf = C.c_int64()
        self._check(self._lib.pce_frame_energy_shape(self._ctx, int(clip), C.byref(nf)))
        ss = np.zeros(nf.value, dtype=np.int64); cnt = np.zeros(nf.value, dtype=np.int32)
        self._check(self._lib.pce_frame_energy_fetch(self._ctx, int(clip), ss.ctypes.data, cnt.ctypes.data))
        return ss, cnt

    def whisper_decode_step(self, token_lists, sample_begin: int, eot: int, timestamp_begin: int, vocab_mask, max_initial_timestamp_index=None):
        """One step of free-running decoding for every encoded clip -> next token ids (int32 [clips]).  ``vocab_mask``:
        uint8 [n_vocab], bit 0 = always suppressed, bit 1 = suppressed at the first sampled position."""
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]), dtype=np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        rules = WhisperDecodeRules(int(eot), int(timestamp_begin), -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), 0)
        vm = np.ascontiguousarray(vocab_mask, dtype=np.uint8)
        nxt = np.zeros(len(token_lists), dtype=np.int32); lp = np.zeros(len(token_lists), dtype=np.float32)
        self._check(self._lib.pce_whisper_decode_step(self._ctx, toks.ctypes.data, off.ctypes.data, int(sample_begin), C.byref(rules),
                                                      vm.ctypes.data, nxt.ctypes.data, lp.ctypes.data))
        self.last_decode_logprobs = lp
        return nxt

    def whisper_decode_step_ex(self, token_lists, sample_begin, eot: int, timestamp_begin: int, vocab_mask, max_initial_timestamp_index=None,
                               temperature: float = 0.0, seed: int = 0, probe_token: int = -1, no_cache: bool = False):
        """``whisper_decode_step`` with a prompt length per sequence (``sample_begin``: int or one per clip), sampling at a
        temperature (one draw from softmax(filtered logits / temperature), reproducible for a given ``seed``) and an
        optional probe of the unfiltered distribution at one token (``probe_token``: no_speech_prob when the prefixes end at
        <|startoftranscript|>).  -> (next ids int32 [clips], log-probabilities float32 [clips], probe float32 [clips] | None)."""
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]), dtype=np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        rules = WhisperDecodeRules(int(eot), int(timestamp_begin), -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), 0)
        vm = np.ascontiguousarray(vocab_mask, dtype=np.uint8)
        n = len(token_lists)
        sb = None if np.isscalar(sample_begin) else np.ascontiguousarray(sample_begin, dtype=np.int32)
        if sb is not None and sb.shape != (n,):
            raise ValueError("sample_begin: one prompt length per sequence")
        opts = WhisperDecodeOpts(sb.ctypes.data if sb is not None else None, int(sample_begin) if sb is None else 0, float(temperature),
                                 int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(probe_token), 1 if no_cache else 0)
        nxt = np.zeros(n, dtype=np.int32); lp = np.zeros(n, dtype=np.float32)
        pr = np.zeros(n, dtype=np.float32) if probe_token >= 0 else None
        self._check(self._lib.pce_whisper_decode_step_ex(self._ctx, toks.ctypes.data, off.ctypes.data, C.byref(rules), vm.ctypes.data, C.byref(opts),
                                                         nxt.ctypes.data, lp.ctypes.data, pr.ctypes.data if pr is not None else None))
        return nxt, lp, pr

    def whisper_decode_loop(self, token_lists, sample_begin, eot: int, timestamp_begin: int, vocab_mask, max_new: int,
                            max_initial_timestamp_index=None, temperature: float = 0.0, seed: int = 0, probe_token: int = -1,
                            no_cache: bool = False, check_every: int = 4):
        """The free-running loop on the device: prompts up once, at most ``max_new`` steps, results down once (the host only reads an
        "ended" counter every ``check_every`` steps).  -> (tokens int32 [clips][steps run], log-probabilities float32 [clips][steps run],
        probe float32 [clips] | None): what ``steps run`` consecutive ``whisper_decode_step_ex`` calls return, column by column."""
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]), dtype=np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        rules = WhisperDecodeRules(int(eot), int(timestamp_begin), -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), 0)
        vm = np.ascontiguousarray(vocab_mask, dtype=np.uint8)
        n = len(token_lists)
        sb = None if np.isscalar(sample_begin) else np.ascontiguousarray(sample_begin, dtype=np.int32)
        if sb is not None and sb.shape != (n,):
            raise ValueError("sample_begin: one prompt length per sequence")
        opts = WhisperDecodeOpts(sb.ctypes.data if sb is not None else None, int(sample_begin) if sb is None else 0, float(temperature),
                                 int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(probe_token), 1 if no_cache else 0)
        out = np.zeros((n, int(max_new)), dtype=np.int32); lp = np.zeros((n, int(max_new)), dtype=np.float32)
        pr = np.zeros(n, dtype=np.float32) if probe_token >= 0 else None
        steps = C.c_int32()
        self._check(self._lib.pce_whisper_decode_loop(self._ctx, toks.ctypes.data, off.ctypes.data, C.byref(rules), vm.ctypes.data, C.byref(opts),
                                                      int(max_new), int(check_every), out.ctypes.data, lp.ctypes.data, C.byref(steps),
                                                      pr.ctypes.data if pr is not None else None))
        return out[:, :steps.value], lp[:, :steps.value], pr

    def whisper_detect_language(self, sot: int, lang_begin: int, n_lang: int):
        """``pce_whisper_detect_language``: openai-whisper's ``detect_language`` for every encoded clip -- the decoder over
        <|startoftranscript|> alone, softmax over the ``n_lang`` language tokens ``lang_begin ..`` (every other token masked) and the
        arg-max.  -> (token ids int32 [clips], probabilities float32 [clips, n_lang]).  The next decoding call behaves as if this one
        had not been made."""
        n = self.whisper_num_encoded()
        ids = np.zeros(max(n, 0), dtype=np.int32); probs = np.zeros((max(n, 0), max(int(n_lang), 0)), dtype=np.float32)
        self._check(self._lib.pce_whisper_detect_language(self._ctx, int(sot), int(lang_begin), int(n_lang), ids.ctypes.data, probs.ctypes.data))
        return ids, probs

    # ---------------------------------------------------------------- probabilistic YIN (viewers)
    def pyin_run(self, plan, tables):
        """``plan`` / ``tables`` from ``visualisation.acoustic_analysis.pyin_plan``."""
        t = np.ascontiguousarray(tables, dtype=np.float64)
        self._check(self._lib.pce_pyin_run(self._ctx, C.byref(plan), t.ctypes.data, t.size))

    def pyin_fetch(self, clip: int):
        """-> (states int32 [n_frames], voiced_prob float64 [n_frames], status)."""
        nf = C.c_int64()
        self._check(self._lib.pce_pyin_shape(self._ctx, int(clip), C.byref(nf)))
        st = np.zeros(nf.value, dtype=np.int32); vp = np.zeros(nf.value, dtype=np.float64); status = C.c_int32()
        self._check(self._lib.pce_pyin_fetch(self._ctx, int(clip), st.ctypes.data, vp.ctypes.data, C.byref(status)))
        return st, vp, status.value

    def pyin_fetch_observations(self, clip: int):
        """``pce_pyin_fetch_observations`` (test hook): what ``k_pyin_frames`` left for ``clip`` -> dict of ``n``, ``status`` int32 [n_frames],
        ``voiced_prob``, ``log_unvoiced`` float64 [n_frames], ``bins`` int32 and ``log_probs`` float64 [n_frames, 512] (entries beyond ``n``: -1 / NaN)."""
        nf = C.c_int64()
        self._check(self._lib.pce_pyin_shape(self._ctx, int(clip), C.byref(nf)))
        o = {"n": np.zeros(nf.value, np.int32), "status": np.zeros(nf.value, np.int32), "voiced_prob": np.zeros(nf.value), "log_unvoiced": np.zeros(nf.value),
             "bins": np.full((nf.value, PYIN_MAX_TROUGHS), -1, np.int32), "log_probs": np.full((nf.value, PYIN_MAX_TROUGHS), np.nan)}
        self._check(self._lib.pce_pyin_fetch_observations(self._ctx, int(clip), *(o[k].ctypes.data for k in ("n", "status", "voiced_prob", "log_unvoiced", "bins", "log_probs"))))
        return o

    def selftest_pyin_viterbi(self, plan, tables, frame_off, n, log_unvoiced, bins, log_probs):
        """``pce_selftest_pyin_viterbi`` (test hook): ``k_pyin_viterbi`` on given observation lists (rows of 512 entries, the first ``n`` count) of
        clips ``frame_off[i] .. frame_off[i + 1]`` -> states int32 [frames]."""
        t = np.ascontiguousarray(tables, dtype=np.float64)
        off = np.ascontiguousarray(frame_off, dtype=np.int64); n = np.ascontiguousarray(n, dtype=np.int32)
        lu = np.ascontiguousarray(log_unvoiced, dtype=np.float64)
        b = np.ascontiguousarray(bins, dtype=np.int32); lp = np.ascontiguousarray(log_probs, dtype=np.float64)
        total = int(off[-1]) if off.size else 0
        if off.ndim != 1 or off.size < 2 or n.shape != (total,) or lu.shape != (total,) or b.shape != (total, PYIN_MAX_TROUGHS) or lp.shape != b.shape:
            raise ValueError("frame_off [clips + 1]; n, log_unvoiced [frames]; bins, log_probs [frames, 512]")
        states = np.zeros(total, dtype=np.int32)
        self._check(self._lib.pce_selftest_pyin_viterbi(self._ctx, C.byref(plan), t.ctypes.data, t.size, off.size - 1, off.ctypes.data, n.ctypes.data,
                                                        lu.ctypes.data, b.ctypes.data, lp.ctypes.data, states.ctypes.data))
        return states

    # ---------------------------------------------------------------- CREPE pitch tracking (evaluate_voice's F0 RMSE)
    def crepe_load(self, capacity_or_dims, weights):
        """``capacity_or_dims``: ``"full"``, ``"tiny"`` or six output widths; ``weights``: the flat float32 vector of
        ``crepe_weights.tensor_order`` (``crepe_weights.fold(state_dict)[1]`` / ``crepe_weights.load(path)[1]``) or a ``state_dict``."""
        from . import crepe_weights as CW
        c_out = CW.dims(capacity_or_dims)
        if isinstance(weights, dict):
            got, weights = CW.fold(weights)
            if tuple(got) != tuple(c_out):
                raise ValueError(f"CREPE state dict has widths {got}, {c_out} were asked for")
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        d = CrepeDims((C.c_int32 * 6)(*c_out), (C.c_int32 * 2)(0, 0))
        self._check(self._lib.pce_crepe_load(self._ctx, C.byref(d), w.ctypes.data, w.size))
        self.crepe_dims = tuple(c_out)

    def crepe(self, hop_length: int, fmin: float, fmax: float, decoder: str = "viterbi", frames_per_chunk: int = 4096,
              return_salience: bool = False):
        """``torchcrepe.predict(..., return_periodicity=True)`` without its dither, of every clip of the resident batch (which must be at
        16 kHz; ``hop_length`` in samples at that rate) -> per-clip lists ``(bins int32, f0 float64 Hz, periodicity float32[, salience
        float32 [n_frames, 360]])``.  ``decoder``: ``"viterbi"`` (torchcrepe's default) or ``"argmax"``.  Frames run ``frames_per_chunk`` at a
        time (torchcrepe's ``batch_size``); no result depends on it.  The caller masks ``f0[periodicity < threshold] = NaN``."""
        from . import crepe_weights as CW
        if decoder not in ("viterbi", "argmax"):
            raise ValueError('decoder: "viterbi" or "argmax" (the dithered decoders of torchcrepe are not offered)')
        lo, hi = CW.mask_range(fmin, fmax)
        plan = CrepePlan(int(hop_length), lo, hi, 0 if decoder == "viterbi" else 1, int(frames_per_chunk), 0)
        self._check(self._lib.pce_crepe_run(self._ctx, C.byref(plan)))
        bins, f0s, pers, sals = [], [], [], []
        for clip in range(len(self.clip_lengths)):
            nf = C.c_int64()
            self._check(self._lib.pce_crepe_shape(self._ctx, clip, C.byref(nf)))
            b = np.zeros(nf.value, dtype=np.int32); f = np.zeros(nf.value, dtype=np.float64); p = np.zeros(nf.value, dtype=np.float32)
            sal = np.zeros((nf.value, CW.PITCH_BINS), dtype=np.float32) if return_salience else None
            self._check(self._lib.pce_crepe_fetch(self._ctx, clip, b.ctypes.data, f.ctypes.data, p.ctypes.data,
                                                  sal.ctypes.data if return_salience else None))
            bins.append(b); f0s.append(f); pers.append(p); sals.append(sal)
        return (bins, f0s, pers, sals) if return_salience else (bins, f0s, pers)

    def selftest_crepe_layer(self, block: int, x16, w16, bias, scale, shift):
        """One CREPE block as the product launches it, on fp16 arrays: ``x16`` [n_frames, t_in, c_in], ``w16`` [c_out, taps, c_in] ->
        fp16 [n_frames, t_in / 2 (block 1: 128), c_out]."""
        x = np.ascontiguousarray(x16, dtype=np.float16); w = np.ascontiguousarray(w16, dtype=np.float16)
        n, t_in, c_in = x.shape; c_out = w.shape[0]
        b, sc, sh = (np.ascontiguousarray(a, dtype=np.float32) for a in (bias, scale, shift))
        out = np.zeros((n, 128 if block == 1 else t_in // 2, c_out), dtype=np.float16)
        self._check(self._lib.pce_selftest_crepe_layer(self._ctx, int(block), c_in, c_out, n, x.ctypes.data, w.ctypes.data, b.ctypes.data,
                                                       sc.ctypes.data, sh.ctypes.data, out.ctypes.data))
        return out

    def selftest_crepe_decode(self, salience, lo: int, hi: int, decoder: str = "viterbi"):
        """The device's decoding of a host salience [n_frames, 360] (one clip) -> (bins, f0, periodicity)."""
        s = np.ascontiguousarray(salience, dtype=np.float32)
        n = s.shape[0]
        b = np.zeros(n, dtype=np.int32); f = np.zeros(n, dtype=np.float64); p = np.zeros(n, dtype=np.float32)
        self._check(self._lib.pce_selftest_crepe_decode(self._ctx, s.ctypes.data, n, int(lo), int(hi), 0 if decoder == "viterbi" else 1,
                                                        b.ctypes.data, f.ctypes.data, p.ctypes.data))
        return b, f, p

    # ---------------------------------------------------------------- break-prediction token classifier
    def bert_load(self, dims: dict, weights: np.ndarray):
        """``weights``: float32 blob in ``bert_weights.tensor_order`` (``bert_weights.pack(model.state_dict(), dims)``)."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        self._bdims = BertDims(*(dims[k] for k in ("n_vocab", "n_pos", "n_type", "n_state", "n_head", "n_layer", "n_labels")))
        self._check(self._lib.pce_bert_load(self._ctx, C.byref(self._bdims), w.ctypes.data, w.size))

    def bert_run(self, token_lists):
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists] + [np.zeros(0, np.int32)]), dtype=np.int32)
        off = np.zeros(len(token_lists) + 1, dtype=np.int32); np.cumsum([len(t) for t in token_lists], out=off[1:])
        self._bert_lens = [len(t) for t in token_lists]
        self._check(self._lib.pce_bert_run(self._ctx, toks.ctypes.data, off.ctypes.data, len(token_lists)))

    def bert_fetch(self, seq: int):
        """-> (logits float32 [len][n_labels], labels int32 [len])."""
        n = self._bert_lens[seq]
        logits = np.zeros((n, self._bdims.n_labels), dtype=np.float32); labels = np.zeros(n, dtype=np.int32)
        self._check(self._lib.pce_bert_fetch(self._ctx, int(seq), logits.ctypes.data, labels.ctypes.data))
        return logits, labels

    def bert_token_classify(self, token_lists):
        self.bert_run(token_lists)
        return [self.bert_fetch(i) for i in range(len(token_lists))]

    # ---------------------------------------------------------------- wav2vec2 / MMS CTC acoustic model
    def w2v_load(self, model_or_config, weights=None):
        """Load a ``transformers`` ``Wav2Vec2ForCTC``: the model itself (its config and ``state_dict`` are packed here), or a config / a dims dict
        of ``w2v_weights.dims`` with ``weights`` = a ``state_dict`` or the flat float32 blob of ``w2v_weights.tensor_order``."""
        from . import w2v_weights as WW
        src = model_or_config
        if weights is None:
            if not hasattr(src, "state_dict"):
                raise ValueError("w2v_load: a model, or a config / dims with weights")
            weights, src = src.state_dict(), src.config
        model = model_or_config if src is not model_or_config else None
        dims = src if isinstance(src, dict) else WW.dims(src)
        w = WW.pack(weights, dims) if hasattr(weights, "keys") else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self._w2v_dims = W2vDims.of(dims)
        self._w2v_epoch += 1                                        # DeviceEmissions made before this call are stale
        self._w2v_held = None
        self._check(self._lib.pce_w2v_load(self._ctx, C.byref(self._w2v_dims), w.ctypes.data, w.size))
        if model is not None:      # which model object the selected operand build now holds (a weak reference: the engine does not keep it alive)
            self._w2v_held = (weakref.ref(model), self._lib.pce_whisper_get_operands(self._ctx))

    def w2v_holds(self, model) -> bool:
        """Did this engine's latest ``w2v_load`` load ``model`` (the same object; weights changed in place since are not seen) into the operand
        build now selected?  What ``ctc_emissions.engine_emissions`` asks before it loads."""
        held = self._w2v_held
        return held is not None and held[0]() is model and held[1] == self._lib.pce_whisper_get_operands(self._ctx)

    def w2v_emissions(self, window_s=30, context_s=2, windows_per_chunk=None, star=True) -> DeviceEmissions:
        """Frame-wise log-probabilities of the resident 16 kHz batch under the loaded model (``pce_w2v_run``), windowed as
        ``Aligners.ctc_emissions.hf_emissions`` windows them; ``star`` appends the zero ``<star>`` column.  ``windows_per_chunk``: windows per
        launch group (default: by ``PCE_W2V_IMAGE_BUDGET``); a window's emissions do not depend on it.  -> ``DeviceEmissions``."""
        window, context = int(window_s * 16000), int(context_s * 16000)
        if int(window / 16000 * 50) != int(window_s * 50) or int(context / 16000 * 50) != int(context_s * 50):
            raise ValueError("window_s / context_s: the whole samples they span must keep their frame counts (int(s * 50))")
        plan = W2vPlan(window, context, int(windows_per_chunk or 0), 1 if star else 0)
        self._w2v_epoch += 1                                        # the run may move or overwrite what earlier DeviceEmissions point to
        self._check(self._lib.pce_w2v_run(self._ctx, C.byref(plan)))
        return self._w2v_device_emissions(int(self._lib.pce_num_clips(self._ctx)))

    def _w2v_device_emissions(self, n: int) -> DeviceEmissions:
        ptr, rs, nf, nc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        self._check(self._lib.pce_w2v_device(self._ctx, C.byref(ptr), C.byref(rs), C.byref(nf), C.byref(nc)))
        row_start = np.ctypeslib.as_array(C.cast(rs, C.POINTER(C.c_int64)), shape=(n,)).copy() if n else np.zeros(0, np.int64)
        n_frames = np.ctypeslib.as_array(C.cast(nf, C.POINTER(C.c_int32)), shape=(n,)).copy() if n else np.zeros(0, np.int32)
        return DeviceEmissions(self, ptr.value or 0, row_start, n_frames, nc.value, self._w2v_epoch)

    def w2v_segment_emissions(self, segments, min_samples=400, segments_per_chunk=None, star=False) -> DeviceEmissions:
        """whisperX's emissions under the loaded model (``pce_w2v_run_segments``): ``segments`` = ``[(clip, begin, end)]``, samples
        ``[begin, end)`` of a clip of the resident 16 kHz batch; each segment runs ALONE (one of fewer than ``min_samples`` samples is followed
        by zeros up to that many), as ``Aligners.ctc_emissions.segment_emissions`` runs them.  ``segments_per_chunk``: segments per launch
        group (default: by ``PCE_W2V_IMAGE_BUDGET``); a segment's emissions do not depend on it, on the order or on its neighbours.
        -> ``DeviceEmissions`` indexed by segment, in the order given; ``wx_align`` / ``ctc_align`` read it in place."""
        segs = [(int(q), int(b), int(e)) for q, b, e in segments]
        arr = (W2vSegment * max(1, len(segs)))(*[W2vSegment(q, 0, b, e) for q, b, e in segs])
        plan = W2vSegPlan(int(min_samples), int(segments_per_chunk or 0), 1 if star else 0)
        self._w2v_epoch += 1                                        # the run may move or overwrite what earlier DeviceEmissions point to
        self._check(self._lib.pce_w2v_run_segments(self._ctx, arr, len(segs), C.byref(plan)))
        return self._w2v_device_emissions(len(segs))

    def w2v_segments_plan(self):
        """-> (chunks, rows computed, rows valid) of the latest ``w2v_segment_emissions`` (``pce_w2v_segments_plan``)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.pce_w2v_segments_plan(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def w2v_fetch(self, clip: int) -> np.ndarray:
        """-> float32 ``[n_frames][n_cols]``: one clip's emissions (or segment's) emissions of the last ``w2v_emissions`` / ``w2v_segment_emissions``."""
        nf, nc = C.c_int64(), C.c_int32()
        self._check(self._lib.pce_w2v_shape(self._ctx, int(clip), C.byref(nf), C.byref(nc)))
        out = np.zeros((nf.value, nc.value), dtype=np.float32)
        if out.size:
            self._check(self._lib.pce_w2v_fetch(self._ctx, int(clip), out.ctypes.data))
        return out

    def w2v_window_plan(self, n_samples: int, window_s=30, context_s=2):
        """-> (windows, frames kept) of one clip, as ``pce_w2v_run`` counts them (host arithmetic: ``pce_w2v_window_plan``)."""
        return w2v_window_plan(n_samples, window_s, context_s, self._lib)

    def selftest_w2v_wave(self, pcm, window: int, context: int, feat_norm: int, w, gamma, beta, bias=None, stride: int = 5):
        """``pce_selftest_w2v_wave``: the waveform layer over the windows of one int16 clip.  w [C][10] float32.  -> uint16 bits [windows][T0][C]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float32); gamma = np.ascontiguousarray(gamma, dtype=np.float32); beta = np.ascontiguousarray(beta, dtype=np.float32)
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        ch = w.shape[0]
        length = window + 2 * context
        t0 = (length - 10) // stride + 1 if length >= 10 else 0
        n_win = max(1, -(-len(pcm) // window))
        out = np.zeros((n_win, t0, ch), dtype=np.uint16)
        self._check(self._lib.pce_selftest_w2v_wave(self._ctx, pcm.ctypes.data, len(pcm), int(window), int(context), int(feat_norm), ch, int(stride),
                                                    w.ctypes.data, None if bias is None else bias.ctypes.data, gamma.ctypes.data, beta.ctypes.data,
                                                    out.ctypes.data))
        return out

    def selftest_w2v_lngelu(self, x_bits, w, b, eps: float = 1e-5, gelu: bool = True):
        """``pce_selftest_w2v_lngelu``: x uint16 bits [rows][C] -> uint16 bits [rows][C]."""
        x = np.ascontiguousarray(x_bits, dtype=np.uint16)
        w = np.ascontiguousarray(w, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
        out = np.zeros_like(x)
        self._check(self._lib.pce_selftest_w2v_lngelu(self._ctx, x.ctypes.data, x.shape[0], x.shape[1], w.ctypes.data, b.ctypes.data, float(eps),
                                                      1 if gelu else 0, out.ctypes.data))
        return out

    def selftest_w2v_posconv(self, x, w_bits, bias, groups: int):
        """``pce_selftest_w2v_posconv``: x float32 [windows][T][d], w uint16 bits [d][128][d / groups] -> float32 [windows][T][d]."""
        x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w_bits, dtype=np.uint16); bias = np.ascontiguousarray(bias, dtype=np.float32)
        n_win, t, d = x.shape
        if w.shape != (d, 128, d // groups):
            raise ValueError("w: [d][128][d / groups]")
        out = np.zeros_like(x)
        self._check(self._lib.pce_selftest_w2v_posconv(self._ctx, x.ctypes.data, n_win, t, d, int(groups), w.ctypes.data, bias.ctypes.data, out.ctypes.data))
        return out

    def selftest_w2v_wave_segments(self, pcm, segments, feat_norm: int, w, gamma, beta, bias=None, stride: int = 5, min_samples: int = 400):
        """``pce_selftest_w2v_wave_segments``: the waveform layer over ``segments`` = ``[(begin, end)]`` of one int16 clip, each with its own
        frame count.  -> (uint16 bits [segments][slot][C], frames per segment); rows behind a segment's frames are zero."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float32); gamma = np.ascontiguousarray(gamma, dtype=np.float32); beta = np.ascontiguousarray(beta, dtype=np.float32)
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        seg = np.ascontiguousarray(segments, dtype=np.int64).reshape(-1, 2)
        frames = [(max(int(e - b), int(min_samples)) - 10) // stride + 1 for b, e in seg]
        out = np.zeros((len(seg), max(frames), w.shape[0]), dtype=np.uint16)
        self._check(self._lib.pce_selftest_w2v_wave_segments(self._ctx, pcm.ctypes.data, len(pcm), seg.ctypes.data, len(seg), int(min_samples), int(feat_norm),
                                                             w.shape[0], int(stride), w.ctypes.data, None if bias is None else bias.ctypes.data,
                                                             gamma.ctypes.data, beta.ctypes.data, out.ctypes.data))
        return out, frames

    def selftest_w2v_posconv_segments(self, x, lens, w_bits, bias, groups: int):
        """``pce_selftest_w2v_posconv_segments``: x float32 [windows][T][d], window i holding ``lens[i] <= T`` frames -> float32 [windows][T][d]."""
        x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w_bits, dtype=np.uint16); bias = np.ascontiguousarray(bias, dtype=np.float32)
        lens = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        n_win, t, d = x.shape
        if w.shape != (d, 128, d // groups) or lens.shape != (n_win,):
            raise ValueError("w: [d][128][d / groups]; lens: one per window")
        out = np.zeros_like(x)
        self._check(self._lib.pce_selftest_w2v_posconv_segments(self._ctx, x.ctypes.data, n_win, lens.ctypes.data, t, d, int(groups), w.ctypes.data,
                                                                bias.ctypes.data, out.ctypes.data))
        return out

    def levenshtein(self, pairs):
        """Levenshtein distances of a batch of string pairs in one launch (``pce_levenshtein``): ``pairs`` = [(s1, s2), ...] of ``str``
        -> int32 array.  Characters are code points, as ``for c in s`` of Code/Aligners/levenshtein_dist_align_txtgrids.py:62."""
        if not len(pairs):
            return np.zeros(0, dtype=np.int32)

        def pack(strings):
            cps = [np.frombuffer(s.encode("utf-32-le", "surrogatepass"), dtype=np.uint32) for s in strings]
            off = np.zeros(len(cps) + 1, dtype=np.int64); np.cumsum([len(x) for x in cps], out=off[1:])
            return np.ascontiguousarray(np.concatenate(cps + [np.zeros(0, np.uint32)])), off
        a, ao = pack([p[0] for p in pairs]); b, bo = pack([p[1] for p in pairs])
        out = np.zeros(len(pairs), dtype=np.int32)
        self._check(self._lib.pce_levenshtein(self._ctx, a.ctypes.data if a.size else None, ao.ctypes.data, b.ctypes.data if b.size else None,
                                              bo.ctypes.data, len(pairs), out.ctypes.data))
        return out

    def levenshtein_ids(self, pairs):
        """``pce_levenshtein`` on sequences of arbitrary uint32 symbols (word ids: the edit distance behind a word error rate):
        ``pairs`` = [(ids_a, ids_b), ...] -> int32 array."""
        if not len(pairs):
            return np.zeros(0, dtype=np.int32)

        def pack(seqs):
            seqs = [np.ascontiguousarray(s, dtype=np.uint32).reshape(-1) for s in seqs]
            off = np.zeros(len(seqs) + 1, dtype=np.int64); np.cumsum([len(x) for x in seqs], out=off[1:])
            return np.ascontiguousarray(np.concatenate(seqs + [np.zeros(0, np.uint32)])), off
        a, ao = pack([p[0] for p in pairs]); b, bo = pack([p[1] for p in pairs])
        out = np.zeros(len(pairs), dtype=np.int32)
        self._check(self._lib.pce_levenshtein(self._ctx, a.ctypes.data if a.size else None, ao.ctypes.data, b.ctypes.data if b.size else None,
                                              bo.ctypes.data, len(pairs), out.ctypes.data))
        return out

    @staticmethod
    def _pack_strings(strings):
        """``str`` list -> (code points uint32, offsets int64 [n + 1]), as ``levenshtein`` packs its strings."""
        cps = [np.frombuffer(s.encode("utf-32-le", "surrogatepass"), dtype=np.uint32) for s in strings]
        off = np.zeros(len(cps) + 1, dtype=np.int64); np.cumsum([len(x) for x in cps], out=off[1:])
        return np.ascontiguousarray(np.concatenate(cps + [np.zeros(0, np.uint32)])), off

    def _seqmatch(self, a, b, pairs, autojunk):
        ac, ao = self._pack_strings(a); bc, bo = self._pack_strings(b)
        if pairs is None:
            pa = pb = None; n = len(a) * len(b)
        else:
            pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            if pr.size and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
                raise ValueError("pair indices do not fit int32")
            pa = np.ascontiguousarray(pr[:, 0], dtype=np.int32); pb = np.ascontiguousarray(pr[:, 1], dtype=np.int32); n = len(pr)
        out = np.zeros(n, dtype=np.int32)
        self._check(self._lib.pce_seqmatch(self._ctx, ac.ctypes.data if ac.size else None, ao.ctypes.data, len(a), bc.ctypes.data if bc.size else None,
                                           bo.ctypes.data, len(b), pa.ctypes.data if pa is not None else None, pb.ctypes.data if pb is not None else None,
                                           n, 1 if autojunk else 0, out.ctypes.data))
        la, lb = np.diff(ao), np.diff(bo)
        total = (la[:, None] + lb[None, :]).reshape(-1) if pairs is None else la[pa] + lb[pb]
        return out, total

    def seqmatch_matches(self, a, b, pairs=None, autojunk=True):
        """``sum(block.size for block in difflib.SequenceMatcher(None, a[i], b[j], autojunk).get_matching_blocks())`` in one launch
        (``pce_seqmatch``): ``a`` / ``b`` lists of ``str``; ``pairs`` = [(i, j), ...] or None for all ``len(a) * len(b)`` pairs, row-major
        -> int32 array.  Elements are code points."""
        return self._seqmatch(a, b, pairs, autojunk)[0]

    def seqmatch_ratio(self, a, b, pairs=None, autojunk=True):
        """``SequenceMatcher(None, a[i], b[j], autojunk).ratio()`` per pair -> float64 array, bit-identical: ``2.0 * matches / length``
        (difflib's ``_calculate_ratio``), 1.0 where both strings are empty."""
        m, total = self._seqmatch(a, b, pairs, autojunk)
        out = np.ones(len(m), dtype=np.float64)
        nz = total > 0
        out[nz] = 2.0 * m[nz].astype(np.float64) / total[nz].astype(np.float64)
        return out

    def seqmatch_align(self, a, b, autojunk=True):
        """The fuzzy alignment of "Compare Breaks" (Code/audioPipeline.py:970-998) in one call (``pce_seqmatch_align``): all
        ``len(a) x len(b)`` ratios and the DP over them on the device -> (matches int32 [k, 2] of (index in a, index in b), ascending;
        sim float64 [len(a), len(b)])."""
        n, m = len(a), len(b)
        ac, ao = self._pack_strings(a); bc, bo = self._pack_strings(b)
        sim = np.zeros((n, m), dtype=np.float64)
        k_max = max(min(n, m), 1)
        ma = np.zeros(k_max, dtype=np.int32); mb = np.zeros(k_max, dtype=np.int32); k = C.c_int32()
        self._check(self._lib.pce_seqmatch_align(self._ctx, ac.ctypes.data if ac.size else None, ao.ctypes.data, n, bc.ctypes.data if bc.size else None,
                                                 bo.ctypes.data, m, 1 if autojunk else 0, sim.ctypes.data if sim.size else None, ma.ctypes.data,
                                                 mb.ctypes.data, C.byref(k)))
        return np.stack([ma[:k.value], mb[:k.value]], axis=1), sim

    def interval_match(self, tables, problems):
        """The text matching of the aligner evaluation (``align_intervals``, Code/whisper_testing/splitting.py:94-128) for a batch of
        problems in one call (``pce_ivl_match``).  ``tables`` = [(gold_texts, pred_texts), ...] of already normalised ``str`` lists;
        ``problems`` = [(table, gold_indices, pred_indices or None), ...]: the gold intervals to walk, in that order, and the predicted
        intervals that may be claimed (None: all; a subset keeps the tier's order, so the indices are a set) -> per problem
        ``(match int32 [len(gold_indices)], cls int8 [...])``: the index of the claimed predicted interval or -1, and its class 3 (equal) /
        2 (substring) / 1 (shared word) / 0."""
        interned = {}

        def pack_words(texts):
            ids = [[interned.setdefault(w, len(interned)) for w in s.split()] for s in texts]
            off = np.zeros(len(ids) + 1, dtype=np.int64); np.cumsum([len(x) for x in ids], out=off[1:])
            return np.array([i for x in ids for i in x], dtype=np.int32), off
        gold = [s for g, _ in tables for s in g]; pred = [s for _, p in tables for s in p]
        gc, go = self._pack_strings(gold); pc, po = self._pack_strings(pred)
        gw, gwo = pack_words(gold); pw, pwo = pack_words(pred)
        pair_gold = np.zeros(len(tables) + 1, dtype=np.int32); np.cumsum([len(g) for g, _ in tables], out=pair_gold[1:])
        pair_pred = np.zeros(len(tables) + 1, dtype=np.int32); np.cumsum([len(p) for _, p in tables], out=pair_pred[1:])
        lists = [np.asarray(g, dtype=np.int64).reshape(-1) for _, g, _ in problems]
        if any(x.size and (x.min() < -2 ** 31 or x.max() >= 2 ** 31) for x in lists):
            raise ValueError("gold indices do not fit int32")
        prob_pair = np.array([t for t, _, _ in problems], dtype=np.int32)
        prob_off = np.zeros(len(problems) + 1, dtype=np.int64); np.cumsum([len(x) for x in lists], out=prob_off[1:])
        gold_idx = np.ascontiguousarray(np.concatenate(lists + [np.zeros(0, np.int64)]), dtype=np.int32)
        member_off = np.full(len(problems), -1, dtype=np.int64)
        bitmaps, n_words = [], 0
        for q, (t, _, members) in enumerate(problems):
            if members is None:
                continue
            if not 0 <= t < len(tables):
                raise ValueError(f"problem {q} names table {t} of {len(tables)}")
            n_pred = len(tables[t][1])
            members = np.asarray(members, dtype=np.int64).reshape(-1)
            if members.size and (members.min() < 0 or members.max() >= n_pred):
                raise ValueError(f"problem {q} names a predicted interval outside its tier of {n_pred}")
            bits = np.zeros(((n_pred + 63) // 64) * 64, dtype=np.uint8); bits[members] = 1
            bitmaps.append(np.packbits(bits, bitorder="little").view("<u8"))
            member_off[q] = n_words; n_words += len(bitmaps[-1])
        member = np.ascontiguousarray(np.concatenate(bitmaps + [np.zeros(0, "<u8")]))
        n_slots = int(prob_off[-1])
        out_match = np.full(max(n_slots, 1), -1, dtype=np.int32); out_class = np.zeros(max(n_slots, 1), dtype=np.int8)

        def ptr(a):
            return a.ctypes.data if a.size else None
        self._check(self._lib.pce_ivl_match(self._ctx, ptr(gc), go.ctypes.data, ptr(gw), gwo.ctypes.data, len(gold), ptr(pc), po.ctypes.data, ptr(pw),
                                            pwo.ctypes.data, len(pred), pair_gold.ctypes.data, pair_pred.ctypes.data, len(tables), ptr(prob_pair),
                                            prob_off.ctypes.data, ptr(gold_idx), member_off.ctypes.data if bitmaps else None, ptr(member),
                                            len(problems), out_match.ctypes.data, out_class.ctypes.data))
        return [(out_match[prob_off[q]:prob_off[q + 1]].copy(), out_class[prob_off[q]:prob_off[q + 1]].copy()) for q in range(len(problems))]

    def nw_align(self, pairs, match=1, mismatch=-1, gap=-1):
        """Batched Needleman-Wunsch over integer token ids: ``pairs`` = [(ids_a, ids_b), ...] ->
        [(i_idx, j_idx), ...] with -1 marking a gap (alignment order)."""
        la = np.array([len(a) for a, _ in pairs], dtype=np.int64); lb = np.array([len(b) for _, b in pairs], dtype=np.int64)
        ao = np.zeros(len(pairs) + 1, dtype=np.int64); bo = np.zeros(len(pairs) + 1, dtype=np.int64)
        np.cumsum(la, out=ao[1:]); np.cumsum(lb, out=bo[1:])
        a = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x, _ in pairs] + [np.zeros(0, np.int32)]))
        b = np.ascontiguousarray(np.concatenate([np.asarray(y, dtype=np.int32) for _, y in pairs] + [np.zeros(0, np.int32)]))
        oo = np.zeros(len(pairs) + 1, dtype=np.int64); np.cumsum(la + lb, out=oo[1:])
        oi = np.zeros(max(int(oo[-1]), 1), dtype=np.int32); oj = np.zeros_like(oi); ol = np.zeros(len(pairs), dtype=np.int32)
        self._check(self._lib.pce_nw_align(self._ctx, a.ctypes.data, ao.ctypes.data, b.ctypes.data, bo.ctypes.data, len(pairs),
                                           int(match), int(mismatch), int(gap), oi.ctypes.data, oj.ctypes.data, ol.ctypes.data))
        return [(oi[oo[k]:oo[k] + ol[k]].copy(), oj[oo[k]:oo[k] + ol[k]].copy()) for k in range(len(pairs))]

    # ---------------------------------------------------------------- the reference's measurement closures
    def closures(self):
        """``(get_part_duration, get_median_pitch, get_lufs, get_duration)`` with the signatures of the closures inside
        ``AudioPipeline.measure_prosody_and_build_ssml`` (Code/audioPipeline.py:314-361), answered by this engine
        (``audio_pipeline.ProsodySeam``: path-keyed, batched when the queries are announced with ``prefetch``)."""
        from .audio_pipeline import ProsodySeam
        return ProsodySeam(self).closures()

    # ---------------------------------------------------------------- measurement
    def profile_enable(self, on=True):
        self._check(self._lib.pce_profile_enable(self._ctx, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.pce_profile_reset(self._ctx))

    def profile(self) -> dict:
        out = {}
        for i, name in enumerate(KERNEL_IDS):
            ms = C.c_double(); n = C.c_int64()
            self._check(self._lib.pce_profile_get(self._ctx, i, C.byref(ms), C.byref(n)))
            if n.value:
                fl = C.c_double()
                self._check(self._lib.pce_profile_get_work(self._ctx, i, C.byref(fl)))
                out[name] = {"total_ms": ms.value, "launches": n.value, "flops": fl.value}
        return out


_DEFAULT_ENGINE = None


def get_default_engine(device: int = None) -> ProsodyEngine:
    """Process-wide engine used by the module-level drop-in functions (``Pipeline.compute_*``).  ONE context per process (the
    reference's process owns one Whisper model on one GPU, config.yaml:58): ``device=None`` takes whatever engine exists -- when none
    does, THIS RANK's device (``shard.local_device()``: ``LOCAL_RANK`` under a one-process-per-GPU launcher, 0 without one; a device-less
    first caller such as ``Pipeline.compute_*`` must not pin rank 3 to GPU 0); naming a device other than the existing engine's is an
    error rather than a silent run on the wrong GPU."""
    global _DEFAULT_ENGINE
    if _DEFAULT_ENGINE is None:
        if device is None:
            from . import shard
            device = shard.local_device()
        _DEFAULT_ENGINE = ProsodyEngine(device)
    elif device is not None and getattr(_DEFAULT_ENGINE, "device", device) != device:
        raise RuntimeError(f"this process's engine lives on device {_DEFAULT_ENGINE.device}; device {device} was asked for "
                           "(one context per process: start one process per GPU, or close the engine first)")
    return _DEFAULT_ENGINE


def set_default_engine(engine: ProsodyEngine):
    global _DEFAULT_ENGINE
    _DEFAULT_ENGINE = engine
