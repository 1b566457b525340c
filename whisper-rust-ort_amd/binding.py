"""ctypes binding of libwhisper_hip.so — the host-side mirror of the reference's seam.

Names follow reference src/main.rs: `whisper_log_mel` (:407), `run_encoder` (:698),
`greedy_decode_with_past` (:753), plus the batch entry that replaces the per-window body of
`transcribe_longform_chunked` (:870-915).  Errors surface as `WhisperHipError` carrying the C
status code and the library's message (the reference propagates `anyhow` errors, :1104-1108).

There is no fallback of any kind: if the shared library or a GPU is missing, loading or the first
call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libwhisper_hip.so")

WH_PREC_F32, WH_PREC_BF16, WH_PREC_FP8, WH_PREC_F16X3 = 0, 1, 2, 3
PRECISIONS = {"f32": WH_PREC_F32, "bf16": WH_PREC_BF16, "fp8": WH_PREC_FP8, "f16x3": WH_PREC_F16X3}
WH_N_FRAMES, WH_CLIP_SAMPLES = 3000, 480000
WH_PCM_S16, WH_PCM_U8, WH_PCM_F32 = 0, 1, 2
WH_MAX_CHANNELS = 64
PCM_FORMATS = {np.dtype(np.int16): WH_PCM_S16, np.dtype(np.uint8): WH_PCM_U8, np.dtype(np.float32): WH_PCM_F32}
KG_NAMES = ("mel", "enc_gemm", "enc_attn", "dec_cross_attn", "dec_gemm", "dec_other")

STATUS = {0: "WH_OK", 1: "WH_ERR_EMPTY_AUDIO", 2: "WH_ERR_BAD_SHAPE", 3: "WH_ERR_STATE", 4: "WH_ERR_ARG",
          5: "WH_ERR_NOMEM", 6: "WH_ERR_HIP", 7: "WH_ERR_IO", 8: "WH_ERR_UNSUPPORTED"}

# every symbol include/whisper_hip.h declares
EXPORTS = ("wh_model_load", "wh_model_create", "wh_model_free", "wh_model_get_dims", "wh_model_precision",
           "wh_model_export_tensor", "wh_ctx_create", "wh_ctx_create_ex", "wh_ctx_free", "wh_ctx_cross_mode", "wh_ctx_placement", "wh_last_error", "wh_get_timings",
           "wh_mel_frames", "wh_log_mel", "wh_encode", "wh_decode_greedy", "wh_decode_greedy_batch", "wh_decode_greedy_rows", "wh_transcribe_batch",
           "wh_transcribe_batch_next", "wh_transcribe_batch_device", "wh_transcribe_batch_device_next", "wh_longform_plan", "wh_transcribe_longform", "wh_profile_enable",
           "wh_profile_get", "wh_synthetic_weights", "wh_e4m3_quantize", "wh_e4m3_dequantize", "wh_abi_version",
           "wh_device_count", "wh_ctx_set_timestamp_rules", "wh_ctx_set_logprobs", "wh_get_logprobs",
           "wh_ctx_set_language_detection", "wh_get_languages", "wh_ctx_set_prefixes", "wh_ctx_set_repetition",
           "wh_ctx_set_alignment", "wh_get_token_frames", "wh_get_alignment_debug", "wh_ctx_set_beam_search", "wh_get_beams", "wh_get_beam_trace",
           "wh_ctx_set_sampling", "wh_resampled_samples", "wh_ingest_raw", "wh_transcribe_batch_raw", "wh_transcribe_batch_raw_next",
           "wh_transcribe_longform_raw", "wh_files_load", "wh_files_load_raw", "wh_transcribe_windows", "wh_files_window_mel", "wh_score_tokens", "wh_align_tokens")


class WhisperHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class WhDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "d_model", "n_heads", "enc_layers", "dec_layers", "ffn", "vocab",
                                         "n_audio_ctx", "n_text_ctx")]


class WhTiming(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("preprocess_s", "encode_s", "decode_s", "total_s", "h2d_s", "d2h_s")]


class WhDecodeParams(C.Structure):
    _fields_ = [("prompt", C.POINTER(C.c_int64)), ("n_prompt", C.c_size_t), ("max_new_tokens", C.c_size_t),
                ("eot", C.c_int64), ("suppress", C.POINTER(C.c_int64)), ("n_suppress", C.c_size_t),
                ("begin_suppress", C.POINTER(C.c_int64)), ("n_begin_suppress", C.c_size_t),
                ("forced", C.POINTER(C.c_int64)), ("n_forced", C.c_size_t)]


class WhClip(C.Structure):
    _fields_ = [("pcm", C.POINTER(C.c_float)), ("n_samples", C.c_size_t)]


class WhRawClip(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_frames", C.c_size_t), ("sample_rate", C.c_uint32), ("channels", C.c_uint16), ("format", C.c_uint16)]


def raw_clips(clips: Sequence[Tuple[np.ndarray, int]]):
    """wh_raw_clip array from (samples, sample_rate) pairs: samples of dtype int16 / uint8 / float32 and shape [frames, channels] (or [frames]
    for mono), interleaved as a file holds them.  A C-contiguous array is passed as it lies in memory, whatever its alignment.  Returns the
    ctypes array and the arrays it points into (keep them alive while the library may read them)."""
    arrs = []
    out = (WhRawClip * len(clips))()
    for i, (a, rate) in enumerate(clips):
        a = np.asarray(a)
        if a.dtype not in PCM_FORMATS:
            raise TypeError(f"raw clip {i}: dtype {a.dtype} (int16, uint8 or float32 expected)")
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2:
            raise ValueError(f"raw clip {i}: shape {a.shape} ([frames, channels] expected)")
        if not a.flags.c_contiguous:
            a = np.ascontiguousarray(a)
        arrs.append(a)
        out[i] = WhRawClip(a.ctypes.data, a.shape[0], int(rate), a.shape[1], PCM_FORMATS[a.dtype])
    return out, arrs


class WhCtxOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("max_batch", C.c_int), ("flags", C.c_int),
                ("enc_cu_mask", C.POINTER(C.c_uint32)), ("enc_cu_mask_words", C.c_size_t),
                ("dec_cu_mask", C.POINTER(C.c_uint32)), ("dec_cu_mask_words", C.c_size_t)]


class WhTimestampRules(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("timestamp_begin", C.c_int64), ("no_timestamps", C.c_int64),
                ("max_initial_timestamp_index", C.c_int32)]


class WhLogprobOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("no_speech", C.c_int64), ("sot_index", C.c_int32)]


class WhLanguageOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("lang_ids", C.POINTER(C.c_int64)), ("n_lang", C.c_size_t), ("sot_index", C.c_int32)]


class WhPrefixOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("ids", C.POINTER(C.c_int64)), ("offsets", C.POINTER(C.c_size_t)), ("n_clips", C.c_size_t),
                ("longform_scope", C.c_int32)]


WH_MAX_NGRAM = 32


class WhRepetitionOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32)]


WH_MAX_ALIGN_HEADS = 32
WH_MAX_ALIGN_DEBUG_ROWS = 8


class WhAlignmentOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("heads", C.POINTER(C.c_int32)), ("n_heads", C.c_size_t), ("debug_rows", C.POINTER(C.c_int32)),
                ("n_debug_rows", C.c_size_t)]


WH_MAX_BEAMS = 8
WH_MAX_BEAM_CANDIDATES = 16
WH_MAX_BEAM_TRACE_CLIPS = 8


class WhBeamOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("beam_size", C.c_int32), ("patience", C.c_float), ("length_penalty", C.c_float),
                ("trace_clips", C.POINTER(C.c_int32)), ("n_trace_clips", C.c_size_t)]


class WhSamplingOpts(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("seed", C.c_uint64), ("temperature", C.POINTER(C.c_float)), ("active", C.POINTER(C.c_uint8)),
                ("row_ids", C.POINTER(C.c_uint64)), ("n_rows", C.c_size_t)]


class WhScoreInput(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("ids", C.POINTER(C.c_int64)), ("offsets", C.POINTER(C.c_size_t)), ("n_hyp", C.c_size_t),
                ("hyps_per_clip", C.c_size_t)]


def pack_hypotheses(hyps: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """wh_score_input's two arrays for a list of ragged hypotheses: (ids int64 back to back, offsets uint64 [n + 1]) — the layout of wh_prefix_opts."""
    return pack_prefixes(hyps)


def align_pack(hyps: Sequence[Sequence[int]], heads: Sequence[Tuple[int, int]], hyps_per_clip: int = 1, debug_hyps: Sequence[int] = ()):
    """The arguments of wh_align_tokens: (WhScoreInput, WhAlignmentOpts, the hypotheses' lengths, cap_tokens, the arrays the two structs point into)."""
    ids, offsets = pack_hypotheses(hyps)
    lens = [len(h) for h in hyps]
    cap = max(lens, default=1) or 1
    inp = WhScoreInput(C.sizeof(WhScoreInput), _i64(ids) if ids.size else None, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(hyps), hyps_per_clip)
    h = np.ascontiguousarray(list(heads), np.int32).reshape(-1, 2) if len(heads) else np.zeros((0, 2), np.int32)
    d = np.ascontiguousarray(list(debug_hyps), np.int32)
    i32p = C.POINTER(C.c_int32)
    opts = WhAlignmentOpts(C.sizeof(WhAlignmentOpts), h.ctypes.data_as(i32p) if h.size else None, h.shape[0], d.ctypes.data_as(i32p) if d.size else None, d.size)
    return inp, opts, lens, cap, (ids, offsets, h, d)


def pack_prefixes(prefixes: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """wh_prefix_opts' two arrays for a list of per-clip prefixes: (ids int64 back to back, offsets uint64 [n + 1])."""
    offsets = np.zeros(len(prefixes) + 1, np.uint64)
    for i, pre in enumerate(prefixes):
        offsets[i + 1] = offsets[i] + np.uint64(len(pre))
    ids = np.ascontiguousarray([t for pre in prefixes for t in pre], np.int64)
    return ids, offsets


WH_MAX_LANGUAGES = 128
WH_PREFIX_FIRST_WINDOW, WH_PREFIX_ALL_WINDOWS = 0, 1
WH_CTX_TWO_STREAMS = 1
WH_CTX_CROSS_ES_ON = 2
WH_CTX_CROSS_ES_OFF = 4
N_CUS = 256   # MI355X: 8 XCDs x 32 compute units


def cu_mask(first: int, count: int, total: int = N_CUS) -> np.ndarray:
    """CU mask words with bits first .. first+count-1 set.  On MI355X bit i is compute unit i // 8 of XCD i % 8
    (tools/cu_mask_probe.hip), so a contiguous bit range whose ends are multiples of 8 takes the same number of
    compute units from every XCD."""
    if first < 0 or count < 1 or first + count > total:
        raise ValueError(f"CU range [{first}, {first + count}) outside 0..{total}")
    w = np.zeros((total + 31) // 32, np.uint32)
    for i in range(first, first + count):
        w[i >> 5] |= np.uint32(1 << (i & 31))
    return w


_lib: Optional[C.CDLL] = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                                "there is no CPU fallback")
    L = C.CDLL(path)
    vp, f32p, i64p, szp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_size_t)
    L.wh_model_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.wh_model_create.argtypes = [C.POINTER(WhDims), f32p, C.c_size_t, C.c_int, C.c_int, C.POINTER(vp)]
    L.wh_model_free.argtypes = [vp]
    L.wh_model_free.restype = None
    L.wh_model_get_dims.argtypes = [vp, C.POINTER(WhDims)]
    L.wh_model_precision.argtypes = [vp]
    L.wh_model_export_tensor.argtypes = [vp, C.c_char_p, f32p, C.c_size_t, szp]
    L.wh_ctx_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.wh_ctx_create_ex.argtypes = [vp, C.POINTER(WhCtxOpts), C.POINTER(vp)]
    L.wh_ctx_free.argtypes = [vp]
    L.wh_ctx_free.restype = None
    L.wh_ctx_cross_mode.argtypes = [vp]
    L.wh_ctx_placement.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.wh_last_error.argtypes = [vp]
    L.wh_last_error.restype = C.c_char_p
    L.wh_get_timings.argtypes = [vp, C.POINTER(WhTiming)]
    L.wh_mel_frames.argtypes = [C.c_size_t]
    L.wh_mel_frames.restype = C.c_size_t
    L.wh_log_mel.argtypes = [vp, f32p, C.c_size_t, f32p, C.c_size_t, szp]
    L.wh_encode.argtypes = [vp, f32p, f32p]
    L.wh_decode_greedy.argtypes = [vp, C.POINTER(WhDecodeParams), i64p, C.c_size_t, szp, f32p, C.c_size_t]
    L.wh_decode_greedy_batch.argtypes = [vp, C.POINTER(WhDecodeParams), i64p, C.c_size_t, szp, C.c_size_t, szp, f32p, C.c_size_t]
    L.wh_decode_greedy_rows.argtypes = [vp, C.POINTER(WhDecodeParams), C.POINTER(C.c_int32), C.c_size_t, i64p, C.c_size_t, szp, C.c_size_t, szp, f32p, C.c_size_t]
    L.wh_transcribe_batch.argtypes = [vp, C.POINTER(WhClip), C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_transcribe_batch_next.argtypes = [vp, C.POINTER(WhClip), C.c_size_t, C.POINTER(WhClip), C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_transcribe_batch_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_transcribe_batch_device_next.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_longform_plan.argtypes = [C.c_size_t, C.c_double, C.c_double, szp, C.c_size_t, szp]
    L.wh_transcribe_longform.argtypes = [vp, f32p, C.c_size_t, C.c_double, C.c_double, C.POINTER(WhDecodeParams), i64p,
                                         szp, C.c_size_t, szp]
    rawp = C.POINTER(WhRawClip)
    L.wh_resampled_samples.argtypes = [C.c_size_t, C.c_uint32]
    L.wh_resampled_samples.restype = C.c_size_t
    L.wh_ingest_raw.argtypes = [vp, rawp, C.c_size_t, f32p, C.c_size_t, szp]
    L.wh_transcribe_batch_raw.argtypes = [vp, rawp, C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_transcribe_batch_raw_next.argtypes = [vp, rawp, C.c_size_t, rawp, C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_transcribe_longform_raw.argtypes = [vp, rawp, C.c_double, C.c_double, C.POINTER(WhDecodeParams), i64p, szp, C.c_size_t, szp]
    L.wh_profile_enable.argtypes = [vp, C.c_int]
    L.wh_profile_get.argtypes = [vp, C.POINTER(C.c_double), i64p]
    L.wh_synthetic_weights.argtypes = [C.c_char_p, C.c_uint64, f32p, C.c_size_t, szp]
    L.wh_e4m3_quantize.argtypes = [f32p, C.c_size_t, C.POINTER(C.c_uint8)]
    L.wh_e4m3_quantize.restype = None
    L.wh_e4m3_dequantize.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, f32p]
    L.wh_e4m3_dequantize.restype = None
    L.wh_ctx_set_timestamp_rules.argtypes = [vp, C.POINTER(WhTimestampRules)]
    L.wh_ctx_set_logprobs.argtypes = [vp, C.POINTER(WhLogprobOpts)]
    L.wh_get_logprobs.argtypes = [vp, f32p, C.c_size_t, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.wh_ctx_set_language_detection.argtypes = [vp, C.POINTER(WhLanguageOpts)]
    L.wh_get_languages.argtypes = [vp, i64p, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.wh_ctx_set_prefixes.argtypes = [vp, C.POINTER(WhPrefixOpts)]
    L.wh_ctx_set_repetition.argtypes = [vp, C.POINTER(WhRepetitionOpts)]
    L.wh_ctx_set_alignment.argtypes = [vp, C.POINTER(WhAlignmentOpts)]
    L.wh_get_token_frames.argtypes = [vp, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int32), C.c_size_t, szp]
    L.wh_get_alignment_debug.argtypes = [vp, C.c_size_t, f32p, f32p, C.c_size_t, C.POINTER(C.c_int32)]
    i32p = C.POINTER(C.c_int32)
    L.wh_ctx_set_beam_search.argtypes = [vp, C.POINTER(WhBeamOpts)]
    L.wh_ctx_set_sampling.argtypes = [vp, C.POINTER(WhSamplingOpts)]
    L.wh_get_beams.argtypes =[vp, i64p, C.c_size_t, szp, f32p, f32p, i32p, C.c_size_t, szp, C.c_size_t, szp]
    L.wh_get_beam_trace.argtypes = [vp, C.c_size_t, i32p, i32p, f32p, i32p, C.c_size_t, szp]
    L.wh_files_load.argtypes = [vp, C.POINTER(WhClip), C.c_size_t, i64p]
    L.wh_files_load_raw.argtypes = [vp, rawp, C.c_size_t, i64p]
    L.wh_transcribe_windows.argtypes = [vp, i32p, i64p, C.c_size_t, C.POINTER(WhDecodeParams), i64p, szp]
    L.wh_files_window_mel.argtypes = [vp, C.c_int32, C.c_int64, f32p]
    L.wh_score_tokens.argtypes = [vp, C.POINTER(WhDecodeParams), C.POINTER(WhScoreInput), f32p, i64p, C.c_size_t, i32p, C.c_size_t, f32p, C.c_size_t]
    L.wh_align_tokens.argtypes = [vp, C.POINTER(WhDecodeParams), C.POINTER(WhScoreInput), C.POINTER(WhAlignmentOpts), i32p, i32p, f32p, C.c_size_t]
    _lib = L
    return L


def _f32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i64(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


@dataclass
class DecodeParams:
    """Arguments of greedy_decode_with_past (reference src/main.rs:753-761) + GenerationCfg (:102-106)."""
    prompt: Sequence[int]
    max_new_tokens: int = 128
    eot: int = 50257
    suppress_tokens: Sequence[int] = ()
    begin_suppress_tokens: Sequence[int] = ()
    forced: Optional[Sequence[int]] = None

    def to_c(self):
        keep = [np.asarray(list(self.prompt), np.int64), np.asarray(list(self.suppress_tokens), np.int64),
                np.asarray(list(self.begin_suppress_tokens), np.int64),
                np.asarray(list(self.forced) if self.forced is not None else [], np.int64)]
        p = WhDecodeParams(_i64(keep[0]), keep[0].size, self.max_new_tokens, self.eot,
                           _i64(keep[1]) if keep[1].size else None, keep[1].size,
                           _i64(keep[2]) if keep[2].size else None, keep[2].size,
                           _i64(keep[3]) if keep[3].size else None, keep[3].size)
        return p, keep


class Model:
    """Replaces the three `ort::Session`s (reference src/main.rs:1103-1108)."""

    def __init__(self, spec_or_dir: str, device: int = 0, precision: int = WH_PREC_BF16):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.wh_model_load(spec_or_dir.encode(), device, precision, C.byref(h))
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(None) or b"").decode())
        self.h = h
        d = WhDims()
        self.lib.wh_model_get_dims(self.h, C.byref(d))
        self.dims = d
        self.precision = precision
        self.device = device

    @classmethod
    def from_weights(cls, dims, wflat: np.ndarray, device: int = 0, precision: int = WH_PREC_BF16) -> "Model":
        self = cls.__new__(cls)
        self.lib = load_library()
        wflat = np.ascontiguousarray(wflat, np.float32)
        cd = WhDims(dims.n_mels, dims.d_model, dims.n_heads, dims.enc_layers, dims.dec_layers, dims.ffn, dims.vocab,
                    dims.n_audio_ctx, dims.n_text_ctx)
        h = C.c_void_p()
        rc = self.lib.wh_model_create(C.byref(cd), _f32(wflat), wflat.size, device, precision, C.byref(h))
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(None) or b"").decode())
        self.h, self.dims, self.precision, self.device = h, cd, precision, device
        return self

    def export_tensor(self, name: str) -> np.ndarray:
        n = C.c_size_t(0)
        rc = self.lib.wh_model_export_tensor(self.h, name.encode(), None, 0, C.byref(n))
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(None) or b"").decode())
        out = np.empty(n.value, np.float32)
        rc = self.lib.wh_model_export_tensor(self.h, name.encode(), _f32(out), out.size, C.byref(n))
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(None) or b"").decode())
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.wh_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One stream's workspace + KV cache (reference: per-thread IoBinding + `past`, src/main.rs:786-791)."""

    def __init__(self, model: Model, max_batch: int = 1, enc_cu_mask: Optional[np.ndarray] = None,
                 dec_cu_mask: Optional[np.ndarray] = None, two_streams: bool = False, cross_es: Optional[bool] = None):
        """enc_cu_mask / dec_cu_mask (uint32 words, see cu_mask()) or two_streams: the chip-partition form of the context
        (wh_ctx_create_ex) — log-mel + encoder on their own stream, beside the token loop of the previous batch.
        cross_es: force the token loop's cross-attention onto the encoder states (True) or onto the projected K / V (False);
        None = the library's rule (bf16 whisper-base geometry, max_batch >= 256)."""
        self.model, self.lib, self.max_batch = model, model.lib, max_batch
        self.beam_size_of_last = 1   # (beam_trace()'s row width: the beam_size of the last set_beam_search)
        self._gen_lens: List[int] = []
        h = C.c_void_p()
        flags = (WH_CTX_TWO_STREAMS if two_streams else 0) | (0 if cross_es is None else (WH_CTX_CROSS_ES_ON if cross_es else WH_CTX_CROSS_ES_OFF))
        if enc_cu_mask is None and dec_cu_mask is None and not flags:
            rc = self.lib.wh_ctx_create(model.h, max_batch, C.byref(h))
        else:
            em = np.ascontiguousarray(enc_cu_mask, np.uint32) if enc_cu_mask is not None else None
            dm = np.ascontiguousarray(dec_cu_mask, np.uint32) if dec_cu_mask is not None else None
            u32p = C.POINTER(C.c_uint32)
            o = WhCtxOpts(C.sizeof(WhCtxOpts), max_batch, flags,
                          em.ctypes.data_as(u32p) if em is not None else None, em.size if em is not None else 0,
                          dm.ctypes.data_as(u32p) if dm is not None else None, dm.size if dm is not None else 0)
            rc = self.lib.wh_ctx_create_ex(model.h, C.byref(o), C.byref(h))
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(None) or b"").decode())
        self.h = h

    def _check(self, rc: int):
        if rc:
            raise WhisperHipError(rc, (self.lib.wh_last_error(self.h) or b"").decode())

    @property
    def cross_mode(self) -> int:
        """0: the token loop streams the projected cross K / V of every layer; 1: the encoder states (wh_cross_es.hip)."""
        return int(self.lib.wh_ctx_cross_mode(self.h))

    @property
    def placement(self) -> dict:
        """wh_ctx_placement: how many workspaces wh_ctx_create_ex timed (0: step not taken) and the cross-attention launch time on the first / kept one."""
        a, b = C.c_float(0), C.c_float(0)
        n = int(self.lib.wh_ctx_placement(self.h, C.byref(a), C.byref(b)))
        return {"workspaces_timed": n, "first_us_per_launch": float(a.value), "kept_us_per_launch": float(b.value)}

    def debug_set_step_split(self, rows: int):
        """Test hook (not in the public header): the generated positions of the following decode calls run rows [0, rows) and [rows, n) of the
        batch as two branches wherever the call is eligible; 0: the context's own rule again."""
        self._check(self.lib.wh_debug_set_step_split(self.h, C.c_int(rows)))

    @property
    def step_split(self) -> int:
        """Rows of the first range the last decode call's generated positions ran with; 0: they ran one chain."""
        return int(self.lib.wh_debug_get_step_split(self.h))

    def debug_set_step_free(self, on: bool):
        """Test hook (not in the public header): where debug_set_step_split makes the following decode calls split, their two ranges run
        whole positions on their own streams if the call is eligible; False: only where the context's own rule splits."""
        self._check(self.lib.wh_debug_set_step_free(self.h, C.c_int(1 if on else 0)))

    @property
    def step_free(self) -> int:
        """1: the generated positions of the last decode call ran as free halves; 0: joined, or one chain."""
        return int(self.lib.wh_debug_get_step_free(self.h))

    def set_timestamp_rules(self, tb: int, no_timestamps: int = -1, max_initial_index: int = 50):
        """wh_ctx_set_timestamp_rules: Whisper's timestamp rules on every decode entry of this context (tb = id of <|0.00|>;
        no_timestamps = <|notimestamps|>, suppressed at every step, -1: none; max_initial_index < 0: no bound on the first timestamp)."""
        r = WhTimestampRules(C.sizeof(WhTimestampRules), tb, no_timestamps, max_initial_index)
        self._check(self.lib.wh_ctx_set_timestamp_rules(self.h, C.byref(r)))

    def clear_timestamp_rules(self):
        self._check(self.lib.wh_ctx_set_timestamp_rules(self.h, None))

    def set_logprobs(self, no_speech: int = -1, sot_index: int = 0):
        """wh_ctx_set_logprobs: every decode entry of this context records the log-probability of each generated token; no_speech >= 0
        also the no-speech probability (softmax of the unfiltered logits at prompt position sot_index, at that id)."""
        o = WhLogprobOpts(C.sizeof(WhLogprobOpts), no_speech, sot_index)
        self._check(self.lib.wh_ctx_set_logprobs(self.h, C.byref(o)))

    def clear_logprobs(self):
        self._check(self.lib.wh_ctx_set_logprobs(self.h, None))

    def logprobs(self) -> Tuple[List[np.ndarray], Optional[np.ndarray]]:
        """wh_get_logprobs of the last decode call: one float32 array per clip / window (one entry per generated token, EOT's included)
        and the no-speech probabilities (None without a probe)."""
        n = C.c_size_t(0)
        self._check(self.lib.wh_get_logprobs(self.h, None, 0, None, 0, C.byref(n)))
        k = int(n.value)
        lens = list(self._gen_lens)
        assert len(lens) == k, (len(lens), k)
        cap = max(1, max(lens, default=0))
        lp = np.zeros((max(1, k), cap), np.float32)
        ns = np.zeros(max(1, k), np.float32)
        rc = self.lib.wh_get_logprobs(self.h, _f32(lp), cap, _f32(ns), k, C.byref(n))
        if rc == 3:   # WH_ERR_STATE: no probe
            ns = None
            rc = self.lib.wh_get_logprobs(self.h, _f32(lp), cap, None, k, C.byref(n))
        self._check(rc)
        return [lp[i, : lens[i]].copy() for i in range(k)], (ns[:k] if ns is not None else None)

    def set_language_detection(self, ids: Sequence[int], sot_index: int = 0):
        """wh_ctx_set_language_detection: every decode entry of this context picks each clip's language among `ids` (distinct token ids, any
        order) from the unfiltered logits of prompt position sot_index and decodes with it at prompt position sot_index + 1 (the prompt's
        own token there is a placeholder)."""
        a = np.ascontiguousarray(list(ids), np.int64)
        o = WhLanguageOpts(C.sizeof(WhLanguageOpts), _i64(a) if a.size else None, a.size, sot_index)
        self._check(self.lib.wh_ctx_set_language_detection(self.h, C.byref(o)))
        self._n_lang = int(a.size)

    def clear_language_detection(self):
        self._check(self.lib.wh_ctx_set_language_detection(self.h, None))

    def languages(self) -> Tuple[np.ndarray, np.ndarray]:
        """wh_get_languages of the last decode call: (ids int64 [n], probs float32 [n, n_lang]) — one row per clip / window, the
        probabilities in the order the ids were listed."""
        n = C.c_size_t(0)
        self._check(self.lib.wh_get_languages(self.h, None, None, 0, C.byref(n)))
        k = int(n.value)
        ids = np.zeros(max(1, k), np.int64)
        probs = np.zeros((max(1, k), getattr(self, "_n_lang", WH_MAX_LANGUAGES)), np.float32)
        self._check(self.lib.wh_get_languages(self.h, _i64(ids), _f32(probs), k, C.byref(n)))
        return ids[:k], probs[:k]

    def set_prefixes(self, prefixes: Sequence[Sequence[int]], all_windows: bool = False):
        """wh_ctx_set_prefixes: clip b of every decode entry of this context decodes as if its prompt were prefixes[b] ++ params.prompt (text
        context: <|startofprev|> previous text ...); the outputs keep their layout, the prefix is not echoed.  transcribe_longform takes one
        prefix, for window 0 only or (all_windows) for every window."""
        ids, offsets = pack_prefixes(prefixes)
        o = WhPrefixOpts(C.sizeof(WhPrefixOpts), _i64(ids) if ids.size else None, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(prefixes),
                         WH_PREFIX_ALL_WINDOWS if all_windows else WH_PREFIX_FIRST_WINDOW)
        self._check(self.lib.wh_ctx_set_prefixes(self.h, C.byref(o)))

    def clear_prefixes(self):
        self._check(self.lib.wh_ctx_set_prefixes(self.h, None))

    def set_repetition(self, penalty: float = 1.0, ngram: int = 0):
        """wh_ctx_set_repetition: every decode entry of this context applies HF's repetition penalty (v > 0 ? v / penalty : v * penalty on the
        ids of the row's generated history) and bans the ids that would repeat an n-gram of `ngram` ids, before the suppress masks and the
        timestamp rules (timestamps are exempt while the rules are on).  (1.0, 0) turns it off."""
        o = WhRepetitionOpts(C.sizeof(WhRepetitionOpts), penalty, ngram)
        self._check(self.lib.wh_ctx_set_repetition(self.h, C.byref(o)))

    def clear_repetition(self):
        self._check(self.lib.wh_ctx_set_repetition(self.h, None))

    def set_alignment(self, heads: Sequence[Tuple[int, int]], debug_rows: Sequence[int] = ()):
        """wh_ctx_set_alignment: every decode entry of this context computes the frame at which each generated token is spoken, from the
        cross-attention of the listed (layer, head) pairs and a dynamic-time-warping path.  debug_rows (parity harness): batch rows whose
        probabilities and alignment matrix are kept for alignment_debug()."""
        h = np.ascontiguousarray(list(heads), np.int32).reshape(-1, 2) if len(heads) else np.zeros((0, 2), np.int32)
        d = np.ascontiguousarray(list(debug_rows), np.int32)
        i32p = C.POINTER(C.c_int32)
        o = WhAlignmentOpts(C.sizeof(WhAlignmentOpts), h.ctypes.data_as(i32p) if h.size else None, h.shape[0], d.ctypes.data_as(i32p) if d.size else None, d.size)
        self._check(self.lib.wh_ctx_set_alignment(self.h, C.byref(o)))

    def clear_alignment(self):
        self._check(self.lib.wh_ctx_set_alignment(self.h, None))

    def token_frames(self) -> Tuple[List[np.ndarray], np.ndarray]:
        """wh_get_token_frames of the last decode call: one int32 array per clip / window (the frame of each generated token, 0.02 s apart)
        and the clips' frame counts S_b."""
        n = C.c_size_t(0)
        self._check(self.lib.wh_get_token_frames(self.h, None, 0, None, 0, C.byref(n)))
        k = int(n.value)
        lens = list(self._gen_lens)
        assert len(lens) == k, (len(lens), k)
        cap = max(1, max(lens, default=0))
        fr = np.zeros((max(1, k), cap), np.int32)
        nf = np.zeros(max(1, k), np.int32)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.wh_get_token_frames(self.h, fr.ctypes.data_as(i32p), cap, nf.ctypes.data_as(i32p), k, C.byref(n)))
        return [fr[i, : lens[i]].copy() for i in range(k)], nf[:k].copy()

    def alignment_debug(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """wh_get_alignment_debug: (probs float32 [n_heads, n_gen, S_b], matrix float32 [n_gen, S_b]) of debug row k of the last decode call."""
        shape = (C.c_int32 * 3)()
        self._check(self.lib.wh_get_alignment_debug(self.h, k, None, None, 0, shape))
        nh, ng, sb = int(shape[0]), int(shape[1]), int(shape[2])
        probs = np.zeros((nh, ng, sb), np.float32)
        matrix = np.zeros((ng, sb), np.float32)
        self._check(self.lib.wh_get_alignment_debug(self.h, k, _f32(probs), _f32(matrix), max(1, probs.size), shape))
        return probs, matrix

    def set_beam_search(self, beam_size: int, patience: float = 1.0, length_penalty: float = -1.0, trace_clips: Sequence[int] = ()):
        """wh_ctx_set_beam_search: every decode entry of this context decodes each clip with `beam_size` beams (openai-whisper's
        BeamSearchDecoder: round(beam_size * patience) finished candidates; length_penalty < 0 ranks by score / length).  trace_clips (parity
        harness): clips whose per-position decisions beam_trace() returns."""
        t = np.ascontiguousarray(list(trace_clips), np.int32)
        o = WhBeamOpts(C.sizeof(WhBeamOpts), beam_size, patience, length_penalty, t.ctypes.data_as(C.POINTER(C.c_int32)) if t.size else None, t.size)
        self._check(self.lib.wh_ctx_set_beam_search(self.h, C.byref(o)))
        self.beam_size_of_last = beam_size

    def clear_beam_search(self):
        self._check(self.lib.wh_ctx_set_beam_search(self.h, None))

    def set_sampling(self, seed: int, temperatures: Sequence[float], active: Optional[Sequence[int]] = None, row_ids: Optional[Sequence[int]] = None):
        """wh_ctx_set_sampling: batch row b of every decode entry of this context draws its tokens at temperatures[b] (0: plain argmax) by
        Gumbel-max on Philox4x32-10 streams named by (seed, row_ids[b]); active[b] == 0: the row generates nothing.  Long-form: one row."""
        t = np.ascontiguousarray(temperatures, np.float32)
        a = np.ascontiguousarray(active, np.uint8) if active is not None else None
        r = np.ascontiguousarray(row_ids, np.uint64) if row_ids is not None else None
        if (a is not None and a.size != t.size) or (r is not None and r.size != t.size):
            raise ValueError("set_sampling: active / row_ids must have one entry per temperature")
        o = WhSamplingOpts(C.sizeof(WhSamplingOpts), seed, _f32(t) if t.size else None, a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None,
                           r.ctypes.data_as(C.POINTER(C.c_uint64)) if r is not None else None, t.size)
        self._check(self.lib.wh_ctx_set_sampling(self.h, C.byref(o)))

    def clear_sampling(self):
        self._check(self.lib.wh_ctx_set_sampling(self.h, None))

    def beams(self, cap_hyp: int =WH_MAX_BEAM_CANDIDATES + WH_MAX_BEAMS) -> List[List[dict]]:
        """wh_get_beams of the last decode call: per clip / window the ranked hypotheses, best first, as dicts {tokens (generated ids, EOT
        included when finished), sum_logprob, rank_score, finished}."""
        n = C.c_size_t(0)
        self._check(self.lib.wh_get_beams(self.h, None, 0, None, None, None, None, 0, None, 0, C.byref(n)))
        k, cap_t = max(1, int(n.value)), self.model.dims.n_text_ctx
        toks = np.zeros((k, cap_hyp, cap_t), np.int64)
        nt = np.zeros((k, cap_hyp), np.uint64)
        sums = np.zeros((k, cap_hyp), np.float32)
        rank = np.zeros((k, cap_hyp), np.float32)
        fin = np.zeros((k, cap_hyp), np.int32)
        nh = np.zeros(k, np.uint64)
        szp = C.POINTER(C.c_size_t)
        self._check(self.lib.wh_get_beams(self.h, _i64(toks), cap_t, nt.ctypes.data_as(szp), _f32(sums), _f32(rank), fin.ctypes.data_as(C.POINTER(C.c_int32)),
                                          cap_hyp, nh.ctypes.data_as(szp), k, C.byref(n)))
        return [[{"tokens": toks[b, h, : int(nt[b, h])].copy(), "sum_logprob": float(sums[b, h]), "rank_score": float(rank[b, h]), "finished": bool(fin[b, h])}
                 for h in range(int(nh[b]))] for b in range(int(n.value))]

    def beam_trace(self, k: int) -> dict:
        """wh_get_beam_trace of trace clip k: {parents, tokens int32 [steps, K], scores float32 [steps, K], pool_size int32 [steps]}."""
        ns = C.c_size_t(0)
        self._check(self.lib.wh_get_beam_trace(self.h, k, None, None, None, None, 0, C.byref(ns)))
        steps, K = int(ns.value), self.beam_size_of_last
        par = np.zeros((max(1, steps), K), np.int32)
        tok = np.zeros((max(1, steps), K), np.int32)
        sc = np.zeros((max(1, steps), K), np.float32)
        pool = np.zeros(max(1, steps), np.int32)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.wh_get_beam_trace(self.h, k, par.ctypes.data_as(i32p), tok.ctypes.data_as(i32p), _f32(sc), pool.ctypes.data_as(i32p), steps, C.byref(ns)))
        return {"parents": par[:steps], "tokens": tok[:steps], "scores": sc[:steps], "pool_size": pool[:steps]}

    def decode_resident_rows_raw(self, params: DecodeParams, rows: Sequence[int]) -> Tuple[List[np.ndarray], np.ndarray]:
        """wh_decode_greedy_rows without cutting the logits: tokens of every clip and logits [len(rows)][max_new_tokens][vocab] (with beam
        search `rows` are physical rows, clip * beam_size + beam, and a row's entries stop where its clip was complete: zeros after)."""
        p, keep = params.to_c()
        cap = len(params.prompt) + params.max_new_tokens
        nb = self.max_batch
        toks = np.zeros((nb, cap), np.int64)
        n = (C.c_size_t * nb)()
        got = C.c_size_t(0)
        sel = np.ascontiguousarray(rows, np.int32)
        logits = np.zeros((len(sel), params.max_new_tokens, self.model.dims.vocab), np.float32)
        self._check(self.lib.wh_decode_greedy_rows(self.h, C.byref(p), sel.ctypes.data_as(C.POINTER(C.c_int32)), len(sel), _i64(toks), cap, n, nb,
                                                   C.byref(got), _f32(logits), params.max_new_tokens))
        k = int(got.value)
        return self._took([toks[i, : n[i]].copy() for i in range(k)], params), logits

    def score_tokens(self, params: DecodeParams, hyps: Sequence[Sequence[int]], hyps_per_clip: int = 1, logit_hyps: Sequence[int] = ()):
        """wh_score_tokens: log p(tokens | audio) of `hyps` (hypothesis j of resident clip b is hyps[b * hyps_per_clip + j]) in one decoder pass
        over all their positions.  Returns per hypothesis (log-probabilities float32 [n], masked argmax int64 [n]) as two lists and, for the
        hypotheses listed in logit_hyps, their raw logits [n][vocab] as a third (empty without logit_hyps)."""
        p, keep = params.to_c()
        ids, offsets = pack_hypotheses(hyps)
        lens = [len(h) for h in hyps]
        cap = max(lens, default=1) or 1
        inp = WhScoreInput(C.sizeof(WhScoreInput), _i64(ids) if ids.size else None, offsets.ctypes.data_as(C.POINTER(C.c_size_t)), len(hyps), hyps_per_clip)
        lp = np.zeros((len(hyps), cap), np.float32)
        am = np.zeros((len(hyps), cap), np.int64)
        sel = np.ascontiguousarray(list(logit_hyps), np.int32)
        rows = max([lens[k] for k in sel if 0 <= k < len(lens)], default=1)
        logits = np.zeros((len(sel), rows, self.model.dims.vocab), np.float32) if sel.size else None
        self._check(self.lib.wh_score_tokens(self.h, C.byref(p), C.byref(inp), _f32(lp), _i64(am), cap, sel.ctypes.data_as(C.POINTER(C.c_int32)) if sel.size else None,
                                             sel.size, _f32(logits) if sel.size else None, rows))
        return ([lp[g, :n].copy() for g, n in enumerate(lens)], [am[g, :n].copy() for g, n in enumerate(lens)],
                [logits[j, : lens[int(k)]] for j, k in enumerate(sel)])

    def align_tokens(self, params: DecodeParams, hyps: Sequence[Sequence[int]], heads: Sequence[Tuple[int, int]], hyps_per_clip: int = 1,
                     debug_hyps: Sequence[int] = (), want_logprobs: bool = False):
        """wh_align_tokens: the frame at which each token of the given `hyps` is spoken (hypothesis j of resident clip b is
        hyps[b * hyps_per_clip + j]), from the listed (layer, head) pairs' cross-attention in one decoder pass over all positions.  Returns
        (frames: one int32 array per hypothesis, 0.02 s apart; n_frames int32 [n_hyp], S_b of each hypothesis's clip; the log-probabilities of
        score_tokens as a list of float32 arrays, or None without want_logprobs).  debug_hyps (parity harness): hypotheses whose
        probabilities and alignment matrix are kept for alignment_debug()."""
        p, keep = params.to_c()
        inp, opts, lens, cap, keep2 = align_pack(hyps, heads, hyps_per_clip, debug_hyps)
        fr = np.zeros((max(1, len(hyps)), cap), np.int32)
        nf = np.zeros(max(1, len(hyps)), np.int32)
        lp = np.zeros((max(1, len(hyps)), cap), np.float32) if want_logprobs else None
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.wh_align_tokens(self.h, C.byref(p), C.byref(inp), C.byref(opts), fr.ctypes.data_as(i32p), nf.ctypes.data_as(i32p),
                                             _f32(lp) if want_logprobs else None, cap))
        return ([fr[g, :n].copy() for g, n in enumerate(lens)], nf[: len(hyps)].copy(),
                [lp[g, :n].copy() for g, n in enumerate(lens)] if want_logprobs else None)

    def _took(self, toks: List[np.ndarray], params: "DecodeParams") -> List[np.ndarray]:
        self._gen_lens = [len(t) - len(params.prompt) for t in toks]   # (what logprobs() cuts its rows to)
        return toks

    # --- the reference's three functions -----------------------------------------------------
    def whisper_log_mel(self, audio_16k: np.ndarray) -> np.ndarray:
        """whisper_log_mel_80 (src/main.rs:407-509) → [n_mels, n_frames] f32."""
        pcm = np.ascontiguousarray(audio_16k, np.float32)
        nf = int(self.lib.wh_mel_frames(pcm.size)) if pcm.size else 1
        out = np.empty((self.model.dims.n_mels, nf), np.float32)
        got = C.c_size_t(0)
        self._check(self.lib.wh_log_mel(self.h, _f32(pcm), pcm.size, _f32(out), nf, C.byref(got)))
        return out

    def run_encoder(self, input_features: np.ndarray, want_output: bool = True) -> Optional[np.ndarray]:
        """run_encoder (src/main.rs:698-707): [1?, n_mels, 3000] → [1500, d_model] f32."""
        mel = np.ascontiguousarray(input_features, np.float32)
        if mel.ndim == 3 and mel.shape[0] == 1:
            mel = mel[0]
        if mel.shape != (self.model.dims.n_mels, WH_N_FRAMES):
            raise WhisperHipError(2, f"expected input_features [{self.model.dims.n_mels}, {WH_N_FRAMES}], got {mel.shape}")
        out = np.empty((self.model.dims.n_audio_ctx, self.model.dims.d_model), np.float32) if want_output else None
        self._check(self.lib.wh_encode(self.h, _f32(mel), _f32(out) if want_output else None))
        return out

    def greedy_decode_with_past(self, params: DecodeParams, want_logits: bool = False
                                ) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """greedy_decode_with_past (src/main.rs:753-829) on the encoder states held by this context."""
        p, keep = params.to_c()
        cap = len(params.prompt) + params.max_new_tokens
        toks = np.zeros(cap, np.int64)
        n = C.c_size_t(0)
        logits = np.zeros((params.max_new_tokens, self.model.dims.vocab), np.float32) if want_logits else None
        self._check(self.lib.wh_decode_greedy(self.h, C.byref(p), _i64(toks), cap, C.byref(n),
                                              _f32(logits) if want_logits else None, params.max_new_tokens))
        nt = int(n.value)
        self._gen_lens = [nt - len(params.prompt)]
        return toks[:nt].copy(), (logits[: nt - len(params.prompt)].copy() if want_logits else None)

    def greedy_decode_resident_batch(self, params: DecodeParams, want_logits: bool = False
                                     ) -> Tuple[List[np.ndarray], Optional[List[np.ndarray]]]:
        """Parity harness: greedy_decode_with_past over every clip whose encoder states are resident (the last
        transcribe_batch / run_encoder), decoded as ONE batch, optionally with the logits rows of every clip."""
        p, keep = params.to_c()
        cap = len(params.prompt) + params.max_new_tokens
        nb = self.max_batch
        toks = np.zeros((nb, cap), np.int64)
        n = (C.c_size_t * nb)()
        got = C.c_size_t(0)
        logits = np.zeros((nb, params.max_new_tokens, self.model.dims.vocab), np.float32) if want_logits else None
        self._check(self.lib.wh_decode_greedy_batch(self.h, C.byref(p), _i64(toks), cap, n, nb, C.byref(got),
                                                    _f32(logits) if want_logits else None, params.max_new_tokens))
        k = int(got.value)
        out = self._took([toks[i, : n[i]].copy() for i in range(k)], params)
        lg = [logits[i, : n[i] - len(params.prompt)] for i in range(k)] if want_logits else None
        return out, lg

    def greedy_decode_resident_rows(self, params: DecodeParams, rows: Sequence[int]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """The same batch decode with the logits of the chosen batch rows only (wh_decode_greedy_rows): tokens of every clip,
        logits [len(rows)][generated][vocab]."""
        p, keep = params.to_c()
        cap = len(params.prompt) + params.max_new_tokens
        nb = self.max_batch
        toks = np.zeros((nb, cap), np.int64)
        n = (C.c_size_t * nb)()
        got = C.c_size_t(0)
        sel = np.ascontiguousarray(rows, np.int32)
        logits = np.zeros((len(sel), params.max_new_tokens, self.model.dims.vocab), np.float32)
        self._check(self.lib.wh_decode_greedy_rows(self.h, C.byref(p), sel.ctypes.data_as(C.POINTER(C.c_int32)), len(sel), _i64(toks), cap, n, nb,
                                                   C.byref(got), _f32(logits), params.max_new_tokens))
        k = int(got.value)
        out = self._took([toks[i, : n[i]].copy() for i in range(k)], params)
        return out, [logits[j, : n[int(r)] - len(params.prompt)] for j, r in enumerate(sel)]

    # --- fused batch entries ----------------------------------------------------------------------
    def transcribe_batch_next(self, clips: Sequence[np.ndarray], params: DecodeParams, next_clips: Optional[Sequence[np.ndarray]] = None
                              ) -> List[np.ndarray]:
        """wh_transcribe_batch_next: `clips` transcribed like transcribe_batch while `next_clips` (arrays that stay alive and unchanged
        until the call that transcribes them — views of page-locked memory make the copy asynchronous) are copied to the device."""
        arrs = [np.ascontiguousarray(c, np.float32) for c in clips]
        cl = (WhClip * len(arrs))(*[WhClip(_f32(a), a.size) for a in arrs])
        nxt = [np.ascontiguousarray(c, np.float32) for c in next_clips] if next_clips is not None else None
        ncl = (WhClip * len(nxt))(*[WhClip(_f32(a), a.size) for a in nxt]) if nxt else None
        p, keep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((len(arrs), stride), np.int64)
        n = (C.c_size_t * len(arrs))()
        self._check(self.lib.wh_transcribe_batch_next(self.h, cl, len(arrs), ncl, len(nxt) if nxt else 0, C.byref(p), _i64(toks), n))
        self._keep_next = nxt   # (contiguous copies, if any were made, must outlive the asynchronous copy)
        return self._took([toks[i, : n[i]].copy() for i in range(len(arrs))], params)

    def transcribe_batch(self, clips: Sequence[np.ndarray], params: DecodeParams) -> List[np.ndarray]:
        arrs = [np.ascontiguousarray(c, np.float32) for c in clips]
        cl = (WhClip * len(arrs))(*[WhClip(_f32(a), a.size) for a in arrs])
        p, keep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((len(arrs), stride), np.int64)
        n = (C.c_size_t * len(arrs))()
        self._check(self.lib.wh_transcribe_batch(self.h, cl, len(arrs), C.byref(p), _i64(toks), n))
        return self._took([toks[i, : n[i]].copy() for i in range(len(arrs))], params)

    def transcribe_batch_device(self, d_pcm_ptr: int, n_clips: int, params: DecodeParams, next_ptr: Optional[int] = None,
                                next_n: int = 0) -> List[np.ndarray]:
        """PCM already resident in HBM: `d_pcm_ptr` = device address of [n_clips][480000] f32.  next_ptr / next_n: the
        batch whose log-mel + encoder are to run beside this batch's token loop (wh_transcribe_batch_device_next)."""
        p, keep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((n_clips, stride), np.int64)
        n = (C.c_size_t * n_clips)()
        if next_ptr is None:
            self._check(self.lib.wh_transcribe_batch_device(self.h, C.c_void_p(d_pcm_ptr), n_clips, C.byref(p), _i64(toks), n))
        else:
            self._check(self.lib.wh_transcribe_batch_device_next(self.h, C.c_void_p(d_pcm_ptr), n_clips, C.c_void_p(next_ptr), next_n,
                                                                 C.byref(p), _i64(toks), n))
        return self._took([toks[i, : n[i]].copy() for i in range(n_clips)], params)

    def transcribe_longform(self, audio_16k: np.ndarray, params: DecodeParams, chunk_length_s: float = 30.0,
                            overlap_s: float = 5.0) -> List[np.ndarray]:
        pcm = np.ascontiguousarray(audio_16k, np.float32)
        nch = C.c_size_t(0)
        self.lib.wh_longform_plan(pcm.size, chunk_length_s, overlap_s, None, 0, C.byref(nch))
        k = max(1, int(nch.value))
        p, keep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((k, stride), np.int64)
        n = (C.c_size_t * k)()
        got = C.c_size_t(0)
        self._check(self.lib.wh_transcribe_longform(self.h, _f32(pcm), pcm.size, chunk_length_s, overlap_s, C.byref(p),
                                                    _i64(toks), n, k, C.byref(got)))
        return self._took([toks[i, : n[i]].copy() for i in range(int(got.value))], params)

    # --- raw audio in (src/main.rs:207-316 on the GPU): clips are (samples [frames, channels] int16 / uint8 / float32, sample_rate) pairs ---
    def ingest_raw(self, clips: Sequence[Tuple[np.ndarray, int]]) -> List[np.ndarray]:
        """wh_ingest_raw (parity entry): the clips' 16 kHz mono f32 samples as the device converted them."""
        cl, keep = raw_clips(clips)
        lens = [int(self.lib.wh_resampled_samples(a.shape[0], int(r))) for a, (_, r) in zip(keep, clips)]
        cap = max(1, max(lens))
        out = np.zeros((len(keep), cap), np.float32)
        n = (C.c_size_t * len(keep))()
        self._check(self.lib.wh_ingest_raw(self.h, cl, len(keep), _f32(out), cap, n))
        return [out[i, : n[i]].copy() for i in range(len(keep))]

    def transcribe_batch_raw(self, clips: Sequence[Tuple[np.ndarray, int]], params: DecodeParams,
                             next_clips: Optional[Sequence[Tuple[np.ndarray, int]]] = None, prefetch: bool = False) -> List[np.ndarray]:
        """wh_transcribe_batch_raw, or (prefetch=True or next_clips given) wh_transcribe_batch_raw_next.  The prefetch is recognised by the
        samples' addresses: pass the same arrays again in the call that transcribes them."""
        cl, keep = raw_clips(clips)
        ncl, nkeep = raw_clips(next_clips) if next_clips is not None else (None, None)
        p, pkeep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((len(keep), stride), np.int64)
        n = (C.c_size_t * len(keep))()
        if next_clips is None and not prefetch:
            self._check(self.lib.wh_transcribe_batch_raw(self.h, cl, len(keep), C.byref(p), _i64(toks), n))
        else:
            self._check(self.lib.wh_transcribe_batch_raw_next(self.h, cl, len(keep), ncl, len(nkeep) if nkeep else 0, C.byref(p), _i64(toks), n))
        self._keep_next_raw = nkeep   # (the arrays the asynchronous copy reads)
        return self._took([toks[i, : n[i]].copy() for i in range(len(keep))], params)

    def transcribe_longform_raw(self, samples: np.ndarray, sample_rate: int, params: DecodeParams, chunk_length_s: float = 30.0,
                                overlap_s: float = 5.0) -> List[np.ndarray]:
        cl, keep = raw_clips([(samples, sample_rate)])
        nch = C.c_size_t(0)
        self.lib.wh_longform_plan(int(self.lib.wh_resampled_samples(keep[0].shape[0], int(sample_rate))), chunk_length_s, overlap_s, None, 0, C.byref(nch))
        k = max(1, int(nch.value))
        p, pkeep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((k, stride), np.int64)
        n = (C.c_size_t * k)()
        got = C.c_size_t(0)
        self._check(self.lib.wh_transcribe_longform_raw(self.h, cl, chunk_length_s, overlap_s, C.byref(p), _i64(toks), n, k, C.byref(got)))
        return self._took([toks[i, : n[i]].copy() for i in range(int(got.value))], params)

    # --- sequential long-form: a resident file set and windows cut from it -----------------------------------------------
    def files_load(self, files: Sequence[np.ndarray]) -> List[int]:
        """wh_files_load: the whole-file log-mels of `files` (16 kHz mono f32, any lengths) become the context's file set; returns each
        file's frame count.  An empty list frees the set."""
        arrs = [np.ascontiguousarray(f, np.float32) for f in files]
        if not arrs:
            self._check(self.lib.wh_files_load(self.h, None, 0, None))
            return []
        cl = (WhClip * len(arrs))(*[WhClip(_f32(a), a.size) for a in arrs])
        nf = (C.c_int64 * len(arrs))()
        self._check(self.lib.wh_files_load(self.h, cl, len(arrs), nf))
        return [int(v) for v in nf]

    def files_load_raw(self, files: Sequence[Tuple[np.ndarray, int]]) -> List[int]:
        """wh_files_load_raw: the same from files as they were read, (samples [frames, channels], sample_rate) pairs."""
        if not files:
            self._check(self.lib.wh_files_load_raw(self.h, None, 0, None))
            return []
        cl, keep = raw_clips(files)
        nf = (C.c_int64 * len(keep))()
        self._check(self.lib.wh_files_load_raw(self.h, cl, len(keep), nf))
        return [int(v) for v in nf]

    def transcribe_windows(self, rows: Sequence[Tuple[int, int]], params: DecodeParams) -> List[np.ndarray]:
        """wh_transcribe_windows: `rows` are (file, seek_frame) pairs of the loaded file set, decoded as one batch."""
        fi = np.ascontiguousarray([r[0] for r in rows], np.int32)
        sk = np.ascontiguousarray([r[1] for r in rows], np.int64)
        p, keep = params.to_c()
        stride = len(params.prompt) + params.max_new_tokens
        toks = np.zeros((max(1, len(fi)), stride), np.int64)
        n = (C.c_size_t * max(1, len(fi)))()
        self._check(self.lib.wh_transcribe_windows(self.h, fi.ctypes.data_as(C.POINTER(C.c_int32)), _i64(sk), len(fi), C.byref(p), _i64(toks), n))
        return self._took([toks[i, : n[i]].copy() for i in range(len(fi))], params)

    def files_window_mel(self, file: int, seek_frame: int) -> np.ndarray:
        """wh_files_window_mel (parity entry): the window as the encoder receives it, [n_mels, 3000] f32."""
        out = np.empty((self.model.dims.n_mels, WH_N_FRAMES), np.float32)
        self._check(self.lib.wh_files_window_mel(self.h, file, seek_frame, _f32(out)))
        return out

    # --- measurement -------------------------------------------------------------------------------
    def timings(self) -> dict:
        t = WhTiming()
        self.lib.wh_get_timings(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in WhTiming._fields_}

    def profile_enable(self, groups=True, stride: int = 0):
        """groups: True/False (all/none) or an iterable of KG_NAMES to event-time; stride > 1 samples every
        stride-th decoder position (the rest replay the hipGraph)."""
        if groups is True:
            mask = (1 << len(KG_NAMES)) - 1
        elif not groups:
            mask = 0
        else:
            mask = sum(1 << KG_NAMES.index(g) for g in groups)
        self.lib.wh_profile_enable(self.h, mask | ((stride & 0xFFFF) << 16))

    def profile_get(self) -> dict:
        ms = (C.c_double * len(KG_NAMES))()
        ln = (C.c_int64 * len(KG_NAMES))()
        self.lib.wh_profile_get(self.h, ms, ln)
        return {k: {"ms": ms[i], "launches": int(ln[i])} for i, k in enumerate(KG_NAMES)}

    def close(self):
        if getattr(self, "h", None):
            self.lib.wh_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def longform_plan(n_samples: int, chunk_length_s: float = 30.0, overlap_s: float = 5.0) -> List[int]:
    L = load_library()
    n = C.c_size_t(0)
    L.wh_longform_plan(n_samples, chunk_length_s, overlap_s, None, 0, C.byref(n))
    offs = (C.c_size_t * max(1, n.value))()
    L.wh_longform_plan(n_samples, chunk_length_s, overlap_s, offs, n.value, C.byref(n))
    return [int(offs[i]) for i in range(n.value)]


def synthetic_weights(preset: str, seed: int) -> np.ndarray:
    """Host-only: the C++ generator's f32 blob in canonical order."""
    L = load_library()
    n = C.c_size_t(0)
    rc = L.wh_synthetic_weights(preset.encode(), seed, None, 0, C.byref(n))
    if rc:
        raise WhisperHipError(rc, (L.wh_last_error(None) or b"").decode())
    out = np.empty(n.value, np.float32)
    rc = L.wh_synthetic_weights(preset.encode(), seed, _f32(out), out.size, C.byref(n))
    if rc:
        raise WhisperHipError(rc, (L.wh_last_error(None) or b"").decode())
    return out


def e4m3_quantize(x: np.ndarray) -> np.ndarray:
    """Host-only: f32 -> OCP e4m3fn codes exactly as WH_PREC_FP8 stores weights."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint8)
    load_library().wh_e4m3_quantize(_f32(x), x.size, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def e4m3_dequantize(codes: np.ndarray) -> np.ndarray:
    codes = np.ascontiguousarray(codes, np.uint8)
    out = np.empty(codes.shape, np.float32)
    load_library().wh_e4m3_dequantize(codes.ctypes.data_as(C.POINTER(C.c_uint8)), codes.size, _f32(out))
    return out


def device_count() -> int:
    return int(load_library().wh_device_count())


class HipRuntime:
    """Just enough of the HIP runtime (the instance libwhisper_hip.so already loaded) to keep PCM resident in HBM for
    wh_transcribe_batch_device: bench.py and the GPU tests of that entry."""

    def __init__(self):
        load_library()
        self.lib = C.CDLL("libamdhip64.so.7", mode=C.RTLD_GLOBAL)
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipSetDevice.argtypes = [C.c_int]

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")

    def upload(self, dev: int, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        self.check(self.lib.hipSetDevice(dev), "hipSetDevice")
        p = C.c_void_p()
        self.check(self.lib.hipMalloc(C.byref(p), arr.nbytes), "hipMalloc")
        self.check(self.lib.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1), "hipMemcpy H2D")
        self.check(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")
        return p.value

    def malloc(self, dev: int, nbytes: int) -> int:
        """Uninitialised device memory (probe programs: a placeholder that makes the next allocation land elsewhere)."""
        self.check(self.lib.hipSetDevice(dev), "hipSetDevice")
        p = C.c_void_p()
        self.check(self.lib.hipMalloc(C.byref(p), int(nbytes)), "hipMalloc")
        return p.value

    def free(self, ptr: int):
        self.check(self.lib.hipFree(C.c_void_p(ptr)), "hipFree")

    def host_alloc(self, shape, dtype=np.float32) -> np.ndarray:
        """Page-locked host memory as a numpy array (hipHostMalloc): the source of truly asynchronous host-to-device copies."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self.lib.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        self.check(self.lib.hipHostMalloc(C.byref(p), n, 0), "hipHostMalloc")
        buf = (C.c_char * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        self.lib.hipHostFree.argtypes = [C.c_void_p]
        self.check(self.lib.hipHostFree(C.c_void_p(self._pinned.pop(arr.ctypes.data))), "hipHostFree")

    def sync(self):
        self.check(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")


# ---- timestamped segments (host library libwh_host.so: wh_host.h split_segments / merge_window_segments / SRT / VTT) -------------------
HOST_LIB_PATH = os.path.join(HERE, "libwh_host.so")
_host: Optional[C.CDLL] = None


def load_host_library(path: str = HOST_LIB_PATH) -> C.CDLL:
    global _host
    if _host is None:
        L = C.CDLL(path)
        ll = C.POINTER(C.c_longlong)
        L.whh_segments_json.argtypes = [ll, C.c_size_t, C.c_longlong, C.c_longlong, C.c_double, C.c_char_p, C.c_size_t]
        L.whh_longform_segments_json.argtypes = [ll, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                                 C.c_longlong, C.c_longlong, C.c_char_p, C.c_size_t]
        for f in (L.whh_srt, L.whh_vtt):
            f.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.whh_segments_conf_json.argtypes = [ll, C.c_size_t, C.c_longlong, C.c_longlong, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_size_t]
        for f in (L.whh_segments_json, L.whh_segments_conf_json, L.whh_longform_segments_json, L.whh_srt, L.whh_vtt):
            f.restype = C.c_size_t
        L.whh_synthetic_clip.argtypes = [C.c_ulonglong, C.POINTER(C.c_float), C.c_size_t]
        L.whh_synthetic_clip.restype = C.c_size_t
        L.whh_avg_logprob.argtypes = [C.POINTER(C.c_float), ll, C.c_size_t, C.c_longlong]
        L.whh_avg_logprob.restype = C.c_double
        L.whh_skip_window.argtypes = [C.c_double] * 4
        L.whh_no_speech_token.argtypes = [C.c_char_p] * 3
        L.whh_no_speech_token.restype = C.c_longlong
        L.whh_language_table.argtypes = [C.c_char_p, C.c_longlong, ll, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.whh_language_table.restype = C.c_longlong
        L.whh_words_json.argtypes = [ll, C.POINTER(C.c_int), C.c_size_t, C.c_longlong, C.c_longlong, C.c_double, C.c_double, C.c_char_p, C.c_char_p, C.c_size_t]
        L.whh_words_json.restype = C.c_size_t
        szp, dp = C.POINTER(C.c_size_t), C.POINTER(C.c_double)
        L.whh_seek_advance.argtypes = [ll, C.c_size_t, C.c_longlong, C.c_longlong, C.c_longlong, C.c_char_p, C.c_size_t]
        L.whh_seek_advance.restype = C.c_size_t
        L.whh_run_sequential.argtypes = [ll, C.c_size_t, ll, dp, ll, C.c_size_t, szp, szp, ll, szp, dp, C.c_size_t, C.c_char_p, C.c_size_t]
        L.whh_run_sequential.restype = C.c_size_t
        _host = L
    return _host


def _ll(values) -> np.ndarray:
    return np.ascontiguousarray(list(values) or [0], np.int64)


def seek_advance(generated: Sequence[int], tb: int, eot: int, seg_frames: int) -> dict:
    """wh_host.h seek_advance: {"advance": frames, "segments": [{"start", "end", "ids"}]} of one window's generated tokens."""
    import json
    t = _ll(generated)
    L = load_host_library()
    return json.loads(_host_string(lambda o, c: L.whh_seek_advance(t.ctypes.data_as(C.POINTER(C.c_longlong)), len(generated), tb, eot, seg_frames, o, c)))


def run_sequential_scripted(frames: Sequence[int], script: Sequence[Sequence[dict]], tb: int, eot: int, sot_prev: int, n_text_ctx: int, n_prompt: int,
                            max_new_tokens: int, condition_on_previous_text: bool = True, no_speech_threshold: Optional[float] = None,
                            logprob_threshold: Optional[float] = None, initial_prompt: Sequence[int] = ()) -> dict:
    """wh_host.h run_sequential over a scripted step: script[f][k] = {"tokens", "avg_logprob", "no_speech_prob", "temperature"} is what file f's
    window k decodes to (the file's last entry repeats).  Returns {"steps": [[files]], "files": [{"windows", "segments"}]}."""
    import json
    nan = float("nan")
    ll = C.POINTER(C.c_longlong)
    entries = [e for f in script for e in f]
    first = np.ascontiguousarray(np.cumsum([0] + [len(f) for f in script])[:-1], np.uintp)
    count = np.ascontiguousarray([len(f) for f in script], np.uintp)
    toks = _ll([t for e in entries for t in e["tokens"]])
    lens = np.ascontiguousarray([len(e["tokens"]) for e in entries], np.uintp)
    scores = np.ascontiguousarray([[e.get("avg_logprob", 0.0), e.get("no_speech_prob", 0.0), e.get("temperature", 0.0)] for e in entries], np.float64)
    fr, ini = _ll(frames), _ll(initial_prompt)
    cfg_i = _ll([tb, eot, sot_prev, n_text_ctx, n_prompt, max_new_tokens, int(condition_on_previous_text)])
    cfg_d = np.ascontiguousarray([nan if no_speech_threshold is None else no_speech_threshold, nan if logprob_threshold is None else logprob_threshold], np.float64)
    szp, dp = C.POINTER(C.c_size_t), C.POINTER(C.c_double)
    L = load_host_library()
    return json.loads(_host_string(lambda o, c: L.whh_run_sequential(
        fr.ctypes.data_as(ll), len(frames), cfg_i.ctypes.data_as(ll), cfg_d.ctypes.data_as(dp), ini.ctypes.data_as(ll), len(initial_prompt),
        first.ctypes.data_as(szp), count.ctypes.data_as(szp), toks.ctypes.data_as(ll), lens.ctypes.data_as(szp), scores.ctypes.data_as(dp), len(entries), o, c)))


def _host_string(call) -> str:
    n = call(None, 0)
    buf = C.create_string_buffer(n + 1)
    call(buf, n + 1)
    return buf.value.decode()


def cli_synthetic_clip(seed: int) -> np.ndarray:
    """Clip `seed` of whisper_bench --synthetic-clips (file i of a run is clip --seed + i, --seed defaults to 1000)."""
    x = np.zeros(WH_CLIP_SAMPLES, np.float32)
    n = load_host_library().whh_synthetic_clip(seed, _f32(x), x.size)
    assert n == x.size
    return x


def avg_logprob(logprobs: Sequence[float], tokens: Sequence[int], eot: int) -> float:
    """openai-whisper's sum_logprobs / (len(tokens) + 1) of one window's generated tokens and their log-probabilities (EOT's included
    in the sum when it was emitted, not in the length)."""
    n = min(len(logprobs), len(tokens))
    lp = np.ascontiguousarray(list(logprobs)[:n] or [0.0], np.float32)
    t = np.ascontiguousarray(list(tokens)[:n] or [0], np.int64)
    return float(load_host_library().whh_avg_logprob(lp.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_longlong)), n, eot))


def skip_window(no_speech_prob: float, avg_lp: float, no_speech_threshold: Optional[float] = None, logprob_threshold: Optional[float] = None) -> bool:
    """The CLI's silence rule: no_speech_prob > no_speech_threshold and avg_logprob < logprob_threshold (None: that threshold is off)."""
    nan = float("nan")
    return bool(load_host_library().whh_skip_window(no_speech_prob, avg_lp, nan if no_speech_threshold is None else no_speech_threshold,
                                                    nan if logprob_threshold is None else logprob_threshold))


def no_speech_token(language: str = "en", task: str = "transcribe", tokenizer_json: str = "") -> int:
    """WhisperSpecial::no_speech: the tokenizer's <|nospeech|> / <|nocaptions|>, else the id before <|notimestamps|> (50362)."""
    return int(load_host_library().whh_no_speech_token(language.encode(), task.encode(), tokenizer_json.encode()))


def language_table(vocab: int, tokenizer_json: str = "") -> Tuple[List[str], List[int]]:
    """The CLI's --language auto table: (codes, token ids) — the tokenizer's <|xx|> tokens when one is given, else the multilingual block
    from 50259 on (99 codes, 100 when the vocabulary has 51866 ids).  ValueError with the CLI's message when the vocabulary cannot hold it."""
    ids = (C.c_longlong * WH_MAX_LANGUAGES)()
    codes, err = C.create_string_buffer(1024), C.create_string_buffer(1024)
    n = load_host_library().whh_language_table(tokenizer_json.encode(), vocab, ids, len(ids), codes, len(codes), err, len(err))
    if n < 0:
        raise ValueError(err.value.decode())
    return codes.value.decode().split(","), [int(ids[i]) for i in range(n)]


def words_from_tokens(generated: Sequence[int], frames: Sequence[int], tb: int, eot: int, duration: float, offset: float = 0.0,
                      tokenizer_json: str = "") -> List[dict]:
    """One window's generated tokens and their frames (Context.token_frames) -> [{word, start, end}]: openai-whisper's split on spaces;
    timestamp tokens (ids >= tb; tb < 0: none), EOT and special tokens dropped; times in seconds, offset by the window's start."""
    import json
    n = min(len(generated), len(frames))
    t = np.ascontiguousarray(list(generated)[:n] or [0], np.int64)
    f = np.ascontiguousarray(list(frames)[:n] or [0], np.int32)
    L = load_host_library()
    return json.loads(_host_string(lambda o, c: L.whh_words_json(t.ctypes.data_as(C.POINTER(C.c_longlong)), f.ctypes.data_as(C.POINTER(C.c_int)), n, tb, eot,
                                                                 duration, offset, tokenizer_json.encode(), o, c)))


def split_segments(generated: Sequence[int], tb: int, eot: int, duration: float, avg_logprob: Optional[float] = None,
                   no_speech_prob: Optional[float] = None) -> List[dict]:
    """One window's generated tokens -> [{start, end, tokens}] (openai-whisper's slicing rule; tokens = the segment's text ids).  With
    avg_logprob and no_speech_prob each segment also carries the window's two values."""
    import json
    t = np.ascontiguousarray(list(generated), np.int64)
    L = load_host_library()
    if avg_logprob is not None and no_speech_prob is not None:
        return json.loads(_host_string(lambda o, c: L.whh_segments_conf_json(t.ctypes.data_as(C.POINTER(C.c_longlong)), t.size, tb, eot, duration,
                                                                              avg_logprob, no_speech_prob, o, c)))
    return json.loads(_host_string(lambda o, c: L.whh_segments_json(t.ctypes.data_as(C.POINTER(C.c_longlong)), t.size, tb, eot, duration, o, c)))


def longform_segments(windows: Sequence[Sequence[int]], starts: Sequence[float], durations: Sequence[float], overlap_s: float, tb: int,
                      eot: int) -> List[dict]:
    """Long-form: each window's segments shifted by its start; in the overlap of windows k and k+1 a segment belongs to k if it starts
    before start(k+1) + overlap_s / 2."""
    import json
    t = np.ascontiguousarray([x for w in windows for x in w] or [0], np.int64)
    lens = (C.c_size_t * max(1, len(windows)))(*[len(w) for w in windows])
    st = (C.c_double * max(1, len(windows)))(*starts)
    du = (C.c_double * max(1, len(windows)))(*durations)
    L = load_host_library()
    return json.loads(_host_string(lambda o, c: L.whh_longform_segments_json(t.ctypes.data_as(C.POINTER(C.c_longlong)), lens, len(windows), st, du,
                                                                             overlap_s, tb, eot, o, c)))


def _cue_call(fn, cues):
    st = (C.c_double * max(1, len(cues)))(*[c[0] for c in cues])
    en = (C.c_double * max(1, len(cues)))(*[c[1] for c in cues])
    texts = b"".join(c[2].encode() + b"\0" for c in cues) + b"\0"
    return _host_string(lambda o, cap: fn(st, en, texts, len(cues), o, cap))


def srt(cues: Sequence[Tuple[float, float, str]]) -> str:
    """SubRip text of (start, end, text) cues: 1-based numbers, HH:MM:SS,mmm."""
    return _cue_call(load_host_library().whh_srt, cues)


def vtt(cues: Sequence[Tuple[float, float, str]]) -> str:
    """WebVTT text of (start, end, text) cues: WEBVTT header, 1-based numbers, HH:MM:SS.mmm."""
    return _cue_call(load_host_library().whh_vtt, cues)
