"""ctypes shim into libwhisper_hip.so — the role whisper/coreml.py:19-244 plays for
the reference's CoreML library, bound to the C ABI of include/whisper_hip.h.

Differences from the reference shim, on purpose:
  * the library owns a *context* (not process globals, coreml.mm:18-23) and every
    call returns a status that is turned into ``HipBackendError`` here (the
    reference's void calls only NSLog failures, coreml.mm:54-56);
  * there is no CPU fallback: if the library or a HIP device is missing, every
    entry point raises.  The product path never computes on the host.
"""

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(os.path.dirname(_PKG_DIR), "lib", "libwhisper_hip.so")

WH_F32 = 0
WH_F16 = 1
WH_PCM_S16, WH_PCM_S32, WH_PCM_F32 = 0, 1, 2


class HipBackendError(RuntimeError):
    pass


class WhDims(ctypes.Structure):
    _fields_ = [(k, c_int) for k in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                     "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class WhDecodeOpts(ctypes.Structure):
    _fields_ = [("group", c_int), ("beam", c_int), ("patience", c_float), ("temperature", c_float),
                ("sample_len", c_int), ("suppress_blank", c_int), ("timestamps", c_int), ("max_initial", c_int),
                ("eot", c_int), ("no_speech", c_int), ("no_timestamps", c_int), ("timestamp_begin", c_int),
                ("blank", c_int * 4), ("n_blank", c_int), ("suppress", POINTER(c_int)), ("n_suppress", c_int),
                ("seed", c_uint64), ("max_candidates", c_int),
                ("no_repeat_ngram", c_int), ("repetition_penalty", c_float)]


class WhVadOpts(ctypes.Structure):
    _fields_ = [("ratio_q8", c_uint64), ("t_lo", c_uint64), ("t_hi", c_uint64), ("percentile", c_int),
                ("min_silence", c_int), ("min_speech", c_int), ("pad", c_int)]


class WhSvadOpts(ctypes.Structure):
    _fields_ = [("ratio_q8", c_uint64), ("t_lo", c_uint64), ("t_hi", c_uint64), ("percentile", c_int),
                ("window", c_int), ("min_silence", c_int), ("min_speech", c_int)]


class WhSvadState(ctypes.Structure):
    _fields_ = [(k, c_int64) for k in ("frames", "samples", "run_start", "run_end", "closed_start", "closed_end",
                                       "closed_total")] + [("threshold", c_uint64), ("partial", c_uint64),
                                                           ("state", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WhWavFmt(ctypes.Structure):
    _fields_ = [("encoding", c_int), ("channels", c_int), ("sample_rate", c_int), ("valid_bits", c_int),
                ("data_offset", c_int64), ("n_frames", c_int64)]


class WavInfo(NamedTuple):
    """What ``wh_wav_info`` reads from a WAV header (``encoding``: a WH_WAV_* code)."""
    encoding: int
    channels: int
    sample_rate: int
    valid_bits: int
    data_offset: int
    n_frames: int


_lib = None
_EXPORTS = {
    # name: (restype, argtypes)
    "wh_last_error": (c_char_p, []),
    "wh_version": (c_int, []),
    "wh_create": (c_int, [c_int, POINTER(WhDims), c_int, c_int, c_int, POINTER(c_void_p)]),
    "wh_destroy": (c_int, [c_void_p]),
    "wh_load_tensor": (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int]),
    "wh_finalize": (c_int, [c_void_p]),
    "wh_set_mel_filters": (c_int, [c_void_p, c_int, c_void_p]),
    "wh_set_phrase_bias": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float]),
    "wh_log_mel": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, POINTER(c_int64)]),
    "wh_log_mel_frames": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_int64, c_int,
                                  POINTER(c_int64)]),
    "wh_audio_upload": (c_int, [c_void_p, c_void_p, c_int64]),
    "wh_audio_ingest": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                c_int64, c_int64, POINTER(c_int64)]),
    "wh_audio_read": (c_int, [c_void_p, c_void_p, c_int64, c_int64]),
    "wh_speech_spans": (c_int, [c_void_p, POINTER(WhVadOpts), c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "wh_frame_energy_read": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "wh_mel_max": (c_int, [c_void_p, POINTER(c_float)]),
    "wh_mel_normalize": (c_int, [c_void_p, c_float]),
    "wh_log_mel_batch": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p]),
    "wh_mel_max_batch": (c_int, [c_void_p, c_void_p, c_int]),
    "wh_mel_read": (c_int, [c_void_p, c_void_p, c_int64, c_int64]),
    "wh_mel_write": (c_int, [c_void_p, c_void_p, c_int64]),
    "wh_encode": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "wh_read_audio_features": (c_int, [c_void_p, c_int, c_void_p]),
    "wh_read_cross_kv": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "wh_decode_begin": (c_int, [c_void_p, c_int, POINTER(WhDecodeOpts), c_void_p, c_void_p, c_int, c_void_p]),
    "wh_decode_begin_slots": (c_int, [c_void_p, c_int, c_void_p, POINTER(WhDecodeOpts), c_void_p, c_void_p, c_int,
                                      c_void_p]),
    "wh_decode_steps": (c_int, [c_void_p, c_int, POINTER(c_int)]),
    "wh_decode_read": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "wh_decode_maxc": (c_int, [c_void_p]),
    "wh_prefill": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "wh_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "wh_reorder_kv": (c_int, [c_void_p, c_void_p]),
    "wh_prefill_logits": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "wh_align": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                         POINTER(c_int)]),
    "wh_align_batch": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                               c_int, c_void_p, c_void_p, c_void_p]),
    "wh_dtw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, POINTER(c_int)]),
    "wh_dtw_open": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, POINTER(c_int),
                            POINTER(c_int), c_void_p]),
    "wh_align_batch_open": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                    c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wh_stats": (c_int, [c_void_p, POINTER(c_double), c_int]),
    "wh_sync": (c_int, [c_void_p]),
    "wh_time_stage": (c_int, [c_void_p, c_int, c_int, POINTER(c_double)]),
    "wh_step_kernels": (c_int, [c_void_p, c_int, c_int, ctypes.c_char_p, c_int]),
    "wh_token_ms": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_int), c_int]),
    "wh_flac_info": (c_int, [c_void_p, c_int64, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int64)]),
    "wh_flac_decode": (c_int, [c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64)]),
    "wh_flac_last_error": (c_char_p, []),
    "wh_flac_index": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    "wh_flac_decode_indexed": (c_int, [c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64)]),
    "wh_flac_last_path": (c_int, []),
    "wh_flac_decode_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64),
                                      POINTER(c_int)]),
    "wh_flac_ingest": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int64, c_int64,
                               POINTER(c_int64), POINTER(c_int)]),
    "wh_wav_info": (c_int, [c_void_p, c_int64, POINTER(WhWavFmt)]),
    "wh_wav_last_error": (c_char_p, []),
    "wh_wav_ingest": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int64, c_int64,
                              POINTER(c_int64)]),
    "wh_audio_ingest_split": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                      c_void_p, c_int, c_int64, c_int64, POINTER(c_int64)]),
    "wh_flac_ingest_split": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_int64, c_int64, POINTER(c_int64), POINTER(c_int)]),
    "wh_wav_ingest_split": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                    c_int64, c_int64, POINTER(c_int64)]),
    "wh_stream_begin": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int64]),
    "wh_stream_append": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    "wh_stream_finish": (c_int, [c_void_p, POINTER(c_int64)]),
    "wh_stream_trim": (c_int, [c_void_p, c_int64]),
    "wh_stream_info": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int)]),
    "wh_stream_emitted": (c_int64, [c_int64, c_int, c_int, c_int]),
    "wh_pool_create": (c_int, [c_void_p, c_int, c_int64]),
    "wh_pool_destroy": (c_int, [c_void_p]),
    "wh_pool_open": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int]),
    "wh_pool_close": (c_int, [c_void_p, c_int]),
    "wh_pool_append": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wh_pool_finish": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "wh_pool_trim": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "wh_pool_info": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int)]),
    "wh_pool_read": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int64]),
    "wh_pool_log_mel": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p]),
    "wh_pool_vad_enable": (c_int, [c_void_p, c_int, POINTER(WhSvadOpts)]),
    "wh_pool_vad_state": (c_int, [c_void_p, c_int, c_void_p, POINTER(WhSvadState)]),
    "wh_pool_vad_read": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "wh_stream_vad_enable": (c_int, [c_void_p, POINTER(WhSvadOpts)]),
    "wh_stream_vad_state": (c_int, [c_void_p, POINTER(WhSvadState)]),
}
N_STATS = 16  # WH_N_STATS
FLAC_PATHS = ("device", "host")


def lib_path() -> str:
    return os.environ.get("WHISPER_HIP_LIB", _DEFAULT_LIB)


def load_library(path: Optional[str] = None):
    """Load libwhisper_hip.so (raises if absent: no silent fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or lib_path()
    if not os.path.exists(p):
        raise HipBackendError(f"libwhisper_hip.so not found at {p}; build it with `make -C whisper.coreml_amd`")
    lib = ctypes.CDLL(p)
    for name, (res, args) in _EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(c_void_p)


def decode_flac(data: bytes):
    """FLAC bytes -> (int32 samples [frames][channels], sample_rate, bits_per_sample),
    decoded by the library's host FLAC reader (wh_flac_decode; bit-exact)."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    rate, ch, bps, total = c_int(), c_int(), c_int(), c_int64()
    rc = lib.wh_flac_info(_ptr(buf), len(buf), ctypes.byref(rate), ctypes.byref(ch), ctypes.byref(bps),
                          ctypes.byref(total))
    if rc != 0:
        raise HipBackendError(f"wh_flac_info failed ({rc}): {lib.wh_flac_last_error().decode(errors='replace')}")
    # STREAMINFO may leave the total unknown (0): size the output from the byte count
    # (a FLAC frame cannot carry more samples than a 1-bit-per-sample verbatim one)
    cap = total.value if total.value > 0 else len(buf) * 8
    out = np.empty((cap, ch.value), np.int32)
    n = c_int64()
    rc = lib.wh_flac_decode(_ptr(buf), len(buf), _ptr(out), cap, ctypes.byref(n))
    if rc != 0:
        raise HipBackendError(f"wh_flac_decode failed ({rc}): {lib.wh_flac_last_error().decode(errors='replace')}")
    return out[: n.value], rate.value, bps.value


def flac_info(data: bytes):
    """(sample rate, channels, bits per sample, total samples per channel) from STREAMINFO."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    rate, ch, bps, total = c_int(), c_int(), c_int(), c_int64()
    rc = lib.wh_flac_info(_ptr(buf), len(buf), ctypes.byref(rate), ctypes.byref(ch), ctypes.byref(bps),
                          ctypes.byref(total))
    if rc != 0:
        raise HipBackendError(f"wh_flac_info failed ({rc}): {lib.wh_flac_last_error().decode(errors='replace')}")
    return rate.value, ch.value, bps.value, total.value


def flac_index(data: bytes):
    """The frame-header candidates of a FLAC stream (wh_flac_index), sorted by offset:
    (offsets int64 [n], fields int32 [n][4] = header length, block size, channel assignment,
    bits per sample).  False candidates inside frame bodies may be among them."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    n = c_int64()
    rc = lib.wh_flac_index(_ptr(buf), len(buf), None, None, 0, ctypes.byref(n))
    if rc != 0:
        raise HipBackendError(f"wh_flac_index failed ({rc}): {lib.wh_flac_last_error().decode(errors='replace')}")
    offsets, fields = np.empty(n.value, np.int64), np.empty((n.value, 4), np.int32)
    lib.wh_flac_index(_ptr(buf), len(buf), _ptr(offsets), _ptr(fields), n.value, ctypes.byref(n))
    return offsets, fields


def decode_flac_indexed(data: bytes):
    """``decode_flac`` through the frame index on the host (wh_flac_decode_indexed, the CPU
    twin of the device decoder): (samples, sample_rate, bits_per_sample, path), path "device"
    when the indexed path ran and "host" when the stream went through wh_flac_decode."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    rate, ch, bps, total = flac_info(data)
    cap = total if total > 0 else len(buf) * 8
    out = np.empty((cap, ch), np.int32)
    n = c_int64()
    rc = lib.wh_flac_decode_indexed(_ptr(buf), len(buf), _ptr(out), cap, ctypes.byref(n))
    if rc != 0:
        raise HipBackendError(f"wh_flac_decode_indexed failed ({rc}): "
                              f"{lib.wh_flac_last_error().decode(errors='replace')}")
    return out[: n.value], rate, bps, FLAC_PATHS[lib.wh_flac_last_path()]


def wav_info(data: bytes) -> WavInfo:
    """The header of a WAV file's bytes (wh_wav_info; host only)."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    f = WhWavFmt()
    rc = lib.wh_wav_info(_ptr(buf) if len(buf) else None, len(buf), ctypes.byref(f))
    if rc != 0:
        msg = lib.wh_wav_last_error().decode(errors="replace") if len(buf) else "wav: empty file"
        raise HipBackendError(f"wh_wav_info failed ({rc}): {msg}")
    return WavInfo(f.encoding, f.channels, f.sample_rate, f.valid_bits, f.data_offset, f.n_frames)


class DeviceAudio:
    """Audio already resident in a context's HBM (``HipContext.audio_upload`` /
    ``audio_ingest`` / ``flac_ingest`` / ``wav_ingest``); ``transcribe`` then starts from device memory (no
    host-to-device copy).  ``offset``: where the segment starts in the resident buffer (0
    unless it was ingested behind other files).  ``decoded_on``: "device" or "host" for a
    FLAC stream given to ``flac_ingest``, None for anything else."""

    def __init__(self, ctx, n_samples: int, offset: int = 0, decoded_on: Optional[str] = None):
        self.ctx = ctx
        self.n_samples = n_samples
        self.offset = offset
        self.decoded_on = decoded_on


def max_windows_limit(dims: dict, dtype: str, max_group: int) -> int:
    """Largest max_windows a context can hold: the self-attention kernels address one
    layer's self-K / V cache ([windows][max_group][n_text_ctx][n]) with 32-bit byte offsets,
    so it must stay under 2 GiB (wh_runtime.hip init refuses larger caches)."""
    elem = 2 if dtype == "fp16" else 4
    per_window = int(max_group) * int(dims["n_text_ctx"]) * int(dims["n_text_state"]) * elem
    return max(0, ((1 << 31) - 4096 - 1) // per_window)


class HipContext:
    """One libwhisper_hip context = one model on one GPU (per process)."""

    def __init__(self, dims: dict, device: int = 0, dtype: str = "fp16", max_windows: int = 8, max_group: int = 5):
        lim = max_windows_limit(dims, dtype, max_group)
        if max_windows > lim:
            raise ValueError(f"max_windows={max_windows} with max_group={max_group} in {dtype}: one layer's self-KV cache "
                             f"would exceed 2 GiB (32-bit offsets in the self-attention kernels); at most {lim} windows")
        self.lib = load_library()
        self.dims = dict(dims)
        self.dtype = dtype
        self.device = device
        self.max_windows = max_windows
        self.max_group = max_group
        d = WhDims(**{k: int(dims[k]) for k, _ in WhDims._fields_})
        h = c_void_p()
        code = {"fp16": WH_F16, "fp32": WH_F32}[dtype]
        self._check(self.lib.wh_create(device, ctypes.byref(d), code, max_windows, max_group, ctypes.byref(h)),
                    "wh_create")
        self.h = h
        self.phrase_bias = None  # what set_phrase_bias installed: (phrases, boosts, start)

    # -- errors
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.wh_last_error().decode(errors="replace")
            raise HipBackendError(f"{what} failed ({rc}): {msg}")

    def close(self):
        """Release the context; raises HipBackendError if a HIP release failed (wh_destroy
        reports it instead of leaving the error pending for the next context)."""
        if getattr(self, "h", None):
            rc = self.lib.wh_destroy(self.h)
            # -1: refused (other contexts still read this one's weights), the context is
            # intact: keep the handle so close() can be retried once they are gone.  Any
            # other code: the context is released (a non-zero code reports a failed release)
            if rc != -1:
                self.h = None
            self._check(rc, "wh_destroy")

    def __del__(self):
        try:
            self.close()
        except HipBackendError as e:  # no raising from a finalizer: report it
            import warnings
            warnings.warn(str(e), RuntimeWarning)
        except Exception:
            pass

    # -- weights
    def load_tensor(self, name: str, value: np.ndarray):
        v = np.ascontiguousarray(value, dtype=np.float32)
        shape = (c_int64 * max(v.ndim, 1))(*v.shape)
        self._check(self.lib.wh_load_tensor(self.h, name.encode(), _ptr(v), shape, v.ndim), f"load {name}")

    def finalize(self):
        self._check(self.lib.wh_finalize(self.h), "wh_finalize")

    def set_mel_filters(self, n_mels: int, filters: np.ndarray):
        f = np.ascontiguousarray(filters, dtype=np.float32)
        assert f.shape == (n_mels, 201)
        self._check(self.lib.wh_set_mel_filters(self.h, n_mels, _ptr(f)), "wh_set_mel_filters")

    def set_phrase_bias(self, phrases: Optional[Sequence[Sequence[int]]] = None,
                        boosts: Optional[Sequence[float]] = None, start: float = 0.5):
        """Install the phrase table of the device decode loop (wh_set_phrase_bias,
        include/whisper_hip.h): ``phrases[j]`` are token ids, ``boosts[j]`` its boost, ``start``
        the share of a boost the first token gets.  No phrases: the table is cleared.  The next
        ``decode_begin`` uploads it; the library checks the limits and a refused call
        (HipBackendError) leaves the previous table, and ``self.phrase_bias``, as they were."""
        ph = tuple(tuple(int(t) for t in p) for p in (phrases or ()))
        if not ph:
            self._check(self.lib.wh_set_phrase_bias(self.h, 0, None, None, None, 0.0), "wh_set_phrase_bias")
            self.phrase_bias = None
            return
        bo = tuple(float(b) for b in boosts)
        if len(bo) != len(ph):
            raise ValueError("set_phrase_bias: one boost per phrase")
        tok = np.asarray([t for p in ph for t in p] or [0], dtype=np.int32)
        off = np.cumsum([0] + [len(p) for p in ph]).astype(np.int32)
        b = np.asarray(bo, dtype=np.float32)
        self._check(self.lib.wh_set_phrase_bias(self.h, len(ph), _ptr(tok), _ptr(off), _ptr(b), float(start)),
                    "wh_set_phrase_bias")
        self.phrase_bias = (ph, bo, float(start))

    # -- mel
    def log_mel(self, audio: np.ndarray, n_mels: int, padding: int = 0, normalize: bool = True) -> int:
        a = np.ascontiguousarray(audio, dtype=np.float32)
        nf = c_int64()
        self._check(self.lib.wh_log_mel(self.h, _ptr(a), a.shape[0], int(padding), n_mels, int(normalize),
                                        ctypes.byref(nf)), "wh_log_mel")
        return nf.value

    def audio_upload(self, audio: np.ndarray) -> "DeviceAudio":
        a = np.ascontiguousarray(audio, dtype=np.float32)
        self._check(self.lib.wh_audio_upload(self.h, _ptr(a), a.shape[0]), "wh_audio_upload")
        return DeviceAudio(self, a.shape[0])

    def _split_segments(self, n: int, count: int, dst_offset: int, decoded_on: Optional[str] = None):
        """What a split ingest returns: ``count`` segments of ``n`` samples back to back."""
        return [DeviceAudio(self, n, int(dst_offset) + k * n, decoded_on) for k in range(count)]

    def audio_ingest(self, pcm: np.ndarray, rate: int, bits: int, dst_offset: int = 0,
                     reserve: int = 0, channels: Optional[Sequence[int]] = None):
        """A decoded file's PCM ([frames][channels] integers of ``bits`` bits at ``rate`` Hz)
        -> the mono 16 kHz float32 waveform of ``audio.pcm_to_waveform``, computed on the
        device (wh_audio_ingest) into the resident buffer at sample ``dst_offset`` (0: a new
        list of segments; the end of the last one: appended).  int16 is uploaded when
        ``bits <= 16``, else int32.  A 1-D float32 array with ``rate == 16000`` is a
        waveform: copied unchanged.  ``channels`` (a sequence of channel indices): no mix, every
        selected channel becomes a segment of its own (wh_audio_ingest_split, the rows of
        ``audio.load_audio_channels``); the result is then a list of ``DeviceAudio`` in
        selection order, at consecutive offsets."""
        from .audio import SAMPLE_RATE, resample_filter
        a = np.asarray(pcm)
        n_out = c_int64()
        if a.dtype == np.float32 and a.ndim == 1 and int(rate) == SAMPLE_RATE:
            a = np.ascontiguousarray(a)
            args = (_ptr(a), WH_PCM_F32, a.shape[0], 1, 32, 1, 1, None, 0)
        else:
            if not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"audio_ingest: integer PCM or a float32 waveform at {SAMPLE_RATE} Hz, not "
                                f"{a.dtype} at {rate} Hz")
            a = a.reshape(a.shape[0], -1)
            fmt = WH_PCM_S16 if bits <= 16 else WH_PCM_S32
            a = np.ascontiguousarray(a, dtype=np.int16 if fmt == WH_PCM_S16 else np.int32)
            up, down, taps = resample_filter(int(rate))
            args = (_ptr(a), fmt, a.shape[0], a.shape[1], int(bits), up, down,
                    None if taps is None else _ptr(taps), 0 if taps is None else taps.shape[0])
        if channels is not None:
            sel = np.asarray(list(channels), dtype=np.int32)
            self._check(self.lib.wh_audio_ingest_split(self.h, *args, _ptr(sel), len(sel), int(dst_offset), int(reserve),
                                                       ctypes.byref(n_out)), "wh_audio_ingest_split")
            return self._split_segments(n_out.value, len(sel), dst_offset)
        self._check(self.lib.wh_audio_ingest(self.h, *args, int(dst_offset), int(reserve), ctypes.byref(n_out)),
                    "wh_audio_ingest")
        return DeviceAudio(self, n_out.value, int(dst_offset))

    def flac_ingest(self, data: bytes, dst_offset: int = 0, reserve: int = 0,
                    channels: Optional[Sequence[int]] = None):
        """A FLAC stream -> the waveform of ``audio.load_audio`` in the resident buffer, decoded
        on the device (wh_flac_ingest: frames in parallel, the PCM never on the host) with
        ``audio_ingest``'s segment semantics.  ``decoded_on`` of the result tells which decoder
        ran: "host" means the stream was outside the device path and went through
        ``decode_flac`` and ``audio_ingest``, with the same samples or the same error.
        ``channels``: as for ``audio_ingest`` (wh_flac_ingest_split), a list of ``DeviceAudio``."""
        from .audio import resample_filter
        buf = np.frombuffer(data, np.uint8)
        up, down, taps = resample_filter(flac_info(data)[0])
        n_out, path = c_int64(), c_int(-1)
        if channels is not None:
            sel = np.asarray(list(channels), dtype=np.int32)
            self._check(self.lib.wh_flac_ingest_split(
                self.h, _ptr(buf), len(buf), up, down, None if taps is None else _ptr(taps),
                0 if taps is None else taps.shape[0], _ptr(sel), len(sel), int(dst_offset), int(reserve),
                ctypes.byref(n_out), ctypes.byref(path)), "wh_flac_ingest_split")
            return self._split_segments(n_out.value, len(sel), dst_offset, FLAC_PATHS[path.value])
        self._check(self.lib.wh_flac_ingest(self.h, _ptr(buf), len(buf), up, down, None if taps is None else _ptr(taps),
                                            0 if taps is None else taps.shape[0], int(dst_offset), int(reserve),
                                            ctypes.byref(n_out), ctypes.byref(path)), "wh_flac_ingest")
        return DeviceAudio(self, n_out.value, int(dst_offset), FLAC_PATHS[path.value])

    def wav_ingest(self, data: bytes, dst_offset: int = 0, reserve: int = 0,
                   channels: Optional[Sequence[int]] = None):
        """A WAV file's bytes -> the waveform of ``audio.load_audio`` in the resident buffer
        (wh_wav_ingest), with ``audio_ingest``'s segment semantics.  Only the data chunk is
        uploaded, in the file's own sample encoding (8 / 16 / 24 / 32-bit PCM, 32 / 64-bit
        float, A-law, mu-law), and the resampling kernel reads it.  ``channels``: as for
        ``audio_ingest`` (wh_wav_ingest_split), a list of ``DeviceAudio``."""
        from .audio import resample_filter
        buf = np.frombuffer(data, np.uint8)
        up, down, taps = resample_filter(wav_info(data).sample_rate)
        n_out = c_int64()
        if channels is not None:
            sel = np.asarray(list(channels), dtype=np.int32)
            self._check(self.lib.wh_wav_ingest_split(
                self.h, _ptr(buf), len(buf), up, down, None if taps is None else _ptr(taps),
                0 if taps is None else taps.shape[0], _ptr(sel), len(sel), int(dst_offset), int(reserve),
                ctypes.byref(n_out)), "wh_wav_ingest_split")
            return self._split_segments(n_out.value, len(sel), dst_offset)
        self._check(self.lib.wh_wav_ingest(self.h, _ptr(buf), len(buf), up, down, None if taps is None else _ptr(taps),
                                           0 if taps is None else taps.shape[0], int(dst_offset), int(reserve),
                                           ctypes.byref(n_out)), "wh_wav_ingest")
        return DeviceAudio(self, n_out.value, int(dst_offset))

    # -- a resident stream (include/whisper_hip.h): audio that arrives in chunks
    def stream_begin(self, encoding: int, channels: int, rate: int, reserve: int = 0):
        """Open the context's stream of raw frames in ``encoding`` (a WH_WAV_* code) at ``rate``
        Hz; the resident audio becomes one empty segment that the appends grow."""
        from .audio import resample_filter
        up, down, taps = resample_filter(int(rate))
        self._check(self.lib.wh_stream_begin(self.h, int(encoding), int(channels), up, down,
                                             None if taps is None else _ptr(taps),
                                             0 if taps is None else taps.shape[0], int(reserve)), "wh_stream_begin")

    def stream_append(self, data, n_frames: int) -> int:
        """``n_frames`` frames (a contiguous uint8 array, or None with 0 frames) -> the samples
        this call added to the resident segment."""
        n_out = c_int64()
        self._check(self.lib.wh_stream_append(self.h, None if data is None else _ptr(data), int(n_frames),
                                              ctypes.byref(n_out)), "wh_stream_append")
        return n_out.value

    def stream_finish(self) -> int:
        """End of the input: the samples the resampler still held back are added; how many."""
        n_out = c_int64()
        self._check(self.lib.wh_stream_finish(self.h, ctypes.byref(n_out)), "wh_stream_finish")
        return n_out.value

    def stream_trim(self, n_drop: int):
        """Drop the first ``n_drop`` resident samples; the rest moves to sample 0."""
        self._check(self.lib.wh_stream_trim(self.h, int(n_drop)), "wh_stream_trim")

    def stream_info(self):
        """(frames appended, samples emitted, samples dropped, finished) of the open stream."""
        fi, so, sd, fin = c_int64(), c_int64(), c_int64(), c_int()
        self._check(self.lib.wh_stream_info(self.h, ctypes.byref(fi), ctypes.byref(so), ctypes.byref(sd),
                                            ctypes.byref(fin)), "wh_stream_info")
        return fi.value, so.value, sd.value, bool(fin.value)

    # -- a pool of streams (include/whisper_hip.h): many live recordings, fed and decoded together
    def pool_create(self, n_slots: int, slot_samples: int):
        """Give the context ``n_slots`` stream slots of at most ``slot_samples`` 16 kHz samples."""
        self._check(self.lib.wh_pool_create(self.h, int(n_slots), int(slot_samples)), "wh_pool_create")

    def pool_destroy(self):
        self._check(self.lib.wh_pool_destroy(self.h), "wh_pool_destroy")

    def pool_open(self, slot: int, encoding: int, channels: int, rate: int):
        """Open ``slot`` for raw frames in ``encoding`` (a WH_WAV_* code) at ``rate`` Hz."""
        from .audio import resample_filter
        up, down, taps = resample_filter(int(rate))
        self._check(self.lib.wh_pool_open(self.h, int(slot), int(encoding), int(channels), up, down,
                                          None if taps is None else _ptr(taps),
                                          0 if taps is None else taps.shape[0]), "wh_pool_open")

    def pool_close(self, slot: int):
        self._check(self.lib.wh_pool_close(self.h, int(slot)), "wh_pool_close")

    def pool_append(self, slots: Sequence[int], packets: Sequence, n_frames: Sequence[int]) -> List[int]:
        """One packet per slot in one call: ``packets[i]`` (a contiguous uint8 array, or None with
        0 frames) holds ``n_frames[i]`` frames for ``slots[i]``.  Returns the samples each slot
        emitted.  One upload, one launch and one synchronisation for the whole call."""
        n = len(slots)
        sl = np.asarray(list(slots), dtype=np.int32).reshape(-1)
        nf = np.asarray(list(n_frames), dtype=np.int64).reshape(-1)
        if len(packets) != n or nf.shape[0] != n:
            raise ValueError(f"pool_append: {n} slots, {len(packets)} packets, {nf.shape[0]} frame counts")
        ptrs = (c_void_p * max(n, 1))(*[None if p is None else p.ctypes.data for p in packets])
        n_out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self.lib.wh_pool_append(self.h, n, _ptr(sl) if n else None, ptrs, _ptr(nf) if n else None,
                                            _ptr(n_out)), "wh_pool_append")
        return [int(x) for x in n_out[:n]]

    def pool_finish(self, slots: Sequence[int]) -> List[int]:
        """End the input of ``slots``: the samples each resampler still held back; how many each."""
        sl = np.asarray(list(slots), dtype=np.int32).reshape(-1)
        n_out = np.zeros(max(len(sl), 1), dtype=np.int64)
        self._check(self.lib.wh_pool_finish(self.h, len(sl), _ptr(sl) if len(sl) else None, _ptr(n_out)),
                    "wh_pool_finish")
        return [int(x) for x in n_out[:len(sl)]]

    def pool_trim(self, slots: Sequence[int], n_drop: Sequence[int]):
        """Drop the first ``n_drop[i]`` resident samples of ``slots[i]``, all in one launch."""
        sl = np.asarray(list(slots), dtype=np.int32).reshape(-1)
        nd = np.asarray(list(n_drop), dtype=np.int64).reshape(-1)
        if nd.shape[0] != sl.shape[0]:
            raise ValueError(f"pool_trim: {sl.shape[0]} slots, {nd.shape[0]} counts")
        self._check(self.lib.wh_pool_trim(self.h, len(sl), _ptr(sl) if len(sl) else None,
                                          _ptr(nd) if len(sl) else None), "wh_pool_trim")

    def pool_info(self, slot: int):
        """(frames appended, samples emitted, samples dropped, finished) of an open slot."""
        fi, so, sd, fin = c_int64(), c_int64(), c_int64(), c_int()
        self._check(self.lib.wh_pool_info(self.h, int(slot), ctypes.byref(fi), ctypes.byref(so), ctypes.byref(sd),
                                          ctypes.byref(fin)), "wh_pool_info")
        return fi.value, so.value, sd.value, bool(fin.value)

    def pool_read(self, slot: int, offset: int, n: int) -> np.ndarray:
        """Resident samples [offset, offset + n) of ``slot`` as a host array."""
        out = np.empty(max(int(n), 0), dtype=np.float32)
        self._check(self.lib.wh_pool_read(self.h, int(slot), _ptr(out), int(offset), int(n)), "wh_pool_read")
        return out

    def pool_log_mel(self, slots: Sequence[int], n_mels: int, padding: int = 0) -> np.ndarray:
        """``log_mel_batch`` with the files taken from the slots' resident buffers, in the given
        order.  Returns the frame bases (int64, ``len(slots) + 1``)."""
        sl = np.asarray(list(slots), dtype=np.int32).reshape(-1)
        base = np.zeros(len(sl) + 1, dtype=np.int64)
        self._check(self.lib.wh_pool_log_mel(self.h, len(sl), _ptr(sl) if len(sl) else None, int(padding), n_mels,
                                             _ptr(base)), "wh_pool_log_mel")
        return base

    # -- the causal speech detector of a live stream (include/whisper_hip.h)
    @staticmethod
    def _svad_opts(params) -> WhSvadOpts:
        return WhSvadOpts(ratio_q8=int(params.ratio_q8), t_lo=int(params.t_lo), t_hi=int(params.t_hi),
                          percentile=int(params.percentile), window=int(params.window),
                          min_silence=int(params.min_silence), min_speech=int(params.min_speech))

    @staticmethod
    def _svad_state(s: WhSvadState):
        from .vad import StreamVadState
        return StreamVadState(*(int(getattr(s, k)) for k in StreamVadState._fields))

    def pool_vad_enable(self, slot: int, params):
        """Give ``slot`` (open, no frames taken yet) a detector; ``params``: ``vad.StreamVadParams``."""
        o = self._svad_opts(params)
        self._check(self.lib.wh_pool_vad_enable(self.h, int(slot), ctypes.byref(o)), "wh_pool_vad_enable")

    def pool_vad_state(self, slots: Sequence[int]):
        """``vad.StreamVadState`` of each detecting slot as of its last append or finish."""
        sl = np.asarray(list(slots), dtype=np.int32).reshape(-1)
        out = (WhSvadState * max(len(sl), 1))()
        self._check(self.lib.wh_pool_vad_state(self.h, len(sl), _ptr(sl) if len(sl) else None, out), "wh_pool_vad_state")
        return [self._svad_state(out[i]) for i in range(len(sl))]

    def pool_vad_read(self, slot: int, window: int):
        """(ring uint8 [window], hist uint32 [160]) of a detecting slot, for inspection."""
        ring = np.zeros(max(int(window), 1), dtype=np.uint8)
        hist = np.zeros(160, dtype=np.uint32)
        self._check(self.lib.wh_pool_vad_read(self.h, int(slot), _ptr(ring), int(window), _ptr(hist)), "wh_pool_vad_read")
        return ring[:max(int(window), 0)], hist

    def stream_vad_enable(self, params):
        """Give the open stream (no frames taken yet) a detector; ``params``: ``vad.StreamVadParams``."""
        o = self._svad_opts(params)
        self._check(self.lib.wh_stream_vad_enable(self.h, ctypes.byref(o)), "wh_stream_vad_enable")

    def stream_vad_state(self):
        """``vad.StreamVadState`` of the stream as of its last append or finish."""
        out = WhSvadState()
        self._check(self.lib.wh_stream_vad_state(self.h, ctypes.byref(out)), "wh_stream_vad_state")
        return self._svad_state(out)

    def flac_decode_device(self, data: bytes):
        """``decode_flac`` on the device (wh_flac_decode_device): (samples int32
        [frames][channels], sample_rate, bits_per_sample, path), path "device" or "host"."""
        buf = np.frombuffer(data, np.uint8)
        rate, ch, bps, total = flac_info(data)
        cap = total if total > 0 else len(buf) * 8
        out = np.empty((cap, ch), np.int32)
        n, path = c_int64(), c_int(-1)
        self._check(self.lib.wh_flac_decode_device(self.h, _ptr(buf), len(buf), _ptr(out), cap, ctypes.byref(n),
                                                   ctypes.byref(path)), "wh_flac_decode_device")
        return out[: n.value], rate, bps, FLAC_PATHS[path.value]

    def audio_read(self, offset: int, n: int) -> np.ndarray:
        """Resident samples [offset, offset + n) as a host array."""
        out = np.empty(max(int(n), 0), dtype=np.float32)
        self._check(self.lib.wh_audio_read(self.h, _ptr(out), int(offset), int(n)), "wh_audio_read")
        return out

    # -- speech spans
    def speech_spans(self, params, n_files: int = 1, cap: int = 256):
        """wh_speech_spans on the first ``n_files`` resident segments: per file (spans int32
        [k][2] in frames, threshold T).  ``params``: ``vad.VadParams`` (the integers of the
        definition).  ``cap`` is the room per file of the first try (the library trims it to
        what the largest file could fill, so a generous value costs a short file nothing); a
        file with more spans reports how many and the call, both kernels, is repeated once
        with that room."""
        o = WhVadOpts(ratio_q8=int(params.ratio_q8), t_lo=int(params.t_lo), t_hi=int(params.t_hi),
                      percentile=int(params.percentile), min_silence=int(params.min_silence),
                      min_speech=int(params.min_speech), pad=int(params.pad))
        n_files, cap = int(n_files), max(int(cap), 0)
        counts = np.zeros(max(n_files, 1), dtype=np.int32)
        thr = np.zeros(max(n_files, 1), dtype=np.uint64)
        for _ in range(2):
            spans = np.zeros((max(n_files, 1), max(cap, 1), 2), dtype=np.int32)
            self._check(self.lib.wh_speech_spans(self.h, ctypes.byref(o), n_files, _ptr(spans), cap, _ptr(counts),
                                                 _ptr(thr)), "wh_speech_spans")
            need = int(counts[:n_files].max())
            if need <= cap:
                return [(spans[i, :counts[i]].copy(), int(thr[i])) for i in range(n_files)]
            cap = need
        raise HipBackendError(f"wh_speech_spans asked for room twice ({need} spans after {cap})")

    def frame_energy(self, file: int = 0):
        """(E uint64 [F], histogram uint32 [160]) of resident segment ``file``
        (wh_frame_energy_read: the detector's first kernel alone)."""
        n = self.lib.wh_frame_energy_read(self.h, int(file), None, 0, None)  # the size query
        self._check(0 if n > 0 else (n or -1), "wh_frame_energy_read")
        energy = np.zeros(n, dtype=np.uint64)
        hist = np.zeros(160, dtype=np.uint32)
        self._check(self.lib.wh_frame_energy_read(self.h, int(file), _ptr(energy), n, _ptr(hist)),
                    "wh_frame_energy_read")
        return energy, hist

    def log_mel_batch_resident(self, n_samples: Sequence[int], n_mels: int, padding: int = 0) -> np.ndarray:
        """``log_mel_batch`` of the resident segments (``audio_ingest`` back to back), which
        must be exactly these lengths; nothing is uploaded and they stay resident."""
        n = np.asarray(list(n_samples), dtype=np.int64)
        base = np.zeros(len(n) + 1, dtype=np.int64)
        self._check(self.lib.wh_log_mel_batch(self.h, None, len(n), _ptr(n) if len(n) else None, int(padding), n_mels,
                                              _ptr(base)), "wh_log_mel_batch")
        return base

    def log_mel_resident(self, n_samples: int, n_mels: int, padding: int = 0, normalize: bool = True) -> int:
        nf = c_int64()
        self._check(self.lib.wh_log_mel(self.h, None, n_samples, int(padding), n_mels, int(normalize),
                                        ctypes.byref(nf)), "wh_log_mel")
        return nf.value

    def log_mel_frames(self, audio: Optional[np.ndarray], n_samples: int, n_mels: int, frame0: int, count: int,
                       padding: int = 0, normalize: bool = True) -> int:
        """Frames [frame0, frame0+count) of the padded file's log-mel (audio None: the
        resident buffer).  Returns the whole file's frame count."""
        a = None if audio is None else np.ascontiguousarray(audio, dtype=np.float32)
        tot = c_int64()
        self._check(self.lib.wh_log_mel_frames(self.h, None if a is None else _ptr(a), int(n_samples), int(padding),
                                               n_mels, int(frame0), int(count), int(normalize), ctypes.byref(tot)),
                    "wh_log_mel_frames")
        return tot.value

    def mel_max(self) -> float:
        g = c_float()
        self._check(self.lib.wh_mel_max(self.h, ctypes.byref(g)), "wh_mel_max")
        return g.value

    def log_mel_batch(self, audios: Sequence[np.ndarray], n_mels: int, padding: int = 0) -> np.ndarray:
        """Log-mel of several files in one device pass, each normalised with its own max
        exactly as ``log_mel`` does for it alone.  Returns the frame bases (int64,
        ``len(audios) + 1``): file i owns absolute frames [base[i], base[i+1]) of the
        context mel, which ``encode`` / ``mel_read`` address as before."""
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in audios]
        n = np.asarray([a.shape[0] for a in arrs], dtype=np.int64)
        cat = np.concatenate(arrs) if arrs and n.sum() > 0 else np.zeros(1, dtype=np.float32)
        base = np.zeros(len(arrs) + 1, dtype=np.int64)
        self._check(self.lib.wh_log_mel_batch(self.h, _ptr(cat), len(arrs), _ptr(n) if len(arrs) else None,
                                              int(padding), n_mels, _ptr(base)), "wh_log_mel_batch")
        return base

    def mel_max_batch(self, n_files: int) -> np.ndarray:
        """Raw log10 max of each file of the last ``log_mel_batch``."""
        g = np.empty(max(int(n_files), 1), dtype=np.float32)
        self._check(self.lib.wh_mel_max_batch(self.h, _ptr(g), int(n_files)), "wh_mel_max_batch")
        return g[:n_files]

    def mel_normalize(self, gmax: float):
        self._check(self.lib.wh_mel_normalize(self.h, float(gmax)), "wh_mel_normalize")

    def mel_read(self, n_mels: int, frame0: int, n_frames: int) -> np.ndarray:
        out = np.empty((n_mels, n_frames), dtype=np.float32)
        self._check(self.lib.wh_mel_read(self.h, _ptr(out), frame0, n_frames), "wh_mel_read")
        return out

    def mel_write(self, mel: np.ndarray):
        m = np.ascontiguousarray(mel, dtype=np.float32)
        self._check(self.lib.wh_mel_write(self.h, _ptr(m), m.shape[1]), "wh_mel_write")

    # -- encoder
    def encode(self, seeks: Sequence[int], segs: Sequence[int]):
        s = np.asarray(seeks, dtype=np.int64)
        g = np.asarray(segs, dtype=np.int32)
        self._check(self.lib.wh_encode(self.h, len(s), _ptr(s), _ptr(g)), "wh_encode")

    def audio_features(self, slot: int) -> np.ndarray:
        out = np.empty((self.dims["n_audio_ctx"], self.dims["n_audio_state"]), dtype=np.float32)
        self._check(self.lib.wh_read_audio_features(self.h, slot, _ptr(out)), "wh_read_audio_features")
        return out

    def cross_kv(self, slot: int, layer: int):
        H = self.dims["n_text_head"]
        k = np.empty((H, self.dims["n_audio_ctx"], 64), dtype=np.float32)
        v = np.empty_like(k)
        self._check(self.lib.wh_read_cross_kv(self.h, slot, layer, _ptr(k), _ptr(v)), "wh_read_cross_kv")
        return k, v

    # -- decoding
    def decode_begin(self, opts: WhDecodeOpts, init_tokens: Sequence[Sequence[int]], sot_index: Sequence[int],
                     slots: Optional[Sequence[int]] = None):
        """Decode window w = init_tokens[w] over encoder slot slots[w] (default w)."""
        n = len(init_tokens)
        mx = max(len(t) for t in init_tokens)
        arr = np.zeros((n, mx), dtype=np.int32)
        for i, t in enumerate(init_tokens):
            arr[i, :len(t)] = t
        nin = np.asarray([len(t) for t in init_tokens], dtype=np.int32)
        si = np.asarray(sot_index, dtype=np.int32)
        if slots is None:
            self._check(self.lib.wh_decode_begin(self.h, n, ctypes.byref(opts), _ptr(arr), _ptr(nin), mx, _ptr(si)),
                        "wh_decode_begin")
        else:
            sl = np.ascontiguousarray(slots, dtype=np.int32)
            assert len(sl) == n
            self._check(self.lib.wh_decode_begin_slots(self.h, n, _ptr(sl), ctypes.byref(opts), _ptr(arr), _ptr(nin),
                                                       mx, _ptr(si)), "wh_decode_begin_slots")

    def decode_steps(self, max_steps: int) -> int:
        nd = c_int()
        self._check(self.lib.wh_decode_steps(self.h, int(max_steps), ctypes.byref(nd)), "wh_decode_steps")
        return nd.value

    def decode_read(self, slot: int, group: int):
        hctx = self.dims["n_text_ctx"] + 1
        maxc = max(1, self.lib.wh_decode_maxc(self.h))
        toks = np.zeros((group, hctx), dtype=np.int32)
        slp = np.zeros(group, dtype=np.float32)
        ln = np.zeros(1, dtype=np.int32)
        fn = np.zeros(1, dtype=np.int32)
        ftok = np.zeros((maxc, hctx), dtype=np.int32)
        flen = np.zeros(maxc, dtype=np.int32)
        fsc = np.zeros(maxc, dtype=np.float32)
        nsp = np.zeros(1, dtype=np.float32)
        self._check(self.lib.wh_decode_read(self.h, slot, _ptr(toks), _ptr(slp), _ptr(ln), _ptr(fn), _ptr(ftok),
                                            _ptr(flen), _ptr(fsc), _ptr(nsp)), "wh_decode_read")
        n = int(fn[0])
        return dict(tokens=toks, sum_logprobs=slp, length=int(ln[0]), fin_tokens=ftok[:n], fin_len=flen[:n],
                    fin_score=fsc[:n], no_speech_prob=float(nsp[0]))

    # -- per-step boundary (decoder256Predict / decoder1Predict / rearrange_mkv roles)
    def prefill(self, init_tokens: Sequence[Sequence[int]], group: int, sot_index: Sequence[int],
                logits: bool = True):
        """wh_prefill: first pass of each window's initial tokens (windows = slots
        0..n-1); returns [n][2][V] logits at (sot_index, last) or None."""
        n = len(init_tokens)
        mx = max(len(t) for t in init_tokens)
        arr = np.zeros((n, mx), dtype=np.int32)
        for i, t in enumerate(init_tokens):
            arr[i, :len(t)] = t
        nin = np.asarray([len(t) for t in init_tokens], dtype=np.int32)
        si = np.asarray(sot_index, dtype=np.int32)
        out = np.empty((n, 2, self.dims["n_vocab"]), dtype=np.float32) if logits else None
        self._check(self.lib.wh_prefill(self.h, n, int(group), _ptr(arr), _ptr(nin), mx, _ptr(si),
                                        _ptr(out) if out is not None else None), "wh_prefill")
        return out

    def step(self, tokens: Sequence[int], text_offsets: Optional[Sequence[int]] = None, logits: bool = True):
        """wh_step: rows append ``tokens`` and run one decoder step; [rows][V] logits."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        off = None if text_offsets is None else np.ascontiguousarray(text_offsets, dtype=np.int32)
        out = np.empty((len(t), self.dims["n_vocab"]), dtype=np.float32) if logits else None
        self._check(self.lib.wh_step(self.h, _ptr(t), _ptr(off) if off is not None else None,
                                     _ptr(out) if out is not None else None), "wh_step")
        return out

    def reorder_kv(self, source_rows: Sequence[int]):
        """wh_reorder_kv: row r continues row source_rows[r] (same window)."""
        s = np.ascontiguousarray(source_rows, dtype=np.int32)
        self._check(self.lib.wh_reorder_kv(self.h, _ptr(s)), "wh_reorder_kv")

    def prefill_logits(self, slot: int, tokens: Sequence[int], align_heads: Sequence[int] = ()):
        t = np.asarray(tokens, dtype=np.int32)
        V = self.dims["n_vocab"]
        lg = np.empty((len(t), V), dtype=np.float32)
        ah = np.asarray(align_heads, dtype=np.int32)
        qk = np.empty((len(ah), len(t), self.dims["n_audio_ctx"]), dtype=np.float32) if len(ah) else None
        self._check(self.lib.wh_prefill_logits(self.h, slot, _ptr(t), len(t), _ptr(lg),
                                               _ptr(ah) if len(ah) else None, len(ah),
                                               _ptr(qk) if qk is not None else None), "wh_prefill_logits")
        return lg, qk

    def align(self, slot: int, tokens: Sequence[int], n_sot: int, num_frames: int, align_heads: Sequence[int],
              medfilt_width: int = 7):
        """find_alignment's device half (timing.py:163-231): returns (text_token_probs [T],
        text_indices, time_indices) of dtw(-matrix)."""
        return self.align_batch([slot], [tokens], n_sot, [num_frames], align_heads, medfilt_width)[0]

    def align_batch(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], n_sot: int,
                    num_frames: Sequence[int], align_heads: Sequence[int], medfilt_width: int = 7):
        """wh_align_batch: one (probs, text_indices, time_indices) per window."""
        n = len(slots)
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]))
        ntok = np.asarray([len(t) for t in token_lists], dtype=np.int32)
        nfr = np.asarray(num_frames, dtype=np.int32)
        sl = np.asarray(slots, dtype=np.int32)
        ah = np.ascontiguousarray(align_heads, dtype=np.int32)
        T = ntok - n_sot - 2
        widths = (T + 1) + nfr // 2
        probs = np.zeros(max(int(T.sum()), 1), dtype=np.float32)
        paths = np.zeros(max(int(2 * widths.sum()), 1), dtype=np.int32)
        plens = np.zeros(n, dtype=np.int32)
        self._check(self.lib.wh_align_batch(self.h, n, _ptr(sl), _ptr(toks), _ptr(ntok), n_sot, _ptr(nfr), _ptr(ah),
                                            len(ah), medfilt_width, _ptr(probs), _ptr(paths), _ptr(plens)),
                    "wh_align_batch")
        out, po, qo = [], 0, 0
        for w in range(n):
            L, W = int(plens[w]), int(widths[w])
            path = paths[qo:qo + 2 * W].reshape(2, W)
            out.append((probs[po:po + T[w]].copy(), path[0, :L].copy(), path[1, :L].copy()))
            po += int(T[w])
            qo += 2 * W
        return out

    def align_batch_open(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], n_sot: int,
                         num_frames: Sequence[int], align_heads: Sequence[int], min_rows: Sequence[int],
                         row_penalty: float, medfilt_width: int = 7):
        """wh_align_batch_open: one (probs, text_indices, time_indices, end_row) per window;
        ``min_rows[w] == 0`` runs window w closed.  It writes the self-KV rows of the slots."""
        n = len(slots)
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in token_lists]))
        ntok = np.asarray([len(t) for t in token_lists], dtype=np.int32)
        nfr = np.asarray(num_frames, dtype=np.int32)
        sl = np.asarray(slots, dtype=np.int32)
        ah = np.ascontiguousarray(align_heads, dtype=np.int32)
        mr = np.ascontiguousarray(min_rows, dtype=np.int32)
        if len(mr) != n or len(ntok) != n or len(nfr) != n:
            raise ValueError("align_batch_open: one token list, num_frames and min_rows per slot")
        T = np.maximum(ntok - n_sot - 2, 0)
        widths = (T + 1) + np.maximum(nfr, 0) // 2
        probs = np.zeros(max(int(T.sum()), 1), dtype=np.float32)
        paths = np.zeros(max(int(2 * widths.sum()), 1), dtype=np.int32)
        plens = np.zeros(n, dtype=np.int32)
        ends = np.zeros(n, dtype=np.int32)
        self._check(self.lib.wh_align_batch_open(self.h, n, _ptr(sl), _ptr(toks), _ptr(ntok), n_sot, _ptr(nfr),
                                                 _ptr(ah), len(ah), medfilt_width, _ptr(mr), float(row_penalty),
                                                 _ptr(probs), _ptr(paths), _ptr(plens), _ptr(ends)),
                    "wh_align_batch_open")
        out, po, qo = [], 0, 0
        for w in range(n):
            L, W = int(plens[w]), int(widths[w])
            path = paths[qo:qo + 2 * W].reshape(2, W)
            out.append((probs[po:po + T[w]].copy(), path[0, :L].copy(), path[1, :L].copy(), int(ends[w])))
            po += int(T[w])
            qo += 2 * W
        return out

    def dtw(self, x: np.ndarray) -> np.ndarray:
        """timing.dtw(x) on the GPU: [2][path length] (text indices, time indices)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        N, M = x.shape
        path = np.zeros((2, N + M), dtype=np.int32)
        n = c_int(0)
        self._check(self.lib.wh_dtw(self.h, _ptr(x), N, M, _ptr(path), ctypes.byref(n)), "wh_dtw")
        return path[:, :n.value].copy()

    def dtw_open(self, x: np.ndarray, min_rows: int = 1, row_penalty: float = 4.0):
        """wh_dtw_open (include/whisper_hip.h, open-end DTW): (path [2][length], end_row,
        scores [N]) of cost matrix x [N][M]; ``min_rows == 0`` is the closed ``dtw(x)``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError(f"dtw_open: x is not a matrix (shape {x.shape})")
        N, M = x.shape
        path = np.zeros((2, N + M), dtype=np.int32)
        scores = np.zeros(max(N, 1), dtype=np.float32)
        n, e = c_int(0), c_int(0)
        self._check(self.lib.wh_dtw_open(self.h, _ptr(x), N, M, int(min_rows), float(row_penalty), _ptr(path),
                                         ctypes.byref(n), ctypes.byref(e), _ptr(scores)), "wh_dtw_open")
        return path[:, :n.value].copy(), e.value, scores[:N].copy()

    def stats(self) -> dict:
        out = (c_double * N_STATS)()
        self._check(self.lib.wh_stats(self.h, out, N_STATS), "wh_stats")
        keys = ["mel_ms", "encode_ms", "prefill_ms", "steps_ms", "steps", "encode_windows", "ingest_copy_ms",
                "ingest_kernel_ms", "flac_upload_ms", "flac_parse_ms", "flac_restore_ms", "flac_gather_ms",
                "flac_resample_ms", "flac_index_ms", "vad_energy_ms", "vad_spans_ms"]
        return {k: out[i] for i, k in enumerate(keys)}

    def sync(self):
        self._check(self.lib.wh_sync(self.h), "wh_sync")

    def token_ms(self, reset: bool = False) -> np.ndarray:
        """Per-token wall ms of each decode_steps chunk since the last reset."""
        n = c_int(0)
        self._check(self.lib.wh_token_ms(self.h, None, 0, ctypes.byref(n), 0), "wh_token_ms")
        out = np.zeros(max(n.value, 1), np.float32)
        self._check(self.lib.wh_token_ms(self.h, _ptr(out), n.value, ctypes.byref(n), int(reset)), "wh_token_ms")
        return out[:n.value]

    def step_kernels(self, n_win: int, group: int) -> dict:
        """The kernels the decoder step runs for this batch shape (wh_step_kernels):
        {"proj", "xattn", "self_attn", "tail"}."""
        buf = ctypes.create_string_buffer(256)
        n = self.lib.wh_step_kernels(self.h, n_win, group, buf, 256)
        self._check(0 if n >= 0 else n, "wh_step_kernels")
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(","))

    def time_stage(self, what: int, iters: int) -> float:
        ms = c_double()
        self._check(self.lib.wh_time_stage(self.h, what, iters, ctypes.byref(ms)), "wh_time_stage")
        return ms.value
