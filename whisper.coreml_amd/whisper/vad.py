"""Speech spans: which parts of a waveform hold speech, so that only those are encoded and
decoded (``transcribe(..., skip_silence=True)``).

The detector is an energy threshold over the mel's own frames (160 samples, 100 per
second), defined in integers so that the device kernels (``wh_speech_spans``,
csrc/wh_vad.hip) and this numpy restatement agree exactly; include/whisper_hip.h holds the
definition:

1. quantise: ``q = clip(rint(32768 * x), -32768, 32767)`` in float32 (NaN counts as 0);
2. frame energy: ``E[f] = sum q^2`` over samples ``[160 f, 160 f + 160)``, zeros past the end;
3. histogram of ``E`` in quarter-octave bins (``energy_bin`` / ``bin_edge``);
4. the noise level ``N`` is the lower edge of the bin that holds the ``percentile``-th
   percentile frame, the threshold ``T = clamp((N * ratio_q8) >> 8, t_lo, t_hi)``;
5. frames with ``E > T`` are active; gaps shorter than ``min_silence`` close, runs shorter
   than ``min_speech`` drop, the rest are padded by ``pad`` and merged where they touch.

The functions here are the reference of the tests and serve arrays that are not resident
on a device; ``speech_spans`` is the device path.  Options are given in decibels (relative
to a full-scale frame, ``160 * 2^30``) and seconds and turned into the integers of steps 4
and 5 by ``resolve_options``.
"""

from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from .audio import FRAMES_PER_SECOND, HOP_LENGTH

N_BINS = 160
FULL_SCALE = HOP_LENGTH << 30  # the largest frame energy: 160 samples of -32768

DEFAULTS = dict(percentile=10, margin_db=10.0, floor_db=-60.0, ceil_db=-35.0, min_silence=2.0, min_speech=0.25,
                pad=0.4)


class VadParams(NamedTuple):
    """The integers of the definition (``wh_vad_opts``); durations in frames."""
    percentile: int
    ratio_q8: int
    t_lo: int
    t_hi: int
    min_silence: int
    min_speech: int
    pad: int


def resolve_options(**opts) -> VadParams:
    """User options (``DEFAULTS``: decibels and seconds) -> ``VadParams``; raises ValueError on
    an unknown option or a value out of range."""
    unknown = set(opts) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"unknown speech-span option(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    o = dict(DEFAULTS, **opts)
    pct = o["percentile"]
    if isinstance(pct, bool) or not isinstance(pct, (int, np.integer)) or not 1 <= pct <= 99:
        raise ValueError(f"percentile must be an integer from 1 to 99, not {pct!r}")
    for k in ("margin_db", "floor_db", "ceil_db", "min_silence", "min_speech", "pad"):
        v = o[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{k} must be a finite number, not {v!r}")
    if not 0 <= o["margin_db"] <= 40:
        raise ValueError(f"margin_db must be within 0..40, not {o['margin_db']!r}")
    if not o["floor_db"] <= o["ceil_db"] <= 0:
        raise ValueError(f"need floor_db <= ceil_db <= 0, not {o['floor_db']!r}, {o['ceil_db']!r}")
    frames = {}
    for k in ("min_silence", "min_speech", "pad"):
        if o[k] < 0:
            raise ValueError(f"{k} is a duration in seconds and cannot be negative ({o[k]!r})")
        frames[k] = int(round(float(o[k]) * FRAMES_PER_SECOND))
        if frames[k] > 1 << 30:
            raise ValueError(f"{k} = {o[k]!r} s is out of range")
    return VadParams(percentile=int(pct), ratio_q8=int(round(256 * 10 ** (float(o["margin_db"]) / 10))),
                     t_lo=int(round(FULL_SCALE * 10 ** (float(o["floor_db"]) / 10))),
                     t_hi=int(round(FULL_SCALE * 10 ** (float(o["ceil_db"]) / 10))), **frames)


# ---------------------------------------------------------------- steps 1-3
def quantise(waveform) -> np.ndarray:
    """Step 1: int32 ``q`` of a float32 waveform."""
    x = np.ascontiguousarray(waveform, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.float32(32768.0) * x)  # float32 product (exact), half to even
    r = np.where(np.isnan(r), np.float32(0.0), np.clip(r, np.float32(-32768.0), np.float32(32767.0)))
    return r.astype(np.int32)


def frame_energy_host(waveform) -> np.ndarray:
    """Step 2: uint64 ``E`` of ``ceil(n / 160)`` frames."""
    q = quantise(waveform).astype(np.int64)
    n_frames = -(-len(q) // HOP_LENGTH)
    sq = np.zeros(n_frames * HOP_LENGTH, dtype=np.int64)
    sq[:len(q)] = q * q
    return sq.reshape(n_frames, HOP_LENGTH).sum(axis=1).astype(np.uint64)


def energy_bin(energy: int) -> int:
    """Step 3: the bin of one energy."""
    e = int(energy)
    if e == 0:
        return 0
    m = e.bit_length() - 1
    sub = ((e >> (m - 2)) if m >= 2 else (e << (2 - m))) & 3
    return 1 + 4 * m + sub


def bin_edge(b: int) -> int:
    """The lower edge of a bin (bin 0 holds only 0)."""
    if b < 1:
        return 0
    m, sub = (b - 1) >> 2, (b - 1) & 3
    return (4 + sub) << (m - 2) if m >= 2 else (4 + sub) >> (2 - m)


def histogram_host(energy: np.ndarray) -> np.ndarray:
    """uint32 counts of the ``N_BINS`` bins (``energy_bin`` of every frame, vectorised)."""
    e = np.asarray(energy, dtype=np.uint64)
    bins = np.zeros(len(e), dtype=np.int64)
    nz = e > 0
    v = e[nz].astype(np.int64)  # at most 160 * 2^30
    m = np.frexp(v.astype(np.float64))[1].astype(np.int64) - 1  # floor(log2), exact below 2^53
    sub = np.where(m >= 2, v >> np.maximum(m - 2, 0), v << np.maximum(2 - m, 0)) & 3
    bins[nz] = 1 + 4 * m + sub
    return np.bincount(bins, minlength=N_BINS).astype(np.uint32)


# ---------------------------------------------------------------- steps 4-5
def threshold_host(hist: Sequence[int], n_frames: int, p: VadParams) -> int:
    """Step 4: ``T`` from a file's histogram."""
    rank = max(1, -(-n_frames * p.percentile // 100))
    cum = 0
    noise = 0
    for b, c in enumerate(hist):
        cum += int(c)
        if cum >= rank:
            noise = bin_edge(b)
            break
    return min(max((noise * p.ratio_q8) >> 8, p.t_lo), p.t_hi)


def spans_from_energy(energy: Sequence[int], threshold: int, min_silence: int, min_speech: int,
                      pad: int) -> List[Tuple[int, int]]:
    """Step 5 on its own: ``[(start, end), ...]`` in frames from ``E`` and ``T``."""
    e = np.asarray(energy, dtype=np.uint64)
    n_frames = len(e)
    active = np.flatnonzero(e > np.uint64(threshold))
    runs: List[List[int]] = []
    for f in active.tolist():  # close the gaps shorter than min_silence
        if runs and (f == runs[-1][1] or f - runs[-1][1] < min_silence):
            runs[-1][1] = f + 1
        else:
            runs.append([f, f + 1])
    out: List[List[int]] = []
    for s, t in runs:
        if t - s < min_speech:
            continue
        s, t = max(0, s - pad), min(n_frames, t + pad)
        if out and s <= out[-1][1]:
            out[-1][1] = t
        else:
            out.append([s, t])
    return [(s, t) for s, t in out]


def speech_frames_host(waveform, **opts) -> Tuple[List[Tuple[int, int]], int]:
    """All five steps on the host: (spans in frames, threshold ``T``)."""
    p = resolve_options(**opts)
    energy = frame_energy_host(waveform)
    t = threshold_host(histogram_host(energy), len(energy), p)
    return spans_from_energy(energy, t, p.min_silence, p.min_speech, p.pad), t


def frames_to_seconds(spans) -> List[Tuple[float, float]]:
    return [(int(s) / FRAMES_PER_SECOND, int(e) / FRAMES_PER_SECOND) for s, e in spans]


def speech_spans_host(waveform, **opts) -> List[Tuple[float, float]]:
    """``[(start_s, end_s), ...]`` of a 16 kHz waveform, computed in numpy: the reference of
    the device detector, for arrays that are not resident."""
    return frames_to_seconds(speech_frames_host(waveform, **opts)[0])


# ---------------------------------------------------------------- device
def resident_spans(ctx, n_files: int, p: VadParams):
    """``HipContext.speech_spans`` as lists: per file (spans in frames, ``T``)."""
    return [([(int(s), int(e)) for s, e in sp], int(t)) for sp, t in ctx.speech_spans(p, n_files)]


def clamp_clips(spans, content_frames: int) -> List[Tuple[int, int]]:
    """Spans as seek clips of a file with ``content_frames`` whole frames: the detector's last
    frame may be a partial one, which the mel does not have."""
    return [(s, min(e, content_frames)) for s, e in spans if s < content_frames]


def speech_spans(model, audio, **opts) -> List[Tuple[float, float]]:
    """``[(start_s, end_s), ...]``: where ``audio`` holds speech, found on the device next to
    the resident waveform (``wh_speech_spans``).  ``audio``: a path (ingested as
    ``load_audio_device`` does), a 16 kHz array (uploaded) or a ``DeviceAudio``.  ``model``: a
    ``Whisper`` or a ``HipContext``.  Options: ``DEFAULTS``, in decibels and seconds."""
    from .audio import load_audio_device
    from .backend_hip import DeviceAudio
    p = resolve_options(**opts)
    ctx = getattr(model, "ctx", model)
    if isinstance(audio, str):
        audio = load_audio_device(ctx, audio)
    elif not isinstance(audio, DeviceAudio):
        a = np.ascontiguousarray(audio.detach().cpu().numpy() if hasattr(audio, "detach") else audio, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] < 1:
            raise ValueError(f"audio must be a non-empty 1-D waveform (shape {a.shape})")
        audio = ctx.audio_upload(a)
    if audio.ctx is not ctx:
        raise ValueError("DeviceAudio belongs to another model context")
    if audio.offset:
        raise ValueError("DeviceAudio is a segment behind other files: speech_spans() takes the first resident one")
    return frames_to_seconds(resident_spans(ctx, 1, p)[0][0])


# ---------------------------------------------------------------- live streams
# The causal detector of a live stream (wh_pool_vad_* / wh_stream_vad_*, csrc/wh_svad.hip):
# steps 1-3 above on an absolute frame grid (frame f is the stream's emitted samples
# [160 f, 160 f + 160), whatever was trimmed), the noise level taken over the last ``window``
# frames only, and step 5's rules evaluated frame by frame.  include/whisper_hip.h holds the
# definition; ``StreamVad`` restates it in numpy and is what the tests compare the kernel with.
SILENCE, ONSET, SPEECH = 0, 1, 2
MAX_WINDOW = 6000
MAX_RUN_FRAMES = 1 << 20

STREAM_DEFAULTS = dict(DEFAULTS, min_silence=0.5, window=30.0)


class StreamVadParams(NamedTuple):
    """The integers of the streaming definition (``wh_svad_opts``); durations in frames.  ``pad``
    is the policy's (``StreamingTranscriber``): the detector reports unpadded frames."""
    percentile: int
    ratio_q8: int
    t_lo: int
    t_hi: int
    window: int
    min_silence: int
    min_speech: int
    pad: int = 0


class StreamVadState(NamedTuple):
    """``wh_svad_state``.  ``run_start`` / ``run_end`` mean something only while ``state`` is not
    SILENCE; ``closed_*`` is the last span that ended (``closed_total`` of them so far)."""
    frames: int = 0
    samples: int = 0
    run_start: int = 0
    run_end: int = 0
    closed_start: int = 0
    closed_end: int = 0
    closed_total: int = 0
    threshold: int = 0
    partial: int = 0
    state: int = SILENCE


def resolve_stream_options(**opts) -> StreamVadParams:
    """User options of a stream's detector -> ``StreamVadParams``: ``DEFAULTS``' keys plus
    ``window``, the seconds the noise percentile looks back (default 30.0, at most 60).
    ``min_silence`` defaults to 0.5 s here: on a stream it is the endpointing delay, the
    silence after which an utterance counts as over, not a file's rule for joining clips.
    Neither that value nor the window has been measured on real speech with this project.
    Raises ValueError on an unknown option or a value out of range."""
    unknown = set(opts) - set(STREAM_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown stream speech option(s) {sorted(unknown)}; known: {sorted(STREAM_DEFAULTS)}")
    o = dict(STREAM_DEFAULTS, **opts)
    w = o.pop("window")
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not np.isfinite(w):
        raise ValueError(f"window must be a finite number, not {w!r}")
    window = int(round(float(w) * FRAMES_PER_SECOND))
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"window = {w!r} s is outside one frame .. {MAX_WINDOW // FRAMES_PER_SECOND} s")
    p = resolve_options(**o)
    if not 1 <= p.min_silence <= MAX_RUN_FRAMES:
        raise ValueError(f"min_silence = {o['min_silence']!r} s: on a stream it is at least one frame and at most "
                         f"{MAX_RUN_FRAMES} frames")
    if p.min_speech > MAX_RUN_FRAMES or p.pad > MAX_RUN_FRAMES:
        raise ValueError(f"min_speech / pad = {o['min_speech']!r} / {o['pad']!r} s is out of range")
    return StreamVadParams(percentile=p.percentile, ratio_q8=p.ratio_q8, t_lo=p.t_lo, t_hi=p.t_hi, window=window,
                           min_silence=p.min_silence, min_speech=p.min_speech, pad=p.pad)


def check_stream_params(p: StreamVadParams) -> StreamVadParams:
    """The ranges ``wh_pool_vad_enable`` accepts (ValueError otherwise)."""
    if not 1 <= p.percentile <= 99:
        raise ValueError(f"percentile = {p.percentile} outside 1..99")
    if not 256 <= p.ratio_q8 <= 2560000:
        raise ValueError(f"ratio_q8 = {p.ratio_q8} outside [256, 2560000]")
    if not 0 <= p.t_lo <= p.t_hi < 1 << 64:
        raise ValueError(f"need 0 <= t_lo <= t_hi, not {p.t_lo}, {p.t_hi}")
    if not 1 <= p.window <= MAX_WINDOW:
        raise ValueError(f"window = {p.window} outside 1..{MAX_WINDOW}")
    if not 1 <= p.min_silence <= MAX_RUN_FRAMES:
        raise ValueError(f"min_silence = {p.min_silence} outside 1..2^20")
    if not 0 <= p.min_speech <= MAX_RUN_FRAMES:
        raise ValueError(f"min_speech = {p.min_speech} outside 0..2^20")
    return p


class StreamVad:
    """The numpy twin of the device detector: ``feed(samples)`` takes the 16 kHz float32 samples
    a stream emitted, ``finish()`` closes a last incomplete frame with zeros; both return the
    ``StreamVadState``.  ``hist`` (uint32 [160]) and ``ring`` (uint8 [window]) are the state
    ``wh_pool_vad_read`` shows; ``spans`` lists every closed span and ``thresholds`` the ``T`` of
    every frame (the device keeps only the last of each)."""

    def __init__(self, params: StreamVadParams):
        self.p = check_stream_params(params)
        self.hist = np.zeros(N_BINS, dtype=np.uint32)
        self.ring = np.zeros(params.window, dtype=np.uint8)
        self.frames = self.samples = self.partial = 0
        self.mode = SILENCE
        self.run_start = self.run_end = self.closed_start = self.closed_end = self.closed_total = 0
        self.threshold = 0
        self.finished = False
        self.spans: List[Tuple[int, int]] = []
        self.thresholds: List[int] = []
        self.onsets_dropped = 0

    @property
    def state(self) -> StreamVadState:
        return StreamVadState(self.frames, self.samples, self.run_start, self.run_end, self.closed_start,
                              self.closed_end, self.closed_total, self.threshold, self.partial, self.mode)

    def _close(self, e: int) -> None:
        p, f = self.p, self.frames
        b = energy_bin(e)
        self.hist[b] += 1
        if f >= p.window:
            self.hist[self.ring[f % p.window]] -= 1
        self.ring[f % p.window] = b
        n = min(f + 1, p.window)
        rank = max(1, -(-n * p.percentile // 100))
        noise = bin_edge(int(np.searchsorted(np.cumsum(self.hist, dtype=np.int64), rank)))
        t = min(max((noise * p.ratio_q8) >> 8, p.t_lo), p.t_hi)
        if e > t:
            if self.mode == SILENCE:
                self.mode, self.run_start = ONSET, f
            self.run_end = f + 1
            if self.mode == ONSET and self.run_end - self.run_start >= p.min_speech:
                self.mode = SPEECH
        elif self.mode != SILENCE and f + 1 - self.run_end >= p.min_silence:
            if self.mode == SPEECH:
                self.closed_start, self.closed_end = self.run_start, self.run_end
                self.closed_total += 1
                self.spans.append((self.run_start, self.run_end))
            else:
                self.onsets_dropped += 1
            self.mode = SILENCE
        self.frames, self.threshold = f + 1, t
        self.thresholds.append(t)

    def feed(self, samples) -> StreamVadState:
        if self.finished:
            raise ValueError("feed() after finish()")
        q = quantise(samples).astype(np.int64)
        sq = q * q
        i, n = 0, len(sq)
        fill = self.samples % HOP_LENGTH
        if fill and n:
            i = min(HOP_LENGTH - fill, n)
            self.partial += int(sq[:i].sum())
            self.samples += i
            if self.samples % HOP_LENGTH == 0:
                e, self.partial = self.partial, 0
                self._close(e)
        whole = (n - i) // HOP_LENGTH
        for e in sq[i:i + whole * HOP_LENGTH].reshape(whole, HOP_LENGTH).sum(axis=1).tolist():
            self.samples += HOP_LENGTH
            self._close(int(e))
        rest = sq[i + whole * HOP_LENGTH:]
        if len(rest):
            self.partial += int(rest.sum())
            self.samples += len(rest)
        return self.state

    def finish(self) -> StreamVadState:
        if not self.finished:
            self.finished = True
            if self.samples % HOP_LENGTH:
                e, self.partial = self.partial, 0
                self._close(e)
        return self.state
