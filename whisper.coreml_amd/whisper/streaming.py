"""Streaming transcription: audio that arrives in packets, text that never changes once shown.

Two layers.

``AudioStream`` is the device half (``wh_stream_*``, include/whisper_hip.h): raw frames in any of
the WAV sample encodings are appended chunk by chunk, mixed down and resampled on the GPU, and
kept as ONE growing resident segment.  The samples are bit for bit those ``load_audio`` gives for
the whole recording, however it was cut into chunks, so everything that reads resident audio
(``transcribe(DeviceAudio)``, ``speech_spans``) works on the stream as it is.

``LocalAgreement`` and ``StreamingTranscriber`` are the policy half, plain Python: the growing
buffer is decoded again after every ``min_chunk`` seconds of input, and a word is committed once
two consecutive hypotheses agree on it (LocalAgreement-2 of Macháček et al., "Turning Whisper
into Real-Time Transcription System", 2023, made definite here).  Committed words are never
retracted; the buffer is trimmed behind them so that it stays inside one 30 s window.

``min_chunk``, ``buffer_trim``, ``max_buffer`` and ``prompt_chars`` are defaults of that paper's
implementation; none of them has been measured on real speech with this backend.

With ``vad=`` a stream carries a causal speech detector on the device (``vad.StreamVad`` is its
numpy twin, include/whisper_hip.h its definition), updated inside the call that ingests the
packets.  The policy reads its state at every decode point: a buffer without confirmed speech is
not decoded (``StreamUpdate.idle``), the silence after an utterance ends it
(``StreamUpdate.endpoint``: the pending words are committed at once) and the buffer is cut so
that it starts just before the next onset.
"""

import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np

from .audio import (HOP_LENGTH, MAX_DEVICE_TAPS, SAMPLE_RATE, WAV_CONTAINER, WAV_ENCODINGS, device_filter_taps, stream_emitted)

SILENCE, ONSET, SPEECH = 0, 1, 2  # vad.StreamVadState.state
_PREPEND = "\"'“¿([{-"
_APPEND = "\"'.。,，!！?？:：”)]}、"
# what an array handed to ``append`` must hold: the encoding's container (packed 24-bit and the
# one-byte encodings are bytes)
_CONTAINER_DTYPE = dict(u8="u1", s16="<i2", s24="u1", s32="<i4", f32="<f4", f64="<f8", alaw="u1", ulaw="u1")
_REFUSED_OPTIONS = ("clip_timestamps", "channels", "schedule", "mel_max_reduce")


def _frame_bytes(data, encoding: str) -> bytes:
    """The bytes of ``data``: bytes-like as it is, an array only in the encoding's container."""
    if isinstance(data, np.ndarray):
        want = np.dtype(_CONTAINER_DTYPE[encoding])
        if data.dtype != want:
            raise TypeError(f"stream data for encoding {encoding!r} must be bytes or an array of {want}, not {data.dtype}")
        return np.ascontiguousarray(data).tobytes()
    return bytes(data)


def resolve_vad(vad):
    """``vad=`` of a stream: None (no detector), True (the defaults), a dict of
    ``vad.resolve_stream_options``' options, or ``vad.StreamVadParams`` -> the params or None."""
    from .vad import StreamVadParams, check_stream_params, resolve_stream_options
    if vad is None or vad is False:
        return None
    if vad is True:
        return resolve_stream_options()
    if isinstance(vad, StreamVadParams):
        return check_stream_params(vad)
    if isinstance(vad, dict):
        return resolve_stream_options(**vad)
    raise TypeError(f"vad must be None, True, a dict of options or StreamVadParams, not {type(vad).__name__}")


def _check_options(transcribe_options: dict, who: str) -> None:
    """The transcribe options a streaming decode cannot take (``ValueError``); ``word_timestamps=True``
    is dropped from the dict, since every decode sets it."""
    if "word_timestamps" in transcribe_options and not transcribe_options.pop("word_timestamps"):
        raise ValueError(f"{who} needs word_timestamps=True: the policy commits words by their times")
    for name in _REFUSED_OPTIONS:
        if name in transcribe_options:
            raise ValueError(f"{who} does not take {name}: every decode is the whole resident buffer")


class AudioStream:
    """A recording that arrives in chunks, resampled to 16 kHz mono on the GPU as it comes.

    ``model``: a ``Whisper``, a ``HipContext`` or a device, as for ``load_audio_device``; a
    context holds one stream, and any other call that replaces its resident audio (an upload,
    an ingest, ``transcribe`` of a path or an array) ends it: the next ``append`` then raises
    ``HipBackendError`` naming that call.  ``encoding``: one of ``audio.WAV_ENCODINGS``; the
    data are raw interleaved frames, no container.  A rate whose filter would exceed
    ``audio.MAX_DEVICE_TAPS`` is refused (``ValueError``): there is no host path for a stream.
    ``vad``: see ``resolve_vad``; the stream then carries a speech detector that every ``append``
    and ``finish`` updates on the device, and ``vad_state`` is its state after the last of them."""

    def __init__(self, model, rate: int, encoding: str = "s16", channels: int = 1, reserve: int = 0, vad=None):
        if encoding not in WAV_ENCODINGS:
            raise ValueError(f"encoding {encoding!r}: one of {', '.join(WAV_ENCODINGS)}")
        rate, channels = int(rate), int(channels)
        if rate < 1:
            raise ValueError(f"rate {rate} Hz: must be positive")
        if device_filter_taps(rate) > MAX_DEVICE_TAPS:
            raise ValueError(f"rate {rate} Hz: its resampling filter has {device_filter_taps(rate)} taps, more than "
                             f"the device path takes ({MAX_DEVICE_TAPS}); resample the stream to a common rate first")
        self.vad = resolve_vad(vad)
        from .audio import _device_index, _mel_context
        ctx = getattr(model, "ctx", model)
        if ctx is None or isinstance(ctx, (int, str)):
            ctx = _mel_context(_device_index(ctx))
        self.ctx = ctx
        self.rate, self.encoding, self.channels = rate, encoding, channels
        self.frame_bytes = WAV_CONTAINER[WAV_ENCODINGS.index(encoding)] * channels
        self.frames_in = 0   # whole frames appended
        self.n_samples = 0   # resident 16 kHz samples
        self.finished = False
        self._tail = b""     # a trailing partial frame, waiting for its rest
        ctx.stream_begin(WAV_ENCODINGS.index(encoding), channels, rate, reserve=reserve)
        if self.vad is not None:
            ctx.stream_vad_enable(self.vad)

    @property
    def vad_state(self):
        """``vad.StreamVadState`` after the last append or finish (None without ``vad``)."""
        return self.ctx.stream_vad_state() if self.vad is not None else None

    def append(self, data) -> int:
        """Bytes-like data, or an array in the encoding's container dtype; a trailing partial
        frame is kept for the next call.  Returns the 16 kHz samples this call made resident:
        ``stream_emitted(after) - stream_emitted(before)``, possibly 0."""
        buf = self._tail + _frame_bytes(data, self.encoding) if self._tail else _frame_bytes(data, self.encoding)
        n = len(buf) // self.frame_bytes
        whole = n * self.frame_bytes
        # no whole frame: still asked, so that a stream another call ended raises with that reason
        got = self.ctx.stream_append(np.frombuffer(buf, np.uint8, whole) if n else None, n)
        self._tail = buf[whole:]
        self.frames_in += n
        self.n_samples += got
        return got

    def finish(self) -> int:
        """End of the input (a trailing partial frame is dropped): the samples the resampler
        held back become resident; returns how many.  ``trim`` still works afterwards."""
        got = self.ctx.stream_finish()
        self._tail = b""
        self.finished = True
        self.n_samples += got
        return got

    def trim(self, n: int):
        """Drop the first ``n`` resident samples (0 <= n <= n_samples)."""
        self.ctx.stream_trim(int(n))
        self.n_samples -= int(n)

    def device_audio(self):
        """The resident segment as the ``DeviceAudio`` that ``transcribe`` takes."""
        from .backend_hip import DeviceAudio
        return DeviceAudio(self.ctx, self.n_samples)


class LocalAgreement:
    """LocalAgreement-2: a word is committed when two consecutive hypotheses agree on it.

    State: ``committed`` (word dicts ``word, start, end, probability`` with absolute times),
    ``T`` (the end of the last committed word, 0.0 at first) and ``pending`` (the uncommitted
    tail of the last hypothesis).  ``update(words)``:
      1. keep the words with ``start > T - 0.1``;
      2. drop from their head the largest ``i <= 5`` such that the last ``i`` committed words
         equal the first ``i`` kept ones (a re-decode of audio that was already committed);
      3. commit the longest common prefix of the rest and ``pending``, in the new hypothesis'
         words and times;
      4. ``pending`` becomes the remainder.
    Words compare by ``word.strip().casefold()`` without leading ``prepend_punctuations`` and
    trailing ``append_punctuations`` characters, so "Hello," agrees with " hello"."""

    def __init__(self, prepend_punctuations: str = _PREPEND, append_punctuations: str = _APPEND):
        self.prepend, self.append = prepend_punctuations, append_punctuations
        self.committed: List[dict] = []
        self.pending: List[dict] = []
        self.T = 0.0

    def key(self, word: dict) -> str:
        return word["word"].strip().casefold().lstrip(self.prepend).rstrip(self.append)

    def _commit(self, words: List[dict]) -> List[dict]:
        if words:
            self.committed.extend(words)
            self.T = float(words[-1]["end"])
        return list(words)

    def update(self, words: List[dict]) -> List[dict]:
        """Take a hypothesis; returns the words it newly committed."""
        kept = [w for w in words if w["start"] > self.T - 0.1]
        for i in range(min(5, len(self.committed), len(kept)), 0, -1):
            if [self.key(w) for w in self.committed[-i:]] == [self.key(w) for w in kept[:i]]:
                kept = kept[i:]
                break
        n = 0
        while n < min(len(kept), len(self.pending)) and self.key(kept[n]) == self.key(self.pending[n]):
            n += 1
        new = self._commit(kept[:n])
        self.pending = kept[n:]
        return new

    def flush(self) -> List[dict]:
        """Commit what is pending (the end of the stream, or a forced trim)."""
        new = self._commit(self.pending)
        self.pending = []
        return new


@dataclass
class StreamUpdate:
    """One decode of the buffer.  ``committed``: the words this update added for good;
    ``tentative``: the rest of the hypothesis, which may still change; ``span``: the buffer
    ``(s0, s1)`` in absolute 16 kHz samples when it was decoded; ``prompt``: the
    ``initial_prompt`` the decode ran with; ``result``: what ``transcribe`` returned, times
    relative to the buffer start (None when nothing was decoded); ``forced``: pending words
    were committed without agreement because the buffer had to be cut.  With a detector
    (``vad=``): ``vad`` is its state at the decode point; ``idle``: the buffer held no confirmed
    speech and was not decoded; ``endpoint``: the utterance in the buffer had ended, so the
    pending words were committed with this update."""
    committed: List[dict] = field(default_factory=list)
    tentative: List[dict] = field(default_factory=list)
    span: Tuple[int, int] = (0, 0)
    prompt: Optional[str] = None
    language: Optional[str] = None
    result: Optional[dict] = None
    forced: bool = False
    final: bool = False
    wall_ms: float = 0.0
    idle: bool = False
    endpoint: bool = False
    vad: Optional[tuple] = None


class StreamingTranscriber:
    """Live transcription of one stream: ``feed(data)`` returns the updates the data completed,
    ``finish()`` the last one.

    A decode runs after every ``round(min_chunk * rate)`` input frames; ``feed`` cuts its data
    at those points, so the updates depend on the samples alone, not on how the caller split
    them.  A decode is ``transcribe(model, stream.device_audio(), language=..., initial_prompt=
    prompt, word_timestamps=True, **transcribe_options)`` on the whole resident buffer; word
    times are shifted by the buffer start and go through ``LocalAgreement``.  ``prompt`` is
    ``initial_prompt`` followed by the committed words that end at or before the buffer start,
    those cut to their last ``prompt_chars`` characters at a word boundary.  With
    ``language=None`` the first decode detects the language and it is kept.

    After each update, with the buffer ``[s0, s1)`` of duration d, starting at t0 = s0 / 16000
    (a cut at time c drops ``floor((c - t0) * 16000 + 0.5)`` samples, clipped to the buffer):
      1. d > buffer_trim: cut at the end of the latest segment of this hypothesis whose end
         lies in (t0, T], T the end of the last committed word;
      2. still d > max_buffer and T > t0: cut at T;
      3. still d > max_buffer: commit the pending words (``update.forced``) and cut at
         t1 - buffer_trim.
    ``buffer_trim < max_buffer <= 30 - min_chunk`` keeps every decode inside one 30 s window.

    With ``vad`` (True, a dict of ``vad.resolve_stream_options``' options, or its result) the
    stream carries a speech detector and every decode point first reads its state ``st`` (frames
    of 160 samples on the stream's absolute grid; ``pad`` in frames):
    ``speech_end = st.frames if st.state == SPEECH else st.closed_end`` and
    ``keep = (st.run_start if st.state == ONSET else st.frames) - pad``.
      idle: ``160 * speech_end <= s0``, the buffer holds no confirmed speech.  No decode
        (``result`` None, ``update.idle``), nothing committed, the buffer cut at frame ``keep``;
        at ``finish`` the pending words are flushed.
      endpoint: speech in the buffer and ``st.state != SPEECH``.  Decode and agreement as usual,
        then the pending words are committed too (``update.endpoint``) and the buffer is cut at
        frame ``max(st.closed_end, keep)``; rules 1-3 are skipped.
      speech: ``st.state == SPEECH``: the update above, unchanged.
    The decode points stay where they are, so the updates still depend on the samples alone.

    ``word_timestamps=False``, ``clip_timestamps``, ``channels``, ``schedule`` and
    ``mel_max_reduce`` are refused (``ValueError``).  ``stream`` and ``decode_fn(prompt, span)``
    replace the device stream and the ``transcribe`` call (tests drive the policy without a GPU);
    with ``vad`` such a ``stream`` has ``vad_state``."""

    def __init__(self, model, rate: int, encoding: str = "s16", channels: int = 1, *, language: Optional[str] = None,
                 min_chunk: float = 1.0, buffer_trim: float = 15.0, max_buffer: float = 25.0, prompt_chars: int = 200,
                 initial_prompt: Optional[str] = None, vad=None, stream=None,
                 decode_fn: Optional[Callable[[Optional[str], Tuple[int, int]], dict]] = None, **transcribe_options):
        _check_options(transcribe_options, "StreamingTranscriber")
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)):
            raise ValueError(f"channels = {channels!r}: here it is the stream's channel count, which is mixed down; "
                             f"transcribe's channels option (\"split\", a selection) is not available on a stream")
        if not min_chunk > 0:
            raise ValueError(f"min_chunk = {min_chunk}: must be positive")
        if not (0 < buffer_trim < max_buffer <= 30.0 - min_chunk):
            raise ValueError(f"need 0 < buffer_trim < max_buffer <= 30 - min_chunk, got buffer_trim = {buffer_trim}, "
                             f"max_buffer = {max_buffer}, min_chunk = {min_chunk}")
        if initial_prompt is not None and not isinstance(initial_prompt, str):
            raise TypeError("initial_prompt must be a string: committed text is appended to it")
        if encoding not in WAV_ENCODINGS:
            raise ValueError(f"encoding {encoding!r}: one of {', '.join(WAV_ENCODINGS)}")
        self.model = model
        self.rate, self.encoding, self.channels = int(rate), encoding, int(channels)
        self.chunk_frames = int(round(min_chunk * self.rate))
        if self.chunk_frames < 1:
            raise ValueError(f"min_chunk = {min_chunk} s is less than one frame at {rate} Hz")
        self.language = language
        self.min_chunk, self.buffer_trim, self.max_buffer = float(min_chunk), float(buffer_trim), float(max_buffer)
        self.prompt_chars = int(prompt_chars)
        self.initial_prompt = initial_prompt
        self.options = dict(transcribe_options)
        self.policy = LocalAgreement(self.options.get("prepend_punctuations", _PREPEND),
                                     self.options.get("append_punctuations", _APPEND))
        self.vad = resolve_vad(vad)
        self.stream = stream if stream is not None else AudioStream(model, rate, encoding, channels, vad=self.vad)
        self._decode_fn = decode_fn
        self.frame_bytes = WAV_CONTAINER[WAV_ENCODINGS.index(encoding)] * self.channels
        self.frames_in = 0
        self._next_decode = self.chunk_frames
        self._tail = b""
        self._s0 = self._s1 = 0    # the buffer in absolute 16 kHz samples
        self._decoded_s1 = 0       # _s1 at the last decode
        self.finished = False

    # -- state
    @property
    def committed(self) -> List[dict]:
        return self.policy.committed

    @property
    def pending(self) -> List[dict]:
        return self.policy.pending

    @property
    def text(self) -> str:
        """The committed text so far."""
        return "".join(w["word"] for w in self.policy.committed).strip()

    @property
    def span(self) -> Tuple[int, int]:
        return self._s0, self._s1

    # -- input
    def feed(self, data) -> List[StreamUpdate]:
        if self.finished:
            raise ValueError("feed() after finish()")
        buf = self._tail + _frame_bytes(data, self.encoding)
        fb = self.frame_bytes
        n = len(buf) // fb
        self._tail = buf[n * fb:]
        view = memoryview(buf)
        updates, pos = [], 0
        while pos < n:
            take = min(n - pos, self._next_decode - self.frames_in)
            self._s1 += self.stream.append(view[pos * fb:(pos + take) * fb])
            self.frames_in += take
            pos += take
            if self.frames_in == self._next_decode:
                self._next_decode += self.chunk_frames
                updates.append(self._update(final=False))
        return updates

    def finish(self) -> StreamUpdate:
        """The end of the stream (a trailing partial frame is dropped): one more decode if
        samples arrived since the last one, then everything pending is committed."""
        if self.finished:
            raise ValueError("finish() called twice")
        self.finished = True
        self._tail = b""
        self._s1 += self.stream.finish()
        return self._update(final=True)

    # -- one decode
    def build_prompt(self, t0: float) -> Optional[str]:
        """``initial_prompt`` plus the committed words that end at or before ``t0``, the latter
        cut to their last ``prompt_chars`` characters at a word boundary."""
        words, room = [], self.prompt_chars
        for w in reversed(self.policy.committed):
            if w["end"] > t0:
                continue
            room -= len(w["word"])
            if room < 0:
                break
            words.append(w["word"])
        tail = "".join(reversed(words)).strip()
        parts = [p for p in ((self.initial_prompt or "").strip(), tail) if p]
        return " ".join(parts) if parts else None

    def _decode(self, prompt: Optional[str], span: Tuple[int, int]) -> dict:
        if self._decode_fn is not None:
            return self._decode_fn(prompt, span)
        from .transcribe import transcribe
        return transcribe(self.model, self.stream.device_audio(), language=self.language, initial_prompt=prompt,
                          word_timestamps=True, **self.options)

    def _cut(self, c: float) -> None:
        """Drop the buffer's samples before time ``c`` (clipped to the buffer)."""
        drop = int(np.floor((c - self._s0 / SAMPLE_RATE) * SAMPLE_RATE + 0.5))
        drop = min(max(drop, 0), self._s1 - self._s0)
        if drop:
            self.stream.trim(drop)
            self._s0 += drop

    def _cut_frame(self, f: int) -> None:
        """Drop the buffer's samples before frame ``f`` of the stream's grid (clipped to the buffer)."""
        drop = min(max(HOP_LENGTH * int(f) - self._s0, 0), self._s1 - self._s0)
        if drop:
            self.stream.trim(drop)
            self._s0 += drop

    def _update(self, final: bool) -> StreamUpdate:
        t_begin = time.perf_counter()
        u, due = self._begin_update(final)
        return self._end_update(u, self._decode(u.prompt, u.span) if due else None, t_begin)

    # an update in two halves, so that a pool can decode the buffers of many streams between them
    def _begin_update(self, final: bool) -> Tuple[StreamUpdate, bool]:
        """The update of the buffer as it is, and whether it needs a decode (then with its prompt)."""
        s0, s1 = self._s0, self._s1
        u = StreamUpdate(span=(s0, s1), final=final, language=self.language)
        if self.vad is not None:
            st = u.vad = self.stream.vad_state
            speech_end = st.frames if st.state == SPEECH else st.closed_end
            u.idle = HOP_LENGTH * speech_end <= s0
            u.endpoint = not u.idle and st.state != SPEECH
        due = not u.idle and s1 > s0 and (not final or s1 > self._decoded_s1)
        if due:
            u.prompt = self.build_prompt(s0 / SAMPLE_RATE)
        return u, due

    def _end_update(self, u: StreamUpdate, result: Optional[dict], t_begin: float) -> StreamUpdate:
        """``result``: what the decode of ``u.span`` with ``u.prompt`` returned (None: there was none)."""
        s0, s1 = u.span
        t0 = s0 / SAMPLE_RATE
        if result is not None:
            self._decoded_s1 = s1
            if self.language is None:
                self.language = result.get("language")
            words = [dict(word=w["word"], start=w["start"] + t0, end=w["end"] + t0, probability=w["probability"])
                     for s in result["segments"] for w in s.get("words", [])]
            u.committed = self.policy.update(words)
        u.result, u.language = result, self.language
        if u.final or u.endpoint:
            u.committed = u.committed + self.policy.flush()
        if u.idle or u.endpoint:
            if not u.final:
                st = u.vad
                keep = (st.run_start if st.state == ONSET else st.frames) - self.vad.pad
                self._cut_frame(keep if u.idle else max(st.closed_end, keep))
        elif not u.final and result is not None:
            self._trim(u, result, t0)
        u.tentative = list(self.policy.pending)
        u.wall_ms = (time.perf_counter() - t_begin) * 1e3
        return u

    def _trim(self, u: StreamUpdate, result: dict, t0: float) -> None:
        def duration():
            return (self._s1 - self._s0) / SAMPLE_RATE
        T = self.policy.T
        if duration() > self.buffer_trim:
            ends = [s["end"] + t0 for s in result["segments"] if t0 < s["end"] + t0 <= T]
            if ends:
                self._cut(max(ends))
        if duration() > self.max_buffer and T > self._s0 / SAMPLE_RATE:
            self._cut(T)
        if duration() > self.max_buffer:
            u.committed = u.committed + self.policy.flush()
            u.forced = True
            self._cut(self._s1 / SAMPLE_RATE - self.buffer_trim)
