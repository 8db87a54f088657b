"""Many live streams on one model: packets of all streams ingested by one call, the buffers that
are due decoded together.

``StreamingPool`` is ``StreamingTranscriber`` for many streams at once.  The device half is the
context's stream pool (``wh_pool_*``, include/whisper_hip.h): a fixed number of slots, each a
stream with its own format and resident buffer, apart from the context's resident audio, so a
``transcribe(path)`` on the same model between two feeds ends nothing.  The policy half is not
restated here: every stream of the pool IS a ``StreamingTranscriber`` (its decode points, its
``LocalAgreement``, ``build_prompt`` and trim rules), only that its device calls are collected
and its decode happens between the two halves of its update.

The contract: for every stream, the list of updates equals that of a lone
``StreamingTranscriber`` with the same options fed the same bytes, in every field but
``wall_ms``, whatever else is in the pool and however the feeds were split or interleaved.  This
holds for deterministic decoding (``temperature=0.0``).  With sampling, one seed is drawn per
due stream per round, in handle order (``decoding.next_seed``), so the samples depend on what
else was due; no equality is promised then.

``feed`` works in rounds:
  1. every stream with data left appends up to its own next decode point: one ``pool_append``;
  2. the streams that reached their decode point are decoded together, one lane each: one
     ``pool_log_mel`` of their slots, then language detection, ``run_lanes`` and the alignment
     round as ``transcribe_batch`` runs them for files (``multifile._transcribe_lanes``); more due
     streams than ``ctx.max_windows`` queue, as files do;
  3. each stream's result goes through its own ``LocalAgreement`` and trim rules;
  4. the cuts of all streams go out as one ``pool_trim``;
and again until no data is left.
"""

import inspect
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .audio import MAX_DEVICE_TAPS, N_SAMPLES, SAMPLE_RATE, WAV_ENCODINGS, device_filter_taps
from .streaming import StreamingTranscriber, StreamUpdate, _check_options, _frame_bytes, resolve_vad

# 30 s of buffer (max_buffer + min_chunk <= 30 s) plus what the resamplers' rounding and the
# samples a finish releases can add
DEFAULT_SLOT_SAMPLES = N_SAMPLES + SAMPLE_RATE // 10
_PER_STREAM = ("rate", "encoding", "channels", "language", "initial_prompt", "min_chunk", "buffer_trim", "max_buffer",
               "prompt_chars")
# transcribe_batch's keywords that are not decoding options of a pool
_NOT_POOL = ("language", "initial_prompt", "clip_timestamps", "skip_silence", "channels", "channel_names",
             "word_timestamps", "mel_budget_frames")


class _SlotStream:
    """What a pool stream's ``StreamingTranscriber`` sees as its device stream: the cuts of an
    update are summed up here and go out with those of the other streams."""

    def __init__(self, slot: int):
        self.slot = slot
        self.drop = 0
        self.vad_state = None  # of a detecting stream: as of the batched call that reached its decode point

    def trim(self, n: int):
        self.drop += int(n)


class StreamingPool:
    """``slots`` live streams on ``model``.  ``open(rate, encoding, channels, ...)`` returns a
    handle, ``feed({handle: bytes})`` the updates the data completed per handle (``StreamUpdate``,
    as ``StreamingTranscriber.feed`` returns them), ``finish(handles)`` the last update of each;
    a finished stream's slot is free again.

    The decoding options (``beam_size``, ``temperature``, ``hotwords``, ``no_repeat_ngram_size``,
    ``repetition_penalty``, the thresholds, ...) are one value for the pool, as ``transcribe_batch``
    has them.  Per stream (``open``): ``rate``, ``encoding``, ``channels``, ``language``,
    ``initial_prompt``, ``min_chunk``, ``buffer_trim``, ``max_buffer`` and ``prompt_chars``, with
    ``StreamingTranscriber``'s checks and defaults; ``language=None`` is detected at the stream's
    first decode.  Everything ``StreamingTranscriber`` refuses is refused here (``ValueError``), and
    so is ``skip_silence``: the span detector reads the context's resident segments, not a slot;
    ``open(vad=...)`` gives a stream the causal detector instead, per stream: a stream without
    confirmed speech in its buffer then takes no lane of a round (``StreamUpdate.idle``), and a
    tick in which nobody has speech runs no decode round at all.

    ``slot_samples``: the room of a slot in 16 kHz samples; the default holds the 30 s that
    ``max_buffer <= 30 - min_chunk`` allows.  ``device`` and ``decode_round_fn(items)`` replace
    the context's pool calls and the batched decode (tests drive the policy without a GPU):
    ``device`` has ``pool_open / pool_close / pool_append / pool_finish / pool_trim`` (and, for
    ``open(vad=...)``, ``pool_vad_enable / pool_vad_state``) as ``HipContext`` does, ``items`` is a list of ``(handle, prompt, span)`` and the function
    returns one ``transcribe`` result dict per item."""

    def __init__(self, model, slots: int = 64, *, slot_samples: int = DEFAULT_SLOT_SAMPLES, device=None,
                 decode_round_fn: Optional[Callable[[List[Tuple[int, Optional[str], Tuple[int, int]]]], List[dict]]] = None,
                 **transcribe_options):
        _check_options(transcribe_options, "StreamingPool")
        if transcribe_options.pop("skip_silence", False):
            raise ValueError("StreamingPool does not take skip_silence: the span detector reads the context's "
                             "resident segments, not a pool slot; give a stream its own causal detector with "
                             "open(vad=...)")
        for name in _PER_STREAM:
            if name in transcribe_options:
                raise ValueError(f"StreamingPool: {name} belongs to a stream, pass it to open()")
        for name in ("clip_timestamps", "channel_names", "mel_budget_frames", "_mel_prepared"):
            if name in transcribe_options:
                raise ValueError(f"StreamingPool does not take {name}: every decode is the whole resident buffer")
        slots, slot_samples = int(slots), int(slot_samples)
        if slots < 1:
            raise ValueError(f"slots = {slots}: a pool has at least one")
        self.model = model
        self.options = dict(transcribe_options)
        self.n_slots, self.slot_samples = slots, slot_samples
        self._decode_round_fn = decode_round_fn
        self._owns_device = device is None
        if device is None:
            from .transcribe import _check_fp16
            _check_fp16(model, self.options.pop("fp16", True))
            device = model.ctx
            device.pool_create(slots, slot_samples)
        self.dev = device
        self._free = list(range(slots))
        self._streams: Dict[int, StreamingTranscriber] = {}
        self._ended = set()
        self._next_handle = 0
        self.rounds: List[List[int]] = []  # the handles every decode round took, in order

    # -- the pool
    def close(self):
        """Drop every stream and free the device pool."""
        if self._owns_device and self.dev is not None:
            self.dev.pool_destroy()
        self.dev = None
        self._ended.update(self._streams)
        self._streams.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def open(self, rate: int, encoding: str = "s16", channels: int = 1, *, language: Optional[str] = None,
             initial_prompt: Optional[str] = None, min_chunk: float = 1.0, buffer_trim: float = 15.0,
             max_buffer: float = 25.0, prompt_chars: int = 200, vad=None) -> int:
        """A new stream in a free slot; returns its handle.  ``vad``: as ``StreamingTranscriber``'s."""
        vad = resolve_vad(vad)
        if encoding not in WAV_ENCODINGS:
            raise ValueError(f"encoding {encoding!r}: one of {', '.join(WAV_ENCODINGS)}")
        if int(rate) < 1:
            raise ValueError(f"rate {rate} Hz: must be positive")
        if device_filter_taps(int(rate)) > MAX_DEVICE_TAPS:
            raise ValueError(f"rate {rate} Hz: its resampling filter has {device_filter_taps(int(rate))} taps, more "
                             f"than the device path takes ({MAX_DEVICE_TAPS}); resample the stream to a common rate first")
        if not self._free:
            raise RuntimeError(f"StreamingPool: all {self.n_slots} slots are in use; finish a stream first")
        slot = self._free[0]
        t = StreamingTranscriber(self.model, rate, encoding, channels, language=language, min_chunk=min_chunk,
                                 buffer_trim=buffer_trim, max_buffer=max_buffer, prompt_chars=prompt_chars,
                                 initial_prompt=initial_prompt, vad=vad, stream=_SlotStream(slot), **self.options)
        self.dev.pool_open(slot, WAV_ENCODINGS.index(encoding), t.channels, t.rate)
        if vad is not None:
            try:
                self.dev.pool_vad_enable(slot, vad)
            except Exception:
                self.dev.pool_close(slot)
                raise
        self._free.pop(0)
        handle = self._next_handle
        self._next_handle += 1
        self._streams[handle] = t
        return handle

    def stream(self, handle: int) -> StreamingTranscriber:
        """The stream's state (``text``, ``committed``, ``pending``, ``span``, ``language``); read only."""
        if handle in self._ended:
            raise ValueError(f"stream {handle} has finished")
        if handle not in self._streams:
            raise ValueError(f"unknown stream handle {handle!r}")
        return self._streams[handle]

    # -- input
    def feed(self, packets: Dict[int, object]) -> Dict[int, List[StreamUpdate]]:
        """``{handle: data}``, data as ``StreamingTranscriber.feed`` takes it.  Returns
        ``{handle: [StreamUpdate, ...]}`` for the handles given."""
        left = {}
        for h in sorted(packets):
            t = self.stream(h)
            buf = t._tail + _frame_bytes(packets[h], t.encoding)
            left[h] = [np.frombuffer(buf, np.uint8), 0, len(buf) // t.frame_bytes]  # bytes, frames taken, frames
        for h, (buf, _, n) in left.items():  # only now: a bad handle or array leaves every stream as it was
            self._streams[h]._tail = bytes(buf[n * self._streams[h].frame_bytes:])
        out: Dict[int, List[StreamUpdate]] = {h: [] for h in left}
        while True:
            todo = [h for h in left if left[h][1] < left[h][2]]
            if not todo:
                return out
            # 1. everyone up to their own next decode point, in one call
            takes = []
            for h in todo:
                t = self._streams[h]
                buf, pos, n = left[h]
                take = min(n - pos, t._next_decode - t.frames_in)
                takes.append(take)
            got = self.dev.pool_append([self._streams[h].stream.slot for h in todo],
                                       [left[h][0][left[h][1] * self._streams[h].frame_bytes:
                                                   (left[h][1] + take) * self._streams[h].frame_bytes]
                                        for h, take in zip(todo, takes)], takes)
            due = []
            for h, take, g in zip(todo, takes, got):
                t = self._streams[h]
                t._s1 += g
                t.frames_in += take
                left[h][1] += take
                if t.frames_in == t._next_decode:
                    t._next_decode += t.chunk_frames
                    due.append(h)
            # 2. - 4. the due streams, together
            if due:
                self._read_vad(due)
                for h, u in zip(due, self._update_round(due, final=False)):
                    out[h].append(u)

    def finish(self, handles: Sequence[int]) -> Dict[int, StreamUpdate]:
        """The end of these streams (a trailing partial frame is dropped): one more decode for
        those that got samples since their last one, then everything pending is committed.  Their
        slots are free afterwards."""
        handles = sorted(set(handles))
        streams = [self.stream(h) for h in handles]
        if not handles:
            return {}
        got = self.dev.pool_finish([t.stream.slot for t in streams])
        for t, g in zip(streams, got):
            t.finished = True
            t._tail = b""
            t._s1 += g
        self._read_vad(handles)
        updates = self._update_round(handles, final=True)
        for h, t in zip(handles, streams):
            self.dev.pool_close(t.stream.slot)
            self._free.append(t.stream.slot)
            self._free.sort()
            del self._streams[h]
            self._ended.add(h)
        return dict(zip(handles, updates))

    def _read_vad(self, handles: Sequence[int]) -> None:
        """The detecting streams' states as the batched call just left them (a host copy: no device call)."""
        streams = [self._streams[h].stream for h in handles if self._streams[h].vad is not None]
        if streams:
            for s, st in zip(streams, self.dev.pool_vad_state([s.slot for s in streams])):
                s.vad_state = st

    # -- one round of updates
    def _update_round(self, handles: List[int], final: bool) -> List[StreamUpdate]:
        t_begin = time.perf_counter()
        streams = [self._streams[h] for h in handles]
        begun = [t._begin_update(final) for t in streams]
        due = [i for i, (_, d) in enumerate(begun) if d]
        results: List[Optional[dict]] = [None] * len(handles)
        if due:
            self.rounds.append([handles[i] for i in due])
            for i, r in zip(due, self._decode_round([(handles[i], begun[i][0].prompt, begun[i][0].span) for i in due])):
                results[i] = r
        updates = [t._end_update(u, r, t_begin) for t, (u, _), r in zip(streams, begun, results)]
        cut = [t.stream for t in streams if t.stream.drop]
        if cut:
            self.dev.pool_trim([s.slot for s in cut], [s.drop for s in cut])
            for s in cut:
                s.drop = 0
        return updates

    def _decode_round(self, items: List[Tuple[int, Optional[str], Tuple[int, int]]]) -> List[dict]:
        if self._decode_round_fn is not None:
            return list(self._decode_round_fn(items))
        from .multifile import _transcribe_lanes, transcribe_batch
        model, ctx = self.model, self.model.ctx
        streams = [self._streams[h] for h, _, _ in items]
        slots = [t.stream.slot for t in streams]
        # transcribe_batch's own defaults for what the pool's options leave out
        named = {k: p.default for k, p in inspect.signature(transcribe_batch).parameters.items()
                 if p.kind is p.KEYWORD_ONLY and k not in _NOT_POOL}
        opts = dict(self.options)
        for k in named:
            if k in opts:
                named[k] = opts.pop(k)
        thresholds = (named.pop("compression_ratio_threshold"), named.pop("logprob_threshold"),
                      named.pop("no_speech_threshold"))

        def prepare_group(group: List[int]):
            return ctx.pool_log_mel([slots[i] for i in group], model.dims.n_mels, padding=N_SAMPLES)

        return _transcribe_lanes(model, [s1 - s0 for _, _, (s0, s1) in items], prepare_group,
                                 [t.language for t in streams], [p for _, p, _ in items], ["0"] * len(items),
                                 thresholds=thresholds, word_timestamps=True, decode_options=opts, **named)
