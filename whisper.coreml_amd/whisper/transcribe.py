"""Long-form transcription driver (reference whisper/transcribe.py:41-524).

Same options and segment semantics as the reference loop (30 s windows, data-
dependent ``seek``, temperature fallback, prompt carry-over, no-speech skip,
empty-segment clearing).

There is one loop body and three drivers of it.  The body is ``_Lane`` (the loop's
state, cut where the GPU work sits: ``next_window`` / ``apply`` / ``finish``) and
``_run_round`` (windows that share one encode: decode with fallback, apply, one
alignment call for the windows that were kept, finish); ``_device_round`` is the GPU
work of a round.  The drivers differ only in which windows they put into a round:

* sequential (``_run_sequential``) — the reference order, one lane, one window at a
  time; required whenever a window depends on the previous one
  (``condition_on_previous_text=True``, ``carry_initial_prompt``,
  ``hallucination_silence_threshold``);
* batched (``_run_batched``) — with ``condition_on_previous_text=False`` and several
  clips (``clip_timestamps`` on a grid), windows of different clips are independent
  (each clip's seek is clip-local, the prompt resets every window:
  transcribe.py:277-287, 513-515), so each clip is a lane and every round takes the
  next window of *all* unfinished clips.  Segments are assembled in clip order
  afterwards, which reproduces the reference's output exactly.  With word timestamps
  the lanes time their words in the round; the words are then re-derived in clip
  order with the reference's running ``last_speech_timestamp``; if that would move
  any window's seek (it can only through a one-word last segment) the file is
  re-run sequentially;
* many files (``multifile.transcribe_batch``) — a lane per file, the next window of
  every live file in a round, a freed place refilled from the pending files.

The log-mel of the whole file is computed on the GPU and stays there; windows
are cut from it on the device.
"""

import os
import warnings
from dataclasses import replace
from typing import TYPE_CHECKING, List, Optional, Tuple, Union

import numpy as np

from .audio import FRAMES_PER_SECOND, HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE, load_audio_device
from .backend_hip import DeviceAudio
from .decoding import DecodingOptions, DecodingResult, detect_language, next_seed, run_windows
from .timing import WordTiming, apply_alignment, find_alignment_batch
from .tokenizer import LANGUAGES, get_tokenizer
from .vad import clamp_clips, frames_to_seconds, resident_spans, resolve_options

if TYPE_CHECKING:
    from .model import Whisper


def _window_seed(file_seed: int, seek: int, temperature_index: int) -> int:
    """Sampling seed of one window's decode at one fallback temperature: a function of
    the file's seed and the window, not of the order in which windows are decoded, so a
    file samples the same tokens whether its windows run alone or next to other files'."""
    x = (file_seed ^ (seek * 0xBF58476D1CE4E5B9) ^ ((temperature_index + 1) * 0x94D049BB133111EB)) % (1 << 64)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) % (1 << 64)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) % (1 << 64)
    return x ^ (x >> 31)


def _decode_with_fallback(model, base_opts: DecodingOptions, temperatures, prompts: List, thresholds,
                          languages: Optional[List[Optional[str]]] = None,
                          seed_keys: Optional[List[Tuple[int, int]]] = None) -> List[DecodingResult]:
    """transcribe.py:188-228 for a batch of windows (slots 0..n-1 already encoded).
    A retry at the next temperature decodes only the windows that still need work,
    from the encoder slots that already hold their audio features (no re-encode).
    ``languages``: one per window (windows of different files), default the options'.
    ``seed_keys``: (file seed, seek) per window.  With them a retry at T > 0 decodes each
    pending window in a call of its own, seeded by ``_window_seed``: the device sampler
    keys its draws by the call's seed and the row in the call, so this is what makes a
    window's samples independent of its neighbours in the round.  Without them the
    pending windows share one call and the process counter's next seed."""
    cr_thr, lp_thr, ns_thr = thresholds
    n = len(prompts)
    results: List[Optional[DecodingResult]] = [None] * n
    pending = list(range(n))
    for ti, t in enumerate(temperatures):
        kw = dict(beam_size=None, patience=None) if t > 0 else dict(best_of=None)
        opts = replace(base_opts, temperature=t, **kw)
        calls = [pending]
        if t > 0 and seed_keys is not None:
            calls = [[i] for i in pending]
        res = []
        for call in calls:
            extra = {}
            if languages is not None:
                extra["languages"] = [languages[i] for i in call]
            if t > 0 and seed_keys is not None:
                extra["seed"] = _window_seed(seed_keys[call[0]][0], seed_keys[call[0]][1], ti)
            res += run_windows(model, opts, [prompts[i] for i in call],
                               slots=None if call == list(range(n)) else call, **extra)
        nxt = []
        for i, r in zip(pending, res):
            results[i] = r
            fallback = False
            if cr_thr is not None and r.compression_ratio > cr_thr:
                fallback = True
            if lp_thr is not None and r.avg_logprob < lp_thr:
                fallback = True
            if ns_thr is not None and r.no_speech_prob > ns_thr and lp_thr is not None and r.avg_logprob < lp_thr:
                fallback = False
            if fallback:
                nxt.append(i)
        pending = nxt
        if not pending:
            break
    return results


def _split_segments(tokenizer, result: DecodingResult, seek: int, time_offset: float, segment_size: int,
                    segment_duration: float, input_stride: int, time_precision: float
                    ) -> Tuple[List[dict], int, bool]:
    """Segment building and seek advance of transcribe.py:350-410; returns (segments,
    seek, single_timestamp_ending)."""
    tokens = np.asarray(result.tokens, dtype=np.int64)
    tb = tokenizer.timestamp_begin

    def new_segment(start, end, toks):
        toks = [int(x) for x in toks]
        return dict(seek=seek, start=start, end=end, text=tokenizer.decode([x for x in toks if x < tokenizer.eot]),
                    tokens=toks, temperature=result.temperature, avg_logprob=result.avg_logprob,
                    compression_ratio=result.compression_ratio, no_speech_prob=result.no_speech_prob)

    segs = []
    is_ts = tokens >= tb
    single_end = is_ts[-2:].tolist() == [False, True]
    consecutive = np.where(is_ts[:-1] & is_ts[1:])[0] + 1
    if len(consecutive) > 0:
        slices = consecutive.tolist()
        if single_end:
            slices.append(len(tokens))
        last = 0
        for cut in slices:
            part = tokens[last:cut]
            segs.append(new_segment(time_offset + (int(part[0]) - tb) * time_precision,
                                    time_offset + (int(part[-1]) - tb) * time_precision, part))
            last = cut
        if single_end:
            seek += segment_size
        else:
            seek += (int(tokens[last - 1]) - tb) * input_stride
    else:
        duration = segment_duration
        ts = tokens[is_ts]
        if len(ts) > 0 and int(ts[-1]) != tb:
            duration = (int(ts[-1]) - tb) * time_precision
        segs.append(new_segment(time_offset, time_offset + duration, tokens))
        seek += segment_size
    return segs, seek, single_end


def _check_fp16(model: "Whisper", fp16: bool):
    """transcribe.py:131-140 picks the compute dtype from ``fp16``; here the precision is
    fixed when the context is created (``load_model(..., dtype=)``).  fp16=True on an
    fp32 context computes in fp32 without a warning (the reference warns only on CPU,
    and this fork has that warning commented out, reference transcribe.py:136);
    fp16=False on an fp16 context cannot be honoured and raises instead of silently
    computing in fp16."""
    if not fp16 and model.dtype != "fp32":
        raise ValueError("fp16=False needs a context loaded with dtype='fp32' "
                         "(load_model(..., dtype='fp32')); this one computes in fp16")


def _clear_empty(tokenizer, segs: List[dict]):
    """transcribe.py:494-499 (after word timestamps)."""
    for s in segs:
        if s["start"] == s["end"] or tokenizer.is_blank_text(s["tokens"]):
            s["text"] = ""
            s["tokens"] = []
            s["words"] = []


def _plan_file(model: "Whisper", content_frames: int, language: str, decode_options: dict, *, temperature,
               thresholds, initial_prompt, word_timestamps, prepend_punctuations, append_punctuations,
               clip_timestamps, hallucination_silence_threshold, seek_clips=None):
    """What one file's loop needs besides its mel (transcribe.py:141-183, 230-254):
    (tokenizer, clips, initial prompt tokens, state of the window loop).  ``seek_clips``:
    the clips already in frames (the speech spans of ``skip_silence``), instead of
    ``clip_timestamps``."""
    task = decode_options.get("task", "transcribe")
    tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language,
                              task=task)
    content_duration = float(content_frames * HOP_LENGTH / SAMPLE_RATE)

    if isinstance(clip_timestamps, str):
        clip_timestamps = [float(ts) for ts in (clip_timestamps.split(",") if clip_timestamps else [])]
    seek_points = [round(ts * FRAMES_PER_SECOND) for ts in clip_timestamps]
    if len(seek_points) == 0:
        seek_points.append(0)
    if len(seek_points) % 2 == 1:
        seek_points.append(content_frames)
    if seek_clips is None:
        seek_clips = list(zip(seek_points[::2], seek_points[1::2]))
    else:
        seek_clips = [(int(s), int(e)) for s, e in seek_clips]

    temperatures = [temperature] if isinstance(temperature, (int, float)) else list(temperature)
    base = DecodingOptions(**{k: v for k, v in decode_options.items() if k in DecodingOptions.__dataclass_fields__})
    input_stride = N_FRAMES // model.dims.n_audio_ctx
    time_precision = input_stride * HOP_LENGTH / SAMPLE_RATE

    if isinstance(initial_prompt, str):  # transcribe.py:243-244
        initial_prompt_tokens = tokenizer.encode(" " + initial_prompt.strip())
    else:
        initial_prompt_tokens = list(initial_prompt) if initial_prompt else []

    if word_timestamps and task == "translate":
        warnings.warn("Word-level timestamps on translations may not be reliable.")
    state = dict(content_frames=content_frames, content_duration=content_duration, tokenizer=tokenizer,
                 temperatures=temperatures, thresholds=thresholds, base=base, input_stride=input_stride,
                 time_precision=time_precision, word_timestamps=word_timestamps, prepend=prepend_punctuations,
                 append=append_punctuations, hallucination=hallucination_silence_threshold)
    return tokenizer, seek_clips, initial_prompt_tokens, state


def transcribe(model: "Whisper", audio: Union[str, np.ndarray], *, verbose: Optional[bool] = None,
               temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
               compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
               no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
               initial_prompt: Optional[Union[str, List[int]]] = None, carry_initial_prompt: bool = False,
               word_timestamps: bool = False, prepend_punctuations: str = "\"'“¿([{-",
               append_punctuations: str = "\"'.。,，!！?？:：”)]}、", clip_timestamps: Union[str, List[float]] = "0",
               hallucination_silence_threshold: Optional[float] = None, schedule: str = "auto",
               mel_max_reduce=None, _mel_prepared: Optional[Tuple[int, int, int]] = None,
               skip_silence: Union[bool, dict] = False, channels=None, channel_names=None,
               **decode_options) -> dict:
    """transcribe.py:41-524.  Extra keywords: ``schedule`` ("auto", "sequential",
    "batched"), ``mel_max_reduce`` (callable local max -> global max, used when
    one file is sharded over GPUs: the log-mel floor is a whole-file max,
    audio.py:155, so ranks all-reduce it before normalizing) and ``skip_silence``
    (True, or a dict of ``vad.DEFAULTS`` options): the speech spans of the resident
    waveform are found on the device (``vad.speech_spans``) and become the clips, so
    only they are encoded and decoded; the result gains ``"speech_spans"`` in seconds.
    ``no_repeat_ngram_size`` and ``repetition_penalty`` are decoding options like the
    others (``DecodingOptions``): they hold for every window and every rung of the
    temperature ladder.  So do ``hotwords``, ``hotword_boost`` and ``hotword_start`` (phrase
    biasing): the table is installed for every window, also with ``skip_silence`` and
    ``condition_on_previous_text=False``; ``avg_logprob`` is then that of the biased
    distribution, which the ``logprob_threshold`` fallback compares.
    ``channels``: None or "mix" is the mix-down of all channels; "split" or a list of channel
    indices transcribes each selected channel of the file (a path, or a float32 array
    ``[C][n]`` at 16 kHz) on its own, through ``transcribe_batch``'s machinery, and returns
    ``merge_channels`` of the per-channel results under ``channel_names``.  A split value
    cannot be combined with ``schedule``, ``mel_max_reduce``, ``_mel_prepared`` or a
    ``DeviceAudio``."""
    if channels is not None and not (isinstance(channels, str) and channels == "mix"):
        for name, given in (("schedule", schedule != "auto"), ("mel_max_reduce", mel_max_reduce is not None),
                            ("_mel_prepared", _mel_prepared is not None),
                            ("DeviceAudio", isinstance(audio, DeviceAudio))):
            if given:
                raise ValueError(f"transcribe(channels={channels!r}) cannot be combined with "
                                 f"{'a ' if name == 'DeviceAudio' else ''}{name}")
        from .multifile import transcribe_batch
        return transcribe_batch(
            model, [audio], channels=[channels], channel_names=None if channel_names is None else [channel_names],
            verbose=verbose, temperature=temperature, compression_ratio_threshold=compression_ratio_threshold,
            logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold,
            condition_on_previous_text=condition_on_previous_text, initial_prompt=initial_prompt,
            carry_initial_prompt=carry_initial_prompt, word_timestamps=word_timestamps,
            prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations,
            clip_timestamps=clip_timestamps, hallucination_silence_threshold=hallucination_silence_threshold,
            skip_silence=skip_silence, **decode_options)[0]
    _check_fp16(model, decode_options.pop("fp16", True))
    ctx = model.ctx
    n_mels = model.dims.n_mels
    vad_params = _skip_silence_params(skip_silence, clip_timestamps)
    if vad_params is not None and _mel_prepared is not None:
        raise ValueError("skip_silence is not available on the sharded path (_mel_prepared)")
    if isinstance(audio, str) and _mel_prepared is None:
        # a path: its PCM is mixed down and resampled on the device and stays there
        audio = load_audio_device(model, audio)
    if _mel_prepared is not None:
        # distributed.run_shard: this rank's frames are already in the context and
        # normalised with the all-reduced max; seeks stay absolute
        if decode_options.get("language") is None:
            raise ValueError("sharded transcription needs an explicit language")

        def compute_mel():
            return _mel_prepared[0]
        mel_max_reduce = None
    elif isinstance(audio, DeviceAudio):
        if audio.ctx is not ctx:
            raise ValueError("DeviceAudio belongs to another model context")
        if audio.offset:
            raise ValueError("DeviceAudio is a segment behind other files: transcribe() takes the only resident one")
        resident = audio.n_samples

        def compute_mel():
            return ctx.log_mel_resident(resident, n_mels, padding=N_SAMPLES, normalize=mel_max_reduce is None)
    else:
        audio = np.ascontiguousarray(audio.detach().cpu().numpy() if hasattr(audio, "detach") else audio,
                                     dtype=np.float32)
        if vad_params is not None:
            # the detector reads the resident waveform: upload once, the mel is computed from it too
            resident = ctx.audio_upload(audio).n_samples

            def compute_mel():
                return ctx.log_mel_resident(resident, n_mels, padding=N_SAMPLES, normalize=mel_max_reduce is None)
        else:
            def compute_mel():
                return ctx.log_mel(audio, n_mels, padding=N_SAMPLES, normalize=mel_max_reduce is None)

    def prepare_mel():
        nf = compute_mel()
        if mel_max_reduce is not None and _mel_prepared is None:
            ctx.mel_normalize(float(mel_max_reduce(ctx.mel_max())))
        return nf

    spans = seek_clips = None
    probe_frame = 0  # where the language probe window starts
    if vad_params is not None:
        # the detector runs first, on the waveform: a file without speech costs neither mel nor encode
        spans = resident_spans(ctx, 1, vad_params)[0][0]
        seek_clips = clamp_clips(spans, resident // HOP_LENGTH)  # the mel's content_frames
        if not seek_clips:
            # nothing to decode; an empty clip list would mean "the whole file" (_plan_file)
            language = decode_options.get("language") or (None if model.is_multilingual else "en")
            return dict(text="", segments=[], language=language, speech_spans=frames_to_seconds(spans))
        probe_frame = seek_clips[0][0]

    frames = prepare_mel()
    content_frames = frames - N_FRAMES

    if decode_options.get("language") is None:
        if not model.is_multilingual:
            decode_options["language"] = "en"
        else:
            seg = ctx.mel_read(n_mels, probe_frame, min(N_FRAMES, frames - probe_frame))
            if seg.shape[1] < N_FRAMES:
                seg = np.pad(seg, ((0, 0), (0, N_FRAMES - seg.shape[1])))
            _, probs = detect_language(model, seg)
            decode_options["language"] = max(probs, key=probs.get)
            # detect_language overwrote the context mel with the probe window
            frames = prepare_mel()
            if verbose is not None:
                print(f"Detected language: {LANGUAGES[decode_options['language']].title()}")
    language = decode_options["language"]
    plan = _plan_file(model, content_frames, language, decode_options, temperature=temperature,
                      thresholds=(compression_ratio_threshold, logprob_threshold, no_speech_threshold),
                      initial_prompt=initial_prompt, word_timestamps=word_timestamps,
                      prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations,
                      clip_timestamps=clip_timestamps,
                      hallucination_silence_threshold=hallucination_silence_threshold, seek_clips=seek_clips)
    tokenizer, seek_clips, initial_prompt_tokens, state = plan
    batched = schedule == "batched" or (
        schedule == "auto" and not condition_on_previous_text and not carry_initial_prompt
        and not initial_prompt_tokens and len(seek_clips) > 1)
    if hallucination_silence_threshold is not None and word_timestamps:
        batched = False  # its seek rules read the running last_speech_timestamp
    segments = None
    if batched:
        segments = _run_batched(model, seek_clips, initial_prompt_tokens, state)
    if segments is None:
        segments = _run_sequential(model, seek_clips, initial_prompt_tokens, condition_on_previous_text,
                                   carry_initial_prompt, state)
    all_tokens = list(initial_prompt_tokens)
    all_segments = []
    for s in segments:
        all_segments.append({"id": len(all_segments), **s})
        all_tokens.extend(s["tokens"])
        if verbose:
            print(f"[{s['start']:.2f} --> {s['end']:.2f}] {s['text']}")
    result = dict(text=tokenizer.decode(all_tokens[len(initial_prompt_tokens):]), segments=all_segments,
                  language=language)
    if spans is not None:
        result["speech_spans"] = frames_to_seconds(spans)
    return result


def _skip_silence_params(skip_silence, clip_timestamps):
    """``skip_silence`` of transcribe() / transcribe_batch() -> ``vad.VadParams``, None when it
    is off.  The spans become the clips, so explicit ``clip_timestamps`` cannot be combined."""
    if skip_silence is None or skip_silence is False:
        return None
    if skip_silence is True:
        skip_silence = {}
    if not isinstance(skip_silence, dict):
        raise TypeError(f"skip_silence must be a bool or a dict of options, not {type(skip_silence).__name__}")
    params = resolve_options(**skip_silence)
    if not (isinstance(clip_timestamps, str) and clip_timestamps == "0"):
        raise ValueError("skip_silence chooses the clips itself: it cannot be combined with clip_timestamps")
    return params


def _window_at(seek: int, clip: Tuple[int, int], content_frames: int):
    segment_size = min(N_FRAMES, content_frames - seek, clip[1] - seek)
    return segment_size, segment_size * HOP_LENGTH / SAMPLE_RATE


def _apply_result(result, seek, segment_size, st) -> Tuple[List[dict], int, bool, bool]:
    """no-speech skip (transcribe.py:308-321) then segment split; returns
    (segments, new seek, skipped, single_timestamp_ending).  Empty segments are not
    cleared yet (word timestamps see them first, transcribe.py:412-499)."""
    thr_ns, thr_lp = st["thresholds"][2], st["thresholds"][1]
    if thr_ns is not None:
        skip = result.no_speech_prob > thr_ns
        if thr_lp is not None and result.avg_logprob > thr_lp:
            skip = False
        if skip:
            return [], seek + segment_size, True, False
    time_offset = float(seek * HOP_LENGTH / SAMPLE_RATE)
    segs, new_seek, single_end = _split_segments(st["tokenizer"], result, seek, time_offset, segment_size,
                                                 segment_size * HOP_LENGTH / SAMPLE_RATE, st["input_stride"],
                                                 st["time_precision"])
    return segs, new_seek, False, single_end


def get_end(segments: List[dict]) -> Optional[float]:
    """utils.py:78-82."""
    return next((w["end"] for s in reversed(segments) for w in reversed(s.get("words", []))),
                segments[-1]["end"] if segments else None)


_PUNCTUATION = "\"'“¿([{-\"'.。,，!！?？:：”)]}、"  # transcribe.py:183


def _word_anomaly_score(word: dict) -> float:
    """transcribe.py:327-337."""
    probability = word.get("probability", 0.0)
    duration = word["end"] - word["start"]
    score = 0.0
    if probability < 0.15:
        score += 1.0
    if duration < 0.133:
        score += (0.133 - duration) * 15
    if duration > 2.0:
        score += duration - 2.0
    return score


def _is_segment_anomaly(segment: Optional[dict]) -> bool:
    """transcribe.py:339-345."""
    if segment is None or not segment["words"]:
        return False
    words = [w for w in segment["words"] if w["word"] not in _PUNCTUATION]
    words = words[:8]
    score = sum(_word_anomaly_score(w) for w in words)
    return score >= 3 or score + 0.01 >= len(words)


def _next_words_segment(segments: List[dict]) -> Optional[dict]:
    return next((s for s in segments if s["words"]), None)


def _words_and_seek(st, segs, alignment, seek, previous_seek, segment_size, single_end, last_speech):
    """transcribe.py:412-426 on a precomputed alignment: words of every segment, the
    seek refinement from the last word; returns (seek, last_speech_timestamp)."""
    fresh = [WordTiming(w.word, list(w.tokens), w.start, w.end, w.probability) for w in alignment]
    apply_alignment(segs, fresh, st["tokenizer"], st["prepend"], st["append"], last_speech)
    time_offset = float(previous_seek * HOP_LENGTH / SAMPLE_RATE)
    if not single_end:
        last_word_end = get_end(segs)
        if last_word_end is not None and last_word_end > time_offset:
            seek = round(last_word_end * FRAMES_PER_SECOND)
    return seek


class _Lane:
    """One file's running state of the reference loop (transcribe.py:256-515): clip
    index, seek, the tokens so far with the prompt-reset mark, the last speech time.
    The loop is cut where the GPU work sits: ``next_window`` offers the next window
    and its prompt, ``apply`` takes the decoded result (no-speech skip, segment
    split), ``finish`` takes the window's word alignment (word timings with the seek
    refinement, hallucination-silence rules, empty-segment clearing, prompt reset).
    ``_run_sequential`` drives one lane alone, ``_run_batched`` one lane per clip,
    ``transcribe_batch`` one lane per file.  Seeks are the file's own frames; ``base``
    is where the file's frames start in the context mel."""

    def __init__(self, n_text_ctx: int, clips, initial_prompt_tokens, condition_on_previous_text: bool,
                 carry_initial_prompt: bool, st: dict, base: int = 0, file_seed: int = 0):
        self.st = st
        self.base = base
        self.file_seed = file_seed  # with the seek: the sampling seed of a window's T > 0 retries
        self.clips = clips
        self.initial_prompt_tokens = list(initial_prompt_tokens)
        self.condition_on_previous_text = condition_on_previous_text
        self.carry_initial_prompt = carry_initial_prompt
        self.all_tokens = list(initial_prompt_tokens)
        self.segments: List[dict] = []
        self.prompt_reset_since = 0
        self.remaining_prompt_length = n_text_ctx // 2 - 1 - len(self.initial_prompt_tokens)
        self.last_speech_timestamp = 0.0
        self.clip_idx, self.seek = 0, clips[0][0]
        self.window: Optional[Tuple[int, int]] = None  # (seek, segment size) being decoded
        self.language = st["tokenizer"].language

    def next_window(self) -> Optional[Tuple[int, int, Optional[List[int]]]]:
        """(absolute first frame, segment size, prompt) of the next window; None: done."""
        clips = self.clips
        while self.clip_idx < len(clips):
            cs, ce = clips[self.clip_idx]
            if self.seek < cs:
                self.seek = cs
            if self.seek >= ce:
                self.clip_idx += 1
                if self.clip_idx < len(clips):
                    self.seek = clips[self.clip_idx][0]
                continue
            segment_size, segment_duration = _window_at(self.seek, clips[self.clip_idx], self.st["content_frames"])
            if segment_duration < 1.0:  # fork: drop < 1 s tails (transcribe.py:292-297)
                self.clip_idx += 1
                continue
            if self.carry_initial_prompt:
                nignored = max(len(self.initial_prompt_tokens), self.prompt_reset_since)
                prompt = self.initial_prompt_tokens + self.all_tokens[nignored:][-self.remaining_prompt_length:]
            else:
                prompt = self.all_tokens[self.prompt_reset_since:]
            self.window = (self.seek, segment_size)
            return self.base + self.seek, segment_size, prompt or None
        self.window = None
        return None

    def apply(self, result: DecodingResult) -> bool:
        """The decoded window: no-speech skip, segments, provisional seek.  False: the
        window was skipped (nothing to align, ``finish`` is not called)."""
        seek, segment_size = self.window
        self.result = result
        self.previous_seek = seek
        self.segs, self.seek, skipped, self.single_end = _apply_result(result, seek, segment_size, self.st)
        return not skipped

    def text_tokens(self) -> List[int]:
        """Text tokens of the applied window, the input of its word alignment."""
        eot = self.st["tokenizer"].eot
        return [t for s in self.segs for t in s["tokens"] if t < eot]

    def finish(self, alignment=None):
        """Second half of the loop body; ``alignment`` is the window's find_alignment
        result (word timestamps only)."""
        st, segs, result = self.st, self.segs, self.result
        previous_seek, segment_size = self.window
        seek, single_end = self.seek, self.single_end
        content_frames = st["content_frames"]
        if st["word_timestamps"]:
            seek = _words_and_seek(st, segs, alignment, seek, previous_seek, segment_size, single_end,
                                   self.last_speech_timestamp)
            time_offset = float(previous_seek * HOP_LENGTH / SAMPLE_RATE)
            window_end_time = float((previous_seek + N_FRAMES) * HOP_LENGTH / SAMPLE_RATE)
            segment_duration = segment_size * HOP_LENGTH / SAMPLE_RATE
            threshold = st["hallucination"]
            if threshold is not None:  # transcribe.py:428-484
                if not single_end:
                    last_word_end = get_end(segs)
                    if last_word_end is not None and last_word_end > time_offset:
                        remaining_duration = window_end_time - last_word_end
                        if remaining_duration > threshold:
                            seek = round(last_word_end * FRAMES_PER_SECOND)
                        else:
                            seek = previous_seek + segment_size
                first_segment = _next_words_segment(segs)
                if first_segment is not None and _is_segment_anomaly(first_segment):
                    gap = first_segment["start"] - time_offset
                    if gap > threshold:
                        self.seek = previous_seek + round(gap * FRAMES_PER_SECOND)
                        return
                hal_last_end = self.last_speech_timestamp
                for si in range(len(segs)):
                    segment = segs[si]
                    if not segment["words"]:
                        continue
                    if _is_segment_anomaly(segment):
                        next_segment = _next_words_segment(segs[si + 1:])
                        if next_segment is not None:
                            hal_next_start = next_segment["words"][0]["start"]
                        else:
                            hal_next_start = time_offset + segment_duration
                        silence_before = (segment["start"] - hal_last_end > threshold
                                          or segment["start"] < threshold or segment["start"] - time_offset < 2.0)
                        silence_after = (hal_next_start - segment["end"] > threshold
                                         or _is_segment_anomaly(next_segment) or window_end_time - segment["end"] < 2.0)
                        if silence_before and silence_after:
                            seek = round(max(time_offset + 1, segment["start"]) * FRAMES_PER_SECOND)
                            if st["content_duration"] - segment["end"] < threshold:
                                seek = content_frames
                            segs[si:] = []
                            break
                    hal_last_end = segment["end"]
            last_word_end = get_end(segs)
            if last_word_end is not None:
                self.last_speech_timestamp = last_word_end
        self.seek = seek
        _clear_empty(st["tokenizer"], segs)
        self.segments.extend(segs)
        self.all_tokens.extend(t for s in segs for t in s["tokens"])
        if not self.condition_on_previous_text or result.temperature > 0.5:
            self.prompt_reset_since = len(self.all_tokens)


Window = Tuple[_Lane, int, int, Optional[List[int]]]  # (lane, absolute first frame, segment size, prompt)


def _run_round(windows: List[Window], decode_round, align_round=None) -> list:
    """The loop body of every schedule for windows that share one encode (window i in
    slot i): ``decode_round(windows)`` gives their results, each lane applies its own,
    ``align_round`` aligns the windows that were not skipped together ((slot, lane,
    segment size) each; None: no word timestamps), each lane finishes.  Returns the
    (lane, alignment) pairs of the windows that were not skipped."""
    results = decode_round(windows)
    if len(results) != len(windows):
        raise RuntimeError("decode_round returned %d results for %d windows" % (len(results), len(windows)))
    kept = [(slot, w[0], w[2]) for slot, (w, r) in enumerate(zip(windows, results)) if w[0].apply(r)]
    aligns = align_round(kept) if align_round is not None else [None] * len(kept)
    done = [(lane, alignment) for (_, lane, _), alignment in zip(kept, aligns)]
    for lane, alignment in done:
        lane.finish(alignment)
    return done


def _device_round(model, per_window: bool = True, per_file: bool = False):
    """(decode_round, align_round) of ``_run_round`` on the model's context.  The lanes
    share the decoding options, temperatures and thresholds.  ``per_window``: T > 0
    retries are seeded per window (``_window_seed``), not by the process counter;
    ``per_file``: every window decodes in its lane's language."""
    ctx = model.ctx

    def decode_round(windows: List[Window]) -> List[DecodingResult]:
        seeks = [w[1] for w in windows]
        sizes = [w[2] for w in windows]
        ctx.encode(seeks, sizes)
        model._last_windows = (seeks, sizes)
        st = windows[0][0].st
        return _decode_with_fallback(
            model, st["base"], st["temperatures"], [w[3] for w in windows], st["thresholds"],
            languages=[w[0].language for w in windows] if per_file else None,
            seed_keys=[(w[0].file_seed, w[0].window[0]) for w in windows] if per_window else None)

    def align_round(kept):
        if not kept:
            return []
        toks = [lane.st["tokenizer"] for _, lane, _ in kept]
        return find_alignment_batch(model, toks[0], [lane.text_tokens() for _, lane, _ in kept],
                                    [size for _, _, size in kept], [slot for slot, _, _ in kept], tokenizers=toks)

    return decode_round, align_round


def _run_sequential(model, clips, initial_prompt_tokens, condition_on_previous_text, carry_initial_prompt, st):
    """The reference's order: one lane, one window at a time."""
    lane = _Lane(model.dims.n_text_ctx, clips, initial_prompt_tokens, condition_on_previous_text,
                 carry_initial_prompt, st, file_seed=next_seed())
    decode_round, align_round = _device_round(model)
    while True:
        window = lane.next_window()
        if window is None:
            return lane.segments
        _run_round([(lane, *window)], decode_round, align_round if st["word_timestamps"] else None)


def _run_batched(model, clips, initial_prompt_tokens, st):
    """The clip grid: a lane per clip (no prompt of its own, nothing carried over); every
    round offers the next window of every unfinished clip, in clip order, cut into chunks
    of ``max_windows``.  A place freed inside a round is not refilled: which windows share
    a call is part of the result (a lone window takes the single-window step path)."""
    words = st["word_timestamps"]
    lanes = [_Lane(model.dims.n_text_ctx, [clip], (), False, False, st) for clip in clips]
    decode_round, align_round = _device_round(model, per_window=False)
    # word timestamps: per lane, what the ordered pass needs of every window that was kept
    records = {lane: [] for lane in lanes}
    # only the very first window offered sees the initial prompt, and only if it is clip 0's
    first_prompt = list(initial_prompt_tokens) or None
    live = lanes
    while live:
        batch = [(lane, lane.next_window()) for lane in live]
        batch = [(lane, *w) for lane, w in batch if w is not None]
        if batch and batch[0][0] is lanes[0] and first_prompt:
            batch[0] = (*batch[0][:3], first_prompt)
        first_prompt = None
        live = [w[0] for w in batch]
        for b0 in range(0, len(batch), model.ctx.max_windows):
            kept = _run_round(batch[b0:b0 + model.ctx.max_windows], decode_round, align_round if words else None)
            if words:
                for lane, alignment in kept:
                    records[lane].append((*lane.window, lane.result, alignment, lane.seek))
    if not words:
        return [s for lane in lanes for s in lane.segments]
    # ordered pass: the lanes timed their words with the clip's own running last-speech
    # time, which gave the seeks above.  Here every kept window's segments and words are
    # derived again, in clip order, with the running last_speech_timestamp of the
    # reference's sequential loop (transcribe.py:271, 412-426, 485-486); a window whose
    # seek would change under it makes the caller re-run the sequential schedule
    out, last_speech = [], 0.0
    for windows in records.values():
        for seek, segment_size, r, alignment, prov_seek in windows:
            segs, new_seek, _, single_end = _apply_result(r, seek, segment_size, st)
            new_seek = _words_and_seek(st, segs, alignment, new_seek, seek, segment_size, single_end, last_speech)
            if new_seek != prov_seek:
                return None
            end = get_end(segs)
            if end is not None:
                last_speech = end
            _clear_empty(st["tokenizer"], segs)
            out.extend(segs)
    return out
