"""transcribe_batch: many files decoded together, one lane per file.

Inside a file every window depends on the previous one (seek, prompt carry-over, the
running last-speech time), so ``transcribe()`` with the default options walks it one
window at a time.  Different files are independent whatever the options are: here
each file is a lane (``transcribe._Lane``, the reference loop's state for one file)
and every round takes the next window of all live lanes.  The round itself — encode,
decode with fallback, apply, one alignment call, finish — is ``transcribe._run_round``,
the body that the sequential and the clip schedule run too; this module is the third
driver of it and adds only which lanes are live.

Files are taken in groups whose log-mel fits ``mel_budget_frames``.  A group's files
are ingested back to back into the context's resident audio (``audio.ingest_source``
decides how: a path's PCM is mixed down and resampled there, ``HipContext.audio_ingest``;
a ``.flac`` path's frames are also decoded there, ``HipContext.flac_ingest``; a ``.wav``
path's data chunk is read there in its own encoding, ``HipContext.wav_ingest``; an array is
copied), and one
``log_mel_batch_resident`` call computes the group's mel (each file normalised with
its own max), the files' frames lying back to back in the context mel.  At most
``ctx.max_windows`` lanes are live; a lane that ends hands its slot to the next
pending file of the group.  ``run_files`` is the scheduler alone, with the GPU work
behind callables, so it can be driven without a device.
"""

from typing import TYPE_CHECKING, Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .audio import HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE, ingest, ingest_source
from .backend_hip import DeviceAudio
from .decoding import DecodingResult, language_probs, next_seed
from .tokenizer import LANGUAGES, get_tokenizer
from .transcribe import Window, _Lane, _check_fp16, _device_round, _plan_file, _run_round, _skip_silence_params
from .vad import clamp_clips, frames_to_seconds, resident_spans

if TYPE_CHECKING:
    from .model import Whisper

# frames of log-mel one group may hold.  A frame is n_mels floats: at 128 mels this is
# 2 GiB of mel (plus 2.4 GiB of concatenated audio), about 11 hours of audio per group.
DEFAULT_MEL_BUDGET_FRAMES = 4_000_000


def file_frames(n_samples: int) -> int:
    """Frames of one file's log-mel with the 30 s padding transcribe() uses."""
    return (int(n_samples) + N_SAMPLES) // HOP_LENGTH


def split_groups(frames: Sequence[int], mel_budget_frames: int) -> List[List[int]]:
    """Consecutive files whose frames fit the budget; a file larger than the budget is a
    group of its own (it needs that much mel under transcribe() as well)."""
    groups: List[List[int]] = []
    used = 0
    for i, f in enumerate(frames):
        if not groups or used + f > mel_budget_frames:
            groups.append([])
            used = 0
        groups[-1].append(i)
        used += f
    return groups


def run_lanes(lanes: Sequence["_Lane"], max_windows: int, decode_round: Callable[[List[Window]], List[DecodingResult]],
              align_round: Optional[Callable[[List[Tuple[int, "_Lane", int]]], List[list]]] = None) -> None:
    """Rounds over ``lanes`` (taken in the given order): every live lane offers its next
    window, ``decode_round`` decodes them together (window i in slot i), each lane applies
    its result; with ``align_round`` the windows that were not skipped are aligned together
    ((slot, lane, segment size) each) before the lanes finish them.  At most ``max_windows``
    lanes are live; a lane that ends frees its place for the next pending one."""
    if max_windows < 1:
        raise ValueError("max_windows must be at least 1")
    pending = list(lanes)
    live: List["_Lane"] = []
    while True:
        windows: List[Window] = []
        still: List["_Lane"] = []
        for lane in live:
            w = lane.next_window()
            if w is not None:
                still.append(lane)
                windows.append((lane, *w))
        while len(still) < max_windows and pending:
            lane = pending.pop(0)
            w = lane.next_window()
            if w is not None:  # None: nothing to decode (shorter than 1 s)
                still.append(lane)
                windows.append((lane, *w))
        live = still
        if not windows:
            return
        _run_round(windows, decode_round, align_round)


def run_files(n_samples: Sequence[int], *, max_windows: int, mel_budget_frames: int,
              prepare_group: Callable[[List[int]], Sequence[int]],
              make_lanes: Callable[[List[int], Sequence[int]], List["_Lane"]],
              decode_round, align_round=None) -> List["_Lane"]:
    """The scheduler: checks the lengths, splits the files into mel groups, and runs each
    group's lanes longest-first.  ``prepare_group(indices)`` computes the group's mel and
    returns the files' frame bases; ``make_lanes(indices, bases)`` builds their lanes
    (language detection sits there).  Returns the finished lanes in input order."""
    for i, n in enumerate(n_samples):
        if int(n) < 1:
            raise ValueError(f"audio {i} is empty")
    if mel_budget_frames < 1:
        raise ValueError("mel_budget_frames must be positive")
    frames = [file_frames(n) for n in n_samples]
    out: List[Optional["_Lane"]] = [None] * len(frames)
    for group in split_groups(frames, mel_budget_frames):
        bases = prepare_group(group)
        lanes = make_lanes(group, bases)
        for i, lane in zip(group, lanes):
            out[i] = lane
        order = sorted(range(len(group)), key=lambda k: -frames[group[k]])  # stable: ties keep input order
        run_lanes([lanes[k] for k in order], max_windows, decode_round, align_round)
    return out


def _per_file(value, n: int, name: str, is_single) -> list:
    """One value for all files, or a list with one per file."""
    if is_single(value):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} values for {n} files")
    return value


def _is_number(x) -> bool:
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def transcribe_batch(model: "Whisper", audios: Sequence[Union[str, np.ndarray]], *,
                     language: Union[None, str, Sequence[Optional[str]]] = None,
                     mel_budget_frames: int = DEFAULT_MEL_BUDGET_FRAMES, verbose: Optional[bool] = None,
                     temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                     compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                     no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
                     initial_prompt=None, carry_initial_prompt: bool = False, word_timestamps: bool = False,
                     prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                     clip_timestamps="0", hallucination_silence_threshold: Optional[float] = None,
                     skip_silence: Union[bool, dict] = False, **decode_options) -> List[dict]:
    """``[transcribe(model, a, **kwargs) for a in audios]`` with the files decoded
    together: ``result[i]`` is what ``transcribe(model, audios[i], ...)`` returns.

    ``audios``: paths and/or 1-D arrays.  ``language``: None (detected per file on a
    multilingual model), one code, or one per file.  ``initial_prompt`` and
    ``clip_timestamps``: one value for all files, or a list with one per file (a list of
    ints is one token prompt, a list of numbers one clip list).  ``mel_budget_frames``
    bounds the log-mel frames held on the device at a time.  ``skip_silence``: the speech
    spans of all files of a group come from one detector call after the group's ingest and
    become the files' clips; a file without speech takes no lane.  The other keywords are
    transcribe()'s; the decoding options among them (``no_repeat_ngram_size`` and
    ``repetition_penalty`` included) are one value for all files, and ``hotwords`` with
    ``hotword_boost`` / ``hotword_start`` are one phrase table for all files."""
    for k in ("schedule", "mel_max_reduce", "_mel_prepared"):
        if k in decode_options:
            raise TypeError(f"transcribe_batch() does not take {k!r}")
    _check_fp16(model, decode_options.pop("fp16", True))
    vad_params = _skip_silence_params(skip_silence, clip_timestamps)
    ctx = model.ctx
    n_mels = model.dims.n_mels
    if isinstance(audios, (str, np.ndarray, DeviceAudio)):
        raise TypeError("audios must be a sequence of paths and/or 1-D arrays")
    # what audio_ingest takes per file, (pcm or waveform, rate, bits), (FLAC bytes,) for
    # flac_ingest or (WAV bytes, its wav_info) for wav_ingest, and the 16 kHz length it gives
    sources: List[tuple] = []
    lengths: List[int] = []
    for i, a in enumerate(audios):
        if isinstance(a, DeviceAudio):
            raise TypeError(f"audio {i}: DeviceAudio is one file resident in the context; pass paths or arrays")
        if isinstance(a, str):
            # FLAC bytes and PCM wait for the group's turn; the length has to be known before
            a, length = ingest_source(a, need_length=True)
            if isinstance(a, tuple):
                sources.append(a)
                lengths.append(length)
                continue
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"audio {i} is not 1-D (shape {a.shape})")
        sources.append((a, SAMPLE_RATE, 32))
        lengths.append(a.shape[0])
    n = len(sources)
    languages = _per_file(language, n, "language", lambda v: v is None or isinstance(v, str))
    prompts = _per_file(initial_prompt, n, "initial_prompt",
                        lambda v: v is None or isinstance(v, str) or all(_is_number(x) for x in v))
    clips = _per_file(clip_timestamps, n, "clip_timestamps",
                      lambda v: isinstance(v, str) or all(_is_number(x) for x in v))
    thresholds = (compression_ratio_threshold, logprob_threshold, no_speech_threshold)
    probe = get_tokenizer(model.is_multilingual, num_languages=model.num_languages) if model.is_multilingual else None

    def prepare_group(group: List[int]):
        # the group's files back to back in the resident buffer (PCM resampled there, arrays
        # copied), then the log-mel of the resident segments
        total = sum(lengths[i] for i in group)
        offset = 0
        for i in group:
            seg = ingest(ctx, sources[i], dst_offset=offset, reserve=total)
            if seg.n_samples != lengths[i]:
                raise RuntimeError(f"audio {i}: {seg.n_samples} samples ingested, {lengths[i]} planned")
            offset += seg.n_samples
        if vad_params is not None:
            # one detector call for the group, on the segments that were just ingested
            for i, (sp, _) in zip(group, resident_spans(ctx, len(group), vad_params)):
                spans[i] = sp
        return ctx.log_mel_batch_resident([lengths[i] for i in group], n_mels, padding=N_SAMPLES)

    spans: dict = {}       # skip_silence: file -> its speech spans in frames
    clips_of: dict = {}    # and the clips they give (clamped to the file's whole frames)

    def file_clips(k: int, i: int, bases):
        if vad_params is not None and i not in clips_of:
            clips_of[i] = clamp_clips(spans[i], int(bases[k + 1] - bases[k]) - N_FRAMES)
        return clips_of.get(i)

    def detect(group: List[int], bases) -> None:
        """Language of every file of the group that has none: the first window of up to
        max_windows files per encode, one <|startoftranscript|> pass per slot."""
        # with skip_silence the probe window starts at the first span; a file without one is not probed
        first = {k: (file_clips(k, i, bases) or [(0, 0)])[0][0] for k, i in enumerate(group)}
        todo = [k for k, i in enumerate(group) if languages[i] is None and file_clips(k, i, bases) != []]
        for c0 in range(0, len(todo), ctx.max_windows):
            chunk = todo[c0:c0 + ctx.max_windows]
            seeks = [int(bases[k]) + first[k] for k in chunk]
            sizes = [min(N_FRAMES, int(bases[k + 1] - bases[k]) - first[k]) for k in chunk]
            ctx.encode(seeks, sizes)
            model._last_windows = (seeks, sizes)
            for slot, k in enumerate(chunk):
                _, probs = language_probs(model, slot, probe)
                languages[group[k]] = max(probs, key=probs.get)
                if verbose is not None:
                    print(f"[{group[k]}] Detected language: {LANGUAGES[languages[group[k]]].title()}")

    plans = {}
    # one sampling seed per file, drawn in input order as a loop of transcribe() calls draws them
    file_seeds = [next_seed() for _ in range(n)]

    def make_lanes(group: List[int], bases) -> List[_Lane]:
        if not model.is_multilingual:
            for i in group:
                languages[i] = languages[i] or "en"
        else:
            detect(group, bases)
        lanes = []
        for k, i in enumerate(group):
            content_frames = int(bases[k + 1] - bases[k]) - N_FRAMES
            clips_i = file_clips(k, i, bases)
            if clips_i == []:
                clips_i = [(0, 0)]  # no speech: a clip that offers no window, so the file takes no lane
            opts = dict(decode_options, language=languages[i])
            plan = _plan_file(model, content_frames, languages[i], opts, temperature=temperature,
                              thresholds=thresholds, initial_prompt=prompts[i], word_timestamps=word_timestamps,
                              prepend_punctuations=prepend_punctuations, append_punctuations=append_punctuations,
                              clip_timestamps=clips[i],
                              hallucination_silence_threshold=hallucination_silence_threshold, seek_clips=clips_i)
            plans[i] = plan
            tokenizer, seek_clips, prompt_tokens, st = plan
            lanes.append(_Lane(model.dims.n_text_ctx, seek_clips, prompt_tokens, condition_on_previous_text,
                               carry_initial_prompt, st, base=int(bases[k]), file_seed=file_seeds[i]))
        return lanes

    decode_round, align_round = _device_round(model, per_file=True)
    lanes = run_files(lengths, max_windows=ctx.max_windows, mel_budget_frames=mel_budget_frames,
                      prepare_group=prepare_group, make_lanes=make_lanes, decode_round=decode_round,
                      align_round=align_round if word_timestamps else None)
    results = []
    for i, lane in enumerate(lanes):
        tokenizer, _, prompt_tokens, _ = plans[i]
        all_tokens = list(prompt_tokens)
        segments = []
        for s in lane.segments:
            segments.append({"id": len(segments), **s})
            all_tokens.extend(s["tokens"])
            if verbose:
                print(f"[{i}] [{s['start']:.2f} --> {s['end']:.2f}] {s['text']}")
        results.append(dict(text=tokenizer.decode(all_tokens[len(prompt_tokens):]), segments=segments,
                            language=languages[i]))
        if vad_params is not None:
            results[-1]["speech_spans"] = frames_to_seconds(spans[i])
    return results
