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

A file given with ``channels="split"`` (or a list of channel indices) is not mixed down:
every selected channel is a lane of its own, as if it were a file (``expand_channels``).
The channels of a file are ingested by one call (``HipContext.*_ingest(channels=...)``: one
upload, one launch, the segments back to back), form a unit that ``split_groups`` never cuts,
and come back as one dict (``merge_channels``).
"""

from typing import TYPE_CHECKING, Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from .audio import (HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE, ingest, ingest_source, select_channels,
                    source_channels)
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


def split_groups(frames: Sequence[int], mel_budget_frames: int,
                 units: Optional[Sequence[int]] = None) -> List[List[int]]:
    """Consecutive files whose frames fit the budget; a file larger than the budget is a
    group of its own (it needs that much mel under transcribe() as well).  ``units`` names
    what must not be cut: ``units[i]`` is the unit of entry i, the entries of a unit are
    consecutive (the channels of a split file), and a unit goes into a group whole; one larger
    than the budget is a group of its own.  Without it every entry is its own unit."""
    if units is None:
        units = range(len(frames))
    elif len(units) != len(frames):
        raise ValueError(f"units: {len(units)} values for {len(frames)} entries")
    groups: List[List[int]] = []
    used = 0
    i = 0
    while i < len(frames):
        j = i + 1
        while j < len(frames) and units[j] == units[i]:
            j += 1
        f = sum(frames[i:j])
        if not groups or used + f > mel_budget_frames:
            groups.append([])
            used = 0
        groups[-1].extend(range(i, j))
        used += f
        i = j
    return groups


def expand_channels(counts: Sequence[Optional[int]]) -> Tuple[List[int], List[int]]:
    """Files -> lanes.  ``counts[i]`` is None for a file that is mixed down (one lane) or the
    number of channels selected from it (that many lanes, in selection order).  Returns
    (file_of, channel_of): per lane the file it belongs to, which is also its unit for
    ``split_groups``, and its place in the file's selection."""
    file_of: List[int] = []
    channel_of: List[int] = []
    for i, c in enumerate(counts):
        if c is not None and c < 1:
            raise ValueError(f"audio {i}: no channel selected")
        for k in range(1 if c is None else c):
            file_of.append(i)
            channel_of.append(k)
    return file_of, channel_of


def merge_channels(results: Sequence[dict], names: Optional[Sequence[str]] = None) -> dict:
    """The per-channel results of one recording as one two-sided (or C-sided) dialogue; a pure
    host function.  ``results[k]`` is what ``transcribe`` returns for channel k's waveform;
    ``names`` default to "0", "1", ... and must be as many.  The dict holds
    ``"channels"``: the results as given, in order (each keeps its own ``"speech_spans"``);
    ``"segments"``: copies of all channels' segments with ``"channel"`` (the name) and
    ``"channel_index"`` (k), sorted by (start, end, channel_index), ``"id"`` renumbered from 0,
    words carried along;
    ``"text"``: one line ``"<name>: <text>"`` per merged segment whose stripped text is not empty;
    ``"language"``: the common one when all channels agree, otherwise that of the channel with
    the largest summed segment duration (ties: the lowest index)."""
    results = list(results)
    if not results:
        raise ValueError("merge_channels: no channels")
    names = [str(k) for k in range(len(results))] if names is None else [str(x) for x in names]
    if len(names) != len(results):
        raise ValueError(f"merge_channels: {len(names)} names for {len(results)} channels")
    merged = []
    for k, r in enumerate(results):
        for seg in r["segments"]:
            merged.append(dict(seg, channel=names[k], channel_index=k))
    merged.sort(key=lambda g: (g["start"], g["end"], g["channel_index"]))  # stable: a channel's order is kept
    for i, seg in enumerate(merged):
        seg["id"] = i
    lines = [f"{seg['channel']}: {seg['text'].strip()}" for seg in merged if seg["text"].strip()]
    langs = [r.get("language") for r in results]
    if all(x == langs[0] for x in langs):
        language = langs[0]
    else:
        spoken = [sum(float(g["end"]) - float(g["start"]) for g in r["segments"]) for r in results]
        language = langs[max(range(len(results)), key=lambda k: (spoken[k], -k))]
    return dict(text="\n".join(lines), segments=merged, language=language, channels=results)


class _SplitSource(NamedTuple):
    """A split file waiting for its group: what ``audio.ingest`` takes (an ``ingest_source``
    tuple, or rows ``[C][n]``) and the channels to select (None: all rows)."""
    source: object
    channels: Optional[list]


def _channel_value(value, what: str):
    """One ``channels`` value -> None (mix), "split", or a list of ints."""
    if value is None or (isinstance(value, str) and value == "mix"):
        return None
    if isinstance(value, str):
        if value != "split":
            raise ValueError(f"{what}: channels={value!r} is none of None, 'mix', 'split' or a list of channel indices")
        return "split"
    return [int(c) for c in value]


def _is_channel_value(v) -> bool:
    if v is None or isinstance(v, str):
        return True
    try:
        return len(v) > 0 and all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in v)
    except TypeError:
        return False


def ingest_group(ctx, group: Sequence[int], sources: Sequence, lengths: Sequence[int],
                 file_of: Optional[Sequence[int]] = None) -> None:
    """The audios ``group`` back to back in the context's resident buffer: ``sources[i]`` is what
    ``audio.ingest`` takes, a ``_SplitSource`` (one call makes the segments of all its channels,
    entries i, i + 1, ...) or None (a further channel of a split file), ``lengths[i]`` the 16 kHz
    samples planned for it, ``file_of[i]`` the file named in errors (default: i)."""
    total = sum(lengths[i] for i in group)
    offset = 0
    for i in group:
        if sources[i] is None:
            continue  # a further channel of a split file: its first channel's call made the segment
        if isinstance(sources[i], _SplitSource):
            segs = ingest(ctx, sources[i].source, dst_offset=offset, reserve=total, channels=sources[i].channels)
        else:
            segs = [ingest(ctx, sources[i], dst_offset=offset, reserve=total)]
        for k, seg in enumerate(segs):
            if seg.n_samples != lengths[i + k] or seg.offset != offset:
                raise RuntimeError(f"audio {i if file_of is None else file_of[i]}: {seg.n_samples} samples ingested "
                                   f"at {seg.offset}, {lengths[i + k]} planned at {offset}")
            offset += seg.n_samples


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
              decode_round, align_round=None, units: Optional[Sequence[int]] = None) -> List["_Lane"]:
    """The scheduler: checks the lengths, splits the files into mel groups, and runs each
    group's lanes longest-first.  ``prepare_group(indices)`` computes the group's mel and
    returns the files' frame bases; ``make_lanes(indices, bases)`` builds their lanes
    (language detection sits there).  Returns the finished lanes in input order.  ``units``:
    ``split_groups``'s, for entries that are the channels of one file."""
    for i, n in enumerate(n_samples):
        if int(n) < 1:
            raise ValueError(f"audio {i} is empty")
    if mel_budget_frames < 1:
        raise ValueError("mel_budget_frames must be positive")
    frames = [file_frames(n) for n in n_samples]
    out: List[Optional["_Lane"]] = [None] * len(frames)
    for group in split_groups(frames, mel_budget_frames, units):
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


def _transcribe_lanes(model: "Whisper", lengths: Sequence[int], prepare_group: Callable[[List[int]], Sequence[int]],
                      languages: List[Optional[str]], prompts: Sequence, clips: Sequence, *,
                      units: Optional[Sequence[int]] = None, spans: Optional[dict] = None,
                      mel_budget_frames: int = DEFAULT_MEL_BUDGET_FRAMES, verbose: Optional[bool] = None,
                      temperature, thresholds, condition_on_previous_text: bool, carry_initial_prompt: bool,
                      word_timestamps: bool, prepend_punctuations: str, append_punctuations: str,
                      hallucination_silence_threshold: Optional[float], decode_options: dict) -> List[dict]:
    """What follows the ingest: ``lengths[i]`` samples of audio i (one lane each) are somewhere
    ``prepare_group(indices)`` can reach; it computes the log-mel of those audios into the context
    mel and returns their frame bases.  Then, per group: language detection for the lanes whose
    ``languages[i]`` is None (filled in here), the plans, ``run_files`` and the per-lane result
    dicts.  ``prompts`` and ``clips`` are per lane.  ``spans`` (skip_silence): the dict that
    ``prepare_group`` fills with each audio's speech spans in frames, which become its clips.
    ``transcribe_batch`` (the files of the resident segments) and ``StreamingPool`` (the buffers of
    its slots) both run this."""
    ctx = model.ctx
    n = len(lengths)
    probe = get_tokenizer(model.is_multilingual, num_languages=model.num_languages) if model.is_multilingual else None
    clips_of: dict = {}    # skip_silence: the clips the spans give (clamped to the file's whole frames)

    def file_clips(k: int, i: int, bases):
        if spans is not None and i not in clips_of:
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
    # one sampling seed per file (per channel of a split file), drawn in input order as a loop of
    # transcribe() calls over the files and the channel waveforms draws them
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
                      align_round=align_round if word_timestamps else None, units=units)
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
        if spans is not None:
            results[-1]["speech_spans"] = frames_to_seconds(spans[i])
    return results


def transcribe_batch(model: "Whisper", audios: Sequence[Union[str, np.ndarray]], *,
                     language: Union[None, str, Sequence[Optional[str]]] = None,
                     mel_budget_frames: int = DEFAULT_MEL_BUDGET_FRAMES, verbose: Optional[bool] = None,
                     temperature: Union[float, Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                     compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                     no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
                     initial_prompt=None, carry_initial_prompt: bool = False, word_timestamps: bool = False,
                     prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                     clip_timestamps="0", hallucination_silence_threshold: Optional[float] = None,
                     skip_silence: Union[bool, dict] = False, channels=None, channel_names=None,
                     **decode_options) -> List[dict]:
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
    ``hotword_boost`` / ``hotword_start`` are one phrase table for all files.

    ``channels``: one value for all files or a list with one per file; None or "mix" is the
    mix-down above, "split" transcribes every channel of the file on its own, a list of
    channel indices those channels.  A split file's result is ``merge_channels`` of its
    channels' results: ``result[i]["channels"][k]`` is what ``transcribe(model,
    load_audio_channels(audios[i])[k], ...)`` returns.  A 2-D float32 array ``[C][n]`` at 16 kHz
    is accepted only with a split value; its rows are the channels.  Lengths, language
    detection, speech spans, plans and sampling seeds are per channel; ``language``,
    ``initial_prompt`` and ``clip_timestamps`` given per file hold for all its channels.
    ``channel_names``: the names ``merge_channels`` uses, one list for all split files or a
    list with one (or None) per file."""
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
    # A split file has one entry per selected channel: the first holds the file's source and the
    # selection (one ingest call makes all its segments), the others None.
    audios = list(audios)
    n_files = len(audios)
    selections = [_channel_value(v, f"audio {i}") for i, v in
                  enumerate(_per_file(channels, n_files, "channels", _is_channel_value))]
    sources: List[Optional[tuple]] = []
    lengths: List[int] = []
    selected: List[Optional[list]] = [None] * n_files  # per split file, the channel indices
    for i, a in enumerate(audios):
        if isinstance(a, DeviceAudio):
            raise TypeError(f"audio {i}: DeviceAudio is one file resident in the context; pass paths or arrays")
        if isinstance(a, str):
            # FLAC bytes and PCM wait for the group's turn; the length has to be known before
            a, length = ingest_source(a, need_length=True, channels=selections[i])
            if isinstance(a, tuple):
                if selections[i] is not None:
                    selected[i] = select_channels(selections[i], source_channels(a))
                    sources.extend([_SplitSource(a, selected[i])] + [None] * (len(selected[i]) - 1))
                    lengths.extend([length] * len(selected[i]))
                    continue
                sources.append(a)
                lengths.append(length)
                continue
            if selections[i] is not None:  # resampled on the host: the selected rows already
                selected[i] = list(range(a.shape[0]))
                rows = np.ascontiguousarray(a, dtype=np.float32)
                sources.extend([_SplitSource(rows, None)] + [None] * (a.shape[0] - 1))
                lengths.extend([a.shape[1]] * a.shape[0])
                continue
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
        if selections[i] is not None:
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2:
                raise ValueError(f"audio {i} is neither 1-D nor [channels][samples] (shape {a.shape})")
            selected[i] = select_channels(selections[i], a.shape[0])
            sources.extend([_SplitSource(a, selected[i])] + [None] * (len(selected[i]) - 1))
            lengths.extend([a.shape[1]] * len(selected[i]))
            continue
        if a.ndim != 1:
            raise ValueError(f"audio {i} is not 1-D (shape {a.shape}); a [channels][samples] array needs "
                             "channels='split' or a list of channel indices")
        sources.append((a, SAMPLE_RATE, 32))
        lengths.append(a.shape[0])
    file_of, _ = expand_channels([None if sel is None else len(sel) for sel in selected])
    n = len(sources)
    if channel_names is None or (len(channel_names) > 0 and all(isinstance(x, str) for x in channel_names)):
        names_of = [channel_names] * n_files
    else:
        names_of = _per_file(channel_names, n_files, "channel_names", lambda v: False)
    for i, sel in enumerate(selected):
        if sel is not None and names_of[i] is not None and len(names_of[i]) != len(sel):
            raise ValueError(f"audio {i}: {len(names_of[i])} channel_names for {len(sel)} channels")

    def per_lane(value, name, is_single):
        per_file = _per_file(value, n_files, name, is_single)
        return [per_file[i] for i in file_of]

    languages = per_lane(language, "language", lambda v: v is None or isinstance(v, str))
    prompts = per_lane(initial_prompt, "initial_prompt",
                       lambda v: v is None or isinstance(v, str) or all(_is_number(x) for x in v))
    clips = per_lane(clip_timestamps, "clip_timestamps",
                     lambda v: isinstance(v, str) or all(_is_number(x) for x in v))
    thresholds = (compression_ratio_threshold, logprob_threshold, no_speech_threshold)
    spans: Optional[dict] = None if vad_params is None else {}  # skip_silence: file -> its speech spans in frames

    def prepare_group(group: List[int]):
        # the group's files back to back in the resident buffer (PCM resampled there, arrays
        # copied), then the log-mel of the resident segments
        ingest_group(ctx, group, sources, lengths, file_of)
        if vad_params is not None:
            # one detector call for the group, on the segments that were just ingested
            for i, (sp, _) in zip(group, resident_spans(ctx, len(group), vad_params)):
                spans[i] = sp
        return ctx.log_mel_batch_resident([lengths[i] for i in group], n_mels, padding=N_SAMPLES)

    results = _transcribe_lanes(
        model, lengths, prepare_group, languages, prompts, clips, units=file_of, spans=spans,
        mel_budget_frames=mel_budget_frames, verbose=verbose, temperature=temperature, thresholds=thresholds,
        condition_on_previous_text=condition_on_previous_text, carry_initial_prompt=carry_initial_prompt,
        word_timestamps=word_timestamps, prepend_punctuations=prepend_punctuations,
        append_punctuations=append_punctuations, hallucination_silence_threshold=hallucination_silence_threshold,
        decode_options=decode_options)
    if all(sel is None for sel in selected):
        return results
    out = []
    for i, sel in enumerate(selected):
        mine = [results[j] for j in range(n) if file_of[j] == i]
        out.append(mine[0] if sel is None else merge_channels(mine, names_of[i]))
    return out
