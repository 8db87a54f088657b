"""Scoring: how well given transcripts fit a recording.

``score(model, audio, candidates)`` teacher-forces every candidate text through the decoder
over the recording's audio features and returns the log-probability of each of its tokens
and of the end-of-text behind it; ``score_batch`` does it for many recordings, up to
``max_windows`` per encode, all their candidates in one ``wh_score_batch``
(include/whisper_hip.h).  The vocabulary projection and the log-softmax run fused on the
device (csrc/wh_score.hip): no logits are stored or copied.

A candidate is a string, encoded as ``" " + text.strip()`` (the rule of ``hotwords``), or a
list of token ids.  Its sequence is ``[<|startofprev|>] + prompt`` (with ``initial_prompt``),
the SOT sequence, ``<|notimestamps|>``, the text and ``<|endoftext|>``; the text tokens and
the end-of-text are scored.

The log-probabilities are over the whole vocabulary of the RAW logits: no token suppression,
no timestamp rules, no hotword bias.  They are the model's own distribution, not the filtered
one ``transcribe`` samples from, so ``avg_logprob`` here and ``DecodingResult.avg_logprob``
are the same quantity only up to those filters.
"""

from typing import TYPE_CHECKING, List, Optional, Sequence, Tuple, Union

import numpy as np

from .audio import FRAMES_PER_SECOND, HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE, ingest_source
from .backend_hip import DeviceAudio
from .tokenizer import Tokenizer, get_tokenizer

if TYPE_CHECKING:
    from .model import Whisper


def _is_clip(v) -> bool:
    return isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, (int, float)) for x in v)


def _per_file(value, n: int, name: str, single) -> list:
    if value is None or single(value):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} values for {n} files")
    return value


def candidate_tokens(tokenizer: Tokenizer, candidate) -> List[int]:
    """A candidate's text tokens."""
    if isinstance(candidate, str):
        return list(tokenizer.encode(" " + candidate.strip())) if candidate.strip() else []
    return [int(t) for t in candidate]


def context_tokens(tokenizer: Tokenizer, initial_prompt: Optional[str], n_text_ctx: int) -> List[int]:
    """What stands before the scored tokens: the prompt as a decode would carry it (its last
    ``n_text_ctx // 2 - 1`` tokens behind <|startofprev|>), the SOT sequence, <|notimestamps|>."""
    ids: List[int] = []
    if initial_prompt is not None and initial_prompt.strip():
        prompt = tokenizer.encode(" " + initial_prompt.strip())
        ids = [tokenizer.sot_prev, *prompt[-(n_text_ctx // 2 - 1):]]
    return [*ids, *tokenizer.sot_sequence, tokenizer.no_timestamps]


def summarize(tokenizer: Tokenizer, candidate, tokens: Sequence[int], logprob, top_id, top_logprob) -> dict:
    """One candidate's result from the per-position values of its text tokens and its eot."""
    lp = [float(x) for x in logprob]
    total = 0.0
    for x in lp:  # fp64, in order
        total += x
    return dict(text=candidate if isinstance(candidate, str) else tokenizer.decode(list(tokens)), tokens=list(tokens),
                token_logprobs=lp[:-1], eot_logprob=lp[-1], sum_logprob=total, avg_logprob=total / len(lp),
                top_tokens=[int(t) for t in top_id], top_logprobs=[float(x) for x in top_logprob])


def best_index(candidates: Sequence[dict]) -> int:
    """The highest ``avg_logprob``, the lowest index on a tie."""
    best = 0
    for k, c in enumerate(candidates):
        if c["avg_logprob"] > candidates[best]["avg_logprob"]:
            best = k
    return best


def _window(i: int, length: int, clip) -> Tuple[int, int]:
    """(seek, frames) of file i's window; refuses what does not fit 30 s."""
    if clip is None:
        if length > N_SAMPLES:
            raise ValueError(f"audio {i} is {length / SAMPLE_RATE:.2f} s long: score() takes at most 30 s, "
                             f"or clip=(t0, t1) of a longer recording")
        return 0, max(1, length // HOP_LENGTH)
    if not _is_clip(clip):
        raise ValueError(f"audio {i}: clip is (t0, t1) in seconds, not {clip!r}")
    seek, end = int(round(clip[0] * FRAMES_PER_SECOND)), int(round(clip[1] * FRAMES_PER_SECOND))
    end = min(end, length // HOP_LENGTH)
    if seek < 0 or end <= seek:
        raise ValueError(f"audio {i}: clip {clip!r} is empty or outside the recording")
    if end - seek > N_FRAMES:
        raise ValueError(f"audio {i}: clip {clip!r} is longer than 30 s")
    return seek, end - seek


def score_batch(model: "Whisper", audios: Sequence[Union[str, np.ndarray]], candidates: Sequence[Sequence], *,
                language: Union[None, str, Sequence[Optional[str]]] = None,
                initial_prompt: Union[None, str, Sequence[Optional[str]]] = None, clip=None,
                mel_budget_frames: Optional[int] = None, max_windows: Optional[int] = None,
                verbose: Optional[bool] = None) -> List[dict]:
    """``[score(model, a, c) for a, c in zip(audios, candidates)]`` with up to ``max_windows``
    recordings per encode and all their candidates scored together.  ``result[i]`` has the
    fields of ``score(model, audios[i], candidates[i])``; the numbers agree to the tolerance of
    batched against single first passes, not bit for bit (the first-pass GEMMs are selected by
    row count).

    ``audios``: paths and/or 1-D 16 kHz arrays, each at most 30 s long unless ``clip`` (one
    ``(t0, t1)`` in seconds for all files, or one per file) selects at most 30 s of it.
    ``candidates[i]``: the texts (strings or token id lists) to score on file i.  ``language``:
    None (detected from the file's first window on a multilingual model, as ``transcribe``
    does), one code, or one per file.  ``initial_prompt``: None, one prompt, or one per file.

    The result per file: ``language``, ``best`` (the index of the highest ``avg_logprob``, the
    lowest on a tie) and ``candidates``, one dict each: ``text``, ``tokens``,
    ``token_logprobs``, ``eot_logprob``, ``sum_logprob`` (their fp64 sum in order),
    ``avg_logprob`` (``sum_logprob / (len(tokens) + 1)``), and the model's own first choice
    at every scored position, ``top_tokens`` / ``top_logprobs``."""
    if isinstance(audios, (str, np.ndarray, DeviceAudio)):
        raise TypeError("score_batch: audios and candidates are sequences with one entry per file")
    audios, candidates = list(audios), [list(c) if not isinstance(c, str) else [c] for c in candidates]
    n = len(audios)
    if len(candidates) != n:
        raise ValueError(f"candidates: {len(candidates)} values for {n} files")
    for i, c in enumerate(candidates):
        if not c:
            raise ValueError(f"audio {i} has no candidates")
    languages = _per_file(language, n, "language", lambda v: isinstance(v, str))
    prompts = _per_file(initial_prompt, n, "initial_prompt", lambda v: isinstance(v, str))
    clips = _per_file(clip, n, "clip", _is_clip)
    if not model.is_multilingual:
        languages = [x or "en" for x in languages]
    n_text_ctx = model.dims.n_text_ctx
    ctx = model.ctx
    if max_windows is None:
        max_windows = ctx.max_windows
    if not 1 <= max_windows <= ctx.max_windows:
        raise ValueError(f"max_windows must be 1..{ctx.max_windows}")

    def tokenizer_of(lang) -> Tokenizer:
        return get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=lang, task="transcribe")

    # sources, lengths and windows; every refusal comes before any device work (a sequence's
    # length does not depend on the language: every SOT sequence is equally long)
    sources: List[Optional[tuple]] = []
    lengths: List[int] = []
    for i, a in enumerate(audios):
        if isinstance(a, DeviceAudio):
            raise TypeError(f"audio {i}: DeviceAudio is one file resident in the context; score() takes it")
        if isinstance(a, str):
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
    windows = []
    for i, length in enumerate(lengths):
        if length < 1:
            raise ValueError(f"audio {i} is empty")
        windows.append(_window(i, length, clips[i]))
    for i in range(n):
        _sequences(tokenizer_of(languages[i]), candidates[i], prompts[i], n_text_ctx, i)

    from .align import _detect_languages
    from .multifile import DEFAULT_MEL_BUDGET_FRAMES, file_frames, ingest_group, split_groups
    budget = DEFAULT_MEL_BUDGET_FRAMES if mel_budget_frames is None else int(mel_budget_frames)
    if budget < 1:
        raise ValueError("mel_budget_frames must be positive")
    frames = [file_frames(x) for x in lengths]
    results: List[Optional[dict]] = [None] * n
    for group in split_groups(frames, budget):
        ingest_group(ctx, group, sources, lengths)
        bases = ctx.log_mel_batch_resident([lengths[i] for i in group], model.dims.n_mels, padding=N_SAMPLES)
        _detect_languages(model, group, bases, languages, verbose)
        for c0 in range(0, len(group), max_windows):
            chunk = list(range(c0, min(c0 + max_windows, len(group))))
            _score_round(model, [group[k] for k in chunk], [int(bases[k]) for k in chunk], windows, candidates,
                         prompts, languages, tokenizer_of, results)
    return results


def _sequences(tokenizer: Tokenizer, cands: Sequence, prompt: Optional[str], n_text_ctx: int, file: int):
    """(context length, [text tokens], [whole sequences]) of one file's candidates."""
    head = context_tokens(tokenizer, prompt, n_text_ctx)
    texts = [candidate_tokens(tokenizer, c) for c in cands]
    for k, t in enumerate(texts):
        if len(head) + len(t) + 1 > n_text_ctx:
            raise ValueError(f"candidate {k} of audio {file}: {len(head)} context tokens + {len(t)} text tokens + "
                             f"<|endoftext|> exceed the {n_text_ctx} text positions")
    return len(head), texts, [[*head, *t, tokenizer.eot] for t in texts]


def _score_round(model, files, bases, windows, candidates, prompts, languages, tokenizer_of, results) -> None:
    """One encode of the windows of ``files`` (slot k holds files[k]) and one ``wh_score_batch``
    of all their candidates."""
    ctx = model.ctx
    seeks = [b + windows[i][0] for i, b in zip(files, bases)]
    sizes = [windows[i][1] for i in files]
    ctx.encode(seeks, sizes)
    model._last_windows = (seeks, sizes)
    slots, seqs, n_ctx = [], [], []
    per_file = []
    for slot, i in enumerate(files):
        tok = tokenizer_of(languages[i])
        n_head, texts, whole = _sequences(tok, candidates[i], prompts[i], model.dims.n_text_ctx, i)
        per_file.append((tok, texts))
        slots += [slot] * len(whole)
        seqs += whole
        n_ctx += [n_head] * len(whole)
    answers = ctx.score_batch(slots, seqs, n_ctx)
    at = 0
    for i, (tok, texts) in zip(files, per_file):
        out = [summarize(tok, c, t, *answers[at + k]) for k, (c, t) in enumerate(zip(candidates[i], texts))]
        at += len(texts)
        results[i] = dict(language=languages[i], best=best_index(out), candidates=out)


def score(model: "Whisper", audio, candidates: Sequence, *, language: Optional[str] = None,
          initial_prompt: Optional[str] = None, clip: Optional[Tuple[float, float]] = None, **options) -> dict:
    """Log-probabilities of ``candidates`` (texts or token id lists) given ``audio``: a path, a
    1-D 16 kHz array or a ``DeviceAudio``, at most 30 s long unless ``clip=(t0, t1)`` selects at
    most 30 s of it (``score_batch`` for the result's fields and the other keywords)."""
    if language is not None and not isinstance(language, str):
        raise TypeError("score: language is one code or None")
    if isinstance(candidates, str):
        candidates = [candidates]
    if isinstance(audio, DeviceAudio):
        if audio.ctx is not model.ctx:
            raise ValueError("DeviceAudio belongs to another model context")
        if audio.offset:
            raise ValueError("DeviceAudio is a segment behind other files: score() takes the only resident one")
        audio = model.ctx.audio_read(0, audio.n_samples)
    return score_batch(model, [audio], [candidates], language=language, initial_prompt=initial_prompt, clip=clip,
                       **options)[0]
