"""Forced alignment: word times for a transcript the caller already has.

``align(model, audio, text)`` says when each word of ``text`` was spoken in ``audio``;
``align_batch`` does it for many files at once, one lane per file.  The device work is
``wh_align_batch_open`` (include/whisper_hip.h): the teacher-forced first pass with the
alignment heads' cross-QK, the softmax / z-norm / median / head-mean matrix, the token
probabilities and an open-end DTW, one workgroup per window.  A closed DTW forces all the
tokens it is given onto all the frames of one 30 s window; the open end lets the kernel
say how many of the offered tokens this window's audio accounts for, which is what takes
the alignment past one window.

The text
    ``text`` is a string (split at newlines) or a list of lines.  A line is a string,
    encoded as ``" " + line.strip()``, or a list of token ids.  Empty lines are dropped;
    every id must be below ``eot``.  Words come from ``tokenizer.split_to_word_tokens`` per
    line, so no word spans two lines, and each line becomes one segment.

The policy (per file; what tests/test_forced_align_host.py pins)
    There is a cursor ``seek`` (in frames) and a cursor ``w`` (the next word).  For the
    window ``[seek, seek + seg)`` with ``seg = min(3000, content - seek)``:

    1. Candidate: the longest run of whole words from ``w`` whose token count is at most
       ``min(max_tokens, n_text_ctx // 2 - n_sot - 2)`` (the default ``max_tokens`` is that
       bound).  A single word longer than the bound is a ``ValueError`` before any window.
    2. Closed or open: the candidate is ``full`` if it reaches the last word, the window is
       ``last`` if it reaches the end of the audio.  The window is closed (``min_rows = 0``)
       iff ``full and last``; otherwise it is open with ``min_rows = 1``.
    3. Covered words: with the end row ``e``, ``k`` is the number of candidate words that
       lie wholly in rows ``< e``.  Word times are the path's jump times, computed by
       ``timing._words_from_path`` itself; in an open window a word whose last token is the
       path's last row ends at ``seg / 100``.
    4. Accept.  Closed: all ``k``, and the file is done.  Open and ``last``: all ``k``; the
       words left over go to ``result["unaligned"]`` with ``start = end =`` the audio's end
       and probability NaN.  Open with ``k >= 2``: the first ``k - 1`` (the last covered word
       always runs into the window's edge, so the next window aligns it again) and
       ``seek += round(100 * end of the last accepted word)``, the end as the path gives it,
       before step 6.  Open with ``k <= 1``: the ``k`` words and ``seek += seg``.
    5. Every round advances ``w`` or ``seek``, so the loop terminates.  It also ends, with
       the remaining words unaligned, when fewer than 2 frames of audio are left (a window
       needs one DTW column of two frames).
    6. Per window and line, timing.py's duration clipping (``_duration_limits``,
       ``_clip_at_sentence_marks``) and ``merge_punctuations`` run on the accepted words.

``row_penalty`` (default 4.0) is the open-end DTW's price per row: a token must own
evidence worth about two frames at 2 sigma.  Without a penalty the end overshoots (a row
beyond the spoken text can always be entered through one frame whose z-score happens to
be positive).  The value comes from planted z-normalised matrices; like the hotword boost
and the streaming defaults it has NOT been measured on real speech with this project.
"""

import math
from typing import TYPE_CHECKING, Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from .audio import FRAMES_PER_SECOND, HOP_LENGTH, N_FRAMES, N_SAMPLES, SAMPLE_RATE, ingest_source
from .timing import (WordTiming, _alignment_head_ids, _clip_at_sentence_marks, _duration_limits, _words_from_path,
                     merge_punctuations)
from .tokenizer import LANGUAGES, Tokenizer, get_tokenizer

if TYPE_CHECKING:
    from .model import Whisper

DEFAULT_ROW_PENALTY = 4.0
_PREPEND = "\"'“¿([{-"
_APPEND = "\"'.。,，!！?？:：”)]}、"


class AlignWindow(NamedTuple):
    """One window offered to an align round: file ``file`` (its frames start at ``base`` of the
    context mel), frames ``[seek, seek + seg)`` of it, the candidate ``tokens`` (the file's text
    tokens from index ``first_token``) and ``min_rows`` (0: closed)."""
    file: int
    base: int
    seek: int
    seg: int
    first_token: int
    tokens: List[int]
    min_rows: int


# what an align round answers per window: (token probabilities [T], text indices, time
# indices, end row), as ``HipContext.align_batch_open`` returns them
AlignAnswer = Tuple[np.ndarray, np.ndarray, np.ndarray, int]
AlignRound = Callable[[List[AlignWindow]], List[AlignAnswer]]


class _Word(NamedTuple):
    word: str
    tokens: List[int]
    line: int


class _Presplit:
    """What ``timing._words_from_path`` asks of a tokenizer, answering with the words this
    module already split per line (its own split of the joined tokens could join a word
    across two lines)."""

    def __init__(self, words: Sequence[_Word], eot: int):
        self.words, self.eot = words, eot

    def split_to_word_tokens(self, tokens):
        return [w.word for w in self.words] + [""], [list(w.tokens) for w in self.words] + [[self.eot]]


def token_bound(n_text_ctx: int, n_sot: int, max_tokens: Optional[int] = None) -> int:
    """The most text tokens one window is offered."""
    bound = n_text_ctx // 2 - n_sot - 2
    if max_tokens is not None:
        if int(max_tokens) < 1:
            raise ValueError("max_tokens must be at least 1")
        bound = min(bound, int(max_tokens))
    return bound


def split_lines(text) -> list:
    """``text`` -> its non-empty lines (strings stripped, token lists as lists of ints)."""
    if isinstance(text, str):
        text = text.split("\n")
    lines = []
    for line in text:
        if isinstance(line, str):
            if line.strip():
                lines.append(line.strip())
        else:
            ids = [int(t) for t in line]
            if ids:
                lines.append(ids)
    if not lines:
        raise ValueError("align: the text is empty")
    return lines


def text_words(tokenizer: Tokenizer, lines: Sequence, bound: int) -> Tuple[List[_Word], List[List[int]]]:
    """(words, tokens per line) of ``split_lines``'s lines."""
    words: List[_Word] = []
    line_tokens: List[List[int]] = []
    for k, line in enumerate(lines):
        ids = tokenizer.encode(" " + line) if isinstance(line, str) else list(line)
        bad = [t for t in ids if t < 0 or t >= tokenizer.eot]
        if bad:
            raise ValueError(f"align: line {k} holds token {bad[0]}, which is no text token (eot is {tokenizer.eot})")
        line_tokens.append(ids)
        for word, toks in zip(*tokenizer.split_to_word_tokens(ids)):
            if len(toks) > bound:
                raise ValueError(f"align: the word {word!r} of line {k} has {len(toks)} tokens; a window is "
                                 f"offered at most {bound}")
            words.append(_Word(word, list(toks), k))
    return words, line_tokens


def check_text(tokenizer: Tokenizer, lines: Sequence, bound: int) -> None:
    """What can be refused of a text whose language is not known yet: an id that is no text
    token (eot and the BPE are the same for every language) and a UTF-8-complete piece longer
    than ``bound``.  Pieces are what the languages written without spaces take as words and
    what every other language joins into words, so such a piece is an over-long word in any
    language; a word that is over-long only as the detected language splits it is refused by
    ``text_words`` once the language is known."""
    for k, line in enumerate(lines):
        ids = tokenizer.encode(" " + line) if isinstance(line, str) else list(line)
        bad = [t for t in ids if t < 0 or t >= tokenizer.eot]
        if bad:
            raise ValueError(f"align: line {k} holds token {bad[0]}, which is no text token (eot is {tokenizer.eot})")
        for piece, toks in zip(*tokenizer.split_tokens_on_unicode(ids)):
            if len(toks) > bound:
                raise ValueError(f"align: the word {piece!r} of line {k} has {len(toks)} tokens; a window is "
                                 f"offered at most {bound}")


class _AlignLane:
    """The policy's state for one file (module docstring)."""

    def __init__(self, file: int, words: Sequence[_Word], content_frames: int, bound: int, eot: int, *,
                 base: int = 0, prepend: str = _PREPEND, append: str = _APPEND):
        self.file, self.words, self.content, self.bound, self.eot = file, list(words), int(content_frames), bound, eot
        self.base, self.prepend, self.append = base, prepend, append
        self.token_start = np.concatenate(([0], np.cumsum([len(w.tokens) for w in self.words]))).astype(int)
        self.seek = 0
        self.w = 0
        self.done = False
        self.windows: List[Tuple[int, int, int, int, int]] = []
        self.aligned: List[Tuple[WordTiming, int]] = []  # (word with absolute times, line)
        self.offer: Optional[Tuple[int, int, bool]] = None  # (seg, words offered, closed)

    def next_window(self) -> Optional[AlignWindow]:
        if self.done or self.w >= len(self.words) or self.content - self.seek < 2:
            self.done = True
            return None
        seg = min(N_FRAMES, self.content - self.seek)
        n, count = 0, 0
        while self.w + n < len(self.words) and count + len(self.words[self.w + n].tokens) <= self.bound:
            count += len(self.words[self.w + n].tokens)
            n += 1
        full = self.w + n == len(self.words)
        last = self.seek + seg >= self.content
        closed = full and last
        self.offer = (seg, n, closed)
        t0 = int(self.token_start[self.w])
        tokens = [t for w in self.words[self.w:self.w + n] for t in w.tokens]
        return AlignWindow(self.file, self.base, self.seek, seg, t0, tokens, 0 if closed else 1)

    def apply(self, answer: AlignAnswer) -> None:
        seg, n, closed = self.offer
        probs, text_indices, time_indices, end_row = answer
        cand = self.words[self.w:self.w + n]
        ends = np.cumsum([len(w.tokens) for w in cand])
        n_tokens = int(ends[-1])
        e = int(end_row)
        if not 1 <= e <= n_tokens + 1 or (closed and e != n_tokens + 1):
            raise RuntimeError(f"align: end row {e} for {n_tokens} text tokens ({'closed' if closed else 'open'})")
        k = int(np.searchsorted(ends, e, side="right"))  # words wholly in rows < e
        last = self.seek + seg >= self.content
        timings: List[WordTiming] = []
        if k > 0:
            covered = int(ends[k - 1])
            text_indices, time_indices = np.asarray(text_indices), np.asarray(time_indices)
            if covered == e:
                # the last covered word's last token is the path's last row: it ends at the window's edge
                text_indices = np.append(text_indices, e)
                time_indices = np.append(time_indices, seg // 2)
            timings = _words_from_path(_Presplit(cand[:k], self.eot), [t for w in cand[:k] for t in w.tokens],
                                       np.asarray(probs)[:covered], text_indices, time_indices)
        if closed or last:
            accept = k
        elif k >= 2:
            accept = k - 1
        else:
            accept = k
        timings = timings[:accept]
        self.windows.append((self.seek, seg, n_tokens, e, accept))
        advance = seg
        if not (closed or last) and k >= 2:
            advance = int(round(FRAMES_PER_SECOND * timings[-1].end))
        self._accept(timings, [w.line for w in cand[:accept]], self.seek * HOP_LENGTH / SAMPLE_RATE)
        self.w += accept
        self.seek += advance
        if closed or last:
            self.done = True

    def _accept(self, timings: List[WordTiming], lines: List[int], t0: float) -> None:
        for line in sorted(set(lines)):
            group = [t for t, li in zip(timings, lines) if li == line]
            _, max_d, any_duration = _duration_limits(group)
            if any_duration:
                _clip_at_sentence_marks(group, max_d)
            merge_punctuations(group, self.prepend, self.append)
            for t in group:
                if t.word:
                    t.start, t.end = round(t0 + t.start, 2), round(t0 + t.end, 2)
                    self.aligned.append((t, line))

    def result(self, tokenizer: Tokenizer, line_tokens: List[List[int]], language: Optional[str]) -> dict:
        end = round(self.content * HOP_LENGTH / SAMPLE_RATE, 2)
        segments = []
        for k, ids in enumerate(line_tokens):
            words = [dict(word=t.word, tokens=list(t.tokens), start=t.start, end=t.end, probability=t.probability)
                     for t, line in self.aligned if line == k]
            segments.append(dict(id=k, line=k, start=words[0]["start"] if words else end,
                                 end=words[-1]["end"] if words else end, text=tokenizer.decode(ids), tokens=list(ids),
                                 words=words))
        unaligned = [dict(word=w.word, tokens=list(w.tokens), line=w.line, start=end, end=end, probability=math.nan)
                     for w in self.words[self.w:]]
        return dict(text="\n".join(s["text"].strip() for s in segments), language=language, segments=segments,
                    unaligned=unaligned, windows=list(self.windows))


def run_align_lanes(lanes: Sequence[_AlignLane], max_windows: int, align_round: AlignRound) -> None:
    """Rounds over ``lanes`` in the given order: every live lane offers its next window,
    ``align_round`` answers them together (window i in slot i), each lane applies its own.
    At most ``max_windows`` lanes are live; one that ends frees its place for the next."""
    if max_windows < 1:
        raise ValueError("max_windows must be at least 1")
    pending = list(lanes)
    live: List[_AlignLane] = []
    while True:
        windows: List[AlignWindow] = []
        still: List[_AlignLane] = []
        for lane in live:
            w = lane.next_window()
            if w is not None:
                still.append(lane)
                windows.append(w)
        while len(still) < max_windows and pending:
            lane = pending.pop(0)
            w = lane.next_window()
            if w is not None:
                still.append(lane)
                windows.append(w)
        live = still
        if not windows:
            return
        answers = list(align_round(windows))
        if len(answers) != len(windows):
            raise RuntimeError("align_round returned %d answers for %d windows" % (len(answers), len(windows)))
        for lane, answer in zip(live, answers):
            lane.apply(answer)


def _device_align_round(model: "Whisper", tokenizers: dict, row_penalty: float, medfilt_width: int) -> AlignRound:
    """The round on the model's context: one encode and one ``wh_align_batch_open``."""
    ctx = model.ctx
    heads = _alignment_head_ids(model)

    def align_round(windows: List[AlignWindow]) -> List[AlignAnswer]:
        seeks = [w.base + w.seek for w in windows]
        sizes = [w.seg for w in windows]
        ctx.encode(seeks, sizes)
        model._last_windows = (seeks, sizes)
        toks = [tokenizers[w.file] for w in windows]
        n_sot = len(toks[0].sot_sequence)
        seqs = [[*t.sot_sequence, t.no_timestamps, *w.tokens, t.eot] for t, w in zip(toks, windows)]
        return ctx.align_batch_open(list(range(len(windows))), seqs, n_sot, sizes, heads,
                                    [w.min_rows for w in windows], row_penalty, medfilt_width)

    return align_round


def _refuse_options(options: dict, who: str) -> None:
    for name in ("skip_silence", "clip_timestamps", "channels"):
        if name in options:
            raise ValueError(f"{who}() does not take {name}: it aligns the whole mixed-down file")
    if options:
        raise TypeError(f"{who}() got an unexpected keyword argument {sorted(options)[0]!r}")


def _per_file(value, n: int, name: str) -> list:
    if value is None or isinstance(value, str):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} values for {n} files")
    return value


def align_batch(model: Optional["Whisper"], audios: Sequence[Union[str, np.ndarray]], texts: Sequence, *,
                language: Union[None, str, Sequence[Optional[str]]] = None, max_tokens: Optional[int] = None,
                row_penalty: float = DEFAULT_ROW_PENALTY, medfilt_width: int = 7,
                prepend_punctuations: str = _PREPEND, append_punctuations: str = _APPEND,
                mel_budget_frames: Optional[int] = None, max_windows: Optional[int] = None,
                verbose: Optional[bool] = None, align_round_fn: Optional[AlignRound] = None, **options) -> List[dict]:
    """``[align(model, a, t) for a, t in zip(audios, texts)]`` with the files aligned together,
    one lane per file: every round encodes the next window of all live lanes with one
    ``ctx.encode`` and aligns them with one ``wh_align_batch_open``; at most
    ``ctx.max_windows`` lanes are live.  ``result[i]`` has the words, tokens and times of
    ``align(model, audios[i], texts[i])``; probabilities agree to the tolerance of batched
    against single first passes (rtol 1e-5 per token, tests/test_gpu_words.py).

    ``audios``: paths and/or 1-D 16 kHz arrays.  ``texts``: one text per file (module
    docstring).  ``language``: None (detected from the file's first window on a multilingual
    model, as ``transcribe`` does), one code, or one per file.  ``row_penalty``: the open-end
    DTW's price per row; the default 4.0 has not been measured on real speech.
    ``skip_silence``, ``clip_timestamps`` and ``channels`` are refused.

    ``align_round_fn(windows)`` replaces the device round (tests drive the policy without a
    GPU): it gets the ``AlignWindow`` list of a round and answers (probabilities, text
    indices, time indices, end row) per window.  With it nothing touches a device: ``model``
    may be None (a multilingual tokenizer, 448 text positions, ``max_windows`` default 8), an
    audio may also be its number of 16 kHz samples, and a language that is None is "en".

    The result per file: ``text``, ``language``, ``segments`` (one per non-empty line: ``id``,
    ``line``, ``start``, ``end``, ``text``, ``tokens``, ``words`` of ``word``, ``tokens``,
    ``start``, ``end``, ``probability``), ``unaligned`` (the words the audio did not account
    for) and ``windows``, a list of (seek, seg, candidate tokens, end row, words accepted)."""
    _refuse_options(options, "align_batch")
    if isinstance(audios, (str, np.ndarray)) or isinstance(texts, str):
        raise TypeError("align_batch: audios and texts are sequences with one entry per file")
    audios, texts = list(audios), list(texts)
    n = len(audios)
    if len(texts) != n:
        raise ValueError(f"texts: {len(texts)} values for {n} files")
    row_penalty = float(row_penalty)
    if not (row_penalty >= 0 and math.isfinite(row_penalty)):
        raise ValueError("row_penalty must be finite and >= 0")
    languages = _per_file(language, n, "language")
    stub = align_round_fn is not None
    multilingual = True if model is None else model.is_multilingual
    num_languages = 99 if model is None else model.num_languages
    n_text_ctx = 448 if model is None else model.dims.n_text_ctx
    if max_windows is None:
        max_windows = 8 if model is None else model.ctx.max_windows
    if stub or not multilingual:
        languages = [x or "en" for x in languages]

    def tokenizer_of(lang) -> Tokenizer:
        return get_tokenizer(multilingual, num_languages=num_languages, language=lang, task="transcribe")

    lines = [split_lines(t) for t in texts]
    plans: dict = {}  # file -> (tokenizer, words, line tokens)

    def plan(i: int):
        if i not in plans:
            tok = tokenizer_of(languages[i])
            bound = token_bound(n_text_ctx, len(tok.sot_sequence), max_tokens)
            plans[i] = (tok, *text_words(tok, lines[i], bound), bound)
        return plans[i]

    for i in range(n):  # what can be refused is, before any device work
        if languages[i] is not None:
            plan(i)
        else:  # the rest of a text's refusals needs its language (plan(i) after the detection)
            probe = tokenizer_of(None)
            check_text(probe, lines[i], token_bound(n_text_ctx, len(probe.sot_sequence), max_tokens))

    # sources and lengths (as transcribe_batch takes them, mixed down)
    sources: List[Optional[tuple]] = []
    lengths: List[int] = []
    for i, a in enumerate(audios):
        if stub and isinstance(a, (int, np.integer)):
            sources.append(None)
            lengths.append(int(a))
            continue
        if isinstance(a, str) and not stub:
            a, length = ingest_source(a, need_length=True)
            if isinstance(a, tuple):
                sources.append(a)
                lengths.append(length)
                continue
        if isinstance(a, str):
            raise TypeError(f"audio {i}: with align_round_fn an audio is an array or a sample count")
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"audio {i} is not 1-D (shape {a.shape})")
        sources.append((a, SAMPLE_RATE, 32))
        lengths.append(a.shape[0])
    for i, length in enumerate(lengths):
        if length < 1:
            raise ValueError(f"audio {i} is empty")

    from .multifile import DEFAULT_MEL_BUDGET_FRAMES, file_frames, ingest_group, split_groups
    budget = DEFAULT_MEL_BUDGET_FRAMES if mel_budget_frames is None else int(mel_budget_frames)
    if budget < 1:
        raise ValueError("mel_budget_frames must be positive")
    frames = [file_frames(x) for x in lengths]
    lanes: List[Optional[_AlignLane]] = [None] * n
    tokenizers: dict = {}
    align_round = align_round_fn if stub else _device_align_round(model, tokenizers, row_penalty, medfilt_width)
    for group in split_groups(frames, budget):
        if stub:
            bases = np.concatenate(([0], np.cumsum([frames[i] for i in group])))
        else:
            ctx = model.ctx
            ingest_group(ctx, group, sources, lengths)
            bases = ctx.log_mel_batch_resident([lengths[i] for i in group], model.dims.n_mels, padding=N_SAMPLES)
            _detect_languages(model, group, bases, languages, verbose)
        for k, i in enumerate(group):
            tok, words, _, bound = plan(i)
            tokenizers[i] = tok
            lanes[i] = _AlignLane(i, words, int(bases[k + 1] - bases[k]) - N_FRAMES, bound, tok.eot, base=int(bases[k]),
                                  prepend=prepend_punctuations, append=append_punctuations)
        order = sorted(range(len(group)), key=lambda k: -frames[group[k]])  # longest first; ties keep input order
        run_align_lanes([lanes[group[k]] for k in order], max_windows, align_round)
    results = []
    for i, lane in enumerate(lanes):
        tok, _, line_tokens, _ = plans[i]
        results.append(lane.result(tok, line_tokens, languages[i]))
        if verbose:
            for s in results[-1]["segments"]:
                print(f"[{i}] [{s['start']:.2f} --> {s['end']:.2f}] {s['text']}")
    return results


def _detect_languages(model: "Whisper", group: List[int], bases, languages: list, verbose) -> None:
    """The language of every file of the group that has none, from its first window: up to
    ``max_windows`` files per encode, one <|startoftranscript|> pass per slot."""
    todo = [k for k, i in enumerate(group) if languages[i] is None]
    if not todo:
        return
    from .decoding import language_probs
    ctx = model.ctx
    probe = get_tokenizer(model.is_multilingual, num_languages=model.num_languages)
    for c0 in range(0, len(todo), ctx.max_windows):
        chunk = todo[c0:c0 + ctx.max_windows]
        seeks = [int(bases[k]) for k in chunk]
        sizes = [min(N_FRAMES, int(bases[k + 1] - bases[k])) for k in chunk]
        ctx.encode(seeks, sizes)
        model._last_windows = (seeks, sizes)
        for slot, k in enumerate(chunk):
            _, probs = language_probs(model, slot, probe)
            languages[group[k]] = max(probs, key=probs.get)
            if verbose is not None:
                print(f"[{group[k]}] Detected language: {LANGUAGES[languages[group[k]]].title()}")


def align(model: Optional["Whisper"], audio: Union[str, np.ndarray], text, *, language: Optional[str] = None,
          **options) -> dict:
    """Word times for ``text`` spoken in ``audio``: ``align_batch`` of this one file (its
    keywords, its result dict; module docstring for the text and the policy)."""
    _refuse_options({k: v for k, v in options.items() if k in ("skip_silence", "clip_timestamps", "channels")}, "align")
    if language is not None and not isinstance(language, str):
        raise TypeError("align: language is one code or None")
    return align_batch(model, [audio], [text], language=language, **options)[0]


def dtw_open(model: "Whisper", x: np.ndarray, min_rows: int = 1, row_penalty: float = DEFAULT_ROW_PENALTY):
    """The open-end DTW of cost matrix ``x [N][M]`` on the GPU (``wh_dtw_open``,
    include/whisper_hip.h): (path [2][length], end row, scores [N]).  ``min_rows = 0`` is the
    closed ``timing.dtw``."""
    return model.ctx.dtw_open(np.asarray(x, dtype=np.float32), min_rows, row_penalty)
