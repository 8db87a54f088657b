"""The clip-grid schedule (whisper/transcribe.py _run_batched) without a GPU: the real
_Lane, _run_batched and _decode_with_fallback over a scripted device.  ``ctx.encode``,
``run_windows`` and ``find_alignment_batch`` are stand-ins that record what they are
handed and answer from a script keyed by the window's first frame.  What is pinned is
what the schedule decides and the output depends on: which windows share an encode and
in which slot, which window sees the initial prompt, how T > 0 retries are called and
seeded, and what the ordered word pass emits or refuses."""
import itertools
from types import SimpleNamespace

K_SEED = 0x9E3779B97F4A7C15
WORD = 1000  # any text token


class _Rig:
    """clips: (start s, end s) each.  ``decode(seek, size, temperature)`` gives
    (tokens, avg_logprob, no_speech_prob) with timestamps written as ("t", seconds);
    default <|0.00|> X <|size|>, which advances the clip by the whole window.
    ``align(seek)`` gives the window's words as (start, end) in window time, one per
    text token; default 0.00-0.50 each."""

    def __init__(self, monkeypatch, clips, max_windows, *, temperature=0.0, word_timestamps=False,
                 initial_prompt=None, decode=None, align=None):
        import importlib
        T = importlib.import_module("whisper.transcribe")  # whisper.transcribe is the function
        from whisper.tokenizer import get_tokenizer
        self.T = T
        self.tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
        self.encodes, self.calls, self.aligned, self.drawn = [], [], [], []
        self.decode, self.align = decode, align
        ctx = SimpleNamespace(max_windows=max_windows, encode=self._encode)
        self.model = SimpleNamespace(is_multilingual=True, num_languages=99, ctx=ctx,
                                     dims=SimpleNamespace(n_audio_ctx=1500, n_text_ctx=448))
        content_frames = round(max(e for _, e in clips) * 100)
        _, self.clips, self.prompt, self.st = T._plan_file(
            self.model, content_frames, "en", dict(language="en"), temperature=temperature,
            thresholds=(2.4, -1.0, 0.6), initial_prompt=initial_prompt, word_timestamps=word_timestamps,
            prepend_punctuations="\"'“¿([{-", append_punctuations="\"'.。,，!！?？:：”)]}、",
            clip_timestamps=[t for c in clips for t in c], hallucination_silence_threshold=None)
        monkeypatch.setattr(T, "run_windows", self._run_windows)
        monkeypatch.setattr(T, "find_alignment_batch", self._find_alignment_batch)

    def _encode(self, seeks, sizes):
        self.encodes.append((list(seeks), list(sizes)))

    def _run_windows(self, model, options, prompts, slots=None, **extra):
        from whisper.decoding import DecodingResult, next_seed
        assert model._last_windows == self.encodes[-1]
        self.calls.append(dict(temperature=options.temperature, prompts=list(prompts),
                               slots=None if slots is None else list(slots), extra=sorted(extra)))
        if options.temperature > 0 and extra.get("seed") is None:
            self.drawn.append(next_seed())  # as DecodingTask.wh_opts does
        seeks, sizes = self.encodes[-1]
        tb = self.tok.timestamp_begin
        out = []
        for slot in (range(len(prompts)) if slots is None else slots):
            seek, size = seeks[slot], sizes[slot]
            tokens, avg_logprob, no_speech = [("t", 0.0), WORD, ("t", size / 100)], -0.1, 0.0
            if self.decode is not None:
                tokens, avg_logprob, no_speech = self.decode(seek, size, options.temperature)
            tokens = [tb + round(t[1] * 50) if isinstance(t, tuple) else t for t in tokens]
            out.append(DecodingResult(audio_features=None, language="en", tokens=tokens, text="x",
                                      avg_logprob=avg_logprob, no_speech_prob=no_speech,
                                      temperature=options.temperature, compression_ratio=1.0))
        return out

    def _find_alignment_batch(self, model, tokenizer, text_tokens, num_frames, slots, **kw):
        from whisper.timing import WordTiming
        seeks, sizes = self.encodes[-1]
        out = []
        for text, frames, slot in zip(text_tokens, num_frames, slots):
            assert frames == sizes[slot]
            if not text:
                out.append([])
                continue
            self.aligned.append(seeks[slot])
            spans = self.align(seeks[slot]) if self.align is not None else [(0.0, 0.5)] * len(text)
            assert len(spans) == len(text)
            out.append([WordTiming(" w%d" % k, [t], s, e, 0.9) for k, (t, (s, e)) in enumerate(zip(text, spans))])
        return out

    def run(self):
        return self.T._run_batched(self.model, self.clips, self.prompt, self.st)


def _grid(n, seconds, pitch=30):
    return [(pitch * i, pitch * i + seconds) for i in range(n)]


def _short_then_rest(short_clips):
    """Clips in `short_clips` advance by the whole 25 s window; the others' first window
    ends <|0.00|> X <|10.00|><|10.00|>, which advances 10 s and leaves a second window."""
    def decode(seek, size, temperature):
        if seek % 3000 == 0 and seek // 3000 not in short_clips:
            return [("t", 0.0), WORD, ("t", 10.0), ("t", 10.0)], -0.1, 0.0
        return [("t", 0.0), WORD, ("t", size / 100)], -0.1, 0.0
    return decode


# ---------------------------------------------------------------- 1. grouping
def test_round_offers_every_live_clip_in_chunks(monkeypatch):
    rig = _Rig(monkeypatch, _grid(5, 25), max_windows=2, decode=_short_then_rest({1, 3}))
    segments = rig.run()
    # a round is cut into chunks of max_windows; a place freed inside a round is not
    # refilled (refilling would give [0,3000] [1000,6000] [7000,9000] ...)
    assert rig.encodes == [([0, 3000], [2500, 2500]), ([6000, 9000], [2500, 2500]), ([12000], [2500]),
                           ([1000, 7000], [1500, 1500]), ([13000], [1500])]
    assert [c["slots"] for c in rig.calls] == [None] * 5
    assert [len(c["prompts"]) for c in rig.calls] == [2, 2, 1, 2, 1]
    # segments come out in clip order, not in round order
    assert [s["seek"] for s in segments] == [0, 1000, 3000, 6000, 7000, 9000, 12000, 13000]
    assert [(s["start"], s["end"]) for s in segments] == [
        (0.0, 10.0), (10.0, 25.0), (30.0, 55.0), (60.0, 70.0), (70.0, 85.0), (90.0, 115.0), (120.0, 130.0),
        (130.0, 145.0)]


def test_single_clip_is_a_chunk_of_one(monkeypatch):
    rig = _Rig(monkeypatch, _grid(1, 25), max_windows=2, decode=_short_then_rest(set()))
    segments = rig.run()
    assert rig.encodes == [([0], [2500]), ([1000], [1500])]
    assert [c["slots"] for c in rig.calls] == [None, None]
    assert [s["seek"] for s in segments] == [0, 1000]


def test_three_clips_leave_a_trailing_chunk_of_one(monkeypatch):
    rig = _Rig(monkeypatch, _grid(3, 25), max_windows=2, decode=_short_then_rest({0}))
    segments = rig.run()
    assert rig.encodes == [([0, 3000], [2500, 2500]), ([6000], [2500]), ([4000, 7000], [1500, 1500])]
    assert [s["seek"] for s in segments] == [0, 3000, 4000, 6000, 7000]


# ---------------------------------------------------------------- 2. prompt
PROMPT = [2001, 2002, 2003]


def test_prompt_goes_to_the_first_window_of_clip_0_only(monkeypatch):
    rig = _Rig(monkeypatch, [(0, 40), (60, 100), (120, 150)], max_windows=2, initial_prompt=PROMPT)
    rig.run()
    assert rig.encodes == [([0, 6000], [3000, 3000]), ([12000], [3000]), ([3000, 9000], [1000, 1000])]
    assert [c["prompts"] for c in rig.calls] == [[PROMPT, None], [None], [None, None]]


def test_prompt_is_not_shown_again_after_a_no_speech_skip(monkeypatch):
    def decode(seek, size, temperature):
        if seek == 0:  # skipped: no speech, and a low log-probability
            return [("t", 0.0), WORD, ("t", size / 100)], -2.0, 0.9
        return [("t", 0.0), WORD, ("t", size / 100)], -0.1, 0.0
    rig = _Rig(monkeypatch, [(0, 40), (60, 100)], max_windows=2, initial_prompt=PROMPT, decode=decode)
    segments = rig.run()
    assert rig.encodes == [([0, 6000], [3000, 3000]), ([3000, 9000], [1000, 1000])]
    assert [c["prompts"] for c in rig.calls] == [[PROMPT, None], [None, None]]
    assert [s["seek"] for s in segments] == [3000, 6000, 9000]


def test_prompt_is_dropped_when_clip_0_is_shorter_than_a_second(monkeypatch):
    rig = _Rig(monkeypatch, [(0, 0.5), (30, 50), (60, 80)], max_windows=2, initial_prompt=PROMPT)
    segments = rig.run()
    assert rig.encodes == [([3000, 6000], [2000, 2000])]
    assert [c["prompts"] for c in rig.calls] == [[None, None]]
    assert [s["seek"] for s in segments] == [3000, 6000]


# ---------------------------------------------------------------- 3. seeds
def test_retry_is_one_call_on_the_process_counter(monkeypatch):
    from whisper import decoding

    def decode(seek, size, temperature):
        low = temperature == 0.0 and seek in (0, 6000)  # falls back: log-probability under -1.0
        return [("t", 0.0), WORD, ("t", size / 100)], -2.0 if low else -0.1, 0.0
    monkeypatch.setattr(decoding, "_seed_counter", itertools.count(1))
    rig = _Rig(monkeypatch, _grid(3, 25), max_windows=4, temperature=(0.0, 0.4), decode=decode)
    before = decoding.next_seed()
    segments = rig.run()
    after = decoding.next_seed()
    assert rig.encodes == [([0, 3000, 6000], [2500, 2500, 2500])]
    assert [(c["temperature"], c["slots"], len(c["prompts"])) for c in rig.calls] == [(0.0, None, 3), (0.4, [0, 2], 2)]
    assert all(c["extra"] == [] for c in rig.calls)  # no seed, no languages
    # the retry drew the counter's next seed and nothing else did
    assert (before, rig.drawn, after) == (K_SEED, [2 * K_SEED % (1 << 64)], 3 * K_SEED % (1 << 64))
    assert [s["temperature"] for s in segments] == [0.4, 0.0, 0.4]


# ---------------------------------------------------------------- 4. ordered pass
def _word_script(long_word):
    """Clip 0 (0-30 s) is one segment 28.00-29.50 whose word ends at 29.50.  Clip 1's first
    window is <|0.20|> X <|1.00|><|1.00|>: one one-word segment, not a single-timestamp
    ending, so the seek follows the word's end.  The word is 0.20-2.00 (`long_word`, longer
    than twice the median) or 0.20-1.00.  The long one is shortened from the front when the
    last speech lies more than 2.8 s back: it does from the clip's own 0.0, it does not
    from the file's 29.5, and the segment's end with it."""
    def decode(seek, size, temperature):
        if seek == 0:
            return [("t", 28.0), WORD, ("t", 29.5)], -0.1, 0.0
        if seek == 3000:
            return [("t", 0.2), WORD, ("t", 1.0), ("t", 1.0)], -0.1, 0.0
        return [("t", 0.0), WORD, WORD + 1, ("t", size / 100)], -0.1, 0.0

    def align(seek):
        if seek == 0:
            return [(28.0, 29.5)]
        if seek == 3000:
            return [(0.2, 2.0 if long_word else 1.0)]
        return [(0.0, 0.5), (0.5, 1.0)]
    return dict(decode=decode, align=align)


def _brief(segments):
    return [(s["seek"], s["start"], s["end"], s["tokens"], [(w["word"], w["start"], w["end"]) for w in s["words"]])
            for s in segments]


def test_ordered_pass_emits_words_under_the_file_wide_last_speech(monkeypatch):
    rig = _Rig(monkeypatch, [(0, 30), (30, 60)], max_windows=2, word_timestamps=True, **_word_script(False))
    segments = rig.run()
    assert rig.encodes == [([0, 3000], [3000, 3000]), ([3100], [2900])]
    assert rig.aligned == [0, 3000, 3100]
    tb = rig.tok.timestamp_begin
    # recorded from the schedule before the lanes drove it; the last segment's bounds are its words'
    assert _brief(segments) == [
        (0, 28.1, 29.5, [tb + 1400, WORD, tb + 1475], [(" w0", 28.1, 29.5)]),
        (3000, 30.2, 31.0, [tb + 10, WORD, tb + 50], [(" w0", 30.2, 31.0)]),
        (3100, 31.0, 32.0, [tb, WORD, WORD + 1, tb + 1450], [(" w0", 31.0, 31.5), (" w1", 31.5, 32.0)]),
    ]
    assert all(s["text"] == rig.tok.decode([t for t in s["tokens"] if t < rig.tok.eot]) for s in segments)


def test_ordered_pass_refuses_a_seek_that_moves(monkeypatch):
    rig = _Rig(monkeypatch, [(0, 30), (30, 60)], max_windows=2, word_timestamps=True, **_word_script(True))
    assert rig.run() is None
    # the round's provisional seek (word end 31.30 from the clip's own last speech)
    assert rig.encodes == [([0, 3000], [3000, 3000]), ([3130], [2870])]
