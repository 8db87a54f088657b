"""Forced alignment without a GPU: the numpy statement of the open-end DTW
(tests/dtw_open_ref.py) against the oracle's closed DTW and on planted matrices, and the
window policy of whisper/align.py driven by a stub round that answers from one long planted
matrix per file (``align_round_fn``)."""
import math

import numpy as np
import pytest

from dtw_open_ref import dtw_open_ref, dtw_tables, dtw_tables_cellwise, planted_matrix

ROW_PENALTY = 4.0


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 3), (17, 5), (5, 300), (40, 150)])
@pytest.mark.parametrize("kind", ["zeros", "ints", "randn"])
def test_closed_form_is_the_oracle_dtw(shape, kind):
    from oracle import ref_timing as RT
    rng = np.random.default_rng(sum(shape) * 7 + len(kind))
    x = {"zeros": np.zeros(shape), "ints": rng.integers(0, 3, shape).astype(np.float64),
         "randn": rng.standard_normal(shape)}[kind].astype(np.float32)
    path, e, scores = dtw_open_ref(x, 0, ROW_PENALTY)
    np.testing.assert_array_equal(path, RT.dtw_cpu(x.astype(np.float64)))
    assert e == shape[0] and scores.shape == (shape[0],)
    # min_rows = N leaves no choice: the same path
    np.testing.assert_array_equal(dtw_open_ref(x, shape[0], ROW_PENALTY)[0], path)


def test_tables_by_diagonal_equal_cell_by_cell():
    rng = np.random.default_rng(5)
    for x in (rng.standard_normal((17, 23)), rng.integers(0, 3, (9, 14)), np.zeros((6, 4))):
        x = np.asarray(x, dtype=np.float32)
        a, b = dtw_tables(x), dtw_tables_cellwise(x)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_ties_take_the_smallest_row_and_the_path_ends_there():
    x = np.zeros((6, 9), dtype=np.float32)
    for min_rows in (1, 3, 6):
        path, e, scores = dtw_open_ref(x, min_rows, 0.0)
        assert e == min_rows and np.all(scores == 0)
        assert path[0, -1] == e - 1 and path[1, -1] == 8 and path.shape[1] <= e + 9
        assert path[0, 0] == 0 and path[1, 0] == 0


def _planted_case(seed, noise):
    rng = np.random.default_rng(1000 + seed)
    n_rows = int(rng.integers(12, 40))
    spoken = int(rng.integers(3, n_rows - 2))
    n_cols = int(rng.integers(3 * spoken + 10, 3 * spoken + 200))
    return planted_matrix(n_rows, n_cols, spoken, noise, seed), spoken


@pytest.mark.parametrize("noise", [0.2, 0.5])
def test_planted_end_row_is_recovered(noise):
    """40 z-normalised planted matrices per noise level, every planted row owning at least 3
    frames: row_penalty = 4.0 returns the planted end row every time.  (Without a penalty it
    does not: counted here so that the reason for the penalty stays on record.)"""
    missed_without = 0
    for seed in range(40):
        (x, _), spoken = _planted_case(seed, noise)
        tables = dtw_tables(x)
        path, e, _ = dtw_open_ref(x, 1, ROW_PENALTY, tables)
        assert e == spoken, (seed, e, spoken)
        assert path[0, -1] == spoken - 1 and path[1, -1] == x.shape[1] - 1
        missed_without += dtw_open_ref(x, 1, 0.0, tables)[1] != spoken
    assert missed_without > 0


# ---------------------------------------------------------------- the policy with a stub
LINES = [
    "the quick brown fox jumps over the lazy dog while seven wizards boxing for a prize",
    "every good boy does fine and all cows eat grass under a wide open morning sky",
    "she sells sea shells by the sea shore where the warm wind blows over white sand",
    "a journey of a thousand miles begins with one small step taken on a quiet road",
]


def _tokenizer():
    from whisper.tokenizer import get_tokenizer
    return get_tokenizer(True, num_languages=99, language="en", task="transcribe")


class PlantedFile:
    """A file whose text tokens own consecutive stretches of its DTW columns (20 ms each).
    ``spoken_tokens`` of the text's tokens are spoken (default: all); the raw weights are 1
    where a token owns a column plus uniform noise."""

    def __init__(self, lines, seconds, seed, spoken_tokens=None, noise=0.2, min_frames=3):
        from whisper.align import split_lines, text_words
        self.tok = _tokenizer()
        self.words, self.line_tokens = text_words(self.tok, split_lines(lines), 10 ** 6)
        self.n_tokens = sum(len(w.tokens) for w in self.words)
        self.n_samples = int(seconds * 16000)
        self.cols = self.n_samples // 320
        spoken = self.n_tokens if spoken_tokens is None else spoken_tokens
        rng = np.random.default_rng(seed)
        extra = self.cols - spoken * min_frames
        cuts = np.sort(rng.integers(0, extra + 1, spoken - 1))
        sizes = np.diff(np.concatenate(([0], cuts, [extra]))) + min_frames
        self.bounds = np.concatenate(([0], np.cumsum(sizes))).astype(int)
        self.raw = noise * rng.random((self.n_tokens + 1, self.cols))  # the last row: eot
        for r in range(spoken):
            self.raw[r, self.bounds[r]:self.bounds[r + 1]] += 1.0
        self.spoken = spoken

    def word_bounds(self):
        """(start, end) in seconds of every word whose tokens are all spoken."""
        out, t = [], 0
        for w in self.words:
            if t + len(w.tokens) > self.spoken:
                break
            out.append((self.bounds[t] / 50.0, self.bounds[t + len(w.tokens)] / 50.0))
            t += len(w.tokens)
        return out

    def answer(self, window):
        assert window.seek % 2 == 0 and window.seek // 2 + window.seg // 2 <= self.cols
        t0, T = window.first_token, len(window.tokens)
        c0, F = window.seek // 2, window.seg // 2
        rows = list(range(t0, t0 + T)) + [self.n_tokens]
        w = self.raw[rows, c0:c0 + F]
        w = (w - w.mean(axis=0, keepdims=True)) / w.std(axis=0, keepdims=True)
        path, e, _ = dtw_open_ref((-w).astype(np.float32), window.min_rows, ROW_PENALTY)
        return np.full(T, 0.5, dtype=np.float32), path[0], path[1], e


def _stub(files, log=None):
    def align_round(windows):
        if log is not None:
            log.append([(w.file, w.seek, w.seg, w.first_token, len(w.tokens), w.min_rows) for w in windows])
        return [files[w.file].answer(w) for w in windows]
    return align_round


def _words(result):
    return [(w["word"], tuple(w["tokens"]), w["start"], w["end"]) for s in result["segments"] for w in s["words"]]


@pytest.mark.parametrize("max_tokens", [None, 24])
def test_policy_aligns_a_long_file(max_tokens):
    from whisper.align import align
    f = PlantedFile(LINES, 70.0, seed=3)
    assert len(f.words) == 64 and f.cols == 3500
    r = align(None, f.n_samples, LINES, language="en", max_tokens=max_tokens, align_round_fn=_stub([f]))
    assert r["unaligned"] == [] and r["language"] == "en"
    got = _words(r)
    assert [g[0] for g in got] == [w.word for w in f.words]
    assert [list(g[1]) for g in got] == [w.tokens for w in f.words]
    want = f.word_bounds()
    assert len(want) == len(got)
    for (word, _, start, end), (ws, we) in zip(got, want):
        assert abs(start - ws) <= 0.02 + 1e-9 and abs(end - we) <= 0.02 + 1e-9, (word, start, end, ws, we)
    # rounds: at least 3, each advancing the word cursor or the seek
    wins = r["windows"]
    assert len(wins) >= 3
    done = 0
    for k, (seek, seg, n_cand, end_row, accepted) in enumerate(wins):
        assert seg == min(3000, 7000 - seek) and 1 <= end_row <= n_cand + 1
        if max_tokens is not None:
            assert n_cand <= max_tokens
        if k + 1 < len(wins):
            assert accepted > 0 or wins[k + 1][0] > seek
            assert wins[k + 1][0] >= seek
        done += accepted
    assert done == len(f.words)
    # lines map to segments
    assert [s["line"] for s in r["segments"]] == [0, 1, 2, 3] and [s["id"] for s in r["segments"]] == [0, 1, 2, 3]
    for s, line, ids in zip(r["segments"], LINES, f.line_tokens):
        assert s["text"] == " " + line and s["tokens"] == ids
        assert "".join(w["word"] for w in s["words"]) == " " + line
        assert s["start"] == s["words"][0]["start"] and s["end"] == s["words"][-1]["end"]
    starts = [g[2] for g in got]
    assert starts == sorted(starts) and got[-1][3] <= 70.0


def test_only_the_last_full_window_is_closed():
    from whisper.align import align
    f = PlantedFile(LINES, 70.0, seed=3)
    log = []
    align(None, f.n_samples, LINES, language="en", max_tokens=24, align_round_fn=_stub([f], log))
    flat = [w for rnd in log for w in rnd]
    assert all(len(rnd) == 1 for rnd in log)
    for (_, seek, seg, first, n, min_rows) in flat:
        full, last = first + n == f.n_tokens, seek + seg >= 7000
        assert min_rows == (0 if full and last else 1)
    assert flat[-1][5] == 0


def test_text_longer_than_the_audio_leaves_the_surplus_unaligned():
    from whisper.align import align
    f = PlantedFile(LINES, 40.0, seed=9, spoken_tokens=40)
    r = align(None, f.n_samples, LINES, language="en", max_tokens=12, align_round_fn=_stub([f]))
    got = _words(r)
    n = len(got)
    spoken_words = len(f.word_bounds())
    assert 0 < n <= spoken_words + 1 and len(r["unaligned"]) == len(f.words) - n > 0
    assert [u["word"] for u in r["unaligned"]] == [w.word for w in f.words[n:]]
    for u in r["unaligned"]:
        assert u["start"] == u["end"] == 40.0 and math.isnan(u["probability"])
    # what was spoken before the last window is where it was planted
    for (word, _, start, end), (ws, we) in list(zip(got, f.word_bounds()))[:-2]:
        assert abs(start - ws) <= 0.02 + 1e-9 and abs(end - we) <= 0.02 + 1e-9, (word, start, end, ws, we)
    assert r["windows"][-1][0] + r["windows"][-1][1] == 4000


def test_batch_equals_each_file_alone():
    from whisper.align import align, align_batch
    a = PlantedFile(LINES, 70.0, seed=3)
    b = PlantedFile(LINES[:1], 10.0, seed=4)
    c = PlantedFile(LINES[1:3], 45.0, seed=5)
    files, texts = [a, b, c, a], [LINES, LINES[:1], LINES[1:3], LINES]
    log = []
    for max_windows in (8, 2):
        batch = align_batch(None, [f.n_samples for f in files], texts, language="en", max_tokens=30,
                            max_windows=max_windows, align_round_fn=_stub(files, log))
        for f, t, r in zip(files, texts, batch):
            alone = align(None, f.n_samples, t, language="en", max_tokens=30, align_round_fn=_stub([f]))
            assert _words(r) == _words(alone) and r["windows"] == alone["windows"]
            assert r["unaligned"] == alone["unaligned"] == []
        assert _words(batch[0]) == _words(batch[3])
    assert max(len(rnd) for rnd in log) == 4 and max(len(rnd) for rnd in log[-6:]) <= 2


def test_refusals():
    from whisper.align import align, align_batch
    tok = _tokenizer()
    boom = dict(language="en", align_round_fn=lambda windows: 1 / 0)
    with pytest.raises(ValueError, match="empty"):
        align(None, 16000, " \n\n", **boom)
    with pytest.raises(ValueError, match="empty"):
        align(None, 16000, [[], ""], **boom)
    with pytest.raises(ValueError, match="no text token"):
        align(None, 16000, [[100, tok.eot]], **boom)
    word = tok.encode(" antidisestablishmentarianism")
    assert len(word) >= 3 and len(tok.split_to_word_tokens(word)[1]) == 1
    with pytest.raises(ValueError, match=f"at most {len(word) - 1}"):
        align(None, 16000, [word], max_tokens=len(word) - 1, **boom)
    long_word = word + word[1:] * 120
    assert len(long_word) > 219 and len(tok.split_to_word_tokens(long_word)[1]) == 1
    with pytest.raises(ValueError, match="at most 219"):
        align(None, 16000, [long_word], **boom)
    # a text whose language is still to be detected is checked before any device work too
    # (model=None would fail at the first device call): ids, and pieces that are over-long in
    # every language
    from whisper.align import check_text
    with pytest.raises(ValueError, match="no text token"):
        check_text(tok, [[100, tok.eot]], 219)
    emoji = tok.encode("\U0001f600")  # one UTF-8-complete piece of two tokens
    assert len(emoji) == 2 and len(tok.split_tokens_on_unicode(emoji)[1]) == 1
    with pytest.raises(ValueError, match="at most 1"):
        check_text(tok, [emoji], 1)
    check_text(tok, [word], len(word) - 1)  # over-long only as a space-delimited language joins it
    for name, value in (("skip_silence", True), ("channels", "split"), ("clip_timestamps", "0,5")):
        with pytest.raises(ValueError, match=name):
            align(None, 16000, "hello", **{name: value}, **boom)
        with pytest.raises(ValueError, match=name):
            align_batch(None, [16000], ["hello"], **{name: value}, **boom)
    with pytest.raises(ValueError, match="texts"):
        align_batch(None, [16000, 16000], ["hello"], **boom)
    with pytest.raises(ValueError, match="row_penalty"):
        align(None, 16000, "hello", row_penalty=float("nan"), **boom)
