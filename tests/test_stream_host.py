"""Streaming, host side (no GPU): the C ABI carries the six stream entry points; the emission
count E(n) of include/whisper_hip.h is the same in C and in Python, is safe (the first E(n)
outputs of a prefix are those of the whole recording) and maximal (output E(n) reads frame n);
the LocalAgreement policy on scripted hypotheses; the trimming rules of StreamingTranscriber
driven with a scripted decode function and a stream that only counts samples."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_audio_ingest_host import RATES, direct_resample, ratio


def _has_device():
    try:
        import torch
        return bool(torch.cuda.is_available())
    except Exception:
        return False


# asked once, when the module is collected: before any test of the run has opened a context
HAS_DEVICE = _has_device()

STREAM_SYMBOLS = ("wh_stream_begin", "wh_stream_append", "wh_stream_finish", "wh_stream_trim", "wh_stream_info",
                  "wh_stream_emitted")


def emitted(n, rate, final=False):
    """E(n) written out once more, from the definition: the outputs whose newest frame
    (k * down + half) // up is below n."""
    up, down = ratio(rate)
    if up == down:
        return n
    if final:
        return -(-n * up // down)
    half = 10 * max(up, down)
    k = 0
    while (k * down + half) // up < n:
        k += 1
    return k


# ---------------------------------------------------------------- the C ABI
def test_header_library_and_shim_have_the_stream_entry_points():
    from whisper import backend_hip
    src = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in STREAM_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in backend_hip._EXPORTS, name
    lib.wh_version.restype = ctypes.c_int
    assert lib.wh_version() == 3
    assert backend_hip.N_STATS == 16 and re.search(r"WH_N_STATS = 16\b", src)


@pytest.mark.parametrize("rate", RATES + (16000,))
def test_stream_emitted_is_the_formula(rate):
    from whisper.audio import stream_emitted
    from whisper.backend_hip import load_library
    lib = load_library()
    up, down = ratio(rate)
    reach = 2 * 10 * max(up, down) // up
    ns = sorted(set(range(41)) | {reach - 1, reach, reach + 1, 2 * reach + 3, 100003, 13_500_000})
    for n in ns:
        for final in (False, True):
            want = emitted(n, rate, final) if n < 200000 else stream_emitted(n, rate, final)
            assert stream_emitted(n, rate, final) == want, (n, final)
            assert lib.wh_stream_emitted(n, up, down, int(final)) == want, (n, final)
    assert stream_emitted(0, rate) == 0
    # never ahead of the input, never more than 20 outputs behind the recording's total
    for n in ns:
        assert 0 <= stream_emitted(n, rate, True) - stream_emitted(n, rate) <= 20
    assert lib.wh_stream_emitted(-1, up, down, 0) == -1
    assert lib.wh_stream_emitted(5, 0, down, 0) == -1 and lib.wh_stream_emitted(5, up, 0, 1) == -1


@pytest.mark.parametrize("rate", (8000, 11025, 44100, 48000, 96000))
def test_a_prefix_already_gives_the_first_emitted_outputs(rate):
    """The first E(n) outputs computed from frames [0, n) alone are those of the whole
    recording, and E(n) is maximal: output E(n) reads frame n."""
    from whisper.audio import resample_filter, stream_emitted
    up, down, taps = resample_filter(rate)
    half = 10 * max(up, down)
    reach = 2 * half // up
    rng = np.random.default_rng(rate)
    N = 3 * reach + 37
    pcm = rng.integers(-32768, 32768, (N, 2), dtype=np.int16)
    whole = direct_resample(pcm, 16, up, down, taps)
    for n in sorted({1, 2, reach // 2, reach - 1, reach, reach + 1, 2 * reach + 5, N - 1, N}):
        e = stream_emitted(n, rate)
        assert e == emitted(n, rate)
        part = direct_resample(pcm[:n], 16, up, down, taps)
        assert e <= len(part) and np.array_equal(part[:e], whole[:e]), (rate, n)
        assert (e * down + half) // up >= n          # output e needs a frame that has not arrived
        assert e == 0 or ((e - 1) * down + half) // up < n
    assert stream_emitted(N, rate, True) == len(whole)


# ---------------------------------------------------------------- LocalAgreement
def W(word, start, end=None, p=0.9):
    return dict(word=word, start=start, end=start + 0.3 if end is None else end, probability=p)


def words_of(ws):
    return [w["word"] for w in ws]


def test_agreement_commits_and_disagreement_does_not():
    from whisper.streaming import LocalAgreement
    la = LocalAgreement()
    assert la.update([W(" the", 0.0), W(" cat", 0.4)]) == [] and la.T == 0.0
    assert words_of(la.pending) == [" the", " cat"]
    new = la.update([W(" the", 0.02), W(" cat", 0.41), W(" sat", 0.8)])
    assert words_of(new) == [" the", " cat"] and words_of(la.pending) == [" sat"]
    assert new[0]["start"] == 0.02      # the new hypothesis' times
    assert la.T == pytest.approx(0.71)
    # a different continuation: nothing more is committed, the pending tail is replaced
    assert la.update([W(" sad", 0.8), W(" story", 1.2)]) == []
    assert words_of(la.pending) == [" sad", " story"] and words_of(la.committed) == [" the", " cat"]
    # agreement only on a prefix
    assert words_of(la.update([W(" sad", 0.8), W(" stories", 1.2)])) == [" sad"]
    assert words_of(la.pending) == [" stories"]


def test_punctuation_and_case_flicker_still_agree():
    from whisper.streaming import LocalAgreement
    la = LocalAgreement()
    la.update([W(" Hello", 0.0), W(" world", 0.5)])
    new = la.update([W(" hello,", 0.0), W(" \"World!\"", 0.5), W(" again", 1.0)])
    assert words_of(new) == [" hello,", " \"World!\""]
    assert la.key(W(" ¿Qué?", 0)) == "qué" and la.key(W("-word-", 0)) == "word-"


def test_words_before_the_committed_end_are_dropped():
    from whisper.streaming import LocalAgreement
    la = LocalAgreement()
    la.update([W(" one", 0.0, 0.5), W(" two", 0.6, 1.0)])
    la.update([W(" one", 0.0, 0.5), W(" two", 0.6, 1.0)])
    assert la.T == 1.0
    # start <= T - 0.1 is history; start just above it is kept
    hyp = [W(" uno", 0.0, 0.5), W(" zwei", 0.9, 1.0), W(" three", 0.95, 1.4), W(" four", 1.5, 1.9)]
    assert la.update(hyp) == [] and words_of(la.pending) == [" three", " four"]
    assert words_of(la.update(hyp)) == [" three", " four"]


def test_committed_words_decoded_again_are_dropped_from_the_head():
    from whisper.streaming import LocalAgreement
    la = LocalAgreement()
    first = [W(" a", 0.0, 0.9), W(" b", 1.0, 1.9), W(" c", 2.0, 3.0)]
    la.update(first)
    la.update(first)
    assert la.T == 3.0
    # the same three words again with later times: the 3-gram overlap goes, " d" is new
    again = [W(" a", 2.95), W(" b", 3.0), W(" c", 3.1), W(" d", 3.4)]
    assert la.update(again) == [] and words_of(la.pending) == [" d"]
    assert words_of(la.update(again)) == [" d"]
    assert words_of(la.committed) == [" a", " b", " c", " d"]
    # at most five: a six-word echo is not recognised as a whole
    la = LocalAgreement()
    six = [W(f" w{i}", float(i), i + 0.9) for i in range(6)]
    la.update(six)
    la.update(six)
    echo = [W(f" w{i}", 5.85 + 0.01 * i) for i in range(6)]
    la.update(echo)
    assert words_of(la.pending) == words_of(echo)


def test_flush_commits_what_is_pending():
    from whisper.streaming import LocalAgreement
    la = LocalAgreement()
    la.update([W(" so", 0.0), W(" long", 0.5, 0.9)])
    assert words_of(la.flush()) == [" so", " long"] and la.pending == [] and la.T == 0.9
    assert la.flush() == []


# ---------------------------------------------------------------- the transcriber's rules
class CountingStream:
    """What StreamingTranscriber asks of a stream, counting samples only (16 kHz mono s16)."""

    def __init__(self, rate=16000, frame_bytes=2):
        self.rate, self.frame_bytes = rate, frame_bytes
        self.frames, self.n_samples, self.trims = 0, 0, []

    def append(self, data):
        assert len(data) % self.frame_bytes == 0
        before = emitted(self.frames, self.rate)
        self.frames += len(data) // self.frame_bytes
        got = emitted(self.frames, self.rate) - before
        self.n_samples += got
        return got

    def finish(self):
        got = emitted(self.frames, self.rate, True) - emitted(self.frames, self.rate)
        self.n_samples += got
        return got

    def trim(self, n):
        assert 0 < n <= self.n_samples
        self.n_samples -= n
        self.trims.append(n)


def truth_word(i):
    return dict(word=f" w{i}", start=0.5 * i, end=0.5 * i + 0.4, probability=0.5)


def scripted_decode(per_segment, log, rename=None):
    """A decode of ground-truth words every 0.5 s: the hypothesis of a buffer (s0, s1) holds the
    words that lie inside it, in segments of ``per_segment`` words, times relative to s0."""
    def decode(prompt, span):
        log.append((prompt, span))
        t0, t1 = span[0] / 16000, span[1] / 16000
        segs = {}
        for i in range(int(t1 * 2) + 1):
            w = truth_word(i)
            if w["start"] >= t0 and w["end"] <= t1:
                if rename:
                    w["word"] = rename(i, len(log))
                w["start"] -= t0
                w["end"] -= t0
                segs.setdefault(i // per_segment, []).append(w)
        return dict(language="en", text="", segments=[dict(start=ws[0]["start"], end=ws[-1]["end"], words=ws)
                                                      for ws in segs.values()])
    return decode


def make(per_segment=4, rename=None, **kw):
    from whisper.streaming import StreamingTranscriber
    log, stream = [], CountingStream()
    opts = dict(min_chunk=1.0, buffer_trim=4.0, max_buffer=6.0)
    opts.update(kw)
    t = StreamingTranscriber(None, 16000, stream=stream, decode_fn=scripted_decode(per_segment, log, rename), **opts)
    return t, stream, log


SECOND = np.zeros(16000, np.int16).tobytes()


def test_rule_1_cuts_at_the_last_committed_segment_end():
    t, stream, log = make(per_segment=4)
    ups = [u for _ in range(5) for u in t.feed(SECOND)]
    assert [u.span for u in ups] == [(0, 16000 * k) for k in range(1, 6)]
    # decode k commits the words that decode k - 1 already had: those ending by k - 1
    assert words_of(t.committed) == [f" w{i}" for i in range(8)] and t.policy.T == pytest.approx(3.9)
    # 5 s > buffer_trim: segment 1 (words 4..7) ends at 3.9 = T, the latest end in (t0, T]
    assert stream.trims == [62400] and t.span == (62400, 80000)
    assert not ups[-1].forced and words_of(ups[-1].tentative) == [" w8", " w9"]
    u = t.feed(SECOND)[0]
    assert u.span == (62400, 96000) and words_of(u.committed) == [" w8", " w9"]
    assert u.prompt == " ".join(f"w{i}" for i in range(8))
    for _ in range(20):
        t.feed(SECOND)
    assert all(s1 - s0 <= 30 * 16000 for _, (s0, s1) in log)
    assert max(s1 - s0 for _, (s0, s1) in log) <= (6 + 1) * 16000
    final = t.finish()
    assert final.final and t.pending == [] and final.result is None       # nothing new since the last decode
    assert words_of(t.committed) == [f" w{i}" for i in range(len(t.committed))]  # in order, none twice
    assert t.text == " ".join(f"w{i}" for i in range(len(t.committed)))


def test_rule_2_cuts_at_the_committed_end_when_no_segment_ends_before_it():
    t, stream, log = make(per_segment=10 ** 6)  # one segment that ends with the newest word
    ups = [u for _ in range(7) for u in t.feed(SECOND)]
    # 5 s and 6 s exceed buffer_trim, but the only segment ends after T: nothing to cut at
    assert [u.span for u in ups] == [(0, 16000 * k) for k in range(1, 8)]
    # 7 s > max_buffer: cut at T = 5.9
    assert t.policy.T == pytest.approx(5.9) and stream.trims == [94400] and t.span == (94400, 112000)
    assert not any(u.forced for u in ups)


def test_rule_3_forces_a_commit_when_nothing_agrees():
    t, stream, log = make(rename=lambda i, k: f" v{k}_{i}")  # every decode spells every word anew
    ups = [u for _ in range(7) for u in t.feed(SECOND)]
    assert all(u.committed == [] and not u.forced for u in ups[:6])
    last = ups[6]
    # 7 s > max_buffer and T = 0: the pending words are committed, the cut is at t1 - buffer_trim
    assert last.forced and words_of(last.committed) == [f" v7_{i}" for i in range(14)]
    assert last.tentative == [] and t.pending == []
    assert stream.trims == [48000] and t.span == (48000, 112000)
    assert t.policy.T == pytest.approx(6.9)


def test_prompt_is_initial_prompt_plus_committed_text_before_the_buffer():
    t, stream, log = make(prompt_chars=10, initial_prompt="Glossary:")
    for _ in range(6):
        t.feed(SECOND)
    assert [p for p, _ in log[:5]] == ["Glossary:"] * 5
    # the buffer starts at 3.9: words 0..7 lie before it, the last 10 characters hold three
    assert log[5] == ("Glossary: w5 w6 w7", (62400, 96000))
    assert t.build_prompt(0.3) == "Glossary:" and t.build_prompt(0.4) == "Glossary: w0"
    t.prompt_chars, t.initial_prompt = 200, None
    assert t.build_prompt(3.9) == " ".join(f"w{i}" for i in range(8))
    assert make()[0].build_prompt(0.0) is None


def test_cuts_are_whole_samples_and_stay_inside_the_buffer():
    t, stream, log = make()
    t.feed(SECOND * 3)
    assert t.span == (0, 48000)
    t._cut(16000.6 / 16000)           # rounds to the nearest sample: floor(x + 0.5)
    assert t.span == (16001, 48000) and stream.trims == [16001]
    t._cut(0.5)                       # before the buffer: nothing
    assert t.span == (16001, 48000) and stream.trims == [16001]
    t._cut((16001 + 7.49) / 16000)
    assert t.span == (16008, 48000)
    t._cut(99.0)                      # past the end: the whole buffer, no more
    assert t.span == (48000, 48000) and stream.n_samples == 0


def test_updates_do_not_depend_on_how_the_input_was_split():
    def run(sizes):
        t, stream, log = make()
        data = SECOND * 9 + b"\0" * 801          # the last byte is half a frame
        ups, pos = [], 0
        for n in sizes:
            ups += t.feed(data[pos:pos + n])
            pos += n
        ups += t.feed(data[pos:])
        ups.append(t.finish())
        return [(u.span, words_of(u.committed), words_of(u.tentative), u.prompt, u.forced, u.final) for u in ups]
    whole = run([])
    assert len(whole) == 10 and whole[-1][5] and whole[-1][0][1] == 9 * 16000 + 400
    assert run([3200] * 80) == whole
    assert run([1, 3, 31999, 7, 100001, 5]) == whole


def test_finish_of_an_empty_stream_decodes_nothing():
    t, stream, log = make()
    u = t.finish()
    assert u.final and u.committed == [] and u.tentative == [] and u.result is None and log == []
    with pytest.raises(ValueError):
        t.feed(SECOND)


def test_finish_decodes_the_rest_and_flushes():
    t, stream, log = make()
    t.feed(SECOND + SECOND[:16000])   # 1.5 s: one decode at 1 s
    assert len(log) == 1
    u = t.finish()
    assert len(log) == 2 and u.span == (0, 24000) and u.final and u.result is not None
    assert words_of(u.committed) == [" w0", " w1", " w2"] and t.pending == []


def test_options_are_validated():
    from whisper.streaming import AudioStream, StreamingTranscriber
    ok = dict(stream=CountingStream(), decode_fn=lambda p, s: dict(segments=[]))
    StreamingTranscriber(None, 16000, word_timestamps=True, temperature=0.0, **ok)
    with pytest.raises(ValueError, match="word_timestamps"):
        StreamingTranscriber(None, 16000, word_timestamps=False, **ok)
    for name, value in (("clip_timestamps", "0,5"), ("channels", "split"), ("schedule", "batched"),
                        ("mel_max_reduce", max)):
        with pytest.raises(ValueError, match=name):
            StreamingTranscriber(None, 16000, **{name: value}, **ok)
    for bad in (dict(buffer_trim=25.0, max_buffer=25.0), dict(max_buffer=29.5), dict(min_chunk=6.0),
                dict(min_chunk=0.0), dict(buffer_trim=0.0)):
        with pytest.raises(ValueError, match="buffer_trim|min_chunk"):
            StreamingTranscriber(None, 16000, **bad, **ok)
    StreamingTranscriber(None, 16000, min_chunk=5.0, **ok)  # 25 <= 30 - 5
    with pytest.raises(ValueError, match="encoding"):
        StreamingTranscriber(None, 16000, "mp3", **ok)
    # a rate nearly coprime with 16000 has no device filter: refused by name, before any device call
    with pytest.raises(ValueError, match="16001"):
        AudioStream(None, 16001)
    with pytest.raises(ValueError, match="encoding"):
        AudioStream(None, 8000, "s12")
    with pytest.raises(TypeError, match="int16|<i2"):
        StreamingTranscriber(None, 16000, **ok).feed(np.zeros(4, np.float32))


def test_a_stream_needs_a_device():
    """No CPU fallback: without a HIP device opening a stream raises."""
    import whisper
    if HAS_DEVICE:
        s = whisper.AudioStream(None, 8000, "ulaw")
        assert s.append(bytes(800)) == whisper.audio.stream_emitted(800, 8000) and s.n_samples == 1580
    else:
        with pytest.raises(whisper.HipBackendError):
            whisper.AudioStream(None, 8000, "ulaw")
        with pytest.raises(whisper.HipBackendError):
            whisper.StreamingTranscriber(None, 8000, "ulaw")
