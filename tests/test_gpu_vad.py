"""Speech spans on the GPU (wh_speech_spans / wh_frame_energy_read): frame energies,
histograms, thresholds and spans are equal to the host definition (whisper/vad.py) — every
comparison here is exact — at every file offset and length class, at each boundary of the
run-length rules, with several frames per thread and with too little room for the spans;
``transcribe(..., skip_silence=True)`` equals ``transcribe`` over the same spans given as
explicit clips, alone and in ``transcribe_batch``."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")


def _ctx():
    from whisper.audio import _mel_context
    return _mel_context(0)


@pytest.fixture(scope="module")
def jfk():
    from whisper.audio import load_audio
    return load_audio(JFK)


@pytest.fixture(scope="module")
def fixture(jfk):
    return np.concatenate([np.zeros(48000, np.float32), jfk, np.zeros(80000, np.float32)])


def _host(x, p):
    """(E, histogram, T, spans) of the host definition."""
    from whisper import vad
    e = vad.frame_energy_host(x)
    h = vad.histogram_host(e)
    t = vad.threshold_host(h, len(e), p)
    return e, h, t, vad.spans_from_energy(e, t, p.min_silence, p.min_speech, p.pad)


def _tolist(spans):
    return [(int(s), int(e)) for s, e in spans]


# ---------------------------------------------------------------- energies and histograms
def _awkward(n, seed):
    """Samples that exercise the quantiser: +-1.0, beyond +-1 (clipped), exact rounding ties
    (k + 0.5) / 32768, values far below one step (subnormal ones too), NaN (counts as 0) and
    +-inf (clipped), ordinary noise."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.2).astype(np.float32)
    k = rng.integers(-32768, 32767, n)
    ties = ((k + 0.5) / 32768).astype(np.float32)  # exact in float32: 17 significant bits
    special = np.array([1.0, -1.0, 1.5, -7.0, 32767.5 / 32768, -32768.5 / 32768, 1e-40, -1e-42, 1e-7, 0.0, -0.0,
                        np.nan, -np.nan, np.inf, -np.inf],
                       np.float32)
    pick = rng.integers(0, 4, n)
    x = np.where(pick == 1, ties, x)
    x = np.where(pick == 2, special[rng.integers(0, len(special), n)], x)
    return x.astype(np.float32)


@pytest.mark.parametrize("n", [1, 159, 160, 161, 320, 16007])
def test_energy_and_histogram_equal_the_host(n):
    from whisper import vad
    ctx = _ctx()
    x = _awkward(n, 100 + n)
    ctx.audio_upload(x)
    e, h = ctx.frame_energy(0)
    want = vad.frame_energy_host(x)
    assert e.dtype == np.uint64 and len(e) == -(-n // 160)
    assert np.array_equal(e, want), np.flatnonzero(e != want)[:5]
    assert np.array_equal(h, vad.histogram_host(want))
    assert int(h.sum()) == len(e)


def test_nan_and_inf_samples():
    """NaN counts as 0, +-inf clip to 32767 / -32768: one known frame of each."""
    ctx = _ctx()
    x = np.zeros(480, np.float32)
    x[5], x[100] = np.nan, 3.0 / 32768
    x[160], x[161] = np.inf, np.nan
    x[320] = -np.inf
    ctx.audio_upload(x)
    e, _ = ctx.frame_energy(0)
    assert e.tolist() == [9, 32767 * 32767, 1 << 30]


def test_full_scale_frames():
    """160 samples of -1.0: the largest energy, 160 * 2^30, past 32 bits."""
    ctx = _ctx()
    ctx.audio_upload(np.full(480, -3.0, np.float32))
    e, h = ctx.frame_energy(0)
    assert e.tolist() == [160 << 30] * 3 and h[1 + 4 * 37 + 1] == 3


@pytest.mark.parametrize("lengths", [(300, 12345, 48007), (1, 161, 321, 12346)], ids=["issue", "every_phase"])
def test_files_back_to_back_equal_each_file_alone(lengths):
    """Files ingested back to back start at offsets that are no multiple of 160 or of 4 (the
    second set puts one at each of the four float4 phases): every file's energies,
    histogram, threshold and spans are those of the file alone."""
    from whisper import vad
    ctx = _ctx()
    rng = np.random.default_rng(7)
    files = []
    for i, n in enumerate(lengths):
        x = _awkward(n, 200 + i)
        gate = np.repeat(rng.random(-(-n // 800)) < 0.6, 800)[:n]  # 50 ms bursts and pauses
        files.append(np.where(gate, x, np.float32(0)).astype(np.float32))
    offset = 0
    for x in files:
        seg = ctx.audio_ingest(x, 16000, 32, dst_offset=offset, reserve=sum(lengths))
        assert seg.offset == offset and seg.n_samples == len(x)
        offset += len(x)
    assert {o % 4 for o in np.cumsum((0,) + lengths[:-1])} == ({0, 1} if len(lengths) == 3 else {0, 1, 2, 3})
    p = vad.resolve_options(min_silence=0.1, min_speech=0.03, pad=0.02)
    got = ctx.speech_spans(p, len(files))
    for i, x in enumerate(files):
        e, h, t, spans = _host(x, p)
        ge, gh = ctx.frame_energy(i)
        assert np.array_equal(ge, e) and np.array_equal(gh, h), i
        assert got[i][1] == t and _tolist(got[i][0]) == spans, (i, got[i], t, spans)
        if len(x) == max(lengths):
            assert len(spans) >= 2  # the data: the longest file's reference has spans to compare


# ---------------------------------------------------------------- spans
OPTION_SETS = {
    "defaults": dict(),
    "short": dict(min_silence=0.07, min_speech=0.04, pad=0.03),
    "no_closing": dict(min_silence=0.01, min_speech=0.0, pad=0.0),
}


def _pattern(n_frames, seed):
    """On/off frames whose run and gap lengths sit on the boundaries of every option set:
    gaps of min_silence - 1, min_silence, min_silence + 1 and of 2 pad - 1, 2 pad, 2 pad + 1
    (pads that overlap, touch, stay apart), runs of min_speech - 1 and min_speech."""
    rng = np.random.default_rng(seed)
    gaps = [1, 2, 3, 5, 6, 7, 8, 24, 79, 80, 81, 199, 200, 201, 240, 281]
    runs = [1, 2, 3, 4, 5, 24, 25, 26, 60]
    active = np.zeros(n_frames, bool)
    pos = int(rng.integers(0, 3))
    while pos < n_frames:
        r = int(rng.choice(runs))
        active[pos:pos + r] = True
        pos += r + int(rng.choice(gaps))
    return active


@pytest.fixture(scope="module", params=[3077, 70005], ids=["F3077", "F70005"])
def pattern_file(request):
    """A waveform of F frames (the last one partial), its host energies and its pattern."""
    from whisper import vad
    n_frames = request.param
    active = _pattern(n_frames, n_frames)
    amp = np.where(active, np.float32(0.25), np.float32(0)).astype(np.float32)
    x = np.repeat(amp, 160)[:n_frames * 160 - 37]
    return x, vad.frame_energy_host(x), active


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_spans_equal_the_host(pattern_file, name):
    from whisper import vad
    x, e, active = pattern_file
    ctx = _ctx()
    ctx.audio_upload(x)
    p = vad.resolve_options(**OPTION_SETS[name])
    t = vad.threshold_host(vad.histogram_host(e), len(e), p)
    want = vad.spans_from_energy(e, t, p.min_silence, p.min_speech, p.pad)
    assert t == p.t_lo  # more than a tenth of the frames are digital silence
    # little room first: the call reports what it needs and the shim repeats it
    (spans, thr), = ctx.speech_spans(p, 1, cap=2)
    assert thr == t and _tolist(spans) == want
    (spans, thr), = ctx.speech_spans(p, 1, cap=len(want))
    assert thr == t and _tolist(spans) == want
    print(name, len(e), "frames,", len(want), "spans")
    assert len(want) > 2
    if name == "no_closing":
        # nothing closes, drops or pads: the spans are the active runs themselves
        edges = np.flatnonzero(np.diff(np.concatenate([[0], active.astype(np.int8), [0]])))
        assert want == list(zip(edges[::2].tolist(), edges[1::2].tolist()))


def test_too_little_room_reports_the_count_and_writes_nothing(pattern_file):
    from whisper import vad
    from whisper.backend_hip import WhVadOpts
    x, e, _ = pattern_file
    ctx = _ctx()
    ctx.audio_upload(x)
    p = vad.resolve_options(**OPTION_SETS["no_closing"])
    want = vad.spans_from_energy(e, p.t_lo, p.min_silence, p.min_speech, p.pad)
    o = WhVadOpts(ratio_q8=p.ratio_q8, t_lo=p.t_lo, t_hi=p.t_hi, percentile=p.percentile,
                  min_silence=p.min_silence, min_speech=p.min_speech, pad=p.pad)
    cap = 3
    spans = np.full((cap, 2), -5, np.int32)
    count, thr = np.zeros(1, np.int32), np.zeros(1, np.uint64)
    rc = ctx.lib.wh_speech_spans(ctx.h, ctypes.byref(o), 1, spans.ctypes.data_as(ctypes.c_void_p), cap,
                                 count.ctypes.data_as(ctypes.c_void_p), thr.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and int(count[0]) == len(want) > cap and int(thr[0]) == p.t_lo
    assert (spans == -5).all()
    # far more room than the file could fill: the library stages and copies only what the file
    # can hold, and the caller's buffer is written for the spans that exist
    spans = np.full((len(want), 2), -5, np.int32)
    rc = ctx.lib.wh_speech_spans(ctx.h, ctypes.byref(o), 1, spans.ctypes.data_as(ctypes.c_void_p), 1 << 29,
                                 count.ctypes.data_as(ctypes.c_void_p), thr.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and int(count[0]) == len(want) and _tolist(spans) == want
    # no room at all, and no buffer
    rc = ctx.lib.wh_speech_spans(ctx.h, ctypes.byref(o), 1, None, 0, count.ctypes.data_as(ctypes.c_void_p),
                                 thr.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0 and int(count[0]) == len(want)


def test_refusals_and_stage_counters():
    from whisper import vad
    from whisper.backend_hip import HipBackendError
    ctx = _ctx()
    ctx.audio_upload(np.zeros(1000, np.float32))
    p = vad.resolve_options()
    before = ctx.stats()
    with pytest.raises(HipBackendError, match="resident"):
        ctx.speech_spans(p, 2)  # one segment is resident
    with pytest.raises(HipBackendError, match="resident"):
        ctx.frame_energy(1)
    with pytest.raises(HipBackendError, match="resident"):
        ctx.frame_energy(2 ** 31 - 1)
    with pytest.raises(HipBackendError, match="n_files"):
        ctx.speech_spans(p, 0)
    with pytest.raises(HipBackendError, match="percentile"):
        ctx.speech_spans(p._replace(percentile=0), 1)
    with pytest.raises(HipBackendError, match="ratio_q8"):
        ctx.speech_spans(p._replace(ratio_q8=2560001), 1)
    with pytest.raises(HipBackendError, match="t_lo"):
        ctx.speech_spans(p._replace(t_lo=p.t_hi + 1), 1)
    with pytest.raises(HipBackendError, match="frame counts"):
        ctx.speech_spans(p._replace(pad=-1), 1)
    assert ctx.stats() == before  # refused before anything was launched
    (got, thr), = ctx.speech_spans(p, 1)
    assert len(got) == 0 and thr == p.t_lo
    after = ctx.stats()
    moved = {k for k in after if after[k] != before[k]}
    assert moved == {"vad_energy_ms", "vad_spans_ms"}, moved
    assert after["vad_energy_ms"] > before["vad_energy_ms"] and after["vad_spans_ms"] > before["vad_spans_ms"]
    assert np.array_equal(ctx.audio_read(0, 1000), np.zeros(1000, np.float32))  # the segment is untouched


# ---------------------------------------------------------------- the three threshold branches
def test_threshold_branches(jfk, fixture):
    from whisper import vad
    ctx = _ctx()
    p = vad.resolve_options()
    rng = np.random.default_rng(55)
    noisy = (fixture + rng.standard_normal(len(fixture)) * 10 ** (-55 / 20)).astype(np.float32)
    seen = []
    for name, x in (("zeros", fixture), ("noise", noisy), ("jfk", jfk)):
        e, h, t, spans = _host(x, p)
        ctx.audio_upload(x)
        (got, thr), = ctx.speech_spans(p, 1)
        assert thr == t and _tolist(got) == spans, (name, thr, t, got, spans)
        seen.append(thr)
    assert seen[0] == p.t_lo and p.t_lo < seen[1] < p.t_hi and seen[2] == p.t_hi
    assert vad.speech_spans_host(fixture) == [(2.66, 14.40)] and vad.speech_spans_host(jfk) == [(0.0, 11.0)]


# ---------------------------------------------------------------- transcribe
@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def two_spans(fixture, jfk):
    """The fixture and a second utterance 5 s behind the first: two spans, so that
    condition_on_previous_text=False takes the batched schedule."""
    return np.concatenate([fixture, jfk[:100000], np.zeros(24000, np.float32)])


SEG_KEYS = ("seek", "tokens", "start", "end", "temperature", "text")


def _same(got, ref, words=False):
    assert got["language"] == ref["language"] and got["text"] == ref["text"]
    assert len(got["segments"]) == len(ref["segments"])
    for a, b in zip(got["segments"], ref["segments"]):
        for k in SEG_KEYS:
            assert a[k] == b[k], (k, a[k], b[k])
        if words:
            assert a["words"] == b["words"]


@pytest.mark.parametrize("case", ["sequential", "batched", "words"])
def test_skip_silence_equals_the_explicit_clips(micro32, fixture, two_spans, case):
    import whisper
    kw = dict(temperature=0.0, language="en", condition_on_previous_text=case != "batched",
              word_timestamps=case == "words")
    for name, audio, n_spans in (("fixture", fixture, 1), ("two_spans", two_spans, 2)):
        spans = whisper.speech_spans(micro32, audio)
        assert len(spans) == n_spans and spans[0] == (2.66, 14.40)
        got = whisper.transcribe(micro32, audio, skip_silence=True, **kw)
        ref = whisper.transcribe(micro32, audio, clip_timestamps=[t for s in spans for t in s], **kw)
        assert got["speech_spans"] == spans and "speech_spans" not in ref
        _same(got, ref, words=case == "words")
        seeks = [s["seek"] for s in got["segments"]]
        print(case, name, "spans", spans, "seeks", seeks)
        assert got["segments"] and min(seeks) >= 266
        # the spans were the clips: no window starts in the silence between them
        assert all(any(round(a * 100) <= k < round(b * 100) for a, b in spans) for k in seeks)
    # the key is there only when the option is set
    assert "speech_spans" not in whisper.transcribe(micro32, fixture, **kw)


def test_skip_silence_options_and_device_audio(micro32, fixture):
    import whisper
    opts = dict(pad=0.1, min_speech=0.5)
    spans = whisper.speech_spans(micro32, fixture, **opts)
    assert spans == whisper.vad.speech_spans_host(fixture, **opts) and spans != [(2.66, 14.40)]
    got = whisper.transcribe(micro32, fixture, skip_silence=opts, temperature=0.0, language="en")
    assert got["speech_spans"] == spans
    dev = micro32.ctx.audio_upload(fixture)
    assert whisper.speech_spans(micro32, dev, **opts) == spans
    _same(whisper.transcribe(micro32, dev, skip_silence=opts, temperature=0.0, language="en"), got)
    # a path: the file is ingested on the device and the detector reads it there
    assert whisper.speech_spans(micro32, JFK) == [(0.0, 11.0)]


def test_silent_file_gives_the_empty_result(micro32):
    import whisper
    zeros = np.zeros(16000 * 4, np.float32)
    before = micro32.ctx.stats()
    assert whisper.transcribe(micro32, zeros, skip_silence=True, language="en") == \
        dict(text="", segments=[], language="en", speech_spans=[])
    assert whisper.transcribe(micro32, zeros, skip_silence=True)["language"] is None  # nothing to probe
    after = micro32.ctx.stats()
    assert after["encode_windows"] == before["encode_windows"]  # nothing was encoded
    assert after["mel_ms"] == before["mel_ms"]  # the detector ran first: no mel either


def test_batch_equals_the_per_file_calls(micro32, fixture, jfk):
    import whisper
    files = [fixture, jfk, np.zeros(16000 * 4, np.float32)]
    for kw in (dict(language="en"), dict(language="en", condition_on_previous_text=False), dict()):
        batch = whisper.transcribe_batch(micro32, files, skip_silence=True, temperature=0.0, **kw)
        assert len(batch) == 3
        for got, audio in zip(batch, files):
            ref = whisper.transcribe(micro32, audio, skip_silence=True, temperature=0.0, **kw)
            _same(got, ref)
            assert got["speech_spans"] == ref["speech_spans"]
        assert [r["speech_spans"] for r in batch] == [[(2.66, 14.40)], [(0.0, 11.0)], []]
        assert batch[2]["segments"] == [] and batch[2]["text"] == ""
        assert batch[0]["segments"] and batch[1]["segments"]


def test_language_probe_starts_at_the_first_span(micro32, fixture, monkeypatch):
    """The detected language is ``detect_language`` of the mel window that starts at the first
    span.  Random weights may name the same language for two windows, so the window that
    is probed is checked as well: in transcribe() the mel handed to ``detect_language``, in
    transcribe_batch() the frames encoded for the probe."""
    import importlib

    import whisper
    from whisper.decoding import detect_language
    T, multifile = importlib.import_module("whisper.transcribe"), importlib.import_module("whisper.multifile")
    mel = whisper.log_mel_spectrogram(fixture, 80, padding=whisper.audio.N_SAMPLES)
    windows = {first: whisper.pad_or_trim(mel[:, first:first + 3000], 3000) for first in (266, 0)}
    langs = {}
    for first, window in windows.items():
        _, probs = detect_language(micro32, window)
        langs[first] = max(probs, key=probs.get)
    print("language at the first span / at frame 0:", langs)
    assert not np.array_equal(windows[266], windows[0])
    probed = []
    monkeypatch.setattr(T, "detect_language", lambda m, seg: (probed.append(np.array(seg)), detect_language(m, seg))[1])
    assert whisper.transcribe(micro32, fixture, skip_silence=True, temperature=0.0)["language"] == langs[266]
    assert whisper.transcribe(micro32, fixture, temperature=0.0)["language"] == langs[0]
    assert len(probed) == 2 and np.array_equal(probed[0], windows[266]) and np.array_equal(probed[1], windows[0])
    encoded = []
    real = multifile.language_probs
    monkeypatch.setattr(multifile, "language_probs",
                        lambda m, slot, tok: (encoded.append(m._last_windows), real(m, slot, tok))[1])
    out = whisper.transcribe_batch(micro32, [fixture, fixture[48000:]], skip_silence=True, temperature=0.0)
    assert out[0]["language"] == langs[266]
    # file 0's probe starts 266 frames into its mel; file 1 starts with the speech, its span at 0
    n0 = (len(fixture) + whisper.audio.N_SAMPLES) // 160
    assert out[1]["speech_spans"][0][0] == 0.0
    assert encoded[0] == ([266, n0], [3000, 3000])


def test_argument_errors(micro32, fixture):
    import whisper
    with pytest.raises(ValueError, match="clip_timestamps"):
        whisper.transcribe(micro32, fixture, skip_silence=True, clip_timestamps=[0.0, 5.0], language="en")
    with pytest.raises(ValueError, match="sharded"):
        whisper.transcribe(micro32, fixture, skip_silence=True, _mel_prepared=(3000, 0, 3000), language="en")
    with pytest.raises(ValueError, match="clip_timestamps"):
        whisper.transcribe_batch(micro32, [fixture], skip_silence=True, clip_timestamps="0,5", language="en")
    with pytest.raises(ValueError, match="percentile"):
        whisper.transcribe(micro32, fixture, skip_silence=dict(percentile=0), language="en")
    with pytest.raises(ValueError, match="unknown"):
        whisper.speech_spans(micro32, fixture, threshold=1)
    dev = micro32.ctx.audio_ingest(fixture[:1600], 16000, 32, dst_offset=0)
    behind = micro32.ctx.audio_ingest(fixture[:1600], 16000, 32, dst_offset=dev.n_samples)
    with pytest.raises(ValueError, match="first resident"):
        whisper.speech_spans(micro32, behind)
