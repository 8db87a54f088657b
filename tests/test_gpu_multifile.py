"""transcribe_batch on the GPU (micro model): the segmented log-mel is bit-identical per
file to the single-file one, the batch of files equals the CPU oracle and the loop of
per-file transcribe() calls segment for segment in fp32 (lanes refilling, fallback,
prompts, word timestamps, clips, per-file languages), and runs in fp16."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


def _audio(seconds, seed, scale=1.0):
    from whisper import synthetic as S
    return (S.synthetic_audio(seconds, seed=seed) * np.float32(scale)).astype(np.float32)


# ---------------------------------------------------------------- 1, 2: the segmented log-mel
MEL_LENGTHS = (300, 12345, 16000, 48007)  # shorter than a frame block; not / exactly multiples of 160
MEL_SCALES = (1.0, 0.01, 10.0, 1.0)       # a shared maximum would mis-floor the quiet file


@pytest.fixture(scope="module")
def mel_files():
    from whisper import synthetic as S
    long = S.synthetic_audio(4.0, seed=31)
    return [(long[o:o + n] * np.float32(s)).astype(np.float32)
            for o, n, s in zip((0, 1000, 3000, 5000), MEL_LENGTHS, MEL_SCALES)]


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("padding", [480000, 0])
def test_batch_mel_is_bit_identical_per_file(mel_files, n_mels, padding):
    """Both paths do the same fp32 arithmetic per frame and a max does not depend on the
    order, so the bound is equality."""
    from whisper.audio import _mel_context
    ctx = _mel_context(0)
    alone, maxes = [], []
    for a in mel_files:
        nf = ctx.log_mel(a, n_mels, padding=padding)
        assert nf == (len(a) + padding) // 160
        alone.append(ctx.mel_read(n_mels, 0, nf))
        maxes.append(ctx.mel_max())
    base = ctx.log_mel_batch(mel_files, n_mels, padding=padding)
    assert base[0] == 0 and list(np.diff(base)) == [m.shape[1] for m in alone]
    got_max = ctx.mel_max_batch(len(mel_files))
    for i, ref in enumerate(alone):
        got = ctx.mel_read(n_mels, int(base[i]), ref.shape[1])
        assert np.array_equal(got, ref), (i, float(np.abs(got - ref).max()))
        assert got_max[i] == np.float32(maxes[i]), (i, got_max[i], maxes[i])
    assert len({float(x) for x in got_max}) > 1  # the files' maxima do differ


def test_batch_mel_state_hygiene(mel_files):
    from whisper.audio import _mel_context
    from whisper.backend_hip import HipBackendError
    ctx = _mel_context(0)
    a = mel_files[3]
    nf = ctx.log_mel(a, 80, padding=480000)
    before = ctx.mel_read(80, 0, nf)
    ctx.audio_upload(a)
    assert ctx.log_mel_resident(len(a), 80, padding=480000) == nf
    ctx.log_mel_batch(mel_files, 80, padding=480000)
    # the concatenated upload took the resident buffer: no file's length is resident now
    for n in (len(a), len(mel_files[0]), sum(len(x) for x in mel_files)):
        with pytest.raises(HipBackendError, match="resident"):
            ctx.log_mel_resident(n, 80, padding=480000)
    with pytest.raises(HipBackendError, match="already normalised"):
        ctx.mel_normalize(0.0)  # one max for a mel of several files: refused
    assert ctx.log_mel(a, 80, padding=480000) == nf
    assert np.array_equal(ctx.mel_read(80, 0, nf), before)
    with pytest.raises(HipBackendError, match="batch"):
        ctx.mel_max_batch(4)  # the mel is a single file's again
    with pytest.raises(HipBackendError, match=r"file 2\b"):
        ctx.log_mel_batch([mel_files[0], mel_files[1], np.zeros(0, np.float32), mel_files[2]], 80, padding=480000)
    with pytest.raises(HipBackendError, match=r"file 1\b"):
        ctx.log_mel_batch([mel_files[1], mel_files[0][:150]], 80, padding=0)  # n + padding <= 200
    with pytest.raises(HipBackendError, match=r"n_files = 0"):
        ctx.log_mel_batch([], 80, padding=480000)
    with pytest.raises(HipBackendError, match="filters"):
        ctx.log_mel_batch(mel_files, 96, padding=480000)
    # a refused call launched nothing and left the context's mel as it was
    assert np.array_equal(ctx.mel_read(80, 0, nf), before)


# ---------------------------------------------------------------- 3: the CPU oracle
@pytest.fixture(scope="module")
def oracle_files():
    return [_audio(8.0, 11), _audio(33.0, 12, 0.01), _audio(0.5, 13)]


@pytest.fixture(scope="module")
def oracle_model():
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = S.MODEL_DIMS["micro"]
    return R.OracleWhisper(dims, S.synthetic_state_dict(dims, 0))


@pytest.mark.parametrize("kw", [dict(), dict(beam_size=5, condition_on_previous_text=False)],
                         ids=["defaults", "beam5_nocond"])
def test_batch_matches_oracle(micro32, oracle_model, oracle_files, kw):
    import whisper
    from oracle import ref_whisper as R
    out = whisper.transcribe_batch(micro32, oracle_files, temperature=0.0, language="en", **kw)
    assert len(out) == len(oracle_files)
    for i, (audio, got) in enumerate(zip(oracle_files, out)):
        ref = R.transcribe(oracle_model, audio, **kw)
        print(f"file {i}: seeks {[s['seek'] for s in ref]}")
        assert [s["tokens"] for s in got["segments"]] == [s["tokens"] for s in ref], i
        assert [s["seek"] for s in got["segments"]] == [s["seek"] for s in ref], i
        assert got["language"] == "en"
    assert len(out[1]["segments"]) >= 2 and out[2] == dict(text="", segments=[], language="en")


# ---------------------------------------------------------------- 4: the loop of transcribe() calls
LANE_SECONDS = (3, 31, 65, 12, 0.5, 45)  # max_windows = 4: two files wait; 1, 2, 3, 1, 0, 2 windows


@pytest.fixture(scope="module")
def lane_files():
    return [_audio(s, 40 + i, 0.05 if i == 3 else 1.0) for i, s in enumerate(LANE_SECONDS)]


SEG_KEYS = ("seek", "tokens", "start", "end", "temperature", "text")
LANE_CASES = {
    "defaults": dict(temperature=0.0),
    # the greedy text of random weights repeats itself (compression ratios of 33 and more), so
    # the T = 0 result of a window is over this threshold and the window is sampled at 0.4
    "fallback": dict(temperature=(0.0, 0.4), compression_ratio_threshold=2.0),
    "carried_prompt": dict(temperature=0.0, initial_prompt="hello", carry_initial_prompt=True),
    "words": dict(temperature=0.0, word_timestamps=True),
    "words_hallucination": dict(temperature=0.0, word_timestamps=True, hallucination_silence_threshold=2.0),
    "clips": dict(temperature=0.0),
}
LANE_CLIPS = ["0", "0,2", [5.0, 25.0, 40.0], "1,11", "0", [0.0, 10.0, 20.0, 45.0]]


def _reseed(monkeypatch):
    """Sampling is seeded by a process counter (one draw per file): the same start for both sides."""
    from whisper import decoding
    monkeypatch.setattr(decoding, "_seed_counter", itertools.count(1))


def _same(got, ref, words):
    assert got["language"] == ref["language"] and got["text"] == ref["text"]
    assert len(got["segments"]) == len(ref["segments"])
    for a, b in zip(got["segments"], ref["segments"]):
        for k in SEG_KEYS:
            assert a[k] == b[k], (k, a[k], b[k])
        if words:
            # the batch aligns a round's windows in one wh_align_batch call, the loop one window
            # per wh_align call: paths (so every word and its times) are equal; the token
            # probabilities are fp32 softmax values summed in another order, held to the bound
            # tests/test_gpu_words.py pins for the batched against the single alignment (rel 1e-5;
            # a word's probability is the mean of such values)
            assert [(w["word"], w["start"], w["end"]) for w in a["words"]] == \
                   [(w["word"], w["start"], w["end"]) for w in b["words"]]
            for wa, wb in zip(a["words"], b["words"]):
                assert wa["probability"] == pytest.approx(wb["probability"], rel=1e-5), (wa, wb)


@pytest.mark.parametrize("case", list(LANE_CASES))
def test_batch_equals_per_file_transcribe(micro32, lane_files, monkeypatch, case):
    import whisper
    kw = dict(LANE_CASES[case], language="en")
    per_file = [dict(clip_timestamps=c) for c in LANE_CLIPS] if case == "clips" else [dict()] * len(lane_files)
    _reseed(monkeypatch)
    loop = [whisper.transcribe(micro32, a, **kw, **pf) for a, pf in zip(lane_files, per_file)]
    _reseed(monkeypatch)
    extra = dict(clip_timestamps=LANE_CLIPS) if case == "clips" else {}
    batch = whisper.transcribe_batch(micro32, lane_files, **kw, **extra)
    assert len(batch) == len(lane_files)
    for got, ref in zip(batch, loop):
        _same(got, ref, words=kw.get("word_timestamps", False))
    nseg = [len(r["segments"]) for r in loop]
    print(f"{case}: segments per file {nseg}, temperatures "
          f"{sorted({s['temperature'] for r in loop for s in r['segments']})}")
    print("compression ratios", sorted({round(s["compression_ratio"], 2) for r in loop for s in r["segments"]}))
    assert nseg[4] == 0
    if case == "words_hallucination":
        # every word of a random-weight transcript has a probability far under 0.15, so every
        # segment is an anomaly between silences: the rules drop them all and only move the
        # seeks, in the batch as in the loop (compared above)
        assert all(r["text"] == "" for r in batch)
    else:
        assert sum(nseg) >= 6
    if case == "fallback":
        assert any(s["temperature"] > 0 for r in batch for s in r["segments"])
    # the context is left usable: one file alone still gives its earlier result
    _reseed(monkeypatch)
    next(whisper.decoding._seed_counter)  # file 1 drew the second seed in the loop
    _same(whisper.transcribe(micro32, lane_files[1], **kw, **per_file[1]), loop[1],
          words=kw.get("word_timestamps", False))


# ---------------------------------------------------------------- 5: per-file language
def test_per_file_language(micro32, lane_files):
    import whisper
    from whisper.decoding import detect_language
    files = [lane_files[0], lane_files[3], lane_files[1]]
    want = []
    for a in files:
        mel = whisper.log_mel_spectrogram(a, 80, padding=whisper.audio.N_SAMPLES)
        _, probs = detect_language(micro32, whisper.pad_or_trim(mel[:, :3000], 3000))
        want.append(max(probs, key=probs.get))
    out = whisper.transcribe_batch(micro32, files, temperature=0.0)
    print("detected", want)
    assert [r["language"] for r in out] == want
    langs = ["en", "de", "en"]
    out = whisper.transcribe_batch(micro32, files, temperature=0.0, language=langs)
    for got, a, lg in zip(out, files, langs):
        _same(got, whisper.transcribe(micro32, a, temperature=0.0, language=lg), words=False)
    assert out[1]["language"] == "de"


def test_argument_checks(micro32, lane_files):
    import whisper
    with pytest.raises(TypeError):
        whisper.transcribe_batch(micro32, [micro32.ctx.audio_upload(lane_files[0])], language="en")
    with pytest.raises(ValueError, match=r"audio 1\b"):
        whisper.transcribe_batch(micro32, [lane_files[0], np.zeros(0, np.float32)], language="en")
    with pytest.raises(ValueError, match="language"):
        whisper.transcribe_batch(micro32, lane_files[:2], language=["en"])


# ---------------------------------------------------------------- 6: fp16
def test_fp16_runs_with_segment_invariants(lane_files):
    """Segment-exact equality is an fp32 claim; in fp16 every file's result must still be
    a well-formed walk of that file: seeks inside its content and non-decreasing, and each
    segment's times ordered and inside the 30 s window that starts at its seek (the model
    may emit any timestamp of the window, whatever the file's length, so the window — not
    the file's end — is what the loop guarantees)."""
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp16", max_windows=4, max_group=5, synthetic=True)
    try:
        out = whisper.transcribe_batch(m, lane_files, temperature=0.0, language="en")
    finally:
        m.close()
    assert len(out) == len(lane_files)
    for r, sec in zip(out, LANE_SECONDS):
        seeks = [s["seek"] for s in r["segments"]]
        assert seeks == sorted(seeks) and all(0 <= k < round(sec * 100) for k in seeks)
        assert [s["id"] for s in r["segments"]] == list(range(len(seeks)))
        for s in r["segments"]:
            t0 = s["seek"] * 0.01
            assert t0 - 1e-6 <= s["start"] <= s["end"] <= t0 + 30.0 + 1e-6, s
    assert out[4]["segments"] == [] and sum(len(r["segments"]) for r in out) >= 6
