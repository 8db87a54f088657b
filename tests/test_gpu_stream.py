"""A resident stream on the GPU (wh_stream_*, whisper/streaming.py).

* Chunking invariance: however a recording is cut into appends, the samples the stream emits are
  bit for bit those of the one-shot ingest and of ``pcm_to_waveform`` — every comparison is
  ``np.array_equal`` — and every append emits exactly E(after) - E(before) samples.
* Trim moves the remainder unchanged and later appends stay seamless; refused calls leave the
  stream and the resident samples as they were; a foreign upload ends the stream.
* StreamingTranscriber: every update's hypothesis is what ``transcribe`` gives for the host
  samples of the same span with the same prompt; the updates do not depend on how the input was
  fed; the language is detected once."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_audio_ingest_host import ratio
from wav_fixture import CONTAINER, ENCODINGS, encode, random_values, wav_bytes

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
            n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: no other module's ingest ends these streams."""
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    c = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    c.set_mel_filters(80, mel_filters(None, 80))
    yield c
    c.close()


def E(n, rate, final=False):
    from whisper.audio import stream_emitted
    return stream_emitted(n, rate, final)


def history(rate):
    up, down = ratio(rate)
    return 0 if up == down else 2 * 10 * max(up, down) // up


def values(rng, enc, n, ch):
    v = random_values(rng, enc, n, ch)
    if enc == "f32":  # non-finite and out-of-range samples among the rest
        flat = v.reshape(-1)
        at = rng.choice(flat.size, 12, replace=False)
        flat[at] = np.tile([np.nan, np.inf, -np.inf, 1e30], 3)
    return v


def one_shot(ctx, enc, ch, rate, payload):
    """(device one-shot, host) waveforms of the recording whose data chunk is ``payload``."""
    from whisper.audio import pcm_to_waveform, wav_info, wav_samples
    data = wav_bytes(enc, payload, ch, rate)
    d = ctx.wav_ingest(data)
    dev = ctx.audio_read(0, d.n_samples)
    info = wav_info(data)
    pcm, bits = wav_samples(data, info)
    return dev, pcm_to_waveform(pcm, rate, bits)


def stream(ctx, enc, ch, rate, payload, sizes):
    """The recording appended in chunks of ``sizes`` frames, then finished: the resident samples.
    Every append must emit E(after) - E(before)."""
    fb = CONTAINER[enc] * ch
    raw = np.frombuffer(payload, np.uint8)
    assert sum(sizes) * fb == len(raw)
    ctx.stream_begin(ENCODINGS.index(enc), ch, rate)
    pos = 0
    for n in sizes:
        got = ctx.stream_append(raw[pos * fb:(pos + n) * fb], n)
        assert got == E(pos + n, rate) - E(pos, rate), (enc, ch, rate, pos, n, got)
        pos += n
    tail = ctx.stream_finish()
    total = E(pos, rate, True)
    assert tail == total - E(pos, rate)
    assert ctx.stream_info() == (pos, total, 0, True)
    return ctx.audio_read(0, total)


def chunkings(rng, n, h):
    """Ways to cut n frames: one chunk, random sizes up to twice the history, sizes straddling
    the history by one, and the random ones with empty appends in between."""
    def cut(sizes):
        out, left = [], n
        for s in sizes:
            s = min(s, left)
            out.append(s)
            left -= s
            if not left:
                return out
        raise AssertionError("sizes ran out")
    top = max(2 * h, 40)
    rand = cut(int(s) for s in rng.integers(1, top + 1, n))
    mid = h or 20  # 16 kHz keeps no history: any small size
    around = cut(max(1, mid + d) for _ in range(n) for d in (-1, 0, 1))
    gaps = [s for r in rand[:60] for s in (r, 0)] + rand[60:]
    return dict(one=[n], random=rand, straddle=around, gaps=gaps)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("enc", ["s16", "ulaw", "s24", "f32"])
@pytest.mark.parametrize("rate", [8000, 44100, 48000, 16000])
def test_any_chunking_gives_the_one_shot_samples(ctx, rate, enc, ch):
    rng = np.random.default_rng([rate, ENCODINGS.index(enc), ch])
    n = int(0.3 * rate) + 3
    v = values(rng, enc, n, ch)
    payload = encode(enc, v)
    dev, host = one_shot(ctx, enc, ch, rate, payload)
    assert np.array_equal(dev, host)
    for name, sizes in chunkings(rng, n, history(rate)).items():
        got = stream(ctx, enc, ch, rate, payload, sizes)
        bad = np.flatnonzero(got != dev) if got.shape == dev.shape else [-1]
        assert len(bad) == 0, (name, rate, enc, ch, len(bad), int(bad[0]))
    # all one-frame chunks, on the first 300 frames
    short = encode(enc, v[:300])
    dev, host = one_shot(ctx, enc, ch, rate, short)
    got = stream(ctx, enc, ch, rate, short, [1] * 300)
    assert np.array_equal(got, dev) and np.array_equal(got, host)


def test_frame_index_past_2_to_31(ctx):
    """44.1 kHz: k * 441 passes 2^31 at k = 4 869 615, inside the last of three unequal chunks of
    13.5 M frames (the size tests/test_gpu_audio_ingest.py uses for the same reason)."""
    n, rate = 13_500_000, 44100
    up, down = ratio(rate)
    pcm = np.random.default_rng(31).integers(-32768, 32768, (n, 1), dtype=np.int16)
    want = ctx.audio_read(0, ctx.audio_ingest(pcm, rate, 16).n_samples)
    sizes = [5_000_001, 7_999_990, 500_009]
    assert sum(sizes) == n and (E(n, rate) - 1) * down > 2 ** 31 > E(sizes[0] + sizes[1], rate) * down
    got = stream(ctx, "s16", 1, rate, pcm.tobytes(), sizes)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("rate,enc,ch", [(8000, "ulaw", 1), (44100, "s24", 2), (16000, "s16", 1)])
def test_trim_keeps_the_rest_and_later_appends_are_seamless(ctx, rate, enc, ch):
    rng = np.random.default_rng(rate)
    n = int(0.5 * rate)
    payload = encode(enc, values(rng, enc, n, ch))
    want, _ = one_shot(ctx, enc, ch, rate, payload)
    fb = CONTAINER[enc] * ch
    raw = np.frombuffer(payload, np.uint8)
    cuts = [0, n // 4, n // 2, 3 * n // 4, n]
    ctx.stream_begin(ENCODINGS.index(enc), ch, rate)
    dropped = resident = 0       # the resident segment is want[dropped:dropped + resident]

    def check():
        assert ctx.stream_info()[1:3] == (dropped + resident, dropped)
        assert np.array_equal(ctx.audio_read(0, resident), want[dropped:dropped + resident])
        with pytest.raises(Exception):
            ctx.audio_read(0, resident + 1)      # nothing is resident past the segment

    # (what to drop, as a share of the resident length): below half (the move overlaps itself),
    # above half, nothing
    for (a, b), share in zip(zip(cuts[:-1], cuts[1:]), (0.3, 0.8, 0.0, 0.45)):
        resident += ctx.stream_append(raw[a * fb:b * fb], b - a)
        check()
        drop = int(resident * share)
        ctx.stream_trim(drop)
        dropped += drop
        resident -= drop
        check()
        if resident:
            nf = ctx.log_mel_resident(resident, 80, padding=480000)   # the segment rule: one segment of this length
            assert nf == (resident + 480000) // 160
    resident += ctx.stream_finish()
    assert dropped + resident == len(want)
    check()
    ctx.stream_trim(resident // 3)               # trim after finish
    dropped += resident // 3
    resident -= resident // 3
    check()
    ctx.stream_trim(resident)                    # the whole length: an empty segment
    dropped, resident = dropped + resident, 0
    check()
    assert ctx.stream_info() == (n, len(want), len(want), True)


def _rc(ctx, fn, *args):
    rc = fn(ctx.h, *args)
    return rc, ctx.lib.wh_last_error().decode(errors="replace")


def test_refused_calls_change_nothing(ctx):
    from whisper.audio import resample_filter
    from whisper.backend_hip import _ptr
    lib = ctx.lib
    up, down, taps = resample_filter(44100)
    pcm = np.random.default_rng(2).integers(-32768, 32768, (5000, 2), dtype=np.int16)
    ctx.stream_begin(ENCODINGS.index("s16"), 2, 44100)
    n0 = ctx.stream_append(pcm.view(np.uint8).reshape(-1), 5000)
    before = (ctx.stream_info(), ctx.audio_read(0, n0), ctx.stats())
    n_out = ctypes.c_int64(-5)
    buf = _ptr(pcm)
    refusals = [
        (lib.wh_stream_begin, (8, 2, up, down, _ptr(taps), len(taps), 0), -7, "encoding"),
        (lib.wh_stream_begin, (-1, 2, up, down, _ptr(taps), len(taps), 0), -7, "encoding"),
        (lib.wh_stream_begin, (1, 0, up, down, _ptr(taps), len(taps), 0), -7, "channels"),
        (lib.wh_stream_begin, (1, 257, up, down, _ptr(taps), len(taps), 0), -7, "channels"),
        (lib.wh_stream_begin, (1, 2, 0, down, _ptr(taps), len(taps), 0), -7, "up"),
        (lib.wh_stream_begin, (1, 2, up, -3, _ptr(taps), len(taps), 0), -7, "down"),
        (lib.wh_stream_begin, (1, 2, up, down, _ptr(taps), len(taps) - 2, 0), -7, "n_taps"),
        (lib.wh_stream_begin, (1, 2, up, down, None, len(taps), 0), -7, "n_taps"),
        (lib.wh_stream_begin, (1, 2, up, down, _ptr(taps), len(taps), -1), -7, "reserve"),
        (lib.wh_stream_append, (None, 10, ctypes.byref(n_out)), -1, "data"),
        (lib.wh_stream_append, (buf, -1, ctypes.byref(n_out)), -7, "n_frames"),
        (lib.wh_stream_trim, (-1,), -7, "n_drop"),
        (lib.wh_stream_trim, (n0 + 1,), -7, "n_drop"),
    ]
    for fn, args, code, word in refusals:
        rc, msg = _rc(ctx, fn, *args)
        assert rc == code and "stream" in msg and word in msg, (fn.__name__, args[:4], rc, msg)
        after = (ctx.stream_info(), ctx.audio_read(0, n0), ctx.stats())
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and after[2] == before[2], fn.__name__
        assert n_out.value == -5
    # zero frames: a no-op, with or without a pointer
    assert ctx.stream_append(None, 0) == 0 and ctx.stream_append(pcm.view(np.uint8).reshape(-1), 0) == 0
    assert ctx.stream_info() == before[0]
    # only the two ingest counters move
    ctx.stream_append(pcm.view(np.uint8).reshape(-1), 5000)
    ctx.stream_trim(100)
    moved = {k for k, v in ctx.stats().items() if v != before[2][k]}
    assert moved == {"ingest_copy_ms", "ingest_kernel_ms"}
    # no more input after finish
    ctx.stream_finish()
    state = ctx.stream_info()
    rc, msg = _rc(ctx, lib.wh_stream_append, buf, 10, ctypes.byref(n_out))
    assert rc == -7 and "stream" in msg and "finish" in msg and ctx.stream_info() == state
    assert ctx.stream_finish() == 0 and ctx.stream_info() == state


def test_a_foreign_upload_ends_the_stream(ctx):
    from whisper.backend_hip import HipBackendError
    pcm = np.zeros(1600, np.int16)
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 16000)
    assert ctx.stream_append(pcm.view(np.uint8), 1600) == 1600
    up = np.linspace(-1, 1, 777, dtype=np.float32)
    ctx.audio_upload(up)
    for call in (lambda: ctx.stream_append(pcm.view(np.uint8), 1600), ctx.stream_finish,
                 lambda: ctx.stream_trim(0), ctx.stream_info):
        with pytest.raises(HipBackendError, match="no open stream.*audio_upload"):
            call()
    assert np.array_equal(ctx.audio_read(0, 777), up)
    # so does an ingest; a refused ingest does not
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 16000)
    ctx.stream_append(pcm.view(np.uint8), 1600)
    with pytest.raises(HipBackendError):
        ctx.audio_ingest(pcm.reshape(-1, 1), 16000, 16, dst_offset=5)
    assert ctx.stream_info() == (1600, 1600, 0, False)
    ctx.audio_ingest(pcm.reshape(-1, 1), 16000, 16)
    with pytest.raises(HipBackendError, match="no open stream.*audio_ingest"):
        ctx.stream_append(pcm.view(np.uint8), 1600)
    # and a new stream starts from nothing
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 16000)
    assert ctx.stream_info() == (0, 0, 0, False)


# ---------------------------------------------------------------- the transcriber
@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def jfk():
    """(24-bit stereo frames as bytes, the host waveform)."""
    from whisper.audio import load_audio, read_pcm
    pcm, rate, bits = read_pcm(JFK)
    assert (rate, bits, pcm.shape[1]) == (44100, 24, 2)
    return encode("s24", pcm), load_audio(JFK)


OPTS = dict(min_chunk=2.0, buffer_trim=4, max_buffer=6, temperature=0.0)


def run(model, data, piece, **kw):
    import whisper
    t = whisper.StreamingTranscriber(model, 44100, "s24", 2, **{**OPTS, **kw})
    ups = []
    for at in range(0, len(data), piece):
        ups += t.feed(data[at:at + piece])
    ups.append(t.finish())
    return t, ups


def comparable(u):
    d = dataclasses.asdict(u)
    d.pop("wall_ms")
    return d


@pytest.fixture(scope="module")
def jfk_run(micro32, jfk):
    """jfk.flac fed in 0.37 s pieces."""
    return run(micro32, jfk[0], int(0.37 * 44100) * 6, language="en")


def test_every_update_is_transcribe_of_its_span(micro32, jfk, jfk_run):
    import whisper
    t, ups = jfk_run
    W = jfk[1]
    n_frames = len(jfk[0]) // 6
    assert len(ups) == n_frames // 88200 + 1 and [u.final for u in ups] == [False] * (len(ups) - 1) + [True]
    trims = 0
    for k, u in enumerate(ups):
        s0, s1 = u.span
        # a decode after every min_chunk of input, the buffer inside one window
        assert s1 == (E((k + 1) * 88200, 44100) if not u.final else len(W)) and s1 - s0 <= 30 * 16000
        trims += k > 0 and s0 > ups[k - 1].span[0]
        ref = whisper.transcribe(micro32, W[s0:s1], language=u.language, initial_prompt=u.prompt,
                                 word_timestamps=True, temperature=0.0)
        got = u.result
        assert u.language == "en" and got["language"] == ref["language"] and got["text"] == ref["text"]
        assert [s["tokens"] for s in got["segments"]] == [s["tokens"] for s in ref["segments"]]
        for a, b in zip(got["segments"], ref["segments"]):
            assert (a["text"], a["start"], a["end"]) == (b["text"], b["start"], b["end"])
            assert [(w["word"], w["start"], w["end"]) for w in a["words"]] == \
                   [(w["word"], w["start"], w["end"]) for w in b["words"]]
            for wa, wb in zip(a["words"], b["words"]):
                assert wa["probability"] == pytest.approx(wb["probability"], rel=1e-3)
        # absolute times: the hypothesis' words, shifted by the buffer start
        hyp = [w for s in got["segments"] for w in s["words"]]
        assert all(any(c["word"] == w["word"] and c["start"] == w["start"] + s0 / 16000 for w in hyp)
                   for c in u.committed if not (u.forced or u.final))
    assert trims >= 1
    # the run is not an empty one: hypotheses have words and agreement commits some before the end
    assert all(any(s["words"] for s in u.result["segments"]) for u in ups)
    assert any(u.committed and not u.forced for u in ups[:-1])
    assert [w for u in ups for w in u.committed] == t.committed and t.pending == [] and ups[-1].tentative == []
    assert t.text == "".join(w["word"] for w in t.committed).strip()
    # the model context is the one the reference decodes took: the stream is over, and feed says why
    t2 = whisper.StreamingTranscriber(micro32, 44100, "s24", 2, language="en", **OPTS)
    t2.feed(jfk[0][:6000])
    whisper.transcribe(micro32, JFK, language="en", temperature=0.0)
    with pytest.raises(whisper.HipBackendError, match="no open stream.*ingest"):
        t2.feed(jfk[0][:6000])


def test_updates_do_not_depend_on_the_feed_split(micro32, jfk, jfk_run):
    _, pieces = jfk_run
    _, tenth = run(micro32, jfk[0], 4410 * 6, language="en")
    _, whole = run(micro32, jfk[0], len(jfk[0]), language="en")
    assert len(whole) == len(tenth) == len(pieces)
    for a, b, c in zip(whole, tenth, pieces):
        assert comparable(a) == comparable(b) == comparable(c)


def test_language_is_detected_once(micro32, jfk, monkeypatch):
    import importlib
    T = importlib.import_module("whisper.transcribe")
    calls = []
    detect = T.detect_language

    def counting(*a, **k):
        calls.append(1)
        return detect(*a, **k)
    monkeypatch.setattr(T, "detect_language", counting)
    t, ups = run(micro32, jfk[0][:5 * 88200 * 6], 30000, language=None)
    assert len(calls) == 1 and len(ups) == 6
    assert ups[0].language is not None and {u.language for u in ups} == {ups[0].language} == {t.language}
