"""PCM ingest on the GPU (wh_audio_ingest): the device waveform is bit-identical to the
host's ``pcm_to_waveform`` — every comparison here is ``np.array_equal`` — across rates,
channel counts, sample widths, lengths around the filter's edges, clipping and outputs
whose input index passes 2^31; segments ingested back to back feed the resident
``log_mel_batch``; refused calls leave the context as it was; and a path given to
``transcribe`` / ``transcribe_batch`` gives what its host-loaded waveform gives."""
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN
from test_audio_ingest_host import RATES, ingest_lengths, ratio

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
PAD = 480000


def _ctx():
    from whisper.audio import _mel_context
    return _mel_context(0)


def _fresh_ctx():
    """A context of its own, so its audio buffer starts empty and has to grow."""
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    dims = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
                n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)
    ctx = HipContext(dims, device=0, dtype="fp32", max_windows=1, max_group=1)
    ctx.set_mel_filters(80, mel_filters(None, 80))
    return ctx


def _pcm(rng, n, ch, bits):
    lim = 1 << (bits - 1)
    return rng.integers(-lim, lim, (n, ch), dtype=np.int16 if bits <= 16 else np.int32)


def _check(ctx, pcm, rate, bits, what):
    from whisper.audio import pcm_to_waveform
    want = pcm_to_waveform(pcm, rate, bits)
    d = ctx.audio_ingest(pcm, rate, bits)
    assert d.n_samples == len(want) and d.offset == 0, what
    got = ctx.audio_read(0, d.n_samples)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


def _write_wav(path, pcm, rate):
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, np.int16).tobytes())


# ---------------------------------------------------------------- the samples
@pytest.mark.parametrize("rate", RATES + (16000,))
def test_small_shapes_equal_the_host(rate):
    """Lengths of 1 and 2 frames, around ``down`` and around the filter's reach, 1-3
    channels, 16-bit as int16 and 24-bit in int32; 16000 Hz mixes and quantises only."""
    ctx = _ctx()
    rng = np.random.default_rng(1000 + rate)
    for n in ingest_lengths(rate):
        for ch in (1, 2, 3):
            for bits in (16, 24):
                _check(ctx, _pcm(rng, n, ch, bits), rate, bits, (rate, n, ch, bits))


@pytest.mark.parametrize("rate", RATES)
def test_several_workgroups_with_a_ragged_last_one(rate):
    """About 1.5 s: tens of workgroups, the last one partly filled."""
    ctx = _ctx()
    rng = np.random.default_rng(2000 + rate)
    n = int(1.5 * rate) + 7
    up, down = ratio(rate)
    assert -(-n * up // down) % 1024 not in (0, 1023)
    _check(ctx, _pcm(rng, n, 2, 16), rate, 16, (rate, n, 2, 16))
    _check(ctx, _pcm(rng, n - 3, 3, 24), rate, 24, (rate, n - 3, 3, 24))


def test_full_scale_square_wave_clips_as_the_host_does():
    from whisper.audio import pcm_to_waveform
    n = 4801
    one = np.where(np.arange(n) % 74 < 37, 32767, -32768).astype(np.int16)
    pcm = np.stack([one, one], axis=1)
    want = pcm_to_waveform(pcm, 48000, 16)
    top, bottom = int((want == np.float32(32767 / 32768)).sum()), int((want == -1.0).sum())
    print(f"host clips {top} samples at the top rail, {bottom} at the bottom")
    assert top > 100 and bottom > 100  # the filter overshoots full scale: the host result does clip
    _check(_ctx(), pcm, 48000, 16, "square wave")


def test_input_index_past_2_to_31():
    """44.1 kHz: output k reads frames around k * 441 / 160, and k * 441 passes 2^31 at
    k = 4 869 615 — 13.5 M frames are the smallest file that gets there."""
    n = 13_500_000
    up, down = ratio(44100)
    assert (-(-n * up // down) - 1) * down > 2 ** 31
    pcm = np.random.default_rng(31).integers(-32768, 32768, (n, 1), dtype=np.int16)
    _check(_ctx(), pcm, 44100, 16, "13.5 M frames")


# ---------------------------------------------------------------- jfk.flac
@pytest.fixture(scope="module")
def jfk_host():
    from whisper.audio import load_audio
    return load_audio(JFK)


def test_jfk_samples(jfk_host):
    import whisper
    ctx = _ctx()
    d = whisper.load_audio_device(ctx, JFK)
    assert d.ctx is ctx and d.n_samples == len(jfk_host) == 176000
    assert np.array_equal(ctx.audio_read(0, d.n_samples), jfk_host)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_jfk_log_mel_from_the_resident_samples(jfk_host, n_mels):
    import whisper
    ctx = _ctx()
    nf = ctx.log_mel(jfk_host, n_mels, padding=PAD)
    want = ctx.mel_read(n_mels, 0, nf)
    ctx.mel_write(np.zeros((80, 8), np.float32))
    d = whisper.load_audio_device(ctx, JFK)
    assert ctx.log_mel_resident(d.n_samples, n_mels, padding=PAD) == nf
    assert np.array_equal(ctx.mel_read(n_mels, 0, nf), want)


# ---------------------------------------------------------------- segments
def test_three_segments_back_to_back(tmp_path, jfk_host):
    from whisper.audio import load_audio, read_pcm
    from whisper.backend_hip import HipBackendError
    rng = np.random.default_rng(77)
    wav = str(tmp_path / "s.wav")
    _write_wav(wav, _pcm(rng, 30011, 2, 16), 48000)
    arr = (rng.standard_normal(20003) * 0.1).astype(np.float32)  # not on the 16-bit grid
    assert not np.array_equal(arr * 32768, np.round(arr * 32768))
    host = [load_audio(wav), jfk_host, arr]
    ref = _ctx()
    base = ref.log_mel_batch(host, 80, padding=PAD)
    want_mel = [ref.mel_read(80, int(base[i]), int(base[i + 1] - base[i])) for i in range(3)]
    want_max = ref.mel_max_batch(3).copy()
    ctx = _fresh_ctx()
    try:
        # reserve = 0: the buffer grows under the second and third file, the earlier ones move along
        segs, off = [], 0
        for src in (read_pcm(wav), read_pcm(JFK), (arr, 16000, 32)):
            segs.append(ctx.audio_ingest(*src, dst_offset=off))
            off += segs[-1].n_samples
        assert [s.n_samples for s in segs] == [len(h) for h in host]
        assert [s.offset for s in segs] == [0, len(host[0]), len(host[0]) + len(host[1])]
        for s, h in zip(segs, host):
            assert np.array_equal(ctx.audio_read(s.offset, s.n_samples), h)
        assert ctx.audio_read(segs[2].offset, segs[2].n_samples).tobytes() == arr.tobytes()
        with pytest.raises(HipBackendError, match="resident"):
            ctx.log_mel_resident(segs[0].n_samples, 80, padding=PAD)  # three segments, not one
        for _ in range(2):  # the segments stay resident: a second call gives the same
            got = ctx.log_mel_batch_resident([s.n_samples for s in segs], 80, padding=PAD)
            assert np.array_equal(got, base)
            for i in range(3):
                assert np.array_equal(ctx.mel_read(80, int(base[i]), int(base[i + 1] - base[i])), want_mel[i]), i
            assert np.array_equal(ctx.mel_max_batch(3), want_max)
            ctx.mel_write(np.zeros((80, 8), np.float32))
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals
def test_refused_calls_leave_the_context_alone(jfk_host):
    import ctypes

    from whisper.audio import resample_filter
    from whisper.backend_hip import HipBackendError, _ptr
    ctx = _ctx()
    rng = np.random.default_rng(9)
    pcm = _pcm(rng, 9000, 2, 16)
    d = ctx.audio_ingest(pcm, 48000, 16)
    nf = ctx.log_mel_resident(d.n_samples, 80, padding=PAD)
    samples, mel = ctx.audio_read(0, d.n_samples), ctx.mel_read(80, 0, nf)
    up, down, taps = resample_filter(48000)
    n_out = ctypes.c_int64(-1)

    def raw(ptr=_ptr(pcm), fmt=0, n=len(pcm), ch=2, bits=16, up=up, down=down, taps=_ptr(taps), n_taps=len(taps), dst=0):
        ctx._check(ctx.lib.wh_audio_ingest(ctx.h, ptr, fmt, n, ch, bits, up, down, taps, n_taps, dst, 0,
                                           ctypes.byref(n_out)), "wh_audio_ingest")

    def untouched():
        assert n_out.value == -1
        assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
        assert np.array_equal(ctx.mel_read(80, 0, nf), mel)
        assert ctx.log_mel_resident(d.n_samples, 80, padding=PAD) == nf  # still the one segment

    for kw, msg in ((dict(dst=5), "dst_offset"), (dict(dst=d.n_samples + 1), "dst_offset"),
                    (dict(n_taps=len(taps) - 2), "n_taps"), (dict(taps=None), "n_taps"), (dict(ch=0), "channels"),
                    (dict(ptr=None), "pcm"), (dict(n=0), "n_frames"), (dict(fmt=3), "format"),
                    (dict(bits=17), "bits"), (dict(bits=0), "bits"), (dict(fmt=1, bits=33), "bits"),
                    (dict(up=0), "up"), (dict(down=0), "down"), (dict(fmt=2, ch=2), "WH_PCM_F32")):
        with pytest.raises(HipBackendError, match=msg):
            raw(**kw)
        untouched()
    with pytest.raises(HipBackendError, match="resident"):
        ctx.log_mel_batch_resident([d.n_samples - 1], 80, padding=PAD)
    untouched()
    with pytest.raises(HipBackendError, match="resident"):
        ctx.log_mel_batch_resident([d.n_samples, 4000], 80, padding=PAD)
    untouched()
    with pytest.raises(HipBackendError, match="audio_read"):
        ctx.audio_read(1, d.n_samples)
    untouched()

    # an upload after ingests leaves exactly one segment: the uploaded file
    ctx.audio_ingest(pcm, 48000, 16, dst_offset=d.n_samples)
    ctx.audio_upload(jfk_host[:5000])
    assert np.array_equal(ctx.audio_read(0, 5000), jfk_host[:5000])
    with pytest.raises(HipBackendError, match="audio_read"):
        ctx.audio_read(0, 5001)
    assert ctx.log_mel_resident(5000, 80, padding=PAD) == (5000 + PAD) // 160
    assert list(ctx.log_mel_batch_resident([5000], 80, padding=PAD)) == [0, (5000 + PAD) // 160]
    with pytest.raises(HipBackendError, match="dst_offset"):
        raw(dst=d.n_samples)


# ---------------------------------------------------------------- stage counters
def test_each_call_charges_its_own_stage_counters():
    """Which ``wh_stats`` counters a front-end call moves (strictly greater) and that every
    other one stays bit-equal, on a fresh context.  The FLAC device path starts its ingest
    with the PCM already on the device, so the copy interval it times is empty:
    ``ingest_copy_ms`` may stay or grow there, never shrink."""
    ctx = _fresh_ctx()
    flac = ("flac_upload_ms", "flac_parse_ms", "flac_restore_ms", "flac_gather_ms", "flac_resample_ms",
            "flac_index_ms")

    def charged(what, call, moves, may_grow=()):
        before = ctx.stats()
        out = call()
        after = ctx.stats()
        print(what, {k: (before[k], after[k]) for k in after if after[k] != before[k]})
        for k in after:
            if k in moves:
                assert after[k] > before[k], (what, k, before[k], after[k])
            elif k in may_grow:
                assert after[k] >= before[k], (what, k, before[k], after[k])
            else:
                assert after[k] == before[k], (what, k, before[k], after[k])
        return out

    try:
        rng = np.random.default_rng(5)
        host = (rng.standard_normal(8000) * 0.1).astype(np.float32)
        charged("log_mel", lambda: ctx.log_mel(host, 80, padding=PAD), {"mel_ms"})
        charged("audio_ingest s16", lambda: ctx.audio_ingest(_pcm(rng, 9000, 2, 16), 48000, 16),
                {"ingest_copy_ms", "ingest_kernel_ms"})
        charged("audio_ingest f32", lambda: ctx.audio_ingest(host, 16000, 32), {"ingest_copy_ms"})
        with open(JFK, "rb") as f:
            data = f.read()
        d = charged("flac_ingest", lambda: ctx.flac_ingest(data), set(flac), may_grow=("ingest_copy_ms",))
        assert d.decoded_on == "device" and d.n_samples == 176000
    finally:
        ctx.close()


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def wav_48k(tmp_path_factory):
    from whisper import synthetic as S
    a = S.synthetic_audio(6.0, seed=17)
    left = np.clip(np.round(a * 32768), -32768, 32767).astype(np.int16)
    pcm = np.stack([left, left[::-1] // 2], axis=1)
    path = str(tmp_path_factory.mktemp("ingest") / "synthetic_48k.wav")
    _write_wav(path, pcm, 48000)
    return path


SEG_KEYS = ("seek", "tokens", "start", "end", "temperature", "text")
# the same single-file schedule on the same samples: the window statistics are equal too
SAME_RUN_KEYS = SEG_KEYS + ("avg_logprob", "no_speech_prob", "compression_ratio")


def _same(got, ref, words=False, exact_words=True):
    """exact_words: both sides ran one file at a time (everything equal); otherwise a batch
    against single calls, compared as tests/test_gpu_multifile.py compares them."""
    assert got["language"] == ref["language"] and got["text"] == ref["text"]
    assert len(got["segments"]) == len(ref["segments"])
    for a, b in zip(got["segments"], ref["segments"]):
        for k in (SAME_RUN_KEYS if exact_words else SEG_KEYS):
            assert a[k] == b[k], (k, a[k], b[k])
        if words:
            assert [(w["word"], w["start"], w["end"]) for w in a["words"]] == \
                   [(w["word"], w["start"], w["end"]) for w in b["words"]]
            for wa, wb in zip(a["words"], b["words"]):
                # one file at a time both sides align with the same call: equal.  The batch
                # aligns a round's windows together: fp32 softmax sums in another order, the
                # bound tests/test_gpu_multifile.py holds the batch to (rel 1e-5)
                if exact_words:
                    assert wa["probability"] == wb["probability"]
                else:
                    assert wa["probability"] == pytest.approx(wb["probability"], rel=1e-5)


@pytest.mark.parametrize("words", [False, True], ids=["plain", "words"])
def test_transcribe_of_a_path_equals_its_host_waveform(micro32, wav_48k, words):
    import whisper
    from whisper.audio import load_audio
    kw = dict(temperature=0.0, language="en", word_timestamps=words)
    for path in (wav_48k, JFK):
        ref = whisper.transcribe(micro32, load_audio(path), **kw)
        got = whisper.transcribe(micro32, path, **kw)
        assert len(ref["segments"]) >= 1
        _same(got, ref, words)


@pytest.mark.parametrize("words", [False, True], ids=["plain", "words"])
def test_transcribe_batch_of_paths_and_arrays(micro32, wav_48k, words):
    import whisper
    from whisper import synthetic as S
    files = [JFK, S.synthetic_audio(7.0, seed=23), wav_48k]
    kw = dict(temperature=0.0, language="en", word_timestamps=words)
    singles = [whisper.transcribe(micro32, f, **kw) for f in files]
    batch = whisper.transcribe_batch(micro32, files, **kw)
    assert len(batch) == 3
    for got, ref in zip(batch, singles):
        _same(got, ref, words, exact_words=False)
