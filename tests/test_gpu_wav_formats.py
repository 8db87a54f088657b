"""WAV decoded from its bytes on the GPU (wh_wav_ingest): for every sample encoding the device
waveform is bit-identical to the host twin (``wav_samples`` + ``pcm_to_waveform``) — every
comparison here is ``np.array_equal`` — across rates, channel counts, lengths around the
filter's edges, every byte phase of 24-bit samples, float edge values and all G.711 codes;
WAV, FLAC and PCM segments ingested back to back feed the resident ``log_mel_batch``; refused
calls leave the context as it was; only the two ingest counters move; and a WAV path given to
``transcribe`` / ``transcribe_batch`` gives what its host-loaded waveform gives."""
import ctypes
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN
from test_audio_ingest_host import RATES, ingest_lengths, ratio
from wav_fixture import ENCODINGS, encode, random_values, wav_bytes

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
PAD = 480000
ALL_RATES = tuple(sorted(set(RATES) | {8000, 16000}))
DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
            n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)


def _ctx():
    from whisper.audio import _mel_context
    return _mel_context(0)


def _fresh_ctx():
    """A context of its own: its audio buffer starts empty and its counters at zero."""
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    ctx = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    ctx.set_mel_filters(80, mel_filters(None, 80))
    return ctx


def _host(data):
    """The definition: the file's samples expanded in numpy, then ``pcm_to_waveform``."""
    from whisper.audio import pcm_to_waveform, wav_info, wav_samples
    info = wav_info(data)
    pcm, bits = wav_samples(data, info)
    return pcm_to_waveform(pcm, info.sample_rate, bits)


def _check(ctx, data, what):
    want = _host(data)
    d = ctx.wav_ingest(data)
    assert d.n_samples == len(want) and d.offset == 0, what
    got = ctx.audio_read(0, d.n_samples)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


# ---------------------------------------------------------------- the samples
@pytest.mark.parametrize("rate", ALL_RATES)
def test_small_shapes_equal_the_host(rate):
    """Every encoding x 1-3 channels x lengths of 1 and 2 frames, around ``down`` and around
    the filter's reach; 16000 Hz mixes and quantises only, 8000 Hz has up = 2.  Two-channel
    files carry an extensible header and an odd LIST chunk, so the data chunk starts at
    another file offset (the device reads from the start of the data, not of the file)."""
    from wav_fixture import chunk
    ctx = _ctx()
    rng = np.random.default_rng(3000 + rate)
    for enc in ENCODINGS:
        for n in ingest_lengths(rate):
            for ch in (1, 2, 3):
                kw = dict(extensible=True, before_data=(chunk(b"LIST", b"abc"),)) if ch == 2 else {}
                data = wav_bytes(enc, encode(enc, random_values(rng, enc, n, ch)), ch, rate, **kw)
                _check(ctx, data, (enc, rate, n, ch))


@pytest.mark.parametrize("rate", [16000, 44100, 8000])
def test_s24_every_byte_phase(rate):
    """Frame counts 1..9 at 1 and 3 channels: a 24-bit span starts and ends at every phase of
    a dword, and the last sample's dword reaches past the data."""
    ctx = _ctx()
    rng = np.random.default_rng(24 + rate)
    for ch in (1, 3):
        for n in range(1, 10):
            vals = random_values(rng, "s24", n, ch)
            vals[-1, -1] = -(1 << 23)  # the last bytes are 00 00 80: what follows them must not leak in
            _check(ctx, wav_bytes("s24", encode("s24", vals), ch, rate), ("s24", rate, n, ch))


@pytest.mark.parametrize("enc,ch,rate", [("s24", 2, 44100), ("f32", 2, 48000), ("ulaw", 1, 8000)])
def test_several_workgroups_with_a_ragged_last_one(enc, ch, rate):
    """About 1.5 s: tens of workgroups, the last one partly filled."""
    n = int(1.5 * rate) + 7
    up, down = ratio(rate)
    n_out = -(-n * up // down)
    assert n_out > 20 * 1024 and n_out % 1024 not in (0, 1023)
    vals = random_values(np.random.default_rng(rate), enc, n, ch)
    _check(_ctx(), wav_bytes(enc, encode(enc, vals), ch, rate), (enc, ch, rate, n))


@pytest.mark.parametrize("enc", ["f32", "f64"])
@pytest.mark.parametrize("rate", [16000, 48000])
def test_float_edge_values(enc, rate):
    """NaN, +-Inf, +-1e30 and (f64) +-1e300 scattered in noise: non-finite counts as 0, the rest
    is clamped to +-256 before the channels are added."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1.0, 1.0, (4001, 2))
    edges = [np.nan, np.inf, -np.inf, 1e30, -1e30, 300.0, -256.5] + ([1e300, -1e300] if enc == "f64" else [])
    at = rng.choice(x.size, 40 * len(edges), replace=False)
    x.reshape(-1)[at] = np.tile(edges, 40)
    x[10] = (np.inf, np.nan)     # both channels of a frame
    x[11] = (1e30, 1e30)         # 256 + 256: the sum stays finite
    data = wav_bytes(enc, encode(enc, x), 2, rate)
    want = _host(data)
    assert np.isfinite(want).all() and (want == np.float32(32767 / 32768)).any() and (want == -1.0).any()
    _check(_ctx(), data, (enc, rate))


@pytest.mark.parametrize("enc", ["alaw", "ulaw"])
def test_g711_files_holding_all_256_codes(enc):
    rng = np.random.default_rng(711)
    codes = np.concatenate([np.arange(256), rng.permutation(256), np.arange(255, -1, -1)])
    for ch, rate in ((1, 16000), (1, 8000), (2, 8000)):
        data = wav_bytes(enc, encode(enc, codes.reshape(-1, ch)), ch, rate)
        if rate == 16000:  # no filter: the waveform is the table itself
            from whisper.audio import WAV_ALAW, WAV_ULAW, g711_table
            table = g711_table(WAV_ALAW if enc == "alaw" else WAV_ULAW)
            assert np.array_equal(_host(data), table[codes].astype(np.float32) / 32768)
        _check(_ctx(), data, (enc, ch, rate))


# ---------------------------------------------------------------- segments
@pytest.fixture(scope="module")
def jfk_host():
    from whisper.audio import load_audio
    return load_audio(JFK)


def test_wav_flac_and_pcm_segments_back_to_back(jfk_host):
    rng = np.random.default_rng(77)
    wav = wav_bytes("s24", encode("s24", random_values(rng, "s24", 30011, 2)), 2, 48000, extensible=True)
    pcm = rng.integers(-32768, 32768, (20003, 1), dtype=np.int16)
    from whisper.audio import pcm_to_waveform
    host = [_host(wav), jfk_host, pcm_to_waveform(pcm, 8000, 16)]
    ref = _ctx()
    base = ref.log_mel_batch(host, 80, padding=PAD)
    want_mel = [ref.mel_read(80, int(base[i]), int(base[i + 1] - base[i])) for i in range(3)]
    with open(JFK, "rb") as f:
        flac = f.read()
    ctx = _fresh_ctx()
    try:
        # reserve = 0: the buffer grows under the second and third file, the earlier ones move along
        segs = [ctx.wav_ingest(wav)]
        segs.append(ctx.flac_ingest(flac, dst_offset=segs[0].n_samples))
        segs.append(ctx.audio_ingest(pcm, 8000, 16, dst_offset=segs[0].n_samples + segs[1].n_samples))
        assert [s.n_samples for s in segs] == [len(h) for h in host]
        assert [s.offset for s in segs] == [0, len(host[0]), len(host[0]) + len(host[1])]
        for s, h in zip(segs, host):
            assert np.array_equal(ctx.audio_read(s.offset, s.n_samples), h)
        got = ctx.log_mel_batch_resident([s.n_samples for s in segs], 80, padding=PAD)
        assert np.array_equal(got, base)
        for i in range(3):
            assert np.array_equal(ctx.mel_read(80, int(base[i]), int(base[i + 1] - base[i])), want_mel[i]), i
        # and a WAV appended behind other segments
        again = ctx.wav_ingest(wav, dst_offset=sum(len(h) for h in host))
        assert again.offset == sum(len(h) for h in host)
        assert np.array_equal(ctx.audio_read(again.offset, again.n_samples), host[0])
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals
def test_refused_calls_leave_the_context_alone():
    from whisper.audio import resample_filter
    from whisper.backend_hip import HipBackendError, _ptr
    ctx = _ctx()
    rng = np.random.default_rng(9)
    data = wav_bytes("s24", encode("s24", random_values(rng, "s24", 9000, 2)), 2, 48000)
    buf = np.frombuffer(data, np.uint8)
    d = ctx.wav_ingest(data)
    nf = ctx.log_mel_resident(d.n_samples, 80, padding=PAD)
    samples, mel = ctx.audio_read(0, d.n_samples), ctx.mel_read(80, 0, nf)
    up, down, taps = resample_filter(48000)
    n_out = ctypes.c_int64(-1)

    def raw(ptr=_ptr(buf), n=len(buf), up=up, down=down, taps=_ptr(taps), n_taps=len(taps), dst=0, reserve=0,
            out=ctypes.byref(n_out)):
        ctx._check(ctx.lib.wh_wav_ingest(ctx.h, ptr, n, up, down, taps, n_taps, dst, reserve, out), "wh_wav_ingest")

    def untouched():
        assert n_out.value == -1
        assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
        assert np.array_equal(ctx.mel_read(80, 0, nf), mel)
        assert ctx.log_mel_resident(d.n_samples, 80, padding=PAD) == nf  # still the one segment

    for kw, msg in ((dict(n=30), "runs past the end"), (dict(n=11), "not a RIFF/WAVE"), (dict(n=44), "no whole frame"),
                    (dict(n_taps=len(taps) - 2), "n_taps"), (dict(taps=None), "n_taps"),
                    (dict(dst=5), "dst_offset"), (dict(dst=d.n_samples + 1), "dst_offset"),
                    (dict(ptr=None), "null data"), (dict(out=None), "n_out"), (dict(up=0), "up"),
                    (dict(down=0), "down"), (dict(reserve=-1), "reserve")):
        with pytest.raises(HipBackendError, match=msg):
            raw(**kw)
        untouched()
    bad = bytearray(data)
    bad[20] = 0x55  # the format tag
    with pytest.raises(HipBackendError, match="0x55"):
        ctx.wav_ingest(bytes(bad))
    untouched()
    raw(dst=d.n_samples)  # a good call still works: appended
    assert n_out.value == d.n_samples
    assert np.array_equal(ctx.audio_read(d.n_samples, d.n_samples), samples)


# ---------------------------------------------------------------- stage counters
def test_wav_ingest_moves_the_two_ingest_counters_and_nothing_else():
    ctx = _fresh_ctx()
    try:
        rng = np.random.default_rng(5)
        for enc, rate in (("s24", 48000), ("ulaw", 8000), ("f32", 16000)):
            data = wav_bytes(enc, encode(enc, random_values(rng, enc, 9000, 2)), 2, rate)
            before = ctx.stats()
            ctx.wav_ingest(data)
            after = ctx.stats()
            print(enc, {k: (before[k], after[k]) for k in after if after[k] != before[k]})
            for k in after:
                if k in ("ingest_copy_ms", "ingest_kernel_ms"):
                    assert after[k] > before[k], (enc, k, before[k], after[k])
                else:
                    assert after[k] == before[k], (enc, k, before[k], after[k])
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
def wav_paths(tmp_path_factory):
    """A 24-bit 48 kHz stereo WAV (extensible header, as writers emit above 16 bits), a mu-law
    8 kHz mono WAV and a plain 16-bit 48 kHz WAV, of seeded synthetic audio."""
    from whisper import synthetic as S
    from whisper.audio import WAV_ULAW, g711_table
    root = tmp_path_factory.mktemp("wavs")
    a = S.synthetic_audio(6.0, seed=17).astype(np.float64)
    left = np.clip(np.round(a * (1 << 23)), -(1 << 23), (1 << 23) - 1).astype(np.int64)
    s24 = str(root / "s24_48k.wav")
    with open(s24, "wb") as f:
        f.write(wav_bytes("s24", encode("s24", np.stack([left, left[::-1] // 2], axis=1)), 2, 48000, extensible=True))
    # mu-law: the nearest code of every second sample (the table is sorted after an argsort)
    table = g711_table(WAV_ULAW).astype(np.int64)
    order = np.argsort(table, kind="stable")
    lin = np.clip(np.round(S.synthetic_audio(12.0, seed=19)[::2] * 32768), -32768, 32767).astype(np.int64)
    pos = np.clip(np.searchsorted(table[order], lin), 1, 255)
    nearer = np.where(np.abs(table[order][pos - 1] - lin) <= np.abs(table[order][pos] - lin), pos - 1, pos)
    ulaw = str(root / "ulaw_8k.wav")
    with open(ulaw, "wb") as f:
        f.write(wav_bytes("ulaw", encode("ulaw", order[nearer].reshape(-1, 1)), 1, 8000))
    plain = str(root / "s16_48k.wav")
    with wave.open(plain, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(np.clip(np.round(S.synthetic_audio(5.0, seed=21) * 32768), -32768, 32767).astype("<i2").tobytes())
    return dict(s24=s24, ulaw=ulaw, plain=plain)


SEG_KEYS = ("seek", "tokens", "start", "end", "temperature", "text")
# the same single-file schedule on the same samples: the window statistics are equal too
SAME_RUN_KEYS = SEG_KEYS + ("avg_logprob", "no_speech_prob", "compression_ratio")


def _same(got, ref, keys):
    assert got["language"] == ref["language"] and got["text"] == ref["text"]
    assert len(got["segments"]) == len(ref["segments"])
    for a, b in zip(got["segments"], ref["segments"]):
        for k in keys:
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("which", ["s24", "ulaw"])
def test_transcribe_of_a_wav_path_equals_its_host_waveform(micro32, wav_paths, which):
    import whisper
    from whisper.audio import ingest_source, load_audio
    path = wav_paths[which]
    assert len(ingest_source(path)[0]) == 2  # the route under test: bytes to wav_ingest
    kw = dict(temperature=0.0, language="en")
    ref = whisper.transcribe(micro32, load_audio(path), **kw)
    got = whisper.transcribe(micro32, path, **kw)
    assert len(ref["segments"]) >= 1
    _same(got, ref, SAME_RUN_KEYS)


def test_transcribe_batch_of_wav_flac_array_and_plain_wav(micro32, wav_paths):
    import whisper
    from whisper import synthetic as S
    files = [wav_paths["s24"], JFK, S.synthetic_audio(7.0, seed=23), wav_paths["plain"]]
    kw = dict(temperature=0.0, language="en")
    singles = [whisper.transcribe(micro32, f, **kw) for f in files]
    batch = whisper.transcribe_batch(micro32, files, **kw)
    assert len(batch) == 4
    for got, ref in zip(batch, singles):
        _same(got, ref, SEG_KEYS)  # the comparison of tests/test_gpu_multifile.py


def test_skip_silence_on_the_24_bit_path_equals_its_host_waveform(micro32, wav_paths):
    import whisper
    from whisper.audio import load_audio
    kw = dict(temperature=0.0, language="en", skip_silence=True)
    ref = whisper.transcribe(micro32, load_audio(wav_paths["s24"]), **kw)
    got = whisper.transcribe(micro32, wav_paths["s24"], **kw)
    assert got["speech_spans"] == ref["speech_spans"]
    _same(got, ref, SAME_RUN_KEYS)
