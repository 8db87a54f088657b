"""FLAC decoded on the GPU (wh_flac_decode_device, wh_flac_ingest): the device PCM is the host
decoder's, sample for sample, for every coding tool the fixture writer can produce; every
device case asserts that the device path ran, so a silent fall-back cannot pass; streams
outside the device path go through the host decoder with its samples or its error; and a
FLAC segment between other segments feeds the resident log-mel like any other."""
import hashlib
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN
from flac_fixture import CASES, case, tone, write_stream

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
PAD = 480000


def _ctx():
    from whisper.audio import _mel_context
    return _mel_context(0)


def _fresh_ctx():
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    dims = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
                n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)
    ctx = HipContext(dims, device=0, dtype="fp32", max_windows=1, max_group=1)
    ctx.set_mel_filters(80, mel_filters(None, 80))
    return ctx


@pytest.fixture(scope="module")
def jfk():
    with open(JFK, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def jfk_host():
    from whisper.audio import load_audio
    return load_audio(JFK)


# ---------------------------------------------------------------- the decoder alone
@pytest.mark.parametrize("name", CASES)
def test_device_decode_equals_the_host_decoder(name):
    """One case per subframe type and FIXED order, LPC orders 1 / 8 / 12 / 32 at 24 bits with
    15-bit coefficients, every channel assignment, wasted bits, escape partitions, Rice method
    1, the highest partition order, block size 16 with order 4, the explicit block-size forms
    and a one-sample last frame, 8 / 12 / 20-bit samples, full-scale values, 333 frames of
    16-64 samples with mixed stereo modes, and the planted false candidate (tests/flac_fixture.py)."""
    from whisper.backend_hip import decode_flac
    stream, _, pcm, bps = case(name)
    want, rate, bits = decode_flac(stream)
    got, rate2, bits2, path = _ctx().flac_decode_device(stream)
    assert path == "device"
    assert (rate2, bits2) == (rate, bits) and got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (name, bad.size, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())
    assert np.array_equal(got, pcm)


def test_many_small_frames_cross_waves_and_workgroups():
    stream, offsets, _, _ = case("many_small_frames")
    assert len(offsets) >= 300 and len(offsets) % 64 != 0 and (2 * len(offsets)) % 64 != 0


def test_jfk_pcm_and_md5(jfk):
    from whisper.backend_hip import decode_flac
    want, _, bits = decode_flac(jfk)
    got, _, _, path = _ctx().flac_decode_device(jfk)
    assert path == "device"
    assert np.array_equal(got, want)
    raw = np.ascontiguousarray(got, "<i4").view(np.uint8).reshape(-1, 4)[:, :(bits + 7) // 8]
    assert hashlib.md5(raw.tobytes()).digest() == jfk[26:42]


@pytest.mark.parametrize("name", ["fixed2", "mid_side_16bit", "mid_side_24bit", "bits_8", "independent_3ch"])
def test_ingest_of_a_stream_equals_the_host_waveform(name):
    """The int16 / int32 device PCM through the resampling kernel: the waveform of pcm_to_waveform."""
    from whisper.audio import pcm_to_waveform
    from whisper.backend_hip import decode_flac
    stream = case(name)[0]
    want = pcm_to_waveform(*decode_flac(stream))
    ctx = _ctx()
    d = ctx.flac_ingest(stream)
    assert d.decoded_on == "device" and d.n_samples == len(want) and d.offset == 0
    assert np.array_equal(ctx.audio_read(0, d.n_samples), want)


# ---------------------------------------------------------------- fall-backs
def test_unknown_total_goes_through_the_host_decoder():
    from whisper.audio import pcm_to_waveform
    from whisper.backend_hip import decode_flac
    pcm = tone(700, 2, 16, seed=3)
    stream, _ = write_stream(pcm, 16, rate=44100, blocks=256, sub={"type": "fixed", "order": 2}, total=0)
    ctx = _ctx()
    got, _, _, path = ctx.flac_decode_device(stream)
    assert path == "host" and np.array_equal(got, pcm) and np.array_equal(got, decode_flac(stream)[0])
    d = ctx.flac_ingest(stream)
    assert d.decoded_on == "host"
    assert np.array_equal(ctx.audio_read(0, d.n_samples), pcm_to_waveform(pcm, 44100, 16))


def test_truncated_stream_raises_the_host_error_and_leaves_the_context(jfk_host):
    from whisper.audio import pcm_to_waveform
    from whisper.backend_hip import HipBackendError, decode_flac
    ctx = _ctx()
    rng = np.random.default_rng(9)
    pcm = rng.integers(-32768, 32768, (9000, 2), dtype=np.int16)
    d = ctx.audio_ingest(pcm, 48000, 16)
    nf = ctx.log_mel_resident(d.n_samples, 80, padding=PAD)
    samples, mel = ctx.audio_read(0, d.n_samples), ctx.mel_read(80, 0, nf)
    stream, offsets = case("lpc8_24bit_p15")[:2]
    for cut in (offsets[-1] + 9, len(stream) - 1):
        with pytest.raises(HipBackendError) as host:
            decode_flac(stream[:cut])
        message = str(host.value).split(": ", 1)[1]
        for call in (lambda: ctx.flac_ingest(stream[:cut]), lambda: ctx.flac_decode_device(stream[:cut]),
                     lambda: ctx.flac_ingest(stream[:cut], dst_offset=d.n_samples)):
            with pytest.raises(HipBackendError) as dev:
                call()
            assert str(dev.value).split(": ", 1)[1] == message
            assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
            assert np.array_equal(ctx.mel_read(80, 0, nf), mel)
            assert ctx.log_mel_resident(d.n_samples, 80, padding=PAD) == nf  # still the one segment
    with pytest.raises(HipBackendError, match="dst_offset"):
        ctx.flac_ingest(stream, dst_offset=5)
    assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
    # a good ingest in the same context afterwards
    good = ctx.flac_ingest(stream)
    assert good.decoded_on == "device"
    assert np.array_equal(ctx.audio_read(0, good.n_samples), pcm_to_waveform(*decode_flac(stream)))


# ---------------------------------------------------------------- segments
def test_flac_segment_between_a_wav_and_an_array(tmp_path, jfk, jfk_host):
    from whisper.audio import load_audio, read_pcm
    rng = np.random.default_rng(77)
    wav = str(tmp_path / "s.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(rng.integers(-32768, 32768, (30011, 2), dtype=np.int16).tobytes())
    arr = (rng.standard_normal(20003) * 0.1).astype(np.float32)
    host = [load_audio(wav), jfk_host, arr]
    ref = _ctx()
    base = ref.log_mel_batch(host, 80, padding=PAD)
    want_mel = [ref.mel_read(80, int(base[i]), int(base[i + 1] - base[i])) for i in range(3)]
    ctx = _fresh_ctx()
    try:
        segs = [ctx.audio_ingest(*read_pcm(wav))]
        segs.append(ctx.flac_ingest(jfk, dst_offset=segs[0].n_samples))
        assert segs[1].decoded_on == "device"
        segs.append(ctx.audio_ingest(arr, 16000, 32, dst_offset=segs[0].n_samples + segs[1].n_samples))
        assert [s.n_samples for s in segs] == [len(h) for h in host]
        assert [s.offset for s in segs] == [0, len(host[0]), len(host[0]) + len(host[1])]
        for s, h in zip(segs, host):
            assert np.array_equal(ctx.audio_read(s.offset, s.n_samples), h)
        got = ctx.log_mel_batch_resident([s.n_samples for s in segs], 80, padding=PAD)
        assert np.array_equal(got, base)
        for i in range(3):
            assert np.array_equal(ctx.mel_read(80, int(base[i]), int(base[i + 1] - base[i])), want_mel[i]), i
    finally:
        ctx.close()


def test_load_audio_device_decodes_on_the_device(jfk_host):
    import whisper
    ctx = _ctx()
    d = whisper.load_audio_device(ctx, JFK)
    assert d.decoded_on == "device" and d.n_samples == len(jfk_host)
    assert np.array_equal(ctx.audio_read(0, d.n_samples), jfk_host)
