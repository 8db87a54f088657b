"""WAV in every common encoding, host side (no GPU): ``wav_info`` (the RIFF/WAVE parser of
csrc/wh_wav.cpp) on plain and extensible headers, header variations and every refusal with
its message; the G.711 tables; ``load_audio`` through the numpy twin that defines what the
device computes; and how ``ingest_source`` routes such files.  The files are built in
``tmp_path`` with ``struct`` (tests/wav_fixture.py)."""
import struct
import wave

import numpy as np
import pytest

from wav_fixture import CONTAINER, ENCODINGS, GUID_TAIL, chunk, encode, expand, fmt_body, random_values, riff, wav_bytes


def _info(data):
    from whisper.audio import wav_info
    return wav_info(data)


def _payload(enc, n=7, ch=2, seed=0):
    return encode(enc, random_values(np.random.default_rng(seed), enc, n, ch))


# ---------------------------------------------------------------- wav_info
@pytest.mark.parametrize("extensible", [False, True], ids=["plain", "extensible"])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_wav_info_of_every_encoding(enc, extensible):
    for ch, rate, n in ((1, 8000, 5), (2, 44100, 7), (3, 48000, 1)):
        data = wav_bytes(enc, _payload(enc, n, ch), ch, rate, extensible=extensible)
        i = _info(data)
        assert ENCODINGS[i.encoding] == enc
        assert (i.channels, i.sample_rate, i.valid_bits, i.n_frames) == (ch, rate, 8 * CONTAINER[enc], n)
        assert i.data_offset == (12 + 8 + (40 if extensible else 16 if enc in ("u8", "s16", "s24", "s32") else 18) + 8)
        size = i.n_frames * ch * CONTAINER[enc]
        assert i.data_offset + size + (size & 1) == len(data)  # an odd data chunk has its pad byte


def test_wav_info_header_variations():
    pay = _payload("s24", 7, 2)
    plain = _info(wav_bytes("s24", pay, 2, 44100))
    # a LIST chunk of odd size (so a pad byte follows) and a fact chunk before the data
    d = wav_bytes("s24", pay, 2, 44100, before_data=(chunk(b"LIST", b"INFOabc"), chunk(b"fact", struct.pack("<I", 7))))
    i = _info(d)
    assert i[:4] == plain[:4] and i.n_frames == 7 and i.data_offset == plain.data_offset + 8 + 8 + 12
    assert d[i.data_offset:i.data_offset + 42] == pay
    # fmt with cbSize extras
    i = _info(wav_bytes("s24", pay, 2, 44100, extra=b"\1\2\3\4"))
    assert i[:4] == plain[:4] and i.n_frames == 7 and i.data_offset == plain.data_offset + 6
    # a second fmt chunk after the first is skipped
    d = riff(chunk(b"fmt ", fmt_body("s24", 2, 44100)), chunk(b"fmt ", fmt_body("u8", 1, 8000)), chunk(b"data", pay))
    assert _info(d)[:4] == plain[:4]
    # declared data size 0 and 0xFFFFFFFF: to the end of the file; larger than the file: what is there
    for size in (0, 0xFFFFFFFF, 4200):
        assert _info(wav_bytes("s24", pay, 2, 44100, data_size=size)).n_frames == 7
    # smaller than the file: the declared size
    assert _info(wav_bytes("s24", pay, 2, 44100, data_size=18)).n_frames == 3
    # a trailing partial frame is dropped (present or declared)
    assert _info(wav_bytes("s24", pay + b"\1\2\3\4\5", 2, 44100)).n_frames == 7
    assert _info(wav_bytes("s24", pay, 2, 44100, data_size=41)).n_frames == 6
    # 20 valid bits in a 24-bit container: reported, the encoding is the container's
    i = _info(wav_bytes("s24", pay, 2, 44100, extensible=True, valid_bits=20))
    assert (ENCODINGS[i.encoding], i.valid_bits) == ("s24", 20)
    i = _info(wav_bytes("s24", pay, 2, 44100, bits=20))
    assert (ENCODINGS[i.encoding], i.valid_bits) == ("s24", 20)
    # 256 channels are the limit
    assert _info(wav_bytes("u8", bytes(512), 256, 8000)).n_frames == 2


REFUSALS = {
    "no RIFF": (b"RIFX" + wav_bytes("s16", _payload("s16"), 2, 8000)[4:], "not a RIFF/WAVE"),
    "no WAVE": (wav_bytes("s16", _payload("s16"), 2, 8000)[:8] + b"AVI " + bytes(40), "not a RIFF/WAVE"),
    "short file": (b"RIFF\x04\0\0\0WAV", "not a RIFF/WAVE"),
    "RF64": (riff(chunk(b"ds64", bytes(28)), chunk(b"fmt ", fmt_body("s16", 2, 8000)), chunk(b"data", bytes(8)),
                  form=b"RF64"), "RF64"),
    "BW64": (riff(chunk(b"fmt ", fmt_body("s16", 2, 8000)), chunk(b"data", bytes(8)), form=b"BW64"), "BW64"),
    "data before fmt": (riff(chunk(b"data", bytes(8)), chunk(b"fmt ", fmt_body("s16", 2, 8000))), "before the fmt"),
    "short fmt": (riff(chunk(b"fmt ", fmt_body("s16", 2, 8000)[:14]), chunk(b"data", bytes(8))), "too short"),
    "tag 0x55": (wav_bytes("s16", bytes(8), 2, 8000, tag=0x55), "0x55"),
    "tag 0x11": (wav_bytes("u8", bytes(8), 2, 8000, tag=0x11, block_align=2), "0x11"),
    "extensible tag 0x55": (wav_bytes("s16", bytes(8), 2, 8000, extensible=True, tag=0x55), "0x55"),
    "bad SubFormat tail": (wav_bytes("s16", bytes(8), 2, 8000, extensible=True,
                                     guid_tail=GUID_TAIL[:13] + b"\x72"), "SubFormat"),
    "extensible cbSize": (wav_bytes("s16", bytes(8), 2, 8000, extensible=True, cb_size=20), "cbSize"),
    "block_align": (wav_bytes("s16", bytes(10), 2, 8000, block_align=5), "block_align"),
    "block_align 0": (wav_bytes("s16", bytes(10), 2, 8000, block_align=0), "block_align"),
    "float at 16 bits": (wav_bytes("s16", bytes(8), 2, 8000, tag=3), "float container of 2"),
    "pcm at 64 bits": (wav_bytes("f64", bytes(32), 2, 8000, tag=1), "PCM container of 8"),
    "alaw at 16 bits": (wav_bytes("s16", bytes(8), 2, 8000, tag=6), "A-law container of 2"),
    "bits and container": (wav_bytes("s24", bytes(12), 2, 8000, bits=16), "bits per sample"),
    "0 channels": (wav_bytes("s16", bytes(8), 0, 8000, block_align=2), "channels = 0"),
    "257 channels": (wav_bytes("u8", bytes(514), 257, 8000), "channels = 257"),
    "rate 0": (wav_bytes("s16", bytes(8), 2, 0), "sample rate"),
    "0 frames": (wav_bytes("s16", b"", 2, 8000), "no whole frame"),
    "less than a frame": (wav_bytes("s24", bytes(5), 2, 8000), "no whole frame"),
    "chunk past the end": (riff(chunk(b"fmt ", fmt_body("s16", 2, 8000)), chunk(b"LIST", bytes(6), size=4000),
                                chunk(b"data", bytes(8))), "runs past the end"),
    "fmt past the end": (riff(chunk(b"fmt ", fmt_body("s16", 2, 8000), size=60)), "runs past the end"),
    "no data": (riff(chunk(b"fmt ", fmt_body("s16", 2, 8000)), chunk(b"LIST", bytes(6))), "no data chunk"),
    "no fmt": (riff(chunk(b"LIST", bytes(6))), "no fmt chunk"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_wav_info_refusals(case):
    from whisper.backend_hip import HipBackendError
    data, msg = REFUSALS[case]
    with pytest.raises(HipBackendError, match=msg):
        _info(data)


def test_wav_info_of_every_prefix_and_empty():
    """No prefix of a valid file crashes the parser or reports frames that are not there."""
    from whisper.backend_hip import HipBackendError
    data = wav_bytes("f32", _payload("f32", 5, 2), 2, 48000, extensible=True, before_data=(chunk(b"LIST", b"abc"),))
    for n in range(len(data)):
        try:
            i = _info(data[:n])
        except HipBackendError:
            continue
        assert i.data_offset + i.n_frames * 8 <= n


def test_header_library_and_shim_have_the_entry_points():
    import ctypes
    import os
    import re

    from conftest import REPO
    from whisper import audio, backend_hip
    src = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in ("wh_wav_info", "wh_wav_last_error", "wh_wav_ingest"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in backend_hip._EXPORTS
    assert re.search(r"WH_WAV_U8 = 0, WH_WAV_S16, WH_WAV_S24, WH_WAV_S32, WH_WAV_F32, WH_WAV_F64, WH_WAV_ALAW, "
                     r"WH_WAV_ULAW", src)
    assert (audio.WAV_U8, audio.WAV_S24, audio.WAV_F32, audio.WAV_ULAW) == (0, 2, 4, 7)
    assert tuple(audio.WAV_ENCODINGS) == ENCODINGS


# ---------------------------------------------------------------- G.711
def test_g711_anchors_and_sums():
    from whisper.audio import WAV_ALAW, WAV_ULAW, g711_table
    u, a = g711_table(WAV_ULAW), g711_table(WAV_ALAW)
    assert u.dtype == a.dtype == np.int16 and u.shape == a.shape == (256,)
    assert [int(u[b]) for b in (0xFF, 0x7F, 0x80, 0x00, 0xE7)] == [0, 0, 32124, -32124, 260]
    assert [int(a[b]) for b in (0xD5, 0x55, 0xAA, 0x2A, 0x80)] == [8, -8, 32256, -32256, 5504]
    assert int(u.astype(np.int64).sum()) == 0 and int(a.astype(np.int64).sum()) == 0
    assert int(np.abs(u.astype(np.int64)).sum()) == 1532928
    assert int(np.abs(a.astype(np.int64)).sum()) == 1564672
    try:
        import audioop
    except ImportError:
        return
    codes = bytes(range(256))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2"), u)
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes, 2), "<i2"), a)


# ---------------------------------------------------------------- load_audio
def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_extensible_16_bit_equals_the_plain_file(tmp_path):
    from whisper.audio import load_audio, read_pcm
    pcm = np.random.default_rng(1).integers(-32768, 32768, (4801, 2), dtype=np.int16)
    plain = str(tmp_path / "plain.wav")
    with wave.open(plain, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(pcm.tobytes())
    ext = _write(tmp_path, "ext.wav", wav_bytes("s16", encode("s16", pcm), 2, 48000, extensible=True))
    got, rate, bits = read_pcm(ext)
    assert np.array_equal(got, pcm) and (rate, bits) == (48000, 16)
    assert np.array_equal(load_audio(ext), load_audio(plain))


@pytest.mark.parametrize("enc", ["u8", "s24", "s32", "alaw", "ulaw"])
@pytest.mark.parametrize("rate", [8000, 16000, 44100])
def test_integer_encodings_equal_pcm_to_waveform_of_the_expanded_integers(tmp_path, enc, rate):
    from whisper.audio import load_audio, pcm_to_waveform, read_pcm
    vals = random_values(np.random.default_rng(rate), enc, 1203, 2)
    if enc not in ("alaw", "ulaw"):  # the rails
        lim = 1 << (8 * CONTAINER[enc] - 1)
        vals[:4, 0] = (-lim, lim - 1, -1, 0)
    p = _write(tmp_path, "x.wav", wav_bytes(enc, encode(enc, vals), 2, rate, extensible=enc == "s24"))
    want, bits = expand(enc, vals)
    got, got_rate, got_bits = read_pcm(p)
    assert np.issubdtype(got.dtype, np.integer) and (got_rate, got_bits) == (rate, bits)
    assert np.array_equal(got, want)
    assert np.array_equal(load_audio(p), pcm_to_waveform(want.astype(np.int64), rate, bits))


def test_20_in_24_scales_by_the_container(tmp_path):
    """WAV left-justifies: a 20-bit sample v is stored as v << 4 and the container is the sample."""
    from whisper.audio import load_audio
    v20 = np.random.default_rng(2).integers(-(1 << 19), 1 << 19, (1601, 1), dtype=np.int64)
    p = _write(tmp_path, "x.wav", wav_bytes("s24", encode("s24", v20 << 4), 1, 16000, extensible=True, valid_bits=20))
    want = np.clip(np.rint(v20[:, 0] / float(1 << 19) * 32768.0), -32768, 32767) / 32768.0
    assert np.array_equal(load_audio(p), want.astype(np.float32))


@pytest.mark.parametrize("enc", ["f32", "f64"])
def test_float_file_on_the_16_bit_grid_is_returned_exactly(tmp_path, enc):
    from whisper.audio import load_audio, read_pcm
    grid = np.random.default_rng(3).integers(-32768, 32768, (1601, 1)) / 32768.0
    p = _write(tmp_path, "x.wav", wav_bytes(enc, encode(enc, grid), 1, 16000))
    pcm, rate, bits = read_pcm(p)
    assert pcm.dtype == np.float64 and pcm.shape == (1601, 1) and (rate, bits) == (16000, 0)
    got = load_audio(p)
    assert got.dtype == np.float32 and np.array_equal(got, grid[:, 0].astype(np.float32))


def test_float_edge_values_follow_the_rule(tmp_path):
    from whisper.audio import load_audio
    x = np.zeros((12, 2))
    x[:, 1] = 0.25
    x[:10, 0] = (np.nan, np.inf, -np.inf, 1e300, -1e300, 300.0, 0.5, -0.5, 255.0, -1e30)
    p = _write(tmp_path, "x.wav", wav_bytes("f64", encode("f64", x), 2, 16000))
    # NaN / Inf -> 0, then clamp to +-256, mean with the 0.25 of the other channel, clip to 16 bits
    left = np.array([0, 0, 0, 256, -256, 256, 0.5, -0.5, 255, -256, 0, 0])
    want = np.clip(np.rint((left + 0.25) / 2 * 32768), -32768, 32767) / 32768
    assert np.array_equal(load_audio(p), want.astype(np.float32))
    # float32 cannot hold 1e300: it is +Inf in the file, so 0
    with np.errstate(over="ignore"):
        y = x.astype(np.float32)
    assert y[3, 0] == np.inf and y[4, 0] == -np.inf
    p = _write(tmp_path, "y.wav", wav_bytes("f32", encode("f32", y), 2, 16000))
    left = np.array([0, 0, 0, 0, 0, 256, 0.5, -0.5, 255, -256, 0, 0])
    want = np.clip(np.rint((left + 0.25) / 2 * 32768), -32768, 32767) / 32768
    assert np.array_equal(load_audio(p), want.astype(np.float32))


def test_nine_channel_float_uses_channel_order_sums(tmp_path):
    """Values whose fp64 sum depends on the order: pairwise (``mean(axis=1)`` from 8 channels
    on) and left-to-right differ on many rows, and the definition is left-to-right."""
    from whisper.audio import load_audio, pcm_to_waveform
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (4001, 9)) * 10.0 ** rng.integers(-8, 1, (4001, 9))
    p = _write(tmp_path, "x.wav", wav_bytes("f64", encode("f64", x), 9, 16000, extensible=True))
    seq = np.zeros(len(x))
    for c in range(9):
        seq = seq + x[:, c]
    assert (seq != x.sum(axis=1)).any()  # numpy's own order is another one
    want = (np.clip(np.rint(seq / 9 * 32768), -32768, 32767) / 32768).astype(np.float32)
    assert np.array_equal(load_audio(p), want)
    assert np.array_equal(pcm_to_waveform(x, 16000, 0), want)


def test_unsupported_names_what_is_supported(tmp_path):
    from whisper.audio import load_audio
    p = tmp_path / "x.mp3"
    p.write_bytes(bytes(16))
    with pytest.raises(RuntimeError, match=r"\.flac and \.wav.*24.*float.*A-law.*mu-law.*extensible"):
        load_audio(str(p))
    q = _write(tmp_path, "adpcm.wav", wav_bytes("u8", bytes(8), 2, 8000, tag=0x11, block_align=2))
    with pytest.raises(RuntimeError, match=r"adpcm\.wav.*0x11.*supported: 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law"):
        load_audio(q)


# ---------------------------------------------------------------- ingest_source
@pytest.mark.parametrize("rate,frames", [(8000, 801), (44100, 4411), (48000, 4801)])
@pytest.mark.parametrize("enc", ["s24", "f32", "ulaw", "s16"])
def test_ingest_source_gives_the_bytes_and_the_planned_length(tmp_path, enc, rate, frames):
    """Every WAV but the plain 16-bit one stays bytes; 16-bit counts when its header is extensible."""
    from whisper.audio import ingest_source, load_audio, wav_info
    data = wav_bytes(enc, _payload(enc, frames, 2, seed=rate), 2, rate, extensible=enc == "s16")
    p = _write(tmp_path, "x.wav", data)
    for need_length in (False, True):
        source, length = ingest_source(p, need_length=need_length)
        assert isinstance(source, tuple) and len(source) == 2
        assert source[0] == data and source[1] == wav_info(data)
        assert length == len(load_audio(p)) == -(-frames * 16000 // rate)


@pytest.mark.parametrize("rate,frames", [(8000, 801), (44100, 4411), (48000, 4801)])
def test_ingest_source_of_a_plain_16_bit_wav_is_unchanged(tmp_path, rate, frames):
    from whisper.audio import ingest_source
    pcm = np.random.default_rng(5).integers(-32768, 32768, (frames, 2), dtype=np.int16)
    p = _write(tmp_path, "x.wav", wav_bytes("s16", encode("s16", pcm), 2, rate))
    source, length = ingest_source(p)
    assert len(source) == 3 and source[1:] == (rate, 16) and source[0].dtype == np.int16
    assert np.array_equal(source[0], pcm) and length == -(-frames * 16000 // rate)


def test_ingest_source_resamples_on_the_host_past_the_device_filter(tmp_path):
    from whisper.audio import ingest_source, load_audio
    p = _write(tmp_path, "x.wav", wav_bytes("s24", _payload("s24", 1601, 1), 1, 16001))
    source, length = ingest_source(p)
    assert isinstance(source, np.ndarray) and source.dtype == np.float32 and length == len(source)
    assert np.array_equal(source, load_audio(p))
