"""The frame-parallel FLAC decoder on the host (no GPU): the fixture writer against the host
decoder that the STREAMINFO MD5 pins, the frame index (wh_flac_index), and the indexed decode
(wh_flac_decode_indexed, the CPU twin of the device path: the same csrc/wh_flacdev.h frame
code, chain and gather) against wh_flac_decode, sample for sample."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
from flac_fixture import CASES, case, crc8, false_header, tone, write_stream

JFK = os.path.join(GOLDEN, "jfk.flac")


@pytest.fixture(scope="module")
def jfk():
    with open(JFK, "rb") as f:
        return f.read()


def _md5_of(pcm, bps):
    """The MD5 STREAMINFO carries: interleaved little-endian samples of ceil(bps / 8) bytes."""
    nbytes = (bps + 7) // 8
    raw = np.ascontiguousarray(pcm, "<i4").view(np.uint8).reshape(-1, 4)[:, :nbytes]
    return hashlib.md5(raw.tobytes()).digest()


# ---------------------------------------------------------------- the writer
@pytest.mark.parametrize("name", CASES)
def test_fixture_stream_decodes_to_its_pcm(name):
    from whisper.backend_hip import decode_flac
    stream, offsets, pcm, bps = case(name)
    got, rate, bits = decode_flac(stream)
    assert bits == bps and got.shape == pcm.shape
    assert np.array_equal(got, pcm)


# ---------------------------------------------------------------- the index
def _check_index(stream, offsets, fields, true_offsets=None):
    from whisper.backend_hip import flac_info
    _, channels, bps, _ = flac_info(stream)
    assert len(offsets) >= 1 and np.all(np.diff(offsets) > 0)
    for off, (hdr, bs, chc, bits) in zip(offsets.tolist(), fields.tolist()):
        head = stream[off:off + hdr]
        assert head[0] == 0xFF and head[1] in (0xF8, 0xF9)
        assert crc8(head[:-1]) == head[-1]
        assert 1 <= bs <= 65536 and 0 <= chc <= 10 and (chc + 1 if chc < 8 else 2) == channels
        assert bits in (bps, 8, 12, 16, 20, 24, 32)
    if true_offsets is not None:
        assert set(true_offsets) <= set(offsets.tolist())
        assert offsets[0] == true_offsets[0]


@pytest.mark.parametrize("name", CASES)
def test_index_holds_every_true_frame(name):
    from whisper.backend_hip import flac_index
    stream, true_offsets, pcm, bps = case(name)
    offsets, fields = flac_index(stream)
    _check_index(stream, offsets, fields, true_offsets)
    at = {o: f for o, f in zip(offsets.tolist(), fields.tolist())}
    assert sum(at[o][1] for o in true_offsets) == len(pcm)
    assert all(at[o][3] == bps for o in true_offsets)


def test_index_of_jfk(jfk):
    from whisper.backend_hip import decode_flac_indexed, flac_index, flac_info
    offsets, fields = flac_index(jfk)
    _check_index(jfk, offsets, fields)
    total = flac_info(jfk)[3]
    first, last = 4, 0  # fLaC, then the metadata blocks up to the one flagged last
    while not last:
        last = jfk[first] & 0x80
        first += 4 + int.from_bytes(jfk[first + 1:first + 4], "big")
    assert offsets[0] == first
    raw = sum(1 for i in range(first, len(jfk) - 1) if jfk[i] == 0xFF and jfk[i + 1] in (0xF8, 0xF9))
    assert raw == 151
    # the chain holds (the indexed path ran) and jfk.flac has one block size (STREAMINFO's
    # minimum = maximum), so the frames on the chain are ceil(total / block size)
    pcm, _, _, path = decode_flac_indexed(jfk)
    bs = int.from_bytes(jfk[8:10], "big")
    assert path == "device" and len(pcm) == total and bs == int.from_bytes(jfk[10:12], "big") == fields[0, 1]
    frames = -(-total // bs)
    assert frames <= len(offsets) <= raw
    print(f"jfk.flac: {raw} sync patterns, {len(offsets)} candidates, {frames} frames")


# ---------------------------------------------------------------- the indexed decode
@pytest.mark.parametrize("name", CASES)
def test_indexed_decode_equals_the_host_decoder(name):
    from whisper.backend_hip import decode_flac, decode_flac_indexed
    stream = case(name)[0]
    want, rate, bits = decode_flac(stream)
    got, rate2, bits2, path = decode_flac_indexed(stream)
    assert path == "device", "the indexed path must run for a valid stream"
    assert (rate2, bits2) == (rate, bits) and got.dtype == np.int32
    assert np.array_equal(got, want)


def test_indexed_decode_of_jfk(jfk):
    from whisper.backend_hip import decode_flac, decode_flac_indexed
    want, _, bits = decode_flac(jfk)
    got, _, _, path = decode_flac_indexed(jfk)
    assert path == "device"
    assert np.array_equal(got, want)
    assert _md5_of(got, bits) == jfk[26:42]  # STREAMINFO's MD5: the last 16 of its 34 bytes


def test_planted_false_candidate():
    from whisper.backend_hip import decode_flac_indexed, flac_index
    stream, true_offsets, pcm, bps = case("planted_false_header")
    fake = false_header(2)
    at = stream.find(fake)
    offsets, fields = flac_index(stream)
    assert at in offsets.tolist() and at not in true_offsets
    assert len(offsets) == len(true_offsets) + 1
    got, _, _, path = decode_flac_indexed(stream)
    assert path == "device" and np.array_equal(got, pcm)


def test_unknown_total_goes_through_the_host_decoder():
    from whisper.backend_hip import decode_flac, decode_flac_indexed
    pcm = tone(600, 2, 16, seed=3)
    stream, _ = write_stream(pcm, 16, blocks=256, sub={"type": "fixed", "order": 2}, total=0)
    got, _, _, path = decode_flac_indexed(stream)
    assert path == "host"
    assert np.array_equal(got, decode_flac(stream)[0]) and np.array_equal(got, pcm)


def test_wrong_total_goes_through_the_host_decoder():
    from whisper.backend_hip import decode_flac, decode_flac_indexed
    pcm = tone(600, 2, 16, seed=4)
    stream, _ = write_stream(pcm, 16, blocks=256, sub={"type": "fixed", "order": 2}, total=700)
    got, _, _, path = decode_flac_indexed(stream)
    assert path == "host" and np.array_equal(got, decode_flac(stream)[0])


@pytest.mark.parametrize("name", ["fixed2", "lpc8_24bit_p15", "escape_24bit", "many_small_frames"])
def test_truncated_streams_raise_in_both_decoders(name):
    from whisper.backend_hip import HipBackendError, decode_flac, decode_flac_indexed
    stream, offsets = case(name)[:2]
    for cut in (offsets[-1] + 7, offsets[1] + 3, len(stream) - 1, len(stream) - 3):
        with pytest.raises(HipBackendError) as host:
            decode_flac(stream[:cut])
        with pytest.raises(HipBackendError) as indexed:
            decode_flac_indexed(stream[:cut])
        assert str(indexed.value).split(": ", 1)[1] == str(host.value).split(": ", 1)[1]
