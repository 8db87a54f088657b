"""WAV files built byte by byte for the tests (``struct`` / numpy; Python's ``wave`` writes
only plain integer PCM): every sample encoding, plain and WAVE_FORMAT_EXTENSIBLE headers,
extra chunks, and the header fields set freely so that malformed files can be made."""
import struct

import numpy as np

ENCODINGS = ("u8", "s16", "s24", "s32", "f32", "f64", "alaw", "ulaw")  # WH_WAV_* order
CONTAINER = dict(u8=1, s16=2, s24=3, s32=4, f32=4, f64=8, alaw=1, ulaw=1)
TAG = dict(u8=1, s16=1, s24=1, s32=1, f32=3, f64=3, alaw=6, ulaw=7)
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def chunk(cid: bytes, body: bytes, size=None) -> bytes:
    """One RIFF chunk; ``size`` overrides the declared size.  Odd bodies get their pad byte."""
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def fmt_body(enc, channels, rate, *, extensible=False, valid_bits=None, tag=None, block_align=None, bits=None,
             extra=b"", guid_tail=GUID_TAIL, cb_size=None) -> bytes:
    container = CONTAINER[enc]
    tag = TAG[enc] if tag is None else tag
    bits = 8 * container if bits is None else bits
    align = container * channels if block_align is None else block_align
    head = struct.pack("<HIIHH", channels, rate, rate * align, align, bits)
    if extensible:
        ext = struct.pack("<HI", bits if valid_bits is None else valid_bits, 0) + struct.pack("<H", tag) + guid_tail
        return struct.pack("<H", 0xFFFE) + head + struct.pack("<H", 22 if cb_size is None else cb_size) + ext
    if extra or tag != 1:  # non-PCM formats carry cbSize
        return struct.pack("<H", tag) + head + struct.pack("<H", len(extra)) + extra
    return struct.pack("<H", tag) + head


def riff(*chunks: bytes, form=b"RIFF") -> bytes:
    body = b"WAVE" + b"".join(chunks)
    return form + struct.pack("<I", len(body) & 0xFFFFFFFF) + body


def wav_bytes(enc, payload: bytes, channels, rate, *, before_data=(), data_size=None, **fmt_kw) -> bytes:
    """A WAV file: ``fmt ``, the chunks of ``before_data``, then ``data`` holding ``payload``."""
    return riff(chunk(b"fmt ", fmt_body(enc, channels, rate, **fmt_kw)), *before_data,
                chunk(b"data", payload, data_size))


def encode(enc, values: np.ndarray) -> bytes:
    """The data-chunk bytes of ``values`` [frames][channels]: integers in the encoding's range
    (G.711: the codes themselves, uint8), floats for f32 / f64."""
    v = np.asarray(values)
    if enc == "u8":
        return (v + 128).astype(np.uint8).tobytes()
    if enc == "s16":
        return v.astype("<i2").tobytes()
    if enc == "s24":
        return v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if enc == "s32":
        return v.astype("<i4").tobytes()
    if enc in ("f32", "f64"):
        return v.astype("<f4" if enc == "f32" else "<f8").tobytes()
    return v.astype(np.uint8).tobytes()


def random_values(rng, enc, n, channels):
    """Values for ``encode`` that cover the encoding's whole range; floats around full scale."""
    if enc in ("alaw", "ulaw"):
        return rng.integers(0, 256, (n, channels), dtype=np.int64)
    if enc in ("f32", "f64"):
        return rng.uniform(-1.2, 1.2, (n, channels))
    lim = 1 << (8 * CONTAINER[enc] - 1)
    return rng.integers(-lim, lim, (n, channels), dtype=np.int64)


def expand(enc, values):
    """What ``read_pcm`` must return for ``encode(enc, values)``: (array, bits)."""
    from whisper.audio import WAV_ALAW, WAV_ULAW, g711_table
    v = np.asarray(values)
    if enc in ("alaw", "ulaw"):
        return g711_table(WAV_ALAW if enc == "alaw" else WAV_ULAW)[v], 16
    if enc == "f32":
        return v.astype(np.float32).astype(np.float64), 0
    if enc == "f64":
        return v.astype(np.float64), 0
    return v, 8 * CONTAINER[enc]
