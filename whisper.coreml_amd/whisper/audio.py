"""Audio front end (reference whisper/audio.py:13-157), computed on the GPU.

``log_mel_spectrogram`` keeps the reference signature and semantics (right zero
padding, centred reflect-padded 400-point periodic-Hann STFT at hop 160, last
frame dropped, |X|^2, Slaney mel projection, log10 clamp, floor at max-8,
(x+4)/4) but the work runs in the HIP kernel ``k_mel_frames`` of
libwhisper_hip; the returned array is a host copy.  There is no CPU path.
"""

import os
import wave
from functools import lru_cache
from math import gcd
from typing import Optional, Union

import numpy as np

SAMPLE_RATE = 16000
N_FFT = 400
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE  # 480000
N_FRAMES = N_SAMPLES // HOP_LENGTH  # 3000
N_SAMPLES_PER_TOKEN = HOP_LENGTH * 2
FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH  # 100
TOKENS_PER_SECOND = SAMPLE_RATE // N_SAMPLES_PER_TOKEN  # 50


def load_audio(file: str, sr: int = SAMPLE_RATE) -> np.ndarray:
    """Mono float32 waveform at ``sr`` (audio.py:25-62).  The reference pipes the file
    through the ffmpeg CLI (``-ac 1 -ar sr -f s16le``), which neither this image nor
    the GPU box has.  Here: FLAC is decoded by the library's host FLAC reader
    (bit-exact, ``wh_flac_decode``), plain 16-bit PCM WAV by ``wave`` and every other WAV
    encoding (8 / 24 / 32-bit PCM, float, A-law, mu-law, extensible headers) by
    ``wav_info`` and ``wav_samples``; then, as ffmpeg's
    command line asks, channels are averaged to mono, the rate is converted to ``sr``
    (polyphase FIR, ``scipy.signal.resample_poly``) and the result is quantised to
    16-bit PCM and scaled by 1/32768.  ffmpeg's own resampling filter is not
    reproduced, so samples differ from the reference's in the low bits wherever the
    file's rate is not ``sr`` (parity unpinned there; exact for 16-bit files at ``sr``)."""
    return pcm_to_waveform(*read_pcm(file), sr)


def select_channels(channels, n_channels: int) -> list:
    """The channel indices a selection names in a file of ``n_channels`` channels: None or
    "split" is all of them, a sequence is itself (distinct ints in [0, n_channels), else
    ValueError)."""
    if channels is None or (isinstance(channels, str) and channels == "split"):
        return list(range(n_channels))
    if isinstance(channels, str):
        raise ValueError(f"channels: {channels!r} is not a selection")
    sel = [int(c) for c in channels]
    if not sel:
        raise ValueError("channels: the selection is empty")
    for c in sel:
        if c < 0 or c >= n_channels:
            raise ValueError(f"channels: {c} is not a channel of a file with {n_channels}")
    if len(set(sel)) != len(sel):
        raise ValueError(f"channels: {sel} repeats a channel")
    return sel


def load_audio_channels(file: str, channels=None) -> np.ndarray:
    """The file's channels as waveforms of their own, float32 ``[C][n]`` at 16 kHz: row k is
    ``pcm_to_waveform(pcm[:, [channels[k]]], rate, bits)`` of ``read_pcm(file)``, that is
    ``load_audio`` of a mono file holding only that channel.  ``channels``: a sequence of
    channel indices, None for all.  The device paths (``HipContext.*_ingest(channels=...)``)
    give the same samples bit for bit."""
    pcm, rate, bits = read_pcm(file)
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    sel = select_channels(channels, pcm.shape[1])
    return np.stack([pcm_to_waveform(pcm[:, [c]], rate, bits) for c in sel])


def read_pcm(file: str):
    """The file's samples as stored: (pcm [frames][channels], sample rate, bits per sample).
    FLAC gives int32 (``wh_flac_decode``), a plain 16-bit PCM WAV gives int16 (read with
    ``wave``).  Every other WAV goes through ``wav_info`` and ``wav_samples``: the integer
    and G.711 encodings give integers at 8 / 16 / 24 / 32 bits, the float encodings give
    ``(float64 [frames][channels], rate, 0)``."""
    low = file.lower()
    if low.endswith(".flac"):
        from .backend_hip import decode_flac
        with open(file, "rb") as f:
            return decode_flac(f.read())
    if low.endswith(".wav"):
        plain = _read_wav16(file)
        if plain is not None:
            return plain
        with open(file, "rb") as f:
            data = f.read()
        try:
            info = wav_info(data)
        except RuntimeError as e:
            raise RuntimeError(f"Failed to load audio: {file}: {e}") from None
        pcm, bits = wav_samples(data, info)
        return pcm, info.sample_rate, bits
    raise RuntimeError(f"Failed to load audio: {file}: without ffmpeg only .flac and .wav are supported (WAV: PCM at "
                       "8, 16, 24 or 32 bits, IEEE float at 32 or 64 bits, A-law, mu-law; plain or extensible header)")


def _read_wav16(file: str):
    """(int16 pcm, rate, 16) of a plain (format tag 1) 16-bit PCM WAV read with ``wave``; None
    for any WAV that ``wave`` does not take or that is not 16-bit."""
    try:
        with wave.open(file, "rb") as w:
            if w.getsampwidth() != 2:
                return None
            pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
            return pcm, w.getframerate(), 16
    except (wave.Error, EOFError):
        return None


WAV_U8, WAV_S16, WAV_S24, WAV_S32, WAV_F32, WAV_F64, WAV_ALAW, WAV_ULAW = range(8)  # WH_WAV_*
WAV_ENCODINGS = ("u8", "s16", "s24", "s32", "f32", "f64", "alaw", "ulaw")
WAV_CONTAINER = (1, 2, 3, 4, 4, 8, 1, 1)  # bytes per sample


def wav_info(data: bytes):
    """``wh_wav_info`` of a WAV file's bytes: ``WavInfo(encoding, channels, sample_rate,
    valid_bits, data_offset, n_frames)``, ``encoding`` one of ``WAV_*`` (include/whisper_hip.h
    has the parsing rules).  Raises ``HipBackendError`` with the parser's message."""
    from .backend_hip import wav_info as _wav_info
    return _wav_info(data)


@lru_cache(maxsize=None)
def g711_table(encoding: int) -> np.ndarray:
    """The 256 int16 values of the A-law / mu-law codes (ITU-T G.711, the formulas of
    include/whisper_hip.h; read-only)."""
    b = np.arange(256, dtype=np.int32)
    if encoding == WAV_ULAW:
        u = ~b & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 0x84) << e) - 0x84
        t = np.where(u & 0x80, -mag, mag)
    elif encoding == WAV_ALAW:
        a = b ^ 0x55
        e, m = (a >> 4) & 7, a & 15
        mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
        t = np.where(a & 0x80, mag, -mag)
    else:
        raise ValueError(f"encoding {encoding} is not G.711")
    t = t.astype(np.int16)
    t.setflags(write=False)
    return t


def wav_samples(data: bytes, info):
    """The samples of a WAV data chunk on the host, the definition the device reader matches:
    (pcm [frames][channels], bits).  U8 is ``byte - 128`` at 8 bits; S16 / S24 / S32 are
    little-endian two's complement at 16 / 24 / 32 bits (the whole container, whatever
    ``valid_bits`` says); A-law / mu-law expand to int16 at 16 bits; the float encodings give
    float64 with ``bits = 0``."""
    enc, ch = info.encoding, info.channels
    raw = np.frombuffer(data, np.uint8, info.n_frames * ch * WAV_CONTAINER[enc], info.data_offset).copy()
    if enc == WAV_U8:
        pcm, bits = raw.astype(np.int16) - 128, 8
    elif enc == WAV_S16:
        pcm, bits = raw.view("<i2"), 16
    elif enc == WAV_S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        pcm, bits = (v ^ 0x800000) - 0x800000, 24
    elif enc == WAV_S32:
        pcm, bits = raw.view("<i4"), 32
    elif enc in (WAV_F32, WAV_F64):
        pcm, bits = raw.view("<f4" if enc == WAV_F32 else "<f8").astype(np.float64), 0
    else:
        pcm, bits = g711_table(enc)[raw], 16
    return pcm.reshape(info.n_frames, ch), bits


def _ratio(rate: int, sr: int = SAMPLE_RATE):
    """(up, down) of the conversion from ``rate`` to ``sr``; n samples give ceil(n * up / down)."""
    g = gcd(int(rate), int(sr))
    return int(sr) // g, int(rate) // g


def pcm_to_waveform(pcm: np.ndarray, rate: int, bits: int, sr: int = SAMPLE_RATE) -> np.ndarray:
    """PCM [frames][channels] -> mono float32 at ``sr`` on the host, in float64: channel mean,
    polyphase FIR, 16-bit quantisation, scaling by 1/32768.  Integers of ``bits`` bits scale
    by 2^-(bits-1).  ``bits == 0``: float samples; a non-finite one counts as 0.0, finite ones
    are clamped to [-256, 256], and a frame's channels are added in channel order.  The device
    paths (``HipContext.audio_ingest`` / ``wav_ingest``) give the same samples bit for bit."""
    if bits == 0:
        x = np.asarray(pcm, dtype=np.float64).reshape(len(pcm), -1)
        x = np.clip(np.where(np.isfinite(x), x, 0.0), -256.0, 256.0)
        total = x[:, 0].copy()
        for c in range(1, x.shape[1]):  # not mean(axis=1): its order changes with the channel count
            total += x[:, c]
        x = total / x.shape[1]
    else:
        x = np.asarray(pcm).reshape(len(pcm), -1).astype(np.float64) / float(1 << (bits - 1))
        x = x.mean(axis=1)
    if rate != sr:
        from scipy.signal import resample_poly
        x = resample_poly(x, *_ratio(rate, sr))
    pcm16 = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return pcm16.astype(np.float32) / 32768.0


@lru_cache(maxsize=None)
def resample_filter(rate: int, sr: int = SAMPLE_RATE):
    """(up, down, taps) of the rate conversion ``pcm_to_waveform`` does: the float64 FIR
    ``scipy.signal.resample_poly(x, up, down)`` designs by default, ``2 * 10 * max(up, down) + 1``
    taps (read-only).  ``rate == sr``: (1, 1, None), there is no filter."""
    up, down = _ratio(rate, sr)
    if up == down:
        return 1, 1, None
    from scipy.signal import firwin
    half = 10 * max(up, down)
    taps = np.ascontiguousarray(firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up, np.float64)
    taps.setflags(write=False)
    return up, down, taps


MAX_DEVICE_TAPS = 32769  # longer filters (rates nearly coprime with 16000) are resampled on the host


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """audio.py:65-88 (numpy arrays; torch tensors are accepted and converted)."""
    if hasattr(array, "numpy") and not isinstance(array, np.ndarray):
        array = array.detach().cpu().numpy()
    if array.shape[axis] > length:
        array = array.take(indices=range(length), axis=axis)
    if array.shape[axis] < length:
        pad = [(0, 0)] * array.ndim
        pad[axis] = (0, length - array.shape[axis])
        array = np.pad(array, pad)
    return array


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * m
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), freqs)


@lru_cache(maxsize=None)
def mel_filters(device=None, n_mels: int = 80) -> np.ndarray:
    """Slaney-normalised mel filterbank [n_mels][201] — the values the reference
    loads from assets/mel_filters.npz (audio.py:91-107, librosa.filters.mel with
    sr=16000, n_fft=400), re-derived here and pinned to the reference values by tests/test_audio_mel.py."""
    assert n_mels in {80, 128}, f"Unsupported n_mels: {n_mels}"
    fft_freqs = np.linspace(0, SAMPLE_RATE / 2, 1 + N_FFT // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SAMPLE_RATE / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


_mel_ctx = {}


def _mel_context(device: int):
    """A small HIP context used only for the free function ``log_mel_spectrogram``
    (a loaded model uses its own context)."""
    from .backend_hip import HipContext
    if device not in _mel_ctx:
        dims = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
                    n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)
        ctx = HipContext(dims, device=device, dtype="fp32", max_windows=1, max_group=1)
        for nm in (80, 128):
            ctx.set_mel_filters(nm, mel_filters(None, nm))
        _mel_ctx[device] = ctx
    return _mel_ctx[device]


def _device_index(device) -> int:
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    s = str(device)
    if s.startswith("cpu"):
        raise RuntimeError("the whisper HIP backend computes on an AMD GPU only (device='cpu' is not supported)")
    return int(s.split(":")[1]) if ":" in s else 0


def device_filter_taps(rate: int, sr: int = SAMPLE_RATE) -> int:
    """Taps of the filter ``resample_filter(rate)`` would design (0: none), without designing it."""
    up, down = _ratio(rate, sr)
    return 0 if up == down else 2 * 10 * max(up, down) + 1


def stream_emitted(n: int, rate: int, final: bool = False, sr: int = SAMPLE_RATE) -> int:
    """How many 16 kHz samples a stream at ``rate`` Hz has emitted after ``n`` frames
    (``wh_stream_emitted``, include/whisper_hip.h): output k is final once its newest frame
    ``(k * down + half) // up`` has arrived, so E(n) = max(0, ceil((n * up - half) / down)), or n
    at 16 kHz; ``final``: the whole recording's ceil(n * up / down)."""
    up, down = _ratio(rate, sr)
    n = int(n)
    if up == down:
        return n
    if final:
        return -(-n * up // down)
    return max(0, -(-(n * up - 10 * max(up, down)) // down))


def source_channels(source) -> int:
    """How many channels the file behind an ``ingest_source`` source has."""
    if isinstance(source, np.ndarray):
        return 1 if source.ndim == 1 else source.shape[0]
    if len(source) == 1:
        from .backend_hip import flac_info
        return flac_info(source[0])[1]
    if len(source) == 2:
        return source[1].channels
    pcm = np.asarray(source[0])
    return 1 if pcm.ndim == 1 else int(np.prod(pcm.shape[1:]))


def ingest_source(file: str, need_length: bool = False, channels=None):
    """How a file's audio reaches the device, decided in one place: (source, length).
    ``source`` is ``(flac bytes,)`` for ``HipContext.flac_ingest`` (the frames are decoded
    on the device), ``(wav bytes, wav_info)`` for ``HipContext.wav_ingest`` (every WAV but the
    plain 16-bit one: the data chunk is uploaded in the file's own encoding and read by the
    resampling kernel), ``(pcm, rate, bits)`` for ``HipContext.audio_ingest`` (a plain 16-bit
    WAV, or a FLAC decoded on the host: mixed down and resampled on the device), or the
    16 kHz waveform as an array when the rate's filter would exceed ``MAX_DEVICE_TAPS`` and
    the host resampled it.  ``length`` is the 16 kHz
    sample count the source gives; None for a FLAC whose STREAMINFO has no total, unless
    ``need_length``: then such a file is decoded on the host instead.  ``channels`` ("split"
    or a sequence of indices) does not change a tuple source, which holds all channels and
    answers ``source_channels``; only the host-resampled form differs: it is then the rows
    ``[C][n]`` of the selected channels (``load_audio_channels``)."""
    if file.lower().endswith(".flac"):
        from .backend_hip import flac_info
        with open(file, "rb") as f:
            data = f.read()
        rate, _, _, frames = flac_info(data)
        if device_filter_taps(rate) <= MAX_DEVICE_TAPS and (frames > 0 or not need_length):
            up, down = _ratio(rate)
            return (data,), (frames * up + down - 1) // down if frames > 0 else None
    plain = _read_wav16(file) if file.lower().endswith(".wav") else None
    if file.lower().endswith(".wav") and plain is None:
        with open(file, "rb") as f:
            data = f.read()
        info = wav_info(data)
        if device_filter_taps(info.sample_rate) <= MAX_DEVICE_TAPS:
            up, down = _ratio(info.sample_rate)
            return (data, info), (info.n_frames * up + down - 1) // down
    pcm, rate, bits = plain if plain is not None else read_pcm(file)
    if device_filter_taps(rate) > MAX_DEVICE_TAPS:
        if channels is not None:
            pcm = np.asarray(pcm).reshape(len(pcm), -1)
            rows = np.stack([pcm_to_waveform(pcm[:, [c]], rate, bits) for c in select_channels(channels, pcm.shape[1])])
            return rows, rows.shape[1]
        waveform = pcm_to_waveform(pcm, rate, bits)
        return waveform, len(waveform)
    up, down = _ratio(rate)
    return (pcm, rate, bits), (len(pcm) * up + down - 1) // down


def ingest(ctx, source, dst_offset: int = 0, reserve: int = 0, channels=None):
    """A tuple ``ingest_source`` returned, sent to the context call its shape names.
    ``channels`` (a sequence of indices) is forwarded: the result is then the list of
    ``DeviceAudio`` of the split call.  Rows ``[C][n]`` (a 2-D array: channels already at
    16 kHz) are copied one behind the other, ``channels`` selecting among them."""
    if isinstance(source, np.ndarray):
        rows = source if channels is None else source[list(channels)]
        out = []
        for row in rows:
            out.append(ctx.audio_ingest(np.ascontiguousarray(row, dtype=np.float32), SAMPLE_RATE, 32,
                                        dst_offset=dst_offset, reserve=reserve))
            dst_offset += out[-1].n_samples
        return out
    kw = {} if channels is None else dict(channels=list(channels))
    if len(source) == 1:
        return ctx.flac_ingest(source[0], dst_offset=dst_offset, reserve=reserve, **kw)
    if len(source) == 2:
        return ctx.wav_ingest(source[0], dst_offset=dst_offset, reserve=reserve, **kw)
    return ctx.audio_ingest(*source, dst_offset=dst_offset, reserve=reserve, **kw)


def load_audio_device(model, file: str, channels=None):
    """``load_audio`` whose mixing, resampling and quantisation run on the GPU: the file's
    PCM is uploaded (int16 or int32) and the 16 kHz waveform is made in the context's
    resident audio buffer (``HipContext.audio_ingest``), the same samples bit for bit.
    Returns the ``DeviceAudio`` that ``transcribe`` accepts.  ``model``: a ``Whisper``, a
    ``HipContext``, or a device (the free-function context of ``log_mel_spectrogram``).
    A ``.flac`` file is not decoded on the host at all: its bytes are uploaded and its frames
    are decoded in parallel on the device (``HipContext.flac_ingest``; ``decoded_on`` of the
    result says "host" when the stream was outside that path and the host decoder ran).
    A ``.wav`` file other than plain 16-bit PCM (24- and 32-bit, 8-bit, float, A-law, mu-law,
    extensible headers) is not unpacked on the host either: its data chunk is uploaded as it
    is and the kernel reads the encoding (``HipContext.wav_ingest``).
    A rate whose filter would exceed ``MAX_DEVICE_TAPS`` is resampled on the host and
    uploaded instead (``ingest_source`` decides).
    ``channels`` ("split" for all, or a sequence of channel indices): no mix, the result is a
    list of ``DeviceAudio``, one resident segment per selected channel (the rows of
    ``load_audio_channels``, made by one upload and one launch)."""
    ctx = getattr(model, "ctx", model)
    if ctx is None or isinstance(ctx, (int, str)):
        ctx = _mel_context(_device_index(ctx))
    if channels is not None:
        source, _ = ingest_source(file, channels=channels)
        if isinstance(source, np.ndarray):
            return ingest(ctx, source)
        return ingest(ctx, source, channels=select_channels(channels, source_channels(source)))
    source, _ = ingest_source(file)
    if isinstance(source, np.ndarray):
        return ctx.audio_upload(source)
    return ingest(ctx, source)


def log_mel_spectrogram(audio: Union[str, np.ndarray], n_mels: int = 80, padding: int = 0,
                        device: Optional[Union[str, int]] = None, *, ctx=None) -> np.ndarray:
    """audio.py:110-157 on the GPU; returns float32 (n_mels, n_frames)."""
    if isinstance(audio, str):
        audio = load_audio(audio)
    if hasattr(audio, "numpy") and not isinstance(audio, np.ndarray):
        audio = audio.detach().cpu().numpy()
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    c = ctx if ctx is not None else _mel_context(_device_index(device))
    nf = c.log_mel(audio, n_mels, padding, normalize=True)
    return c.mel_read(n_mels, 0, nf)
