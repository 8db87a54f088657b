"""PCM ingest, host side (no GPU): the C ABI declares, exports and binds the two entry
points; ``resample_filter`` is the filter ``pcm_to_waveform`` applies (a direct fp64
evaluation of the formula in include/whisper_hip.h equals it exactly); ``load_audio`` is
still ``pcm_to_waveform(read_pcm(...))``; and the device loader raises without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

JFK = os.path.join(GOLDEN, "jfk.flac")
RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000)


def ratio(rate):
    from math import gcd
    g = gcd(rate, 16000)
    return 16000 // g, rate // g


def ingest_lengths(rate):
    """Frames per file for one rate: 1, 2, around ``down``, around the filter's reach in
    frames (2 * half / up), and a few thousand."""
    up, down = ratio(rate)
    reach = 2 * 10 * max(up, down) // up
    return sorted({1, 2, down - 1, down, down + 1, reach - 1, reach + 1, 4001} - {0})


def direct_resample(pcm, bits, up, down, taps):
    """out[k] of the header's formula, summed tap by tap in float64."""
    x = pcm.reshape(len(pcm), -1).astype(np.float64) / float(1 << (bits - 1))
    x = x.sum(axis=1) / x.shape[1]
    n = len(x)
    half = 10 * max(up, down)
    assert len(taps) == 2 * half + 1
    k = np.arange(-(-n * up // down), dtype=np.int64)
    c = k * down + half
    m = c // up          # the newest frame that reaches output k
    t = c - m * up       # and its tap
    y = np.zeros(len(k))
    while (t <= 2 * half).any():
        ok = (t <= 2 * half) & (m >= 0) & (m < n)
        y[ok] += x[m[ok]] * taps[t[ok]]
        t = t + up
        m = m - 1
    return (np.clip(np.rint(y * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def test_header_library_and_shim_have_the_entry_points():
    from whisper import backend_hip
    src = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    declared = set(re.findall(r"^\s*int\s+(wh_\w+)\s*\(", src, re.M))
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in ("wh_audio_ingest", "wh_audio_read"):
        assert name in declared
        assert hasattr(lib, name)
        assert name in backend_hip._EXPORTS
    assert re.search(r"WH_PCM_S16 = 0, WH_PCM_S32 = 1, WH_PCM_F32 = 2", src)
    assert (backend_hip.WH_PCM_S16, backend_hip.WH_PCM_S32, backend_hip.WH_PCM_F32) == (0, 1, 2)


@pytest.mark.parametrize("rate", RATES)
def test_resample_filter_is_the_filter_of_pcm_to_waveform(rate):
    from whisper.audio import pcm_to_waveform, resample_filter
    up, down, taps = resample_filter(rate)
    assert (up, down) == ratio(rate)
    assert taps.dtype == np.float64 and taps.shape == (2 * 10 * max(up, down) + 1,)
    rng = np.random.default_rng(rate)
    for n in ingest_lengths(rate):
        for ch in (1, 2, 3):
            pcm = rng.integers(-32768, 32768, (n, ch), dtype=np.int16)
            want = pcm_to_waveform(pcm, rate, 16)
            got = direct_resample(pcm, 16, up, down, taps)
            assert want.dtype == np.float32 and want.shape == (-(-n * up // down),)
            assert np.array_equal(got, want), (rate, n, ch, float(np.abs(got - want).max()))


def test_resample_filter_at_16k_has_no_filter():
    from whisper.audio import device_filter_taps, resample_filter
    assert resample_filter(16000) == (1, 1, None)
    assert device_filter_taps(16000) == 0
    assert device_filter_taps(44100) == 8821 and device_filter_taps(48000) == 61
    assert device_filter_taps(16001) == 2 * 10 * 16001 + 1


def test_load_audio_is_read_pcm_then_pcm_to_waveform():
    from whisper.audio import load_audio, pcm_to_waveform, read_pcm
    pcm, rate, bits = read_pcm(JFK)
    assert (pcm.dtype, pcm.shape, rate, bits) == (np.int32, (485100, 2), 44100, 24)
    a = load_audio(JFK)
    assert a.dtype == np.float32 and a.shape == (176000,)
    assert np.array_equal(a, pcm_to_waveform(pcm, rate, bits))
    # the samples are whole 16-bit steps
    assert np.array_equal(a * 32768.0, np.round(a * 32768.0))


def test_read_pcm_of_wav(tmp_path):
    import wave
    from whisper.audio import load_audio, pcm_to_waveform, read_pcm
    pcm = np.random.default_rng(5).integers(-32768, 32768, (4801, 2), dtype=np.int16)
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(pcm.tobytes())
    got, rate, bits = read_pcm(p)
    assert got.dtype == np.int16 and np.array_equal(got, pcm) and (rate, bits) == (48000, 16)
    assert np.array_equal(load_audio(p), pcm_to_waveform(pcm, 48000, 16))


def test_load_audio_device_needs_a_device():
    """No CPU fallback: without a HIP device the loader raises; with one it returns the
    resident waveform's handle."""
    import torch

    import whisper
    if torch.cuda.is_available():
        d = whisper.load_audio_device(None, JFK)
        assert d.n_samples == 176000 and d.offset == 0
    else:
        with pytest.raises(whisper.HipBackendError):
            whisper.load_audio_device(None, JFK)
