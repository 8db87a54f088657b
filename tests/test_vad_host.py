"""The speech-span detector's definition on the host (whisper/vad.py, no GPU): the
quarter-octave bins and their edges, known answers on the jfk fixture, the run-length rules
at each of their boundaries on hand-made energies, option validation, and that a span's
frames survive the trip through seconds that explicit clips take."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

JFK = os.path.join(GOLDEN, "jfk.flac")
FULL = 160 << 30


@pytest.fixture(scope="module")
def jfk():
    from whisper.audio import load_audio
    return load_audio(JFK)


def fixture_audio(jfk):
    return np.concatenate([np.zeros(48000, np.float32), jfk, np.zeros(80000, np.float32)])


# ---------------------------------------------------------------- bins and edges
def test_bins_and_edges():
    """``edge(bin(E)) <= E`` everywhere.  From E = 4 on (m >= 2) every bin is reachable and
    ``E < edge(bin(E) + 1)``.  Below that the formula leaves bins nobody lands in (2-4, 6, 8:
    their edges repeat a neighbour's), so for E = 1, 2, 3 the next bin's edge is not above E;
    there each energy has a bin of its own whose edge is E itself, which is the stronger
    statement."""
    from whisper.vad import N_BINS, bin_edge, energy_bin
    assert energy_bin(0) == 0 and bin_edge(0) == 0
    values = list(range(1, 4097)) + [1 << k for k in range(38)] + [FULL]
    for e in values:
        b = energy_bin(e)
        assert 1 <= b < N_BINS
        assert bin_edge(b) <= e, e
        if e >= 4:
            assert e < bin_edge(b + 1), e
        else:
            assert bin_edge(b) == e and energy_bin(e + 1) > b
    assert [energy_bin(e) for e in (1, 2, 3, 4, 5, 6, 7, 8)] == [1, 5, 7, 9, 10, 11, 12, 13]
    # monotone, and a quarter octave wide: four bins per doubling
    assert all(energy_bin(e) <= energy_bin(e + 1) for e in range(1, 4096))
    assert energy_bin(1 << 20) - energy_bin(1 << 19) == 4
    assert energy_bin(FULL) == 1 + 4 * 37 + 1  # 160 * 2^30 = 5 * 2^35


def test_histogram_is_the_bin_of_every_frame():
    from whisper.vad import energy_bin, histogram_host
    rng = np.random.default_rng(5)
    e = np.concatenate([np.arange(0, 70), rng.integers(0, FULL + 1, 500), [FULL, 1 << 37, (1 << 37) - 1]])
    want = np.bincount([energy_bin(int(x)) for x in e], minlength=160)
    assert np.array_equal(histogram_host(e.astype(np.uint64)), want)


def test_quantise_and_frame_energy():
    from whisper.vad import frame_energy_host, quantise
    x = np.array([1.0, -1.0, 2.0, -3.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, 1e-40, np.nan,
                  np.inf, -np.inf], np.float32)
    assert quantise(x).tolist() == [32767, -32768, 32767, -32768, 0, 2, 2, 0, 0, 0, 32767, -32768]
    e = frame_energy_host(np.full(161, -1.0, np.float32))
    assert e.dtype == np.uint64 and e.tolist() == [FULL, 1 << 30]
    assert frame_energy_host(np.ones(1, np.float32)).tolist() == [32767 * 32767]


# ---------------------------------------------------------------- known answers
def test_known_answers_at_the_defaults(jfk):
    from whisper.vad import resolve_options, speech_frames_host, speech_spans_host
    p = resolve_options()
    assert (p.ratio_q8, p.t_lo, p.t_hi) == (2560, 171799, 54327517)
    assert (p.percentile, p.min_silence, p.min_speech, p.pad) == (10, 200, 25, 40)
    fix = fixture_audio(jfk)
    assert speech_spans_host(fix) == [(2.66, 14.40)]
    assert speech_frames_host(fix) == ([(266, 1440)], p.t_lo)  # digital zeros: the floor clamp
    assert speech_spans_host(jfk) == [(0.0, 11.0)]
    assert speech_frames_host(jfk)[1] == p.t_hi  # the recording's own noise: the ceiling clamp
    assert speech_spans_host(np.zeros(16000 * 7, np.float32)) == []
    assert speech_spans_host(np.zeros(1, np.float32)) == []


def test_threshold_between_the_clamps(jfk):
    """-55 dBFS of seeded noise puts the tenth percentile strictly between the clamps."""
    from whisper.vad import resolve_options, speech_frames_host
    rng = np.random.default_rng(55)
    fix = fixture_audio(jfk)
    noisy = (fix + rng.standard_normal(len(fix)) * 10 ** (-55 / 20)).astype(np.float32)
    spans, t = speech_frames_host(noisy)
    p = resolve_options()
    assert p.t_lo < t < p.t_hi
    assert len(spans) == 1 and spans[0][1] == 1440 and 260 <= spans[0][0] <= 280


# ---------------------------------------------------------------- the run-length rules
def _energy(n_frames, runs):
    e = np.zeros(n_frames, np.uint64)
    for s, t in runs:
        e[s:t] = 10
    return e


def _spans(n_frames, runs, min_silence=5, min_speech=3, pad=2, threshold=9):
    from whisper.vad import spans_from_energy
    return spans_from_energy(_energy(n_frames, runs), threshold, min_silence, min_speech, pad)


def test_threshold_is_strict():
    assert _spans(30, [(10, 20)], threshold=10) == []
    assert _spans(30, [(10, 20)], threshold=9) == [(8, 22)]


def test_gap_closing_boundaries():
    # a gap of min_silence - 1 inactive frames closes; min_silence and min_silence + 1 stay open
    assert _spans(60, [(10, 15), (19, 25)], pad=0) == [(10, 25)]
    assert _spans(60, [(10, 15), (20, 25)], pad=0) == [(10, 15), (20, 25)]
    assert _spans(60, [(10, 15), (21, 25)], pad=0) == [(10, 15), (21, 25)]
    # closing comes first: two short bursts that close into one run long enough are kept
    assert _spans(60, [(10, 11), (13, 14)], pad=0) == [(10, 14)]
    # min_silence 0 and 1 close nothing
    assert _spans(60, [(10, 15), (16, 25)], pad=0, min_silence=1) == [(10, 15), (16, 25)]
    assert _spans(60, [(10, 15), (16, 25)], pad=0, min_silence=0) == [(10, 15), (16, 25)]


def test_min_speech_boundaries():
    assert _spans(60, [(10, 12)], pad=0) == []            # min_speech - 1 frames
    assert _spans(60, [(10, 13)], pad=0) == [(10, 13)]    # exactly min_speech
    assert _spans(60, [(10, 12), (30, 40)], pad=0) == [(30, 40)]
    # a dropped run does not bridge its neighbours' pads
    assert _spans(80, [(10, 20), (30, 31), (42, 50)], min_silence=5, pad=1) == [(9, 21), (41, 51)]


def test_pad_clamps_and_merges():
    assert _spans(20, [(1, 6)], pad=4) == [(0, 10)]       # clamped at 0
    assert _spans(20, [(14, 19)], pad=4) == [(10, 20)]    # clamped at F
    assert _spans(20, [(0, 20)], pad=4) == [(0, 20)]
    # pads that touch exactly merge, pads one frame apart do not
    assert _spans(80, [(10, 20), (30, 40)], min_silence=5, pad=5) == [(5, 45)]
    assert _spans(80, [(10, 20), (31, 40)], min_silence=5, pad=5) == [(5, 25), (26, 45)]
    # pads that overlap merge too
    assert _spans(80, [(10, 20), (30, 40)], min_silence=5, pad=9) == [(1, 49)]


def test_one_frame_file():
    assert _spans(1, [(0, 1)], min_speech=1) == [(0, 1)]
    assert _spans(1, [(0, 1)], min_speech=2) == []
    assert _spans(1, [], min_speech=0) == []
    from whisper.vad import speech_frames_host
    loud = np.full(7, 0.5, np.float32)  # one partial frame
    assert speech_frames_host(loud, min_speech=0.0)[0] == [(0, 1)]


# ---------------------------------------------------------------- options
def test_option_validation():
    from whisper.vad import resolve_options
    p = resolve_options(percentile=50, margin_db=0, floor_db=-35, ceil_db=-35, min_silence=0, min_speech=0, pad=0)
    assert p.ratio_q8 == 256 and p.t_lo == p.t_hi == 54327517 and (p.min_silence, p.min_speech, p.pad) == (0, 0, 0)
    assert resolve_options(margin_db=40).ratio_q8 == 2560000
    assert resolve_options(ceil_db=0).t_hi == FULL
    assert resolve_options(min_silence=0.015).min_silence == 2  # rounded to frames
    bad = [dict(percentile=0), dict(percentile=100), dict(percentile=10.0), dict(percentile=True),
           dict(margin_db=-1), dict(margin_db=40.5), dict(margin_db=float("nan")), dict(floor_db=-30),
           dict(ceil_db=1), dict(floor_db=-20, ceil_db=-10, margin_db="3"), dict(min_silence=-0.1),
           dict(min_speech=-1), dict(pad=-1), dict(pad=float("inf")), dict(threshold=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            resolve_options(**kw)


def test_skip_silence_argument():
    from whisper.transcribe import _skip_silence_params
    from whisper.vad import resolve_options
    assert _skip_silence_params(False, "0") is None
    assert _skip_silence_params(True, "0") == resolve_options()
    assert _skip_silence_params(dict(pad=0.1), "0").pad == 10
    with pytest.raises(ValueError, match="clip_timestamps"):
        _skip_silence_params(True, [0.0, 5.0])
    with pytest.raises(ValueError, match="clip_timestamps"):
        _skip_silence_params(True, "0,5")
    with pytest.raises(ValueError):
        _skip_silence_params(dict(percentile=0), "0")
    with pytest.raises(TypeError):
        _skip_silence_params("yes", "0")


def test_skip_silence_is_a_named_parameter():
    """It used to fall into **decode_options and be dropped."""
    import inspect

    import whisper
    for fn in (whisper.transcribe, whisper.transcribe_batch):
        assert inspect.signature(fn).parameters["skip_silence"].default is False


# ---------------------------------------------------------------- frames and seconds
def test_frames_survive_seconds():
    """A span reported in seconds names the same frames when it comes back as a clip
    (transcribe rounds ``ts * 100``), for every frame of 12 hours."""
    from whisper.vad import clamp_clips, frames_to_seconds
    f = np.arange(0, 12 * 3600 * 100 + 1)
    assert np.array_equal(np.round(f / 100 * 100).astype(np.int64), f)
    for k in (0, 1, 266, 1440, 3040, 359999, 360000):
        assert round(frames_to_seconds([(k, k)])[0][0] * 100) == k
    assert frames_to_seconds([(266, 1440)]) == [(2.66, 14.40)]
    assert clamp_clips([(0, 5), (90, 101)], 100) == [(0, 5), (90, 100)]
    assert clamp_clips([(100, 101)], 100) == []
