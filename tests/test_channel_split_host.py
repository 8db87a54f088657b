"""Channels as files, the host side (no GPU): ``load_audio_channels`` is the definition the
device matches; ``merge_channels`` turns per-channel results into one dialogue; ``split_groups``
never cuts a unit; option checking of ``transcribe`` / ``transcribe_batch``; and the scheduler
(``run_files``, driven with a scripted decode) expands a split file to one lane per channel."""
import ctypes
import os
import re
import wave
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import REPO
from test_multifile_host import _Rig, _text_tokens
from wav_fixture import encode, expand, random_values, wav_bytes

HEADER = os.path.join(REPO, "include", "whisper_hip.h")
NEW = ("wh_audio_ingest_split", "wh_flac_ingest_split", "wh_wav_ingest_split")


def test_split_entry_points_are_declared_exported_and_bound():
    from whisper import backend_hip
    names = set(re.findall(r"^\s*int\s+(wh_\w+)\s*\(", open(HEADER).read(), re.M))
    lib = ctypes.CDLL(backend_hip.lib_path())
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in backend_hip._EXPORTS, n
    lib.wh_version.restype = ctypes.c_int
    assert lib.wh_version() == 3  # the feature is detected by the symbols, not by the version
    import whisper
    for n in ("merge_channels", "load_audio_channels"):
        assert n in whisper.__all__ and callable(getattr(whisper, n))


# ---------------------------------------------------------------- load_audio_channels
@pytest.mark.parametrize("enc,rate", [("s24", 44100), ("f32", 48000), ("ulaw", 8000), ("u8", 16000)])
def test_load_audio_channels_rows_are_the_columns(tmp_path, enc, rate):
    from whisper.audio import load_audio_channels, pcm_to_waveform
    vals = random_values(np.random.default_rng(rate), enc, 2001, 3)
    path = str(tmp_path / "x.wav")
    with open(path, "wb") as f:
        f.write(wav_bytes(enc, encode(enc, vals), 3, rate))
    pcm, bits = expand(enc, vals)
    rows = load_audio_channels(path)
    assert rows.dtype == np.float32 and rows.shape[0] == 3
    for c in range(3):
        assert np.array_equal(rows[c], pcm_to_waveform(pcm[:, [c]], rate, bits)), c
    picked = load_audio_channels(path, [2, 0])
    assert np.array_equal(picked, rows[[2, 0]])
    for bad in ([3], [-1], [0, 0], []):
        with pytest.raises(ValueError, match="channels"):
            load_audio_channels(path, bad)


def test_identical_channels_give_load_audio(tmp_path):
    from whisper.audio import load_audio, load_audio_channels
    one = np.random.default_rng(2).integers(-32768, 32768, (3001, 1), dtype=np.int16)
    path = str(tmp_path / "same.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(22050)
        w.writeframes(np.repeat(one, 2, axis=1).astype("<i2").tobytes())
    rows = load_audio_channels(path)
    mix = load_audio(path)
    assert rows.shape == (2, len(mix)) and np.array_equal(rows[0], mix) and np.array_equal(rows[1], mix)


def test_a_rate_beyond_the_device_filter_gives_host_rows(tmp_path):
    """44101 Hz is coprime with 16000: its filter exceeds ``MAX_DEVICE_TAPS``, so ``ingest_source``
    resamples on the host, per channel when a selection is given, and hands out the rows."""
    from whisper.audio import (MAX_DEVICE_TAPS, device_filter_taps, ingest_source, load_audio, load_audio_channels,
                               source_channels)
    assert device_filter_taps(44101) > MAX_DEVICE_TAPS
    vals = random_values(np.random.default_rng(1), "s24", 301, 2)
    path = str(tmp_path / "odd_rate.wav")
    with open(path, "wb") as f:
        f.write(wav_bytes("s24", encode("s24", vals), 2, 44101))
    rows = load_audio_channels(path)
    source, length = ingest_source(path, need_length=True, channels="split")
    assert isinstance(source, np.ndarray) and source.shape == rows.shape == (2, length)
    assert np.array_equal(source, rows) and source_channels(source) == 2
    source, length = ingest_source(path, channels=[1])
    assert source.shape == (1, length) and np.array_equal(source[0], rows[1])
    mixed, length = ingest_source(path)  # without a selection: the mix, as before
    assert mixed.ndim == 1 and np.array_equal(mixed, load_audio(path))
    # the sources of the device paths answer the channel count too
    with open(str(tmp_path / "s24.wav"), "wb") as f:
        f.write(wav_bytes("s24", encode("s24", vals), 2, 48000))
    source, _ = ingest_source(str(tmp_path / "s24.wav"), channels="split")
    assert len(source) == 2 and source_channels(source) == 2
    with wave.open(str(tmp_path / "s16.wav"), "wb") as w:
        w.setnchannels(3)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(np.zeros((10, 3), "<i2").tobytes())
    source, _ = ingest_source(str(tmp_path / "s16.wav"), channels="split")
    assert len(source) == 3 and source_channels(source) == 3


# ---------------------------------------------------------------- merge_channels
def _seg(start, end, text, **kw):
    return dict(id=99, seek=0, start=start, end=end, text=text, tokens=[1], temperature=0.0, **kw)


def _res(segs, language="en", **kw):
    return dict(text="".join(s["text"] for s in segs), segments=segs, language=language, **kw)


def test_merge_orders_renumbers_and_names():
    from whisper import merge_channels
    a = _res([_seg(0.0, 2.0, " hello"), _seg(5.0, 6.0, " bye"), _seg(7.0, 8.0, " tie")], speech_spans=[(0.0, 8.0)])
    b = _res([_seg(0.0, 1.0, " hi"), _seg(5.0, 6.0, " see you"), _seg(7.0, 7.5, "  "), _seg(7.0, 8.0, " tie too")])
    m = merge_channels([a, b], ["agent", "customer"])
    order = [(s["channel"], s["start"], s["end"]) for s in m["segments"]]
    assert order == [("customer", 0.0, 1.0), ("agent", 0.0, 2.0),          # a tie on start: the earlier end first
                     ("agent", 5.0, 6.0), ("customer", 5.0, 6.0),          # a tie on (start, end): the lower index
                     ("customer", 7.0, 7.5), ("agent", 7.0, 8.0), ("customer", 7.0, 8.0)]
    assert [s["id"] for s in m["segments"]] == list(range(7))
    assert [s["channel_index"] for s in m["segments"]] == [1, 0, 0, 1, 1, 0, 1]
    # the empty text is skipped in the text, not in the segments
    assert m["text"] == "customer: hi\nagent: hello\nagent: bye\ncustomer: see you\nagent: tie\ncustomer: tie too"
    assert m["language"] == "en"
    # the per-channel results are the ones given, untouched (copies went into the merge)
    assert m["channels"][0] is a and m["channels"][1] is b
    assert [s["id"] for s in a["segments"]] == [99, 99, 99] and "channel" not in a["segments"][0]
    assert m["channels"][0]["speech_spans"] == [(0.0, 8.0)] and "speech_spans" not in m
    # default names, and a wrong count
    assert [s["channel"] for s in merge_channels([a, b])["segments"]][:2] == ["1", "0"]
    with pytest.raises(ValueError, match="names"):
        merge_channels([a, b], ["only one"])


def test_merge_language_rule_empty_channels_and_words():
    from whisper import merge_channels
    words = [dict(word=" hola", start=0.0, end=0.5, probability=0.9)]
    es = _res([_seg(0.0, 3.0, " hola", words=words)], language="es")
    en = _res([_seg(1.0, 2.0, " hi"), _seg(4.0, 5.0, " there")], language="en")
    none = _res([], language="de")
    assert merge_channels([en, es])["language"] == "es"       # 3 s of speech against 2 s
    assert merge_channels([es, en, none])["language"] == "es"
    en3 = _res([_seg(1.0, 2.5, " hi"), _seg(4.0, 5.5, " there")], language="en")
    assert merge_channels([en3, es])["language"] == "en"      # a tie: the lowest index
    assert merge_channels([es, en3])["language"] == "es"
    m = merge_channels([none, es])
    assert [s["channel"] for s in m["segments"]] == ["1"] and m["text"] == "1: hola" and m["language"] == "es"
    assert m["segments"][0]["words"] == words
    both_empty = merge_channels([none, none])
    assert both_empty == dict(text="", segments=[], language="de", channels=[none, none])


# ---------------------------------------------------------------- split_groups with units
def test_split_groups_keeps_units_whole():
    from whisper.multifile import expand_channels, split_groups
    frames = [4000, 3600, 3600, 5000, 3500, 3500, 3500]
    units = [0, 1, 1, 2, 3, 3, 3]
    assert expand_channels([None, 2, None, 3]) == (units, [0, 0, 1, 0, 0, 1, 2])
    assert split_groups(frames, 8000, units) == [[0], [1, 2], [3], [4, 5, 6]]      # 0 + unit 1 would be 11200
    assert split_groups(frames, 12300, units) == [[0, 1, 2], [3], [4, 5, 6]]
    assert split_groups(frames, 10 ** 9, units) == [list(range(7))]
    # an oversize unit is a group of its own, and so is what follows it
    assert split_groups(frames, 7000, units) == [[0], [1, 2], [3], [4, 5, 6]]
    assert split_groups(frames, 3000, units) == [[0], [1, 2], [3], [4, 5, 6]]
    with pytest.raises(ValueError, match="units"):
        split_groups(frames, 8000, units[:-1])
    # without the argument: the cases tests/test_multifile_host.py pins
    frames = [4000, 10000, 3500, 5000]
    assert split_groups(frames, 14000) == [[0, 1], [2, 3]]
    assert split_groups(frames, 3000) == [[0], [1], [2], [3]]
    assert split_groups(frames, 10 ** 9) == [[0, 1, 2, 3]]
    assert split_groups(frames, 14000, [0, 1, 2, 3]) == split_groups(frames, 14000)


# ---------------------------------------------------------------- option checking
def _model():
    return SimpleNamespace(ctx=None, dtype="fp32", dims=SimpleNamespace(n_mels=80), is_multilingual=False,
                           num_languages=99)


def test_option_checking_before_any_device_work():
    import whisper
    from whisper.backend_hip import DeviceAudio
    one = np.zeros(16000, np.float32)
    two = np.zeros((2, 16000), np.float32)
    with pytest.raises(ValueError, match=r"channels: 3 values for 2 files"):
        whisper.transcribe_batch(_model(), [one, one], channels=["split", None, None])
    with pytest.raises(ValueError, match="channels='split'"):
        whisper.transcribe_batch(_model(), [one, two])
    with pytest.raises(ValueError, match="'both'"):
        whisper.transcribe_batch(_model(), [two], channels="both")
    with pytest.raises(ValueError, match="channels: 2 is not a channel"):
        whisper.transcribe_batch(_model(), [two], channels=[0, 2])
    with pytest.raises(ValueError, match="channel_names"):
        whisper.transcribe_batch(_model(), [two], channels="split", channel_names=["a", "b", "c"])
    with pytest.raises(ValueError, match="schedule"):
        whisper.transcribe(_model(), two, channels="split", schedule="sequential")
    with pytest.raises(ValueError, match="mel_max_reduce"):
        whisper.transcribe(_model(), two, channels=[0], mel_max_reduce=max)
    with pytest.raises(ValueError, match="_mel_prepared"):
        whisper.transcribe(_model(), two, channels="split", _mel_prepared=(1, 0, 1))
    with pytest.raises(ValueError, match="DeviceAudio"):
        whisper.transcribe(_model(), DeviceAudio(None, 16000), channels="split")


# ---------------------------------------------------------------- scheduler
def test_a_split_file_expands_to_its_channels_lanes_in_order():
    """Files: 10 s mixed, 20 s with 3 channels split, 5 s mixed -> lanes 0, 1.0, 1.1, 1.2, 2.  The
    scripted decode names (lane, window number); the lanes come back in input order, the
    channels of the file next to each other in channel order, and no group cuts them."""
    from whisper.multifile import expand_channels, run_files
    seconds, counts = [10, 20, 5], [None, 3, None]
    file_of, channel_of = expand_channels(counts)
    assert file_of == [0, 1, 1, 1, 2] and channel_of == [0, 0, 1, 2, 0]
    rig = _Rig([seconds[i] for i in file_of], max_windows=2)

    def run(budget):
        rig.groups, rig.rounds, rig.count = [], [], {}
        return run_files(rig.n_samples, max_windows=2, mel_budget_frames=budget, prepare_group=rig.prepare_group,
                         make_lanes=rig.make_lanes, decode_round=rig.decode_round, units=file_of)

    tb = rig.tok.timestamp_begin
    lanes = run(10 ** 9)
    assert rig.groups == [[0, 1, 2, 3, 4]]
    assert [_text_tokens(l, tb) for l in lanes] == [[1001], [1011], [1021], [1031], [1041]]
    # longest first, ties in input order: the file's channels run in channel order
    assert rig.rounds == [[1, 2], [3, 0], [4]]
    # lanes are 4000, 5000 x 3, 3500 frames: 9000 would cut the file after its first channel
    lanes = run(9000)
    assert rig.groups == [[0], [1, 2, 3], [4]]
    assert [_text_tokens(l, tb) for l in lanes] == [[1001], [1011], [1021], [1031], [1041]]
    lanes = run(19000)
    assert rig.groups == [[0, 1, 2, 3], [4]]
