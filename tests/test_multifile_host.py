"""transcribe_batch without a GPU: the new C entry points are declared, exported and
bound, and the lane scheduler (whisper/multifile.py run_files / run_lanes) — driven with
real lanes (transcribe._Lane) and a scripted decode in place of the device — returns
results in input order, never exceeds max_windows windows per round, refills freed
lanes, splits groups by the mel budget and refuses empty audio by index."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "whisper_hip.h")
NEW = ("wh_log_mel_batch", "wh_mel_max_batch")


def test_header_declares_batch_mel():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(wh_\w+)\s*\(", src, re.M))
    for n in NEW:
        assert n in names


def test_library_exports_and_shim_binds_batch_mel():
    from whisper import backend_hip
    path = backend_hip.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in backend_hip._EXPORTS
    assert hasattr(backend_hip.HipContext, "log_mel_batch") and hasattr(backend_hip.HipContext, "mel_max_batch")


def test_public_entry_point():
    import whisper
    assert "transcribe_batch" in whisper.__all__ and callable(whisper.transcribe_batch)


# ---------------------------------------------------------------- scheduler with a scripted decode
SR, HOP = 16000, 160


class _Rig:
    """run_files with everything the GPU does replaced: prepare_group lays the files'
    frames back to back, decode_round answers every window with <|0.00|> X <|t|>, X
    naming (file, window number), which advances the lane by the whole window."""

    def __init__(self, seconds, max_windows):
        from whisper.tokenizer import get_tokenizer
        self.n_samples = [int(s * SR) for s in seconds]
        self.max_windows = max_windows
        self.tok = get_tokenizer(True, num_languages=99, language="en", task="transcribe")
        self.model = SimpleNamespace(is_multilingual=True, num_languages=99,
                                     dims=SimpleNamespace(n_audio_ctx=1500, n_text_ctx=448))
        self.groups, self.rounds, self.file_of_base = [], [], {}
        self.count = {}

    def prepare_group(self, group):
        from whisper.multifile import file_frames
        self.groups.append(list(group))
        bases = [0]
        for i in group:
            bases.append(bases[-1] + file_frames(self.n_samples[i]))
        self.file_of_base = {b: i for b, i in zip(bases, group)}
        return bases

    def make_lanes(self, group, bases):
        from whisper.transcribe import _Lane, _plan_file
        lanes = []
        for k, i in enumerate(group):
            content = bases[k + 1] - bases[k] - 3000
            _, clips, prompt, st = _plan_file(
                self.model, content, "en", dict(language="en"), temperature=0.0, thresholds=(2.4, -1.0, 0.6),
                initial_prompt=None, word_timestamps=False, prepend_punctuations="", append_punctuations="",
                clip_timestamps="0", hallucination_silence_threshold=None)
            lanes.append(_Lane(448, clips, prompt, True, False, st, base=bases[k]))
        return lanes

    def decode_round(self, windows):
        from whisper.decoding import DecodingResult
        self.rounds.append([self.file_of_base[lane.base] for lane, _, _, _ in windows])
        out = []
        tb = self.tok.timestamp_begin
        for lane, seek, size, prompt in windows:
            i = self.file_of_base[lane.base]
            assert lane.base <= seek and seek + size <= lane.base + lane.st["content_frames"]
            k = self.count[i] = self.count.get(i, 0) + 1
            out.append(DecodingResult(audio_features=None, language="en", tokens=[tb, 1000 + 10 * i + k, tb + 10],
                                      text="x", avg_logprob=-0.1, no_speech_prob=0.0, temperature=0.0,
                                      compression_ratio=1.0))
        return out

    def run(self, budget=10 ** 9):
        from whisper.multifile import run_files
        return run_files(self.n_samples, max_windows=self.max_windows, mel_budget_frames=budget,
                         prepare_group=self.prepare_group, make_lanes=self.make_lanes,
                         decode_round=self.decode_round)


def _text_tokens(lane, tb):
    return [t for s in lane.segments for t in s["tokens"] if t < tb]


def test_input_order_window_cap_and_refill():
    # content 1000, 7000, 500, 2000 frames -> 1, 3, 1, 1 windows; 0.5 s: nothing to decode
    rig = _Rig([10, 70, 5, 20, 0.5], max_windows=2)
    lanes = rig.run()
    tb = rig.tok.timestamp_begin
    assert [_text_tokens(l, tb) for l in lanes] == [[1001], [1011, 1012, 1013], [1021], [1031], []]
    assert [[s["seek"] for s in l.segments] for l in lanes] == [[0], [0, 3000, 6000], [0], [0], []]
    assert max(len(r) for r in rig.rounds) <= 2
    # longest first; the lane freed by file 3 (then 0) goes to the next pending file at once
    assert rig.rounds == [[1, 3], [1, 0], [1, 2]]
    assert rig.groups == [[0, 1, 2, 3, 4]]


def test_single_lane_context():
    rig = _Rig([10, 40, 5], max_windows=1)
    lanes = rig.run()
    assert all(len(r) == 1 for r in rig.rounds)
    assert rig.rounds == [[1], [1], [0], [2]]
    assert [len(l.segments) for l in lanes] == [1, 2, 1]


def test_groups_follow_mel_budget():
    from whisper.multifile import file_frames, split_groups
    rig = _Rig([10, 70, 5, 20], max_windows=4)
    frames = [file_frames(n) for n in rig.n_samples]
    assert frames == [4000, 10000, 3500, 5000]
    lanes = rig.run(budget=14000)
    assert rig.groups == [[0, 1], [2, 3]]
    # lanes refill inside a group only: no round mixes the groups
    assert all(set(r) <= {0, 1} or set(r) <= {2, 3} for r in rig.rounds)
    tb = rig.tok.timestamp_begin
    assert [_text_tokens(l, tb) for l in lanes] == [[1001], [1011, 1012, 1013], [1021], [1031]]
    # a file larger than the budget is a group of its own
    assert split_groups(frames, 3000) == [[0], [1], [2], [3]]
    assert split_groups(frames, 10 ** 9) == [[0, 1, 2, 3]]


def test_empty_audio_is_refused_by_index_before_any_work():
    rig = _Rig([10, 0, 5], max_windows=2)
    assert rig.n_samples[1] == 0
    with pytest.raises(ValueError, match=r"audio 1\b"):
        rig.run()
    assert rig.groups == [] and rig.rounds == []


def test_window_seed_depends_on_the_window_only():
    """What makes T > 0 retries of a file the same next to other files as alone."""
    from whisper.transcribe import _window_seed
    seeds = {_window_seed(f, s, t) for f in (1, 2) for s in (0, 2974, 3000) for t in (1, 2)}
    assert len(seeds) == 12 and all(0 <= x < 1 << 64 for x in seeds)
    assert _window_seed(7, 2974, 1) == _window_seed(7, 2974, 1)
