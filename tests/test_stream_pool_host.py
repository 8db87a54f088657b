"""The stream pool, host side (no GPU): the C ABI carries the ten pool entry points, and
StreamingPool's policy — rounds of one append call, one decode of the due streams, one trim call —
gives every stream the updates of a lone StreamingTranscriber, driven with a device half that
only counts samples and a scripted decode."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_stream_host import CountingStream, scripted_decode, words_of

POOL_SYMBOLS = ("wh_pool_create", "wh_pool_destroy", "wh_pool_open", "wh_pool_close", "wh_pool_append",
                "wh_pool_finish", "wh_pool_trim", "wh_pool_info", "wh_pool_read", "wh_pool_log_mel")
FRAME_BYTES = dict(s16=2, ulaw=1, s24=3)


def test_header_library_and_shim_have_the_pool_entry_points():
    from whisper import backend_hip
    src = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in POOL_SYMBOLS:
        assert re.search(r"^int %s\s*\(" % name, src, re.M), name
        assert hasattr(lib, name), name
        assert name in backend_hip._EXPORTS, name
        assert hasattr(backend_hip.HipContext, name[3:]), name
    lib.wh_version.restype = ctypes.c_int
    assert lib.wh_version() == 3  # detected by the symbols, not by the version


def emitted(n, rate, final=False):
    # the closed form (tests/test_stream_host.py holds it against the definition)
    from whisper.audio import stream_emitted
    return stream_emitted(n, rate, final)


class FormulaStream(CountingStream):
    """CountingStream with the closed form of E(n): long inputs at 44.1 kHz stay quick."""

    def append(self, data):
        before = emitted(self.frames, self.rate)
        self.frames += len(data) // self.frame_bytes
        self.n_samples += emitted(self.frames, self.rate) - before
        return emitted(self.frames, self.rate) - before

    def finish(self):
        got = emitted(self.frames, self.rate, True) - emitted(self.frames, self.rate)
        self.n_samples += got
        return got


class CountingPool:
    """What StreamingPool asks of a device: per slot the frames in and the resident samples, by
    the emission count alone.  Capacity is enforced as the library does, and every call is logged."""

    def __init__(self, n_slots, slot_samples):
        self.n_slots, self.slot_samples = n_slots, slot_samples
        self.slots = {}
        self.calls = []
        self.peak = 0

    def pool_open(self, slot, encoding, channels, rate):
        from whisper.audio import WAV_CONTAINER
        assert 0 <= slot < self.n_slots and slot not in self.slots
        self.slots[slot] = dict(rate=rate, fb=WAV_CONTAINER[encoding] * channels, frames=0, resident=0, finished=False)
        self.calls.append(("open", slot))

    def pool_close(self, slot):
        del self.slots[slot]
        self.calls.append(("close", slot))

    def pool_append(self, slots, packets, n_frames):
        assert len(slots) == len(packets) == len(n_frames) and len(set(slots)) == len(slots) >= 1
        out = []
        for s, p, n in zip(slots, packets, n_frames):
            st = self.slots[s]
            assert not st["finished"] and len(p) == n * st["fb"] and n > 0
            got = emitted(st["frames"] + n, st["rate"]) - emitted(st["frames"], st["rate"])
            assert st["resident"] + got <= self.slot_samples, "capacity: the caller must trim"
            st["frames"] += n
            st["resident"] += got
            self.peak = max(self.peak, st["resident"])
            out.append(got)
        self.calls.append(("append", tuple(slots), tuple(n_frames)))
        return out

    def pool_finish(self, slots):
        out = []
        for s in slots:
            st = self.slots[s]
            got = emitted(st["frames"], st["rate"], True) - emitted(st["frames"], st["rate"])
            assert st["resident"] + got <= self.slot_samples
            st["resident"] += got
            st["finished"] = True
            out.append(got)
        self.calls.append(("finish", tuple(slots)))
        return out

    def pool_trim(self, slots, n_drop):
        assert len(slots) == len(n_drop) and len(set(slots)) == len(slots) >= 1
        for s, n in zip(slots, n_drop):
            assert 0 < n <= self.slots[s]["resident"]
            self.slots[s]["resident"] -= n
        self.calls.append(("trim", tuple(slots), tuple(n_drop)))


# (rate, encoding, per-stream options, words per segment of its scripted hypotheses, seconds of input)
STREAMS = [
    (16000, "s16", dict(min_chunk=1.0, buffer_trim=4.0, max_buffer=6.0), 4, 13.3),
    (8000, "ulaw", dict(min_chunk=0.7, buffer_trim=3.0, max_buffer=5.0, initial_prompt="Glossary:", prompt_chars=12), 3, 11.0),
    (16000, "s16", dict(min_chunk=2.5, buffer_trim=4.0, max_buffer=6.0, language="de"), 10 ** 6, 16.0),
    (44100, "s24", dict(min_chunk=1.0, buffer_trim=15.0, max_buffer=25.0), 5, 9.1),
]


def rename_for(k):
    # stream 2 never agrees with itself: its commits are forced ones
    return (lambda i, n: f" v{n}_{i}") if k == 2 else None


def data_of(k):
    rate, enc, _, _, seconds = STREAMS[k]
    return np.random.default_rng(k).integers(0, 256, int(seconds * rate) * FRAME_BYTES[enc] + (k % 2), dtype=np.uint8).tobytes()


def comparable(u):
    return (u.span, u.prompt, u.language, u.forced, u.final, u.committed, u.tentative, u.result)


def lone_updates(k, piece):
    from whisper.streaming import StreamingTranscriber
    rate, enc, opts, per_segment, _ = STREAMS[k]
    t = StreamingTranscriber(None, rate, enc, stream=FormulaStream(rate, FRAME_BYTES[enc]),
                             decode_fn=scripted_decode(per_segment, [], rename_for(k)), **opts)
    data = data_of(k)
    ups = [u for at in range(0, len(data), piece) for u in t.feed(data[at:at + piece])]
    return ups + [t.finish()]


def make_pool(n_slots=4, slot_samples=None, **kw):
    from whisper.streampool import DEFAULT_SLOT_SAMPLES, StreamingPool
    dev = CountingPool(n_slots, slot_samples or DEFAULT_SLOT_SAMPLES)
    logs, decoders = {}, {}

    def decode_round(items):
        out = []
        for handle, prompt, span in items:
            out.append(decoders[handle](prompt, span))
        return out
    pool = StreamingPool(None, slots=n_slots, slot_samples=dev.slot_samples, device=dev, decode_round_fn=decode_round,
                         **kw)

    def open_stream(k):
        rate, enc, opts, per_segment, _ = STREAMS[k]
        h = pool.open(rate, enc, 1, **opts)
        logs[h] = []
        decoders[h] = scripted_decode(per_segment, logs[h], rename_for(k))
        return h
    return pool, dev, open_stream, logs


@pytest.mark.parametrize("piece_s", [0.37, 0.02, 100.0])
def test_pool_updates_are_those_of_lone_transcribers(piece_s):
    pool, dev, open_stream, logs = make_pool()
    handles = [open_stream(k) for k in range(3)]
    data = [data_of(k) for k in range(4)]
    pos = [0] * 4
    got = {}
    tick = 0
    while any(pos[k] < len(data[k]) for k in range(4)):
        if tick == 5:
            handles.append(open_stream(3))  # a stream that joins later, in the slot left
            with pytest.raises(RuntimeError, match="slots"):
                pool.open(16000)
        packets = {}
        for k, h in enumerate(handles):
            # pieces of a different size per stream, and stream 1 sits out every third tick
            n = int(piece_s * STREAMS[k][0] * (1 + 0.3 * k)) * FRAME_BYTES[STREAMS[k][1]] + k
            if pos[k] < len(data[k]) and not (k == 1 and tick % 3 == 2):
                packets[h] = data[k][pos[k]:pos[k] + n]
                pos[k] += n
        before = len(dev.calls)
        rounds_before = len(pool.rounds)
        for h, ups in pool.feed(packets).items():
            got.setdefault(h, []).extend(ups)
        # every round: one append call, then at most one trim call
        calls = dev.calls[before:]
        kinds = [c[0] for c in calls]
        assert set(kinds) <= {"append", "trim"} and "trim,trim" not in ",".join(kinds)
        assert kinds.count("append") >= len(pool.rounds) - rounds_before
        for c in calls:
            if c[0] == "append":
                assert set(c[1]) <= {pool.stream(h).stream.slot for h in packets}
        tick += 1
    final = pool.finish(handles)
    assert [c[0] for c in dev.calls[-5:]] == ["finish"] + ["close"] * 4 and len(dev.calls[-5][1]) == 4
    for k, h in enumerate(handles):
        got[h].append(final[h])
        want = lone_updates(k, 1 << 30)
        assert len(got[h]) == len(want) and want[-1].final
        for a, b in zip(got[h], want):
            assert comparable(a) == comparable(b), (k, a.span, b.span)
    # the runs exercised the rules: cuts, forced commits, a prompt carried over, agreement
    assert any(c[0] == "trim" for c in dev.calls)
    assert any(u.forced for u in got[handles[2]]) and not any(u.forced for u in got[handles[0]])
    assert any(u.prompt and u.prompt.startswith("Glossary: w") for u in got[handles[1]])
    assert all(u.language == "de" for u in got[handles[2]])
    # streams that are due in the same round are decoded by one call
    assert any(len(r) >= 2 for r in pool.rounds)
    assert sum(len(r) for r in pool.rounds) == sum(len(v) for v in logs.values())
    # capacity: no slot ever held more than the 30 s the policy allows
    assert dev.peak <= 30 * 16000 + 40 <= dev.slot_samples


def test_one_append_and_one_trim_call_per_round():
    pool, dev, open_stream, logs = make_pool()
    a, b = open_stream(0), open_stream(0)   # the same stream twice: always due together
    second = np.zeros(16000, np.int16).tobytes()
    for _ in range(4):
        pool.feed({a: second, b: second})
    assert [c[0] for c in dev.calls[2:]] == ["append"] * 4 and pool.rounds == [[a, b]] * 4
    before = len(dev.calls)
    ups = pool.feed({a: second * 3, b: second * 2})   # 5 s > buffer_trim: both cut, in one call per round
    calls = dev.calls[before:]
    assert [c[0] for c in calls] == ["append", "trim", "append", "append"]
    assert calls[0][1:] == ((0, 1), (16000, 16000)) and calls[1][1:] == ((0, 1), (62400, 62400))
    assert calls[2][1:] == ((0, 1), (16000, 16000)) and calls[3][1:] == ((0,), (16000,))
    assert len(ups[a]) == 3 and len(ups[b]) == 2
    assert pool.stream(a).span == (62400, 7 * 16000) and pool.stream(b).span == (62400, 6 * 16000)
    assert words_of(pool.stream(a).committed)[:8] == [f" w{i}" for i in range(8)]
    assert pool.stream(a).text.startswith("w0 w1")


def test_arguments_are_checked():
    from whisper.streampool import StreamingPool
    ok = dict(device=CountingPool(2, 500000), decode_round_fn=lambda items: [dict(segments=[]) for _ in items])
    StreamingPool(None, slots=2, word_timestamps=True, temperature=0.0, beam_size=5, hotwords=["Acme"], **ok)
    with pytest.raises(ValueError, match="word_timestamps"):
        StreamingPool(None, word_timestamps=False, **ok)
    for name, value in (("clip_timestamps", "0,5"), ("channels", "split"), ("schedule", "batched"),
                        ("mel_max_reduce", max), ("skip_silence", True), ("language", "en"), ("min_chunk", 2.0),
                        ("initial_prompt", "x")):
        with pytest.raises(ValueError, match=name):
            StreamingPool(None, **{name: value}, **ok)
    with pytest.raises(ValueError, match="slots"):
        StreamingPool(None, slots=0, **ok)
    pool = StreamingPool(None, slots=2, **ok)
    for bad in (dict(buffer_trim=25.0, max_buffer=25.0), dict(max_buffer=29.5), dict(min_chunk=6.0),
                dict(min_chunk=0.0), dict(buffer_trim=0.0)):
        with pytest.raises(ValueError, match="buffer_trim|min_chunk"):
            pool.open(16000, **bad)
    with pytest.raises(ValueError, match="encoding"):
        pool.open(16000, "mp3")
    with pytest.raises(ValueError, match="16001"):
        pool.open(16001)
    with pytest.raises(ValueError, match="channels"):
        pool.open(16000, "s16", "split")
    with pytest.raises(TypeError, match="initial_prompt"):
        pool.open(16000, initial_prompt=[1, 2])
    assert ok["device"].calls == []   # a refused open takes no slot
    a, b = pool.open(16000), pool.open(8000, "ulaw")
    with pytest.raises(RuntimeError, match="slots"):
        pool.open(16000)
    with pytest.raises(ValueError, match="unknown"):
        pool.feed({a: b"", 77: b""})
    with pytest.raises(TypeError, match="int16|<i2"):
        pool.feed({a: np.zeros(4, np.float32)})
    assert pool.feed({}) == {} and pool.feed({a: b"\0"}) == {a: []}
    final = pool.finish([a])
    assert final[a].final and final[a].result is None
    with pytest.raises(ValueError, match="finished"):
        pool.feed({a: bytes(32000)})
    with pytest.raises(ValueError, match="finished"):
        pool.finish([a])
    c = pool.open(16000)   # finish freed the slot
    assert c not in (a, b) and pool.stream(c).stream.slot == 0 and pool.stream(b).stream.slot == 1
    assert len(pool.feed({c: bytes(32000), b: bytes(8000)})[c]) == 1
