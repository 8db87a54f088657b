"""Voice activity of live streams, host side (no GPU): the numpy twin of the device detector
(``vad.StreamVad``) against the file rules and the JFK fixture, its independence of how the
samples were split, the edges of its window, the option checks, and the policy on top of it
(idle / endpoint / speech) in ``StreamingTranscriber`` and ``StreamingPool``, driven with stub
streams that carry a twin and scripted decodes."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from test_stream_host import CountingStream, scripted_decode, words_of
from test_stream_pool_host import CountingPool

JFK = os.path.join(GOLDEN, "jfk.flac")
SVAD_SYMBOLS = ("wh_pool_vad_enable", "wh_pool_vad_state", "wh_pool_vad_read", "wh_stream_vad_enable",
                "wh_stream_vad_state")
SILENCE, ONSET, SPEECH = 0, 1, 2


def P(**kw):
    """StreamVadParams given directly in integers."""
    from whisper.vad import StreamVadParams
    base = dict(percentile=10, ratio_q8=2560, t_lo=1000, t_hi=1000, window=50, min_silence=5, min_speech=3, pad=0)
    base.update(kw)
    return StreamVadParams(**base)


def bursts(rng, n_frames, amps=(0.0, 2e-3, 0.3), longest=8):
    """A float32 signal of ``n_frames`` 10 ms frames: the amplitude is drawn per run of 1..longest frames."""
    out = np.zeros(n_frames * 160, np.float32)
    f = 0
    while f < n_frames:
        k = min(int(rng.integers(1, longest + 1)), n_frames - f)
        out[f * 160:(f + k) * 160] = rng.choice(amps) * rng.uniform(-1, 1, k * 160)
        f += k
    return out


@pytest.fixture(scope="module")
def jfk():
    from whisper.audio import load_audio
    a = load_audio(JFK)
    assert a.shape == (176000,) and a.dtype == np.float32
    return a


@pytest.fixture(scope="module")
def composite(jfk):
    """1.5 s zeros + JFK[0:4.5 s] + 2.5 s zeros + JFK[5.3 s:8 s] + 1.5 s zeros: 12.7 s."""
    z = lambda s: np.zeros(int(round(s * 16000)), np.float32)
    c = np.concatenate([z(1.5), jfk[:72000], z(2.5), jfk[84800:128000], z(1.5)])
    assert len(c) == 203200
    return c


# ---------------------------------------------------------------- the C ABI
def test_header_library_and_shim_have_the_detector_entry_points():
    from whisper import backend_hip
    src = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    lib = ctypes.CDLL(backend_hip.lib_path())
    for name in SVAD_SYMBOLS:
        assert re.search(r"^int %s\s*\(" % name, src, re.M), name
        assert hasattr(lib, name), name
        assert name in backend_hip._EXPORTS, name
        assert hasattr(backend_hip.HipContext, name[3:]), name
    assert ctypes.sizeof(backend_hip.WhSvadState) == 80 and ctypes.sizeof(backend_hip.WhSvadOpts) == 40
    lib.wh_version.restype = ctypes.c_int
    assert lib.wh_version() == 3  # detected by the symbols, not by the version


# ---------------------------------------------------------------- property 1: the file rules, causally
def test_pinned_threshold_gives_the_file_spans():
    from whisper.vad import StreamVad, frame_energy_host, spans_from_energy
    rng = np.random.default_rng(1)
    n_open = 0
    for _ in range(200):
        x = bursts(rng, int(rng.integers(20, 160)), amps=(0.0, 0.0, 1e-3, 0.1), longest=12)
        x = x[:len(x) - int(rng.integers(0, 160))]  # the last frame may be a partial one
        T = int(rng.choice([1000, 200000, 5 * 10 ** 7]))
        p = P(t_lo=T, t_hi=T, window=int(rng.integers(1, 200)), min_silence=int(rng.integers(1, 12)),
              min_speech=int(rng.integers(0, 8)), percentile=int(rng.integers(1, 100)))
        d = StreamVad(p)
        d.feed(x)
        st = d.finish()
        got = list(d.spans) + ([(st.run_start, st.run_end)] if st.state == SPEECH else [])
        n_open += st.state == SPEECH
        E = frame_energy_host(x)
        assert st.frames == len(E) and set(d.thresholds) == {T}
        assert got == spans_from_energy(E, T, p.min_silence, p.min_speech, 0), p
    assert n_open > 10


# ---------------------------------------------------------------- property 2: the JFK fixture
def test_jfk_spans_and_threshold_range(jfk):
    from whisper.vad import StreamVad, resolve_stream_options
    p = resolve_stream_options(percentile=10, margin_db=10, floor_db=-60, ceil_db=-35, window=30.0, min_silence=0.5,
                               min_speech=0.25)
    assert (p.window, p.min_silence, p.min_speech) == (3000, 50, 25)
    d = StreamVad(p)
    st = d.feed(jfk)
    assert d.spans == [(6, 213), (328, 431), (541, 768)]
    assert (st.state, st.run_start, st.run_end) == (SPEECH, 819, 1100)
    assert (st.closed_start, st.closed_end, st.closed_total) == (541, 768, 3)
    assert (min(d.thresholds), max(d.thresholds)) == (171799, 54327517) == (p.t_lo, p.t_hi)
    assert st.frames == 1100 and st.samples == 176000 and st.partial == 0
    assert d.finish() == st


# ---------------------------------------------------------------- split independence
def test_any_split_gives_the_same_states():
    from whisper.vad import StreamVad, resolve_stream_options
    rng = np.random.default_rng(2)
    p = resolve_stream_options(window=0.16, min_silence=0.03, min_speech=0.02, floor_db=-70, ceil_db=-20)
    x = bursts(rng, 150)[:-37]
    whole = StreamVad(p)
    # the state after every prefix length that some split stops at: one feed of that prefix
    def at(n):
        d = StreamVad(p)
        return d.feed(x[:n])
    for trial in range(6):
        d = StreamVad(p)
        pos = 0
        sizes = {0: lambda: int(rng.integers(0, 700)), 1: lambda: 1, 2: lambda: 160, 3: lambda: int(rng.choice([0, 0, 37])),
                 4: lambda: int(rng.choice([0, 1, 159, 160, 161, 320]))}[trial % 5]
        limit = len(x) if trial % 5 != 1 else 400
        checked = 0
        while pos < limit:
            n = min(sizes() if trial else int(rng.integers(0, 700)), limit - pos)
            st = d.feed(x[pos:pos + n])
            pos += n
            if checked < 40 or pos == limit:
                assert st == at(pos), (trial, pos)
                checked += 1
        if limit == len(x):
            final = d.finish()
            whole_d = StreamVad(p)
            whole_d.feed(x)
            assert final == whole_d.finish() and np.array_equal(d.ring, whole_d.ring) and np.array_equal(d.hist, whole_d.hist)
            assert final.frames == -(-len(x) // 160) and final.partial == 0 and d.spans == whole_d.spans
            assert d.finish() == final  # a second finish changes nothing
    assert whole.state.frames == 0


# ---------------------------------------------------------------- window edges
def reference_states(x, p):
    """The definition once more, without a ring: the histogram of the last W energies recounted
    at every frame."""
    from whisper.vad import bin_edge, energy_bin, frame_energy_host
    E = [int(e) for e in frame_energy_host(x)]
    state, run_start, run_end, closed = SILENCE, 0, 0, []
    thr = []
    for f, e in enumerate(E):
        win = sorted(energy_bin(v) for v in E[max(0, f + 1 - p.window):f + 1])
        rank = max(1, -(-len(win) * p.percentile // 100))
        T = min(max((bin_edge(win[rank - 1]) * p.ratio_q8) >> 8, p.t_lo), p.t_hi)
        thr.append(T)
        if e > T:
            if state == SILENCE:
                state, run_start = ONSET, f
            run_end = f + 1
            if state == ONSET and run_end - run_start >= p.min_speech:
                state = SPEECH
        elif state != SILENCE and f + 1 - run_end >= p.min_silence:
            if state == SPEECH:
                closed.append((run_start, run_end))
            state = SILENCE
    return closed, thr, state


@pytest.mark.parametrize("kw", [dict(window=1), dict(window=40), dict(window=41), dict(percentile=1), dict(percentile=99),
                                dict(min_speech=0), dict(min_silence=1), dict(window=7, percentile=50)])
def test_window_edges_against_a_recount(kw):
    from whisper.vad import StreamVad, resolve_stream_options
    base = resolve_stream_options(floor_db=-70, ceil_db=-20)._replace(window=16, min_silence=3, min_speech=2)
    p = base._replace(**kw)
    x = bursts(np.random.default_rng(3), 41 if kw.get("window") in (40, 41) else 120)
    d = StreamVad(p)
    for f in range(len(x) // 160):
        st = d.feed(x[f * 160:(f + 1) * 160])
        if kw.get("window") in (40, 41) and f + 1 in (40, 41):  # frames exactly W and W + 1
            assert int(d.hist.sum()) == min(f + 1, p.window)
    closed, thr, state = reference_states(x, p)
    assert d.spans == closed and d.thresholds == thr and st.state == state
    assert int(d.hist.sum()) == min(st.frames, p.window) and (len(set(thr)) >= 2 or len(x) < 100 * 160)


def test_zeros_stay_silent_at_the_floor():
    from whisper.vad import StreamVad, resolve_stream_options
    p = resolve_stream_options()
    d = StreamVad(p)
    st = d.feed(np.zeros(16000 * 3 + 55, np.float32))
    assert set(d.thresholds) == {p.t_lo} and st.threshold == p.t_lo
    assert st.state == SILENCE and st.closed_total == 0 and d.onsets_dropped == 0 and st.partial == 0
    assert d.finish().frames == 301


# ---------------------------------------------------------------- option checks
def test_resolve_stream_options():
    from whisper.vad import DEFAULTS, STREAM_DEFAULTS, StreamVad, resolve_options, resolve_stream_options
    p = resolve_stream_options()
    assert set(STREAM_DEFAULTS) == set(DEFAULTS) | {"window"}
    assert (p.window, p.min_silence, p.min_speech, p.pad) == (3000, 50, 25, 40)
    f = resolve_options()
    assert (p.percentile, p.ratio_q8, p.t_lo, p.t_hi) == (f.percentile, f.ratio_q8, f.t_lo, f.t_hi)
    assert resolve_stream_options(window=0.01).window == 1 and resolve_stream_options(window=60).window == 6000
    assert resolve_stream_options(min_speech=0).min_speech == 0
    for bad in (dict(window=0), dict(window=60.01), dict(window=True), dict(window="1"), dict(window=float("nan")),
                dict(min_silence=0), dict(min_silence=0.004), dict(min_silence=20000), dict(min_speech=-1),
                dict(min_speech=20000), dict(percentile=0), dict(percentile=100), dict(percentile=True),
                dict(percentile=10.0), dict(margin_db=41), dict(margin_db=True), dict(floor_db=-30, ceil_db=-40),
                dict(ceil_db=1), dict(pad=-1), dict(pad=float("inf")), dict(windows=3), dict(skip_silence=True)):
        with pytest.raises(ValueError):
            resolve_stream_options(**bad)
    for bad in (dict(window=0), dict(window=6001), dict(min_silence=0), dict(min_speech=-1), dict(percentile=0),
                dict(ratio_q8=255), dict(ratio_q8=2560001), dict(t_lo=2000, t_hi=1000), dict(min_silence=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            StreamVad(P(**bad))


def test_resolve_vad():
    from whisper.streaming import resolve_vad
    from whisper.vad import resolve_stream_options
    assert resolve_vad(None) is None and resolve_vad(False) is None
    assert resolve_vad(True) == resolve_stream_options()
    assert resolve_vad(dict(window=5.0)) == resolve_stream_options(window=5.0)
    assert resolve_vad(P()) == P()
    with pytest.raises(TypeError):
        resolve_vad("yes")
    with pytest.raises(ValueError):
        resolve_vad(dict(window=0))


# ---------------------------------------------------------------- the policy with stubs
def to_s16(x):
    s = np.round(x.astype(np.float64) * 32768).astype(np.int16)
    assert np.array_equal(s.astype(np.float32) / 32768, x)
    return s.tobytes()


class VadStream(CountingStream):
    """CountingStream that carries the twin: 16 kHz mono s16, every sample is emitted as it comes."""

    def __init__(self, params):
        super().__init__()
        self.twin = None
        if params is not None:
            from whisper.vad import StreamVad
            self.twin = StreamVad(params)

    @property
    def vad_state(self):
        return self.twin.state

    def append(self, data):
        got = super().append(data)
        if self.twin is not None:
            self.twin.feed(np.frombuffer(bytes(data), "<i2").astype(np.float32) / 32768)
        return got

    def finish(self):
        if self.twin is not None:
            self.twin.finish()
        return super().finish()


def twin_states(x, params, points):
    """The twin's state after the first ``n`` samples of ``x``, for every n of ``points``."""
    from whisper.vad import StreamVad
    d, pos, out = StreamVad(params), 0, []
    for n in points:
        out.append(d.feed(x[pos:n]))
        pos = n
    return out


def test_composite_states_at_the_decode_points(composite):
    from whisper.vad import resolve_stream_options
    sts = twin_states(composite, resolve_stream_options(), [16000 * k for k in range(1, 13)])
    assert sts[0].state == SILENCE and sts[0].closed_total == 0
    for k in (2, 3, 4, 5, 6):
        assert (sts[k - 1].state, sts[k - 1].run_start) == (SPEECH, 156)
    for k in (7, 8):
        assert (sts[k - 1].state, sts[k - 1].closed_start, sts[k - 1].closed_end) == (SILENCE, 156, 600)
    for k in (9, 10, 11):
        assert (sts[k - 1].state, sts[k - 1].run_start) == (SPEECH, 850)
    assert (sts[11].state, sts[11].closed_start, sts[11].closed_end, sts[11].closed_total) == (SILENCE, 850, 1120, 2)


def test_policy_idle_endpoint_speech(composite):
    from whisper.streaming import StreamingTranscriber
    from whisper.vad import resolve_stream_options
    params = resolve_stream_options()
    log, stream = [], VadStream(params)
    t = StreamingTranscriber(None, 16000, vad=True, min_chunk=1.0, stream=stream, decode_fn=scripted_decode(4, log))
    assert t.vad == params
    data = to_s16(composite)
    sts = twin_states(composite, params, [16000 * k for k in range(1, 13)])
    ups, pending_before, s0_before = [], [], []
    for k in range(12):
        pending_before.append(list(t.pending))
        s0_before.append(t.span[0])
        got = t.feed(data[k * 32000:(k + 1) * 32000])
        assert len(got) == 1
        ups.append(got[0])
        # the cut the policy defines, from the twin's state at this point
        st, u = sts[k], got[0]
        assert u.vad == st
        keep = (st.run_start if st.state == ONSET else st.frames) - params.pad
        if u.idle:
            want = min(max(160 * keep, s0_before[k]), 16000 * (k + 1))
        elif u.endpoint:
            want = min(max(160 * max(st.closed_end, keep), s0_before[k]), 16000 * (k + 1))
        else:
            want = s0_before[k]  # 12.7 s never reach buffer_trim = 15 s
        assert t.span == (want, 16000 * (k + 1)), k + 1
    assert [k + 1 for k, u in enumerate(ups) if u.idle] == [1, 8]
    assert [k + 1 for k, u in enumerate(ups) if u.endpoint] == [7, 12]
    assert [k + 1 for k, u in enumerate(ups) if u.result is not None] == [2, 3, 4, 5, 6, 7, 9, 10, 11, 12]
    assert [span for _, span in log] == [ups[k - 1].span for k in (2, 3, 4, 5, 6, 7, 9, 10, 11, 12)]
    # the cuts in numbers: idle keeps the pad before "now", the endpoint cuts behind the utterance
    assert [u.span[0] for u in ups] == [0] + [9600] * 6 + [105600] + [121600] * 4 and t.span == (185600, 192000)
    for k in (1, 8):
        u = ups[k - 1]
        assert u.result is None and u.committed == [] and u.prompt is None and not u.endpoint and not u.forced
    for k in (7, 12):
        u = ups[k - 1]
        assert pending_before[k - 1] and u.tentative == [] and t.pending == [] if k == 12 else u.tentative == []
        keys = [t.policy.key(w) for w in u.committed]
        assert all(t.policy.key(w) in keys for w in pending_before[k - 1])   # the formerly pending words
        hyp = [w for s in u.result["segments"] for w in s["words"]]
        assert keys[-1] == t.policy.key(hyp[-1])                              # and the rest of the hypothesis
    assert not any(u.idle or u.endpoint for k, u in enumerate(ups, 1) if k in (2, 3, 4, 5, 6, 9, 10, 11))
    n_log = len(log)
    assert t.feed(data[12 * 32000:]) == []
    final = t.finish()
    assert final.final and final.idle and final.result is None and len(log) == n_log and t.pending == []
    assert final.span == (185600, 203200) and final.vad.frames == 1270
    # decode_fn never saw a buffer without confirmed speech
    decoded = [u for u in ups if u.result is not None]
    for u in decoded:
        st = u.vad
        assert 160 * (st.frames if st.state == SPEECH else st.closed_end) > u.span[0]
    assert t.committed and words_of(t.committed) == sorted(set(words_of(t.committed)), key=lambda w: int(w[2:]))


def test_an_onset_is_kept_by_the_idle_cut():
    """A buffer that holds only an onset (not yet min_speech long) is idle, and the cut keeps the onset."""
    from whisper.streaming import StreamingTranscriber
    p = P(t_lo=10 ** 6, t_hi=10 ** 6, window=100, min_silence=50, min_speech=25, pad=5)
    x = np.zeros(32000, np.float32)
    x[14400:] = 0.25  # frames 90.. of the first second are loud: an onset of 10 frames at the decode point
    log, stream = [], VadStream(p)
    t = StreamingTranscriber(None, 16000, vad=p, min_chunk=1.0, stream=stream, decode_fn=scripted_decode(4, log))
    u = t.feed(to_s16(x[:16000]))[0]
    assert (u.vad.state, u.vad.run_start) == (ONSET, 90) and u.idle and not log
    assert t.span == (160 * 85, 16000)
    u = t.feed(to_s16(x[16000:]))[0]
    assert u.vad.state == SPEECH and not u.idle and not u.endpoint and u.span == (160 * 85, 32000) and len(log) == 1


# ---------------------------------------------------------------- the pool with stubs
class VadPool(CountingPool):
    """CountingPool whose detecting slots carry a twin (16 kHz mono s16 streams)."""

    def __init__(self, n_slots, slot_samples):
        super().__init__(n_slots, slot_samples)
        self.twins = {}

    def pool_open(self, slot, encoding, channels, rate):
        super().pool_open(slot, encoding, channels, rate)
        self.twins.pop(slot, None)

    def pool_vad_enable(self, slot, params):
        from whisper.vad import StreamVad
        assert self.slots[slot]["frames"] == 0 and slot not in self.twins
        self.twins[slot] = StreamVad(params)
        self.calls.append(("vad_enable", slot))

    def pool_vad_state(self, slots):
        return [self.twins[s].state for s in slots]

    def pool_append(self, slots, packets, n_frames):
        out = super().pool_append(slots, packets, n_frames)
        for s, p in zip(slots, packets):
            if s in self.twins:
                assert self.slots[s]["rate"] == 16000
                self.twins[s].feed(np.frombuffer(bytes(p), "<i2").astype(np.float32) / 32768)
        return out

    def pool_finish(self, slots):
        out = super().pool_finish(slots)
        for s in slots:
            if s in self.twins:
                self.twins[s].finish()
        return out


def same_update(u, v):
    a, b = dataclasses.asdict(u), dataclasses.asdict(v)
    a.pop("wall_ms"), b.pop("wall_ms")
    return a == b


def test_pool_idle_streams_take_no_lane(composite):
    from whisper.streaming import StreamingTranscriber
    from whisper.streampool import StreamingPool
    from whisper.vad import resolve_stream_options
    data = to_s16(composite)
    zeros = np.zeros(13 * 16000, np.int16).tobytes()
    logs = {}

    def decode_round(items):
        return [scripted_decode(4, logs.setdefault(h, []))(prompt, span) for h, prompt, span in items]

    dev = VadPool(4, 30 * 16000)
    pool = StreamingPool(None, slots=4, slot_samples=30 * 16000, device=dev, decode_round_fn=decode_round)
    ha = pool.open(16000, vad=True)                      # the composite, detecting
    hb = pool.open(16000)                                # the composite, no detector
    hc = pool.open(16000, vad=dict(window=10.0))         # silence, detecting
    assert [c for c in dev.calls if c[0] == "vad_enable"] == [("vad_enable", 0), ("vad_enable", 2)]
    got = {ha: [], hb: [], hc: []}
    piece = 2 * 5000  # 5000 frames a tick: the decode points fall inside packets
    for pos in range(0, len(zeros), piece):
        for h, ups in pool.feed({ha: data[pos:pos + piece], hb: data[pos:pos + piece], hc: zeros[pos:pos + piece]}).items():
            got[h].extend(ups)
    final = pool.finish([ha, hb, hc])
    for h in got:
        got[h].append(final[h])
    # lone transcribers with the same options
    def lone(vad, payload):
        log = []
        t = StreamingTranscriber(None, 16000, vad=vad, stream=VadStream(vad), decode_fn=scripted_decode(4, log))
        return t.feed(payload) + [t.finish()]
    for h, vad, payload in ((ha, resolve_stream_options(), data), (hb, None, data),
                            (hc, resolve_stream_options(window=10.0), zeros)):
        want = lone(vad, payload)
        assert len(got[h]) == len(want) and all(same_update(u, v) for u, v in zip(got[h], want)), h
    assert all(u.vad is None and not u.idle and not u.endpoint for u in got[hb])
    assert all(u.idle and u.result is None and u.committed == [] for u in got[hc]) and hc not in logs
    idle_points = [k + 1 for k, u in enumerate(got[ha][:-1]) if u.idle]
    assert idle_points == [1, 8] and got[ha][-1].idle
    # the rounds: B at every one of its 12 points (and at finish: 0.7 s arrived since); A where it is not idle; never C
    assert len(pool.rounds) == 13
    assert [ha in r for r in pool.rounds] == [k not in (1, 8, 13) for k in range(1, 14)]
    assert all(hb in r and hc not in r for r in pool.rounds)
    pool.close()


def test_pool_runs_no_round_when_nobody_has_speech():
    from whisper.streampool import StreamingPool
    dev = VadPool(2, 30 * 16000)
    pool = StreamingPool(None, slots=2, slot_samples=30 * 16000, device=dev, decode_round_fn=lambda items: 1 / 0)
    hs = [pool.open(16000, vad=True), pool.open(16000, vad=True, min_chunk=0.5)]
    ups = pool.feed({h: np.zeros(3 * 16000, np.int16).tobytes() for h in hs})
    assert [len(ups[h]) for h in hs] == [3, 6] and all(u.idle for h in hs for u in ups[h])
    assert all(u.idle and u.final for u in pool.finish(hs).values()) and pool.rounds == []
    # the idle cuts went out as batched trims, and the buffers stayed short (pad = 0.4 s)
    assert any(c[0] == "trim" for c in dev.calls) and dev.peak <= 16000 + 6400


def test_pool_still_refuses_skip_silence_and_points_to_open():
    from whisper.streampool import StreamingPool
    with pytest.raises(ValueError, match=r"open\(vad="):
        StreamingPool(None, slots=1, device=VadPool(1, 1000), skip_silence=True)


# ---------------------------------------------------------------- unchanged behaviour
def test_vad_none_is_todays_transcriber():
    from whisper.streaming import StreamingTranscriber, StreamUpdate
    second = np.zeros(16000, np.int16).tobytes()
    runs = []
    for kw in (dict(), dict(vad=None)):
        log, stream = [], CountingStream()
        t = StreamingTranscriber(None, 16000, stream=stream, decode_fn=scripted_decode(4, log), min_chunk=1.0,
                                 buffer_trim=4.0, max_buffer=6.0, **kw)
        ups = [u for _ in range(12) for u in t.feed(second)] + [t.finish()]
        runs.append((ups, log, stream.trims))
    (a, la, ta), (b, lb, tb) = runs
    assert la == lb and ta == tb and ta and len(a) == len(b) == 13
    assert all(same_update(u, v) for u, v in zip(a, b))
    assert all(u.vad is None and not u.idle and not u.endpoint for u in a)
    # the defaults of an update: the old fields as they were, the three new ones behind them
    fields = [(f.name, getattr(StreamUpdate(), f.name)) for f in dataclasses.fields(StreamUpdate)]
    assert fields == [("committed", []), ("tentative", []), ("span", (0, 0)), ("prompt", None), ("language", None),
                      ("result", None), ("forced", False), ("final", False), ("wall_ms", 0.0), ("idle", False),
                      ("endpoint", False), ("vad", None)]
