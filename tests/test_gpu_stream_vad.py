"""Voice activity of live streams on the GPU (wh_pool_vad_* / wh_stream_vad_*, csrc/wh_svad.hip).

* G1: the detector state after every batched append equals the numpy twin's (``vad.StreamVad``)
  fed the same emitted samples, field by field; ring and histogram too; finish closes the
  zero-padded last frame.
* G2: trims between appends change nothing.
* G3: one append of 30 s (3000 frames, a 3000-frame window), then the ring wraps.
* G4: the single stream gives a pool slot's states; detecting and plain slots in one call.
* G5: refusals change nothing.
* G6: ``StreamingPool`` with ``vad`` gives every stream the updates of a lone
  ``StreamingTranscriber(vad=True)``; idle streams take no lane."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from wav_fixture import CONTAINER, ENCODINGS, encode, wav_bytes

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
# the micro dims and the five formats of tests/test_gpu_stream_pool.py, and its helpers, copied so
# that these tests check what they say whatever becomes of that file
DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
            n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)
FIVE = [(8000, "ulaw", 1), (44100, "s24", 2), (48000, "s16", 1), (16000, "f32", 2), (44100, "s16", 1)]
SIX = FIVE + [(16000, "s16", 1)]
N_SLOTS, SLOT_SAMPLES = 6, 24000
SEEDS = (12, 1, 2, 6, 3, 7)   # per slot, picked on the CPU with the twin so that G1's conditions on the inputs hold
SILENCE, ONSET, SPEECH = 0, 1, 2


def E(n, rate, final=False):
    from whisper.audio import stream_emitted
    return stream_emitted(n, rate, final)


class Rec:
    """A recording in a slot: its bytes, its one-shot samples (device and host, which agree) and
    how far it has been fed."""

    def __init__(self, ctx, slot, rate, enc, ch, v):
        from whisper.audio import pcm_to_waveform, wav_info, wav_samples
        self.v = v
        self.slot, self.rate, self.enc, self.ch, self.n = slot, rate, enc, ch, len(v)
        self.fb = CONTAINER[enc] * ch
        self.raw = np.frombuffer(encode(enc, v), np.uint8)
        data = wav_bytes(enc, self.raw.tobytes(), ch, rate)
        d = ctx.wav_ingest(data)
        self.want = ctx.audio_read(0, d.n_samples)
        pcm, bits = wav_samples(data, wav_info(data))
        self.host = pcm_to_waveform(pcm, rate, bits)
        assert np.array_equal(self.want, self.host)
        self.pos = self.out = self.dropped = 0

    def open(self, ctx):
        ctx.pool_open(self.slot, ENCODINGS.index(self.enc), self.ch, self.rate)
        self.pos = self.out = self.dropped = 0
        return self

    def take(self, n):
        n = min(n, self.n - self.pos)
        return self.raw[self.pos * self.fb:(self.pos + n) * self.fb], n

    def resident(self, ctx):
        return ctx.pool_read(self.slot, 0, self.out - self.dropped)


def append(ctx, recs, sizes):
    """One batched append of ``sizes[i]`` frames of ``recs[i]``; every n_out is E(after) - E(before)."""
    packets = [r.take(n) for r, n in zip(recs, sizes)]
    got = ctx.pool_append([r.slot for r in recs], [p for p, _ in packets], [n for _, n in packets])
    for r, (_, n), g in zip(recs, packets, got):
        assert g == E(r.pos + n, r.rate) - E(r.pos, r.rate), (r.slot, r.pos, n, g)
        r.pos += n
        r.out += g
    return got


def finish(ctx, recs):
    got = ctx.pool_finish([r.slot for r in recs])
    for r, g in zip(recs, got):
        assert g == E(r.pos, r.rate, True) - E(r.pos, r.rate) and r.out + g == E(r.pos, r.rate, True)
        r.out += g


def load(max_windows):
    import whisper
    return whisper.load_model("micro", device=0, dtype="fp32", max_windows=max_windows, max_group=5, synthetic=True)


def assert_same_words(a, b):
    assert [(w["word"], w["start"], w["end"]) for w in a] == [(w["word"], w["start"], w["end"]) for w in b]
    for wa, wb in zip(a, b):
        assert wa["probability"] == pytest.approx(wb["probability"], rel=1e-5)


def assert_same_updates(got, want):
    """The comparison of tests/test_gpu_stream_pool.py, plus ``idle``, ``endpoint`` and ``vad``."""
    assert len(got) == len(want)
    for u, v in zip(got, want):
        assert (u.span, u.prompt, u.language, u.forced, u.final) == (v.span, v.prompt, v.language, v.forced, v.final)
        assert (u.idle, u.endpoint, u.vad) == (v.idle, v.endpoint, v.vad)
        assert_same_words(u.committed, v.committed)
        assert_same_words(u.tentative, v.tentative)
        assert (u.result is None) == (v.result is None)
        if u.result is not None:
            assert u.result["language"] == v.result["language"] and u.result["text"] == v.result["text"]
            assert len(u.result["segments"]) == len(v.result["segments"])
            for a, b in zip(u.result["segments"], v.result["segments"]):
                assert (a["tokens"], a["text"], a["start"], a["end"]) == (b["tokens"], b["text"], b["start"], b["end"])
                assert_same_words(a["words"], b["words"])


def params():
    from whisper.vad import resolve_stream_options
    p = resolve_stream_options(window=0.16, min_silence=0.03, min_speech=0.02, floor_db=-70, ceil_db=-20)
    assert (p.window, p.min_silence, p.min_speech) == (16, 3, 2)
    return p


def burst_values(rng, rate, enc, ch, seconds=1.2):
    """Values for ``encode``: each 10 ms segment's amplitude drawn from {0, 2e-3, 0.3} in runs of
    1..8 segments, times noise."""
    from whisper.audio import WAV_ULAW, g711_table
    seg = rate // 100
    n = int(seconds * 100) * seg + 3
    x = np.zeros((n, ch))
    f = 0
    while f * seg < n:
        k = int(rng.integers(1, 9))
        a = float(rng.choice([0.0, 2e-3, 0.3]))
        m = min((f + k) * seg, n) - f * seg
        x[f * seg:f * seg + m] = a * rng.uniform(-1, 1, (m, 1))
        f += k
    if enc == "f32":
        return x
    if enc == "ulaw":
        table = g711_table(WAV_ULAW).astype(np.int64)
        return np.abs(table[None, :] - np.round(x * 32768).astype(np.int64).reshape(-1, 1)).argmin(axis=1).reshape(n, ch)
    return np.round(x * (1 << (8 * CONTAINER[enc] - 1)) * 0.999).astype(np.int64)


@pytest.fixture(scope="module")
def ctx():
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    c = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    c.set_mel_filters(80, mel_filters(None, 80))
    c.pool_create(N_SLOTS, SLOT_SAMPLES)
    yield c
    c.close()


@pytest.fixture(scope="module")
def six(ctx):
    """The six burst recordings, slots 0..5; computed once, never changed."""
    out = []
    for s, (rate, enc, ch) in enumerate(SIX):
        v = burst_values(np.random.default_rng([SEEDS[s], s]), rate, enc, ch)
        out.append(Rec(ctx, s, rate, enc, ch, v))
    return out


def close_all(ctx):
    from whisper.backend_hip import HipBackendError
    for s in range(N_SLOTS):
        try:
            ctx.pool_close(s)
        except HipBackendError:
            pass


def packet_sizes(rng, r):
    """0 frames; less than one detector frame of output; up to the next frame boundary; several frames."""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return 0
    if kind == 1:
        return int(rng.integers(1, r.rate // 200))
    if kind == 2:
        for n in range(1, r.rate // 40):
            if E(r.pos + n, r.rate) > E(r.pos, r.rate) and E(r.pos + n, r.rate) % 160 == 0:
                return n
    return int(rng.integers(r.rate // 100, 6 * r.rate // 100))


def run_six(ctx, six, trims):
    """The six recordings through batched appends of random packets; the states after every call."""
    from whisper.vad import StreamVad
    close_all(ctx)
    p = params()
    rng = np.random.default_rng(11)
    recs = [r.open(ctx) for r in six]
    twins = [StreamVad(p) for _ in recs]
    for r in recs:
        ctx.pool_vad_enable(r.slot, p)
    assert ctx.pool_vad_state([r.slot for r in recs]) == [t.state for t in twins]
    history, kinds = [], set()
    while any(r.pos < r.n for r in recs):
        on = [r for r in recs if r.pos < r.n]
        sizes = [packet_sizes(rng, r) for r in on]
        before = [r.out for r in on]
        append(ctx, on, sizes)
        for r, b in zip(on, before):
            st = twins[r.slot].feed(r.want[b:r.out])
            kinds.add("none" if r.out == b else "edge" if r.out % 160 == 0 else "small" if r.out - b < 160 else "many")
        got = ctx.pool_vad_state([r.slot for r in recs])
        assert got == [t.state for t in twins], [(g, t.state) for g, t in zip(got, twins) if g != t.state][:1]
        history.append(got)
        if trims:
            live = [r for r in recs if r.out > r.dropped]
            if live:
                ctx.pool_trim([r.slot for r in live], [r.out - r.dropped for r in live])
                for r in live:
                    r.dropped = r.out
    assert kinds == {"none", "small", "edge", "many"}
    for r, t in zip(recs, twins):
        ring, hist = ctx.pool_vad_read(r.slot, p.window)
        assert np.array_equal(ring, t.ring) and np.array_equal(hist, t.hist), r.slot
    finish(ctx, recs)
    for r, t in zip(recs, twins):
        t.feed(r.want[t.samples:r.out])
        t.finish()
    final = ctx.pool_vad_state([r.slot for r in recs])
    assert final == [t.state for t in twins]
    assert all(s.frames == -(-s.samples // 160) and s.partial == 0 and s.samples == len(r.want) for s, r in zip(final, recs))
    assert any(s.samples % 160 for s in final)   # a zero-padded last frame was closed
    for r, t in zip(recs, twins):
        ring, hist = ctx.pool_vad_read(r.slot, p.window)
        assert np.array_equal(ring, t.ring) and np.array_equal(hist, t.hist), r.slot
    # a second finish changes nothing
    assert ctx.pool_finish([r.slot for r in recs]) == [0] * 6 and ctx.pool_vad_state([r.slot for r in recs]) == final
    return history + [final], twins


# ---------------------------------------------------------------- G1, G2
def test_g1_states_equal_the_twin_after_every_batched_append(ctx, six):
    history, twins = run_six(ctx, six, trims=False)
    p = params()
    for t in twins:   # the inputs are not trivial
        assert len(t.spans) >= 3 and t.onsets_dropped >= 1 and len(set(t.thresholds)) >= 3 and t.frames > 4 * p.window
    assert len(history) > 20


def test_g2_trims_do_not_matter(ctx, six):
    plain, _ = run_six(ctx, six, trims=False)
    trimmed, _ = run_six(ctx, six, trims=True)
    assert plain == trimmed
    assert any(s.partial for states in trimmed for s in states)   # trims fell inside frames


# ---------------------------------------------------------------- G3
def G3_signal(rng, n):
    """Bursts over a background that is zero for 1 s, then -60 dB, then -48 dB noise: the
    percentile moves as the window fills and again as the ring wraps."""
    x = np.zeros(n)
    x[16000:240000] = 1e-3
    x[240000:] = 4e-3
    for _ in range(40):
        a = int(rng.integers(0, n - 16000))
        x[a:a + int(rng.integers(800, 16000))] = float(rng.choice([0.02, 0.3]))
    return x * rng.uniform(-1, 1, n)


def test_g3_one_long_append_and_a_wrapping_ring():
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    from whisper.streampool import DEFAULT_SLOT_SAMPLES
    from whisper.vad import StreamVad, resolve_stream_options
    p = resolve_stream_options()
    assert p.window == 3000
    rng = np.random.default_rng(7)
    n = 30 * 16000 + 77
    x = G3_signal(rng, n + 200 * 160)
    s16 = np.round(x * 32767).astype("<i2")
    w = s16.astype(np.float32) / 32768
    c = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    try:
        c.pool_create(1, DEFAULT_SLOT_SAMPLES)
        c.pool_open(0, ENCODINGS.index("s16"), 1, 16000)
        c.pool_vad_enable(0, p)
        twin = StreamVad(p)
        assert c.pool_append([0], [s16[:n].view(np.uint8)], [n]) == [n]
        assert np.array_equal(c.pool_read(0, 0, n), w[:n])
        assert c.pool_vad_state([0]) == [twin.feed(w[:n])] and twin.frames == 3000 and twin.samples % 160 == 77
        ring, hist = c.pool_vad_read(0, 3000)
        assert np.array_equal(ring, twin.ring) and np.array_equal(hist, twin.hist)
        c.pool_trim([0], [n])
        rest = s16[n:]
        assert c.pool_append([0], [rest.view(np.uint8)], [len(rest)]) == [len(rest)]
        assert c.pool_vad_state([0]) == [twin.feed(w[n:])] and twin.frames == 3200
        ring, hist = c.pool_vad_read(0, 3000)
        assert np.array_equal(ring, twin.ring) and np.array_equal(hist, twin.hist) and int(hist.sum()) == 3000
        assert twin.closed_total >= 3 and len(set(twin.thresholds)) >= 2
    finally:
        c.close()


# ---------------------------------------------------------------- G4
def test_g4_single_stream_and_mixed_calls(ctx, six):
    from whisper.backend_hip import HipBackendError
    from whisper.streaming import AudioStream
    from whisper.vad import StreamVad
    close_all(ctx)
    p = params()
    # the single stream against the twin fed the same packets.  G1 holds every pool slot to that same twin
    # after every call, so the stream's states are those of a pool slot fed these packets
    for r in (six[1], six[0], six[5]):
        stream = AudioStream(ctx, r.rate, r.enc, r.ch, vad=p)
        twin = StreamVad(p)
        assert stream.vad_state == twin.state
        rng = np.random.default_rng(3)
        pos = out = 0
        while pos < r.n:
            n = min(int(rng.integers(0, r.rate // 20)), r.n - pos)
            got = stream.append(r.raw[pos * r.fb:(pos + n) * r.fb].tobytes())
            assert stream.vad_state == twin.feed(r.want[out:out + got])
            pos, out = pos + n, out + got
            if rng.integers(0, 3) == 0 and stream.n_samples:
                stream.trim(stream.n_samples)
        got = stream.finish()
        twin.feed(r.want[out:out + got])
        assert stream.vad_state == twin.finish() and twin.samples == len(r.want)
        assert stream.finish() == 0 and stream.vad_state == twin.state
    # a stream without a detector has no state; a new stream drops the old detector
    plain = AudioStream(ctx, 16000, "s16", 1)
    assert plain.vad_state is None
    with pytest.raises(HipBackendError, match="no detector"):
        ctx.stream_vad_state()
    # detecting (0, 2, 4) and plain (1, 3, 5) slots in the same calls
    recs = [r.open(ctx) for r in six]
    for r in recs[::2]:
        ctx.pool_vad_enable(r.slot, p)
    twins = {r.slot: StreamVad(p) for r in recs[::2]}
    rng = np.random.default_rng(9)
    while any(r.pos < r.n for r in recs):
        on = [r for r in recs if r.pos < r.n]
        before = [r.out for r in on]
        append(ctx, on, [int(rng.integers(0, r.rate // 10)) for r in on])
        for r, b in zip(on, before):
            if r.slot in twins:
                twins[r.slot].feed(r.want[b:r.out])
        assert ctx.pool_vad_state([0, 2, 4]) == [twins[s].state for s in (0, 2, 4)]
    finish(ctx, recs)
    for r in recs:   # every slot's samples are the one-shot ingest's, detector or not
        assert np.array_equal(r.resident(ctx), r.want), r.slot
    for s in (1, 3, 5):
        with pytest.raises(HipBackendError, match="no detector"):
            ctx.pool_vad_state([0, s])
        with pytest.raises(HipBackendError, match="no detector"):
            ctx.pool_vad_read(s, 16)
    # closing drops the detector: the slot opens plain again
    ctx.pool_close(0)
    recs[0].open(ctx)
    with pytest.raises(HipBackendError, match="no detector"):
        ctx.pool_vad_state([0])


# ---------------------------------------------------------------- G5
def test_g5_refusals_change_nothing(ctx, six):
    from whisper.backend_hip import WhSvadOpts, WhSvadState
    close_all(ctx)
    p = params()
    lib = ctx.lib
    a, b, c = (six[k].open(ctx) for k in (5, 0, 2))   # slots 5, 0, 2
    ctx.pool_vad_enable(a.slot, p)
    append(ctx, [a, b], [1000, 700])
    ctx.pool_finish([c.slot])

    def opts(**kw):
        o = ctx._svad_opts(p)
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def state():
        return (ctx.pool_vad_state([a.slot]), [ctx.pool_info(s) for s in (a.slot, b.slot, c.slot)],
                a.resident(ctx), b.resident(ctx), ctx.pool_vad_read(a.slot, 16))

    def rc_of(fn, *args):
        rc = fn(ctx.h, *args)
        return rc, lib.wh_last_error().decode()

    out = (WhSvadState * 2)()
    ring = np.zeros(64, np.uint8)
    I32 = lambda *v: np.asarray(v, np.int32).ctypes.data_as(ctypes.c_void_p)
    before = state()
    refusals = [
        (lib.wh_pool_vad_enable, (1, None), -1, ["opts"]),
        (lib.wh_pool_vad_enable, (3, opts()), -7, ["not open"]),
        (lib.wh_pool_vad_enable, (N_SLOTS, opts()), -7, ["outside"]),
        (lib.wh_pool_vad_enable, (b.slot, opts()), -7, ["already taken frames"]),
        (lib.wh_pool_vad_enable, (c.slot, opts()), -7, ["already taken frames"]),
        (lib.wh_pool_vad_enable, (a.slot, opts()), -7, ["already"]),
        (lib.wh_pool_vad_state, (2, I32(a.slot, b.slot), out), -7, ["slots[1]", "no detector"]),
        (lib.wh_pool_vad_state, (1, I32(a.slot), None), -1, ["out"]),
        (lib.wh_pool_vad_state, (1, I32(3), out), -7, ["not open"]),
        (lib.wh_pool_vad_read, (b.slot, ring.ctypes.data_as(ctypes.c_void_p), 64, None), -7, ["no detector"]),
        (lib.wh_pool_vad_read, (a.slot, None, 64, None), -1, ["ring"]),
        (lib.wh_pool_vad_read, (a.slot, ring.ctypes.data_as(ctypes.c_void_p), 15, None), -7, ["cap"]),
    ]
    ctx.pool_open(1, ENCODINGS.index("s16"), 1, 16000)   # an open, empty slot for the option checks
    for kw, word in ((dict(percentile=0), "percentile"), (dict(percentile=100), "percentile"), (dict(ratio_q8=255), "ratio_q8"),
                     (dict(ratio_q8=2560001), "ratio_q8"), (dict(t_lo=p.t_hi + 1), "t_lo"), (dict(window=0), "window"),
                     (dict(window=6001), "window"), (dict(min_silence=0), "min_silence"),
                     (dict(min_silence=(1 << 20) + 1), "min_silence"), (dict(min_speech=-1), "min_speech"),
                     (dict(min_speech=(1 << 20) + 1), "min_speech")):
        refusals.append((lib.wh_pool_vad_enable, (1, opts(**kw)), -7, [word]))
    for fn, args, code, words in refusals:
        rc, msg = rc_of(fn, *args)
        assert rc == code and "pool" in msg and all(w in msg for w in words), (fn.__name__, args, rc, msg)
        after = state()
        assert after[0] == before[0] and after[1] == before[1], fn.__name__
        assert all(np.array_equal(x, y) for x, y in zip(after[2:4], before[2:4])), fn.__name__
        assert np.array_equal(after[4][0], before[4][0]) and np.array_equal(after[4][1], before[4][1])
        assert not ring.any()
    # slot 1 never got a detector from the refused enables
    rc, msg = rc_of(lib.wh_pool_vad_state, 1, I32(1), out)
    assert rc == -7 and "no detector" in msg
    # the single stream's refusals
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 16000)
    for fn, args, code, words in ((lib.wh_stream_vad_enable, (None,), -1, ["opts"]),
                                  (lib.wh_stream_vad_enable, (opts(window=0),), -7, ["window"]),
                                  (lib.wh_stream_vad_state, (None,), -1, ["out"]),
                                  (lib.wh_stream_vad_state, (out,), -7, ["no detector"])):
        rc, msg = rc_of(fn, *args)
        assert rc == code and "stream" in msg and all(w in msg for w in words), (fn.__name__, rc, msg)
    ctx.stream_append(np.zeros(20, np.uint8), 10)
    rc, msg = rc_of(lib.wh_stream_vad_enable, opts())
    assert rc == -7 and "already taken frames" in msg
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 16000)
    ctx.stream_vad_enable(p)
    rc, msg = rc_of(lib.wh_stream_vad_enable, opts())
    assert rc == -7 and "already detecting" in msg
    ctx.audio_upload(np.zeros(100, np.float32))   # ends the stream, and with it the detector
    rc, msg = rc_of(lib.wh_stream_vad_state, out)
    assert rc == -7 and "no open stream" in msg
    # only the two ingest counters move on an append with a detecting slot
    stats = ctx.stats()
    append(ctx, [a, b], [500, 500])
    assert {k for k, v in ctx.stats().items() if v != stats[k]} == {"ingest_copy_ms", "ingest_kernel_ms"}


# ---------------------------------------------------------------- G6
@pytest.fixture(scope="module")
def micro32():
    m = load(4)
    yield m
    m.close()


@pytest.fixture(scope="module")
def streams():
    """(rate, encoding, channels, options, bytes, the 16 kHz samples) of the three streams."""
    from whisper.audio import load_audio, read_pcm
    W = load_audio(JFK)
    z = lambda s: np.zeros(int(round(s * 16000)), np.float32)
    comp = np.concatenate([z(1.5), W[:72000], z(2.5), W[84800:128000], z(1.5)])
    s16 = np.round(comp.astype(np.float64) * 32768).astype(np.int16)
    assert np.array_equal(s16.astype(np.float32) / 32768, comp) and len(comp) == 203200
    pcm, rate, bits = read_pcm(JFK)
    assert (rate, bits, pcm.shape[1]) == (44100, 24, 2)
    return [(16000, "s16", 1, dict(min_chunk=1.0, language="en"), s16.tobytes(), comp),
            (44100, "s24", 2, dict(min_chunk=2.0, language="en"), encode("s24", pcm), W),
            (8000, "ulaw", 1, dict(min_chunk=1.0, language="en"), bytes([0xFF]) * 40000, np.zeros(80000, np.float32))]


@pytest.fixture(scope="module")
def lone(micro32, streams):
    import whisper
    out = []
    for rate, enc, ch, opts, data, _ in streams:
        t = whisper.StreamingTranscriber(micro32, rate, enc, ch, temperature=0.0, vad=True, **opts)
        ups = t.feed(data)
        out.append((ups + [t.finish()], t))
    return out


def test_g6_the_pool_with_detectors_transcribes_as_lone_transcribers_do(micro32, streams, lone):
    """The composite is decoded at 10 of its 12 points: idle at 1 and 8, as the twin's states say
    (a decode at 2-7 and 9-12), and not at finish."""
    import whisper
    from whisper.vad import StreamVad, resolve_stream_options
    p = resolve_stream_options()
    with whisper.StreamingPool(micro32, slots=4, temperature=0.0) as pool:
        handles = [pool.open(*s[:3], vad=True, **s[3]) for s in streams]
        got = {h: [] for h in handles}
        pos = [0, 0, 0]
        piece = [int(0.37 * s[0]) * CONTAINER[s[1]] * s[2] for s in streams]
        cuts_ok = 0
        while any(pos[k] < len(streams[k][4]) for k in range(3)):
            packets = {}
            for k, h in enumerate(handles):
                if pos[k] < len(streams[k][4]):
                    packets[h] = streams[k][4][pos[k]:pos[k] + piece[k]]
                    pos[k] += piece[k]
            for h, ups in pool.feed(packets).items():
                got[h].extend(ups)
                for u in ups:
                    if u.endpoint:   # nothing is left pending behind an endpoint
                        assert u.tentative == [] and pool.stream(h).pending == []
        final = pool.finish(handles)
        rounds = pool.rounds
    ups = [got[h] + [final[h]] for h in handles]
    for k in range(3):
        want = lone[k][0]
        assert_same_updates(ups[k], want)
        assert [(u.idle, u.endpoint, u.vad) for u in ups[k]] == [(v.idle, v.endpoint, v.vad) for v in want]
        # the flags and the cuts are those the twin predicts from the samples
        rate, chunk, x = streams[k][0], int(round(streams[k][3]["min_chunk"] * streams[k][0])), streams[k][5]
        twin, fed = StreamVad(p), 0
        for i, u in enumerate(ups[k]):
            n = len(x) if u.final else E((i + 1) * chunk, rate)
            st = twin.feed(x[fed:n])
            fed = n
            if u.final:
                st = twin.finish()
            assert u.vad == st, (k, i)
            speech_end = st.frames if st.state == SPEECH else st.closed_end
            idle = 160 * speech_end <= u.span[0]
            assert (u.idle, u.endpoint) == (idle, not idle and st.state != SPEECH), (k, i)
            assert u.span[1] == n
            if u.idle:
                assert u.result is None and (u.final or u.committed == [])
            if (u.idle or u.endpoint) and not u.final:
                keep = (st.run_start if st.state == ONSET else st.frames) - p.pad
                cut = keep if u.idle else max(st.closed_end, keep)
                assert ups[k][i + 1].span[0] == min(max(160 * cut, u.span[0]), u.span[1]), (k, i)
    comp, jfk, zeros = ups
    assert [i + 1 for i, u in enumerate(comp[:-1]) if u.idle] == [1, 8] and comp[-1].idle and comp[-1].result is None
    assert [i + 1 for i, u in enumerate(comp[:-1]) if u.endpoint] == [7, 12]
    assert sum(u.result is not None for u in comp) == 10 and len(comp) == 13
    # JFK at min_chunk = 2.0: the twin is in SPEECH at frames 200, 400, 600, 800 and 1000 (its pauses close
    # between the points), so it has no endpoint and no idle point: only the composite has endpoints here
    assert [i + 1 for i, u in enumerate(jfk) if u.endpoint] == [] and [i + 1 for i, u in enumerate(jfk) if u.idle] == []
    assert len(jfk) == 6 and all(u.result is not None for u in jfk)
    assert all(u.idle and u.result is None and u.committed == [] for u in zeros) and len(zeros) == 6
    # idle streams take no lane
    assert all(handles[2] not in r for r in rounds)
    n_rounds_with = {h: sum(h in r for r in rounds) for h in handles}
    assert n_rounds_with[handles[0]] == 10 and n_rounds_with[handles[1]] == sum(u.result is not None for u in jfk)
