"""The stream pool on the GPU (wh_pool_*, whisper/streampool.py).

* Each slot obeys the single stream's contract while its packets travel in batched calls with
  those of other slots: the samples are bit for bit the one-shot ingest's (``np.array_equal``),
  every ``n_out[i]`` is E(after) - E(before).
* The block map: streams that emit nothing, exactly one block, one block and one sample, several
  blocks and no frames at all in one launch, listed against the slot order.
* A batched trim keeps every remainder, later appends stay seamless.
* The pool and the context's resident audio / single stream do not touch each other.
* ``pool_log_mel`` is ``log_mel_batch`` of the same samples.
* Refused calls change nothing.
* ``StreamingPool`` gives every stream the updates of a lone ``StreamingTranscriber``."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_audio_ingest_host import ratio
from wav_fixture import CONTAINER, ENCODINGS, encode, random_values, wav_bytes

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
            n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)
N_SLOTS, SLOT_SAMPLES = 6, 6000
FIVE = [(8000, "ulaw", 1), (44100, "s24", 2), (48000, "s16", 1), (16000, "f32", 2), (44100, "s16", 1)]


@pytest.fixture(scope="module")
def ctx():
    """A context of its own with a small pool."""
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    c = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    c.set_mel_filters(80, mel_filters(None, 80))
    c.pool_create(N_SLOTS, SLOT_SAMPLES)
    yield c
    c.close()


def E(n, rate, final=False):
    from whisper.audio import stream_emitted
    return stream_emitted(n, rate, final)


def history(rate):
    up, down = ratio(rate)
    return 0 if up == down else 2 * 10 * max(up, down) // up


class Rec:
    """A recording in a slot: its bytes, its one-shot samples (device and host, which agree) and
    how far it has been fed."""

    def __init__(self, ctx, slot, rate, enc, ch, n, seed=0, v=None):
        from whisper.audio import pcm_to_waveform, wav_info, wav_samples
        if v is None:
            rng = np.random.default_rng([rate, ENCODINGS.index(enc), ch, seed])
            v = random_values(rng, enc, n, ch)
            if enc == "f32":  # non-finite and out-of-range samples among the rest
                flat = v.reshape(-1)
                flat[rng.choice(flat.size, 12, replace=False)] = np.tile([np.nan, np.inf, -np.inf, 1e30], 3)
        self.v = v
        self.slot, self.rate, self.enc, self.ch, self.n = slot, rate, enc, ch, n
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

    def check(self, ctx, finished=False):
        assert ctx.pool_info(self.slot) == (self.pos, self.out, self.dropped, finished)
        assert np.array_equal(self.resident(ctx), self.want[self.dropped:self.out])
        with pytest.raises(Exception):
            ctx.pool_read(self.slot, 0, self.out - self.dropped + 1)


def close_all(ctx):
    from whisper.backend_hip import HipBackendError
    for s in range(N_SLOTS):
        try:
            ctx.pool_close(s)
        except HipBackendError:
            pass


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


@pytest.fixture(scope="module")
def five(ctx):
    """The five recordings of 0.3 s + 3 frames, slots 0..4; computed once, never changed."""
    return [Rec(ctx, s, rate, enc, ch, int(0.3 * rate) + 3) for s, (rate, enc, ch) in enumerate(FIVE)]


# ---------------------------------------------------------------- the sample contract
def test_batched_appends_give_the_one_shot_samples(ctx, five):
    close_all(ctx)
    rng = np.random.default_rng(5)
    recs = [r.open(ctx) for r in five]
    ticks = 0
    while any(r.pos < r.n for r in recs):
        sizes = [int(rng.integers(0, 2 * (history(r.rate) or 40) + 1)) for r in recs]
        on = [(r, n) for r, n in zip(recs, sizes) if n and r.pos < r.n]  # a draw of 0 leaves the slot out
        if on:
            append(ctx, [r for r, _ in on], [n for _, n in on])
            ticks += 1
    assert ticks > 20
    finish(ctx, recs)
    for r in recs:
        assert r.out == len(r.want)
        got = r.resident(ctx)
        bad = np.flatnonzero(got != r.want)
        assert len(bad) == 0, (r.slot, r.rate, r.enc, len(bad), int(bad[0]))
        assert np.array_equal(got, r.host)
        assert ctx.pool_info(r.slot) == (r.n, len(r.want), 0, True)
    # one-frame chunks, on the first 300 frames of every slot
    close_all(ctx)
    short = [Rec(ctx, r.slot, r.rate, r.enc, r.ch, 300, v=r.v[:300]).open(ctx) for r in five]
    for _ in range(300):
        append(ctx, short, [1] * 5)
    finish(ctx, short)
    for s in short:
        assert np.array_equal(s.resident(ctx), s.want) and np.array_equal(s.resident(ctx), s.host)


def test_block_map_edges_in_one_call(ctx, five):
    close_all(ctx)
    ulaw8, s24, s48, f32, s44 = five
    s48b = Rec(ctx, 5, 48000, "s16", 1, s48.n, seed=1)
    recs = [r.open(ctx) for r in (ulaw8, s24, s48, f32, s44, s48b)]
    # what the first call gives each slot, listed against the slot order
    first = {s44.slot: 20,     # too short to emit anything: only its history block runs
             s48.slot: 798,    # exactly 256 outputs: one output block and the history block
             s48b.slot: 799,   # 257: a second output block with one sample
             s24.slot: 5000,   # several blocks
             f32.slot: 256,    # no filter: 256 outputs in one block, no history block
             ulaw8.slot: 0}    # no frames at all
    assert E(20, 44100) == 0 and history(44100) > 20
    assert E(798, 48000) == 256 and E(799, 48000) == 257 and E(5000, 44100) > 4 * 256 and E(256, 16000) == 256
    order = sorted(recs, key=lambda r: -r.slot)
    got = append(ctx, order, [first[r.slot] for r in order])
    assert got == [257, 0, 256, 256, E(5000, 44100), 0]
    for r in recs:
        r.check(ctx)
    # the next tick proves that the 20 frames went into the history: everything else arrives
    append(ctx, order, [r.n for r in order])
    finish(ctx, order)
    for r in recs:
        r.check(ctx, finished=True)
        assert r.out == len(r.want)


# ---------------------------------------------------------------- trim
def test_batched_trim(ctx, five):
    close_all(ctx)
    recs = [r.open(ctx) for r in five]
    append(ctx, recs, [r.n // 2 for r in recs])
    shares = (0.0, 0.3, 0.8, 1.0)   # slot 4 is not in the call
    for _ in range(2):   # the second time from the other buffer of every slot that moved
        drops = [int((r.out - r.dropped) * s) for r, s in zip(recs, shares)]
        drops[3] = recs[3].out - recs[3].dropped
        ctx.pool_trim([r.slot for r in recs[:4]][::-1], drops[::-1])
        for r, d in zip(recs, drops):
            r.dropped += d
        for r in recs:
            r.check(ctx)
        append(ctx, recs, [r.n // 5 for r in recs])   # seamless against the one-shot samples
        for r in recs:
            r.check(ctx)
    append(ctx, recs, [r.n for r in recs])
    finish(ctx, recs)
    for r in recs:
        r.check(ctx, finished=True)
    # a trim after finish, and down to nothing
    drops = [(r.out - r.dropped) // 3 for r in recs]
    ctx.pool_trim([r.slot for r in recs], drops)
    for r, d in zip(recs, drops):
        r.dropped += d
        r.check(ctx, finished=True)
    ctx.pool_trim([recs[1].slot], [recs[1].out - recs[1].dropped])
    recs[1].dropped = recs[1].out
    for r in recs:
        r.check(ctx, finished=True)
    assert ctx.pool_info(1) == (recs[1].n, len(recs[1].want), len(recs[1].want), True)


# ---------------------------------------------------------------- isolation
def test_pool_and_resident_audio_do_not_touch_each_other(ctx, five):
    close_all(ctx)
    recs = [r.open(ctx) for r in five[:3]]
    append(ctx, recs, [r.n // 3 for r in recs])

    def pool_state():
        return [(ctx.pool_info(r.slot), r.resident(ctx)) for r in recs]

    def same(a, b):
        return all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))

    before = pool_state()
    # the context's own audio calls between pool appends
    up = np.linspace(-1, 1, 777, dtype=np.float32)
    ctx.audio_upload(up)
    assert same(pool_state(), before)
    ctx.wav_ingest(wav_bytes("s16", five[2].raw.tobytes(), 1, 48000))
    assert same(pool_state(), before)
    pcm = np.random.default_rng(4).integers(-32768, 32768, (4000, 1), dtype=np.int16)
    ctx.stream_begin(ENCODINGS.index("s16"), 1, 44100)
    n0 = ctx.stream_append(pcm.view(np.uint8).reshape(-1), 4000)
    ctx.stream_trim(100)
    ctx.log_mel_resident(n0 - 100, 80, padding=480000)
    assert same(pool_state(), before)
    # pool calls leave the single stream and the resident segment as they are
    single = (ctx.stream_info(), ctx.audio_read(0, n0 - 100))
    append(ctx, recs, [r.n // 3 for r in recs])
    ctx.pool_trim([recs[0].slot, recs[2].slot], [50, 60])
    recs[0].dropped, recs[2].dropped = 50, 60
    ctx.pool_log_mel([r.slot for r in recs], 80, padding=480000)
    append(ctx, recs[:1], [recs[0].n])   # the rest of the first recording, so that its end is the one-shot's
    finish(ctx, recs[:1])
    assert ctx.stream_info() == single[0] == (4000, n0, 100, False)
    assert np.array_equal(ctx.audio_read(0, n0 - 100), single[1])
    n1 = ctx.stream_append(pcm.view(np.uint8).reshape(-1), 4000)   # and the single stream goes on
    assert n1 == E(8000, 44100) - E(4000, 44100)
    recs[0].check(ctx, finished=True)
    for r in recs[1:]:
        r.check(ctx)


# ---------------------------------------------------------------- the mel
def test_pool_log_mel_is_log_mel_batch_of_the_same_samples(ctx, five):
    close_all(ctx)
    recs = [r.open(ctx) for r in five[:3]]
    append(ctx, recs, [r.n for r in recs])
    ctx.pool_trim([recs[1].slot], [333])   # this slot now reads its other buffer
    recs[1].dropped = 333
    order = [recs[2], recs[0], recs[1]]
    base = ctx.pool_log_mel([r.slot for r in order], 80, padding=480000)
    host = [r.want[r.dropped:r.out] for r in order]
    assert list(base) == list(np.cumsum([0] + [(len(h) + 480000) // 160 for h in host]))
    got = [ctx.mel_read(80, int(base[i]), int(base[i + 1] - base[i])) for i in range(3)]
    gmax = ctx.mel_max_batch(3)
    base2 = ctx.log_mel_batch(host, 80, padding=480000)
    assert np.array_equal(base, base2)
    for i in range(3):
        assert np.array_equal(got[i], ctx.mel_read(80, int(base2[i]), int(base2[i + 1] - base2[i]))), i
    assert np.array_equal(gmax, ctx.mel_max_batch(3))
    for r in recs:   # the mel read the slots, nothing else
        r.check(ctx)


# ---------------------------------------------------------------- refusals
def _rc(ctx, fn, *args):
    rc = fn(ctx.h, *args)
    return rc, ctx.lib.wh_last_error().decode(errors="replace")


def test_refused_calls_change_nothing(ctx, five):
    from whisper.audio import resample_filter
    from whisper.backend_hip import _ptr
    close_all(ctx)
    lib = ctx.lib
    a, b, c = [r.open(ctx) for r in five[:3]]    # slots 0, 1, 2; 3.. stay closed
    append(ctx, [a, b, c], [a.n // 2, b.n // 2, c.n])
    finish(ctx, [c])
    ctx.pool_log_mel([0, 1], 80, padding=480000)
    up, down, taps = resample_filter(44100)

    def state():
        return ([ctx.pool_info(s) for s in range(3)], [ctx.pool_read(r.slot, 0, r.out) for r in (a, b, c)], ctx.stats(),
                ctx.mel_read(80, 0, 100))

    before = state()
    I32 = lambda *v: np.asarray(v, dtype=np.int32)
    I64 = lambda *v: np.asarray(v, dtype=np.int64)
    n_out = np.full(4, -5, dtype=np.int64)
    out = np.zeros(16, np.float32)
    buf = a.raw[:64].copy()
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*[None if x is None else x.ctypes.data for x in v])
    t = (_ptr(taps), len(taps))
    # (function, arguments, code, words of the message)
    refusals = [
        (lib.wh_pool_create, (4, 1000), -7, ["already"]),
        (lib.wh_pool_open, (N_SLOTS, 1, 2, up, down, *t), -7, ["slot", str(N_SLOTS)]),
        (lib.wh_pool_open, (-1, 1, 2, up, down, *t), -7, ["slot"]),
        (lib.wh_pool_open, (1, 1, 2, up, down, *t), -7, ["slot 1", "already open"]),
        (lib.wh_pool_open, (3, 8, 2, up, down, *t), -7, ["encoding"]),
        (lib.wh_pool_open, (3, 1, 0, up, down, *t), -7, ["channels"]),
        (lib.wh_pool_open, (3, 1, 2, 0, down, *t), -7, ["up"]),
        (lib.wh_pool_open, (3, 1, 2, up, down, _ptr(taps), len(taps) - 2), -7, ["n_taps"]),
        (lib.wh_pool_open, (3, 1, 2, up, down, None, len(taps)), -7, ["n_taps"]),
        (lib.wh_pool_close, (3,), -7, ["slots[0]", "not open"]),
        (lib.wh_pool_close, (N_SLOTS,), -7, ["slots[0]", "outside"]),
        (lib.wh_pool_append, (0, _ptr(I32(0)), ptrs(buf), _ptr(I64(4)), _ptr(n_out)), -7, ["n = 0"]),
        (lib.wh_pool_append, (2, None, ptrs(buf, buf), _ptr(I64(4, 4)), _ptr(n_out)), -1, ["slots"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 1)), None, _ptr(I64(4, 4)), _ptr(n_out)), -1, ["data"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 1)), ptrs(buf, buf), None, _ptr(n_out)), -1, ["n_frames"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, N_SLOTS)), ptrs(buf, buf), _ptr(I64(4, 4)), _ptr(n_out)), -7, ["slots[1]", "outside"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 3)), ptrs(buf, buf), _ptr(I64(4, 4)), _ptr(n_out)), -7, ["slots[1]", "not open"]),
        (lib.wh_pool_append, (3, _ptr(I32(0, 1, 0)), ptrs(buf, buf, buf), _ptr(I64(4, 4, 4)), _ptr(n_out)), -7, ["slots[2]", "twice"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 1)), ptrs(buf, None), _ptr(I64(4, 4)), _ptr(n_out)), -1, ["data[1]"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 1)), ptrs(buf, buf), _ptr(I64(4, -1)), _ptr(n_out)), -7, ["n_frames[1]"]),
        (lib.wh_pool_append, (2, _ptr(I32(0, 2)), ptrs(buf, buf), _ptr(I64(4, 4)), _ptr(n_out)), -7, ["slots[1]", "finish"]),
        (lib.wh_pool_append, (2, _ptr(I32(1, 0)), ptrs(buf, buf), _ptr(I64(4, 8 * SLOT_SAMPLES)), _ptr(n_out)), -7,
         ["n_frames[1]", "capacity", "trim"]),
        (lib.wh_pool_finish, (0, _ptr(I32(0)), _ptr(n_out)), -7, ["n = 0"]),
        (lib.wh_pool_finish, (2, _ptr(I32(0, 0)), _ptr(n_out)), -7, ["slots[1]", "twice"]),
        (lib.wh_pool_finish, (2, _ptr(I32(0, 4)), _ptr(n_out)), -7, ["slots[1]", "not open"]),
        (lib.wh_pool_trim, (2, _ptr(I32(0, 1)), None), -1, ["n_drop"]),
        (lib.wh_pool_trim, (2, _ptr(I32(0, 1)), _ptr(I64(10, -1))), -7, ["n_drop[1]"]),
        (lib.wh_pool_trim, (2, _ptr(I32(0, 1)), _ptr(I64(10, b.out + 1))), -7, ["n_drop[1]"]),
        (lib.wh_pool_trim, (2, _ptr(I32(0, 5)), _ptr(I64(10, 10))), -7, ["slots[1]", "not open"]),
        (lib.wh_pool_info, (3, None, None, None, None), -7, ["not open"]),
        (lib.wh_pool_read, (0, None, 0, 4), -1, ["out"]),
        (lib.wh_pool_read, (0, _ptr(out), a.out - 3, 4), -7, ["resident"]),
        (lib.wh_pool_read, (0, _ptr(out), -1, 4), -7, ["resident"]),
        (lib.wh_pool_log_mel, (2, _ptr(I32(0, 1)), 480000, 80, None), -1, ["frame_base"]),
        (lib.wh_pool_log_mel, (2, _ptr(I32(0, 1)), -1, 80, _ptr(I64(0, 0, 0))), -7, ["padding"]),
        (lib.wh_pool_log_mel, (2, _ptr(I32(1, 1)), 480000, 80, _ptr(I64(0, 0, 0))), -7, ["slots[1]", "twice"]),
        (lib.wh_pool_log_mel, (2, _ptr(I32(0, 1)), 480000, 81, _ptr(I64(0, 0, 0))), -7, ["n_mels"]),
    ]
    for fn, args, code, words in refusals:
        rc, msg = _rc(ctx, fn, *args)
        assert rc == code and "pool" in msg and all(w in msg for w in words), (fn.__name__, rc, msg)
        after = state()
        assert after[0] == before[0] and after[2] == before[2] and np.array_equal(after[3], before[3]), fn.__name__
        assert all(np.array_equal(x, y) for x, y in zip(after[1], before[1])), fn.__name__
        assert (n_out == -5).all() and not out.any(), fn.__name__
    # an empty slot has no mel
    ctx.pool_open(3, ENCODINGS.index("s16"), 1, 16000)
    rc, msg = _rc(ctx, lib.wh_pool_log_mel, 2, _ptr(I32(0, 3)), 480000, 80, _ptr(I64(0, 0, 0)))
    assert rc == -7 and "pool" in msg and "slots[1]" in msg and "no samples" in msg
    ctx.pool_close(3)
    assert state()[0] == before[0] and np.array_equal(state()[3], before[3])
    # zero frames: allowed, emits 0, with or without a pointer
    assert ctx.pool_append([0, 1], [None, buf], [0, 0]) == [0, 0]
    assert state()[0] == before[0] and state()[2] == before[2]
    # only the two ingest counters move on a good append plus trim
    append(ctx, [a, b], [100, 100])
    ctx.pool_trim([0, 1], [10, 10])
    moved = {k for k, v in ctx.stats().items() if v != before[2][k]}
    assert moved == {"ingest_copy_ms", "ingest_kernel_ms"}
    # a second finish emits nothing
    assert ctx.pool_finish([2]) == [0] and ctx.pool_info(2) == before[0][2]
    # without a pool every call is refused; a new pool starts with every slot closed
    ctx.pool_destroy()
    try:
        for fn, args in ((lib.wh_pool_destroy, ()), (lib.wh_pool_open, (0, 1, 2, up, down, *t)), (lib.wh_pool_close, (0,)),
                         (lib.wh_pool_append, (1, _ptr(I32(0)), ptrs(buf), _ptr(I64(4)), _ptr(n_out))),
                         (lib.wh_pool_finish, (1, _ptr(I32(0)), _ptr(n_out))),
                         (lib.wh_pool_trim, (1, _ptr(I32(0)), _ptr(I64(0)))), (lib.wh_pool_info, (0, None, None, None, None)),
                         (lib.wh_pool_read, (0, _ptr(out), 0, 0)),
                         (lib.wh_pool_log_mel, (1, _ptr(I32(0)), 480000, 80, _ptr(I64(0, 0))))):
            rc, msg = _rc(ctx, fn, *args)
            assert rc == -7 and "pool" in msg and "no pool" in msg, (fn.__name__, rc, msg)
        for n_slots, samples, word in ((0, 1000, "n_slots"), (4097, 1000, "n_slots"), (4, 0, "slot_samples")):
            rc, msg = _rc(ctx, lib.wh_pool_create, n_slots, samples)
            assert rc == -7 and "pool" in msg and word in msg
        assert (n_out == -5).all()
    finally:
        ctx.pool_create(N_SLOTS, SLOT_SAMPLES)
    rc, msg = _rc(ctx, lib.wh_pool_info, 0, None, None, None, None)
    assert rc == -7 and "not open" in msg


# ---------------------------------------------------------------- the transcriber
OPTS = dict(buffer_trim=4, max_buffer=6)


@pytest.fixture(scope="module")
def streams():
    """(rate, encoding, channels, options, bytes) of the three streams."""
    from whisper.audio import load_audio, read_pcm
    pcm, rate, bits = read_pcm(JFK)
    assert (rate, bits, pcm.shape[1]) == (44100, 24, 2)
    s24 = encode("s24", pcm)
    W = load_audio(JFK)
    s16 = np.round(W.astype(np.float64) * 32768).astype(np.int16)
    assert np.array_equal(s16.astype(np.float32) / 32768, W)   # the waveform is on the 16-bit grid
    return [(44100, "s24", 2, dict(OPTS, min_chunk=2.0, language="en"), s24),
            (44100, "s24", 2, dict(OPTS, min_chunk=3.0, language=None), s24),
            (16000, "s16", 1, dict(OPTS, min_chunk=2.0, language="en", initial_prompt="hello"), s16.tobytes())]


def load(max_windows):
    import whisper
    return whisper.load_model("micro", device=0, dtype="fp32", max_windows=max_windows, max_group=5, synthetic=True)


@pytest.fixture(scope="module")
def micro32():
    m = load(4)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lone(micro32, streams):
    """The updates of three lone transcribers, one after another; computed once."""
    import whisper
    out = []
    for rate, enc, ch, opts, data in streams:
        t = whisper.StreamingTranscriber(micro32, rate, enc, ch, temperature=0.0, **opts)
        out.append(t.feed(data) + [t.finish()])
    return out


def assert_same_words(a, b):
    assert [(w["word"], w["start"], w["end"]) for w in a] == [(w["word"], w["start"], w["end"]) for w in b]
    for wa, wb in zip(a, b):
        assert wa["probability"] == pytest.approx(wb["probability"], rel=1e-5)


def assert_same_updates(got, want):
    assert len(got) == len(want)
    for u, v in zip(got, want):
        assert (u.span, u.prompt, u.language, u.forced, u.final) == (v.span, v.prompt, v.language, v.forced, v.final)
        assert_same_words(u.committed, v.committed)
        assert_same_words(u.tentative, v.tentative)
        assert (u.result is None) == (v.result is None)
        if u.result is not None:
            assert u.result["language"] == v.result["language"] and u.result["text"] == v.result["text"]
            assert len(u.result["segments"]) == len(v.result["segments"])
            for a, b in zip(u.result["segments"], v.result["segments"]):
                assert (a["tokens"], a["text"], a["start"], a["end"]) == (b["tokens"], b["text"], b["start"], b["end"])
                assert_same_words(a["words"], b["words"])


def pool_run(model, streams, interleaved, transcribe_in_the_middle=False):
    """The three streams through a pool: in 0.37 s packets, the second one opened after the first
    has been fed 3 s, or everything in one feed."""
    import whisper
    with whisper.StreamingPool(model, slots=4, temperature=0.0) as pool:
        opened = lambda k: pool.open(*streams[k][:3], **streams[k][3])
        got = {}
        if not interleaved:
            handles = [opened(k) for k in range(3)]
            for h, ups in pool.feed({h: streams[k][4] for k, h in enumerate(handles)}).items():
                got[h] = ups
        else:
            handles = {0: opened(0), 2: opened(2)}
            pos = [0, 0, 0]
            piece = [int(0.37 * s[0]) * CONTAINER[s[1]] * s[2] for s in streams]
            tick = 0
            while any(pos[k] < len(streams[k][4]) for k in range(3)):
                if 1 not in handles and pos[0] >= 3 * 44100 * 6:
                    handles[1] = opened(1)
                    if transcribe_in_the_middle:
                        whisper.transcribe(model, JFK, language="en", temperature=0.0)
                packets = {}
                for k, h in handles.items():
                    if pos[k] < len(streams[k][4]):
                        packets[h] = streams[k][4][pos[k]:pos[k] + piece[k]]
                        pos[k] += piece[k]
                for h, ups in pool.feed(packets).items():
                    got.setdefault(h, []).extend(ups)
                tick += 1
            handles = [handles[k] for k in range(3)]
        final = pool.finish(handles)
        return [got[h] + [final[h]] for h in handles], pool.rounds


def test_the_pool_transcribes_as_lone_transcribers_do(micro32, streams, lone):
    ups, rounds = pool_run(micro32, streams, interleaved=True, transcribe_in_the_middle=True)
    for k in range(3):
        assert_same_updates(ups[k], lone[k])
    assert any(len(r) >= 2 for r in rounds)                        # streams were decoded together
    assert any(u.span[0] > 0 for k in range(3) for u in ups[k])    # and trimmed
    assert all(u.result is not None and any(s["words"] for s in u.result["segments"]) for u in ups[0])
    assert lone[1][0].language is not None and len(lone[1]) == 4 and len(lone[0]) == 6
    # everything in one feed per stream: the same lists
    whole, rounds = pool_run(micro32, streams, interleaved=False)
    for k in range(3):
        assert_same_updates(whole[k], lone[k])
    assert any(len(r) == 3 for r in rounds)


def test_due_streams_queue_when_the_model_has_fewer_windows(streams, lone):
    m = load(2)
    try:
        ups, rounds = pool_run(m, streams, interleaved=False)
    finally:
        m.close()
    assert any(len(r) == 3 for r in rounds)   # three due streams, two windows
    for k in range(3):
        assert_same_updates(ups[k], lone[k])
