"""Channels as files on the GPU (wh_audio_ingest_split / wh_flac_ingest_split /
wh_wav_ingest_split, ``channels=``): one upload and one launch turn an interleaved file into one
resident waveform per selected channel.  Every device-versus-host comparison is
``np.array_equal`` against the host twin ``load_audio_channels`` (row k is ``pcm_to_waveform``
of column ``channels[k]``): every WAV encoding, 1-3 channels and lengths around the filter's
edges; selections in any order; the device-only invariant (channel c == the existing mixing
kernel on a mono file of that channel); several workgroups; more channels than one workgroup
can stage; every 24-bit byte phase; float edge values; FLAC on both decoders; segments feeding
the resident log-mel; refusals that leave the context alone; the counters.  End to end,
``transcribe(..., channels="split")`` and ``transcribe_batch`` give per channel what
``transcribe`` gives for that channel's host waveform, and the merged dialogue of
``merge_channels``."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from flac_fixture import tone, write_stream
from test_audio_ingest_host import RATES, ingest_lengths, ratio
from wav_fixture import ENCODINGS, encode, random_values, wav_bytes

pytestmark = pytest.mark.gpu

JFK = os.path.join(GOLDEN, "jfk.flac")
PAD = 480000
ALL_RATES = tuple(sorted(set(RATES) | {8000, 16000}))
DIMS = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=128, n_audio_head=2, n_audio_layer=1,
            n_vocab=64, n_text_ctx=448, n_text_state=128, n_text_head=2, n_text_layer=1)


def _ctx():
    from whisper.audio import _mel_context
    return _mel_context(0)


def _fresh_ctx():
    """A context of its own: its audio buffer starts empty and its counters at zero."""
    from whisper.audio import mel_filters
    from whisper.backend_hip import HipContext
    ctx = HipContext(DIMS, device=0, dtype="fp32", max_windows=1, max_group=1)
    ctx.set_mel_filters(80, mel_filters(None, 80))
    return ctx


def _host_rows(data, channels=None):
    """The definition: ``load_audio_channels`` on the file's bytes (``wav_samples`` is what
    ``read_pcm`` runs for these files)."""
    from whisper.audio import pcm_to_waveform, select_channels, wav_info, wav_samples
    info = wav_info(data)
    pcm, bits = wav_samples(data, info)
    return [pcm_to_waveform(pcm[:, [c]], info.sample_rate, bits) for c in select_channels(channels, info.channels)]


def _check_segments(ctx, segs, rows, what, base=0):
    assert len(segs) == len(rows), what
    n = len(rows[0])
    for k, (seg, want) in enumerate(zip(segs, rows)):
        assert seg.n_samples == n == len(want) and seg.offset == base + k * n, (what, k, seg.n_samples, seg.offset)
        got = ctx.audio_read(seg.offset, seg.n_samples)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, k, bad.size, int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


def _check(ctx, data, what, channels=None):
    rows = _host_rows(data, channels)
    segs = ctx.wav_ingest(data, channels=list(range(len(rows))) if channels is None else channels)
    _check_segments(ctx, segs, rows, what)
    return segs


# ---------------------------------------------------------------- the samples
@pytest.mark.parametrize("rate", ALL_RATES)
def test_small_shapes_equal_the_host_rows(rate):
    """Every encoding x 1-3 channels x lengths of 1 and 2 frames, around ``down`` and around the
    filter's reach, all channels split; 16000 Hz de-interleaves and quantises only."""
    ctx = _ctx()
    rng = np.random.default_rng(5000 + rate)
    for enc in ENCODINGS:
        for n in ingest_lengths(rate):
            for ch in (1, 2, 3):
                data = wav_bytes(enc, encode(enc, random_values(rng, enc, n, ch)), ch, rate)
                _check(ctx, data, (enc, rate, n, ch))


def test_selection_order_and_subset():
    ctx = _ctx()
    vals = random_values(np.random.default_rng(55), "s16", 3001, 5)
    data = wav_bytes("s16", encode("s16", vals), 5, 22050)
    segs = _check(ctx, data, "[3, 0]", channels=[3, 0])
    assert len(segs) == 2
    # the rows really are channels 3 and 0 of the file, in that order
    from whisper.audio import pcm_to_waveform
    assert np.array_equal(ctx.audio_read(segs[0].offset, segs[0].n_samples), pcm_to_waveform(vals[:, [3]], 22050, 16))
    assert np.array_equal(ctx.audio_read(segs[1].offset, segs[1].n_samples), pcm_to_waveform(vals[:, [0]], 22050, 16))
    assert len(_check(ctx, data, "[4]", channels=[4])) == 1
    # one selected channel at offset 0 is the one resident segment wh_log_mel reads
    assert ctx.log_mel_resident(segs[0].n_samples, 80, padding=PAD) > 0


@pytest.mark.parametrize("enc,rate", [("s24", 44100), ("ulaw", 8000)])
def test_split_channel_equals_the_mixing_kernel_on_a_mono_file(enc, rate):
    """The device-only invariant: channel c of the split == ``wav_ingest`` (k_pcm_resample) of a
    mono file built from that channel's samples."""
    ctx = _ctx()
    vals = random_values(np.random.default_rng(rate), enc, 6007, 2)
    segs = ctx.wav_ingest(wav_bytes(enc, encode(enc, vals), 2, rate), channels=[0, 1])
    got = [ctx.audio_read(s.offset, s.n_samples) for s in segs]
    for c in (0, 1):
        mono = ctx.wav_ingest(wav_bytes(enc, encode(enc, vals[:, [c]]), 1, rate))
        assert mono.n_samples == segs[c].n_samples
        assert np.array_equal(ctx.audio_read(0, mono.n_samples), got[c]), (enc, c)


def test_identical_channels_equal_the_mix():
    ctx = _ctx()
    one = random_values(np.random.default_rng(8), "s16", 5003, 1)
    data = wav_bytes("s16", encode("s16", np.repeat(one, 2, axis=1)), 2, 44100)
    segs = ctx.wav_ingest(data, channels=[0, 1])
    left, right = (ctx.audio_read(s.offset, s.n_samples) for s in segs)
    mix = ctx.wav_ingest(data)
    assert mix.n_samples == segs[0].n_samples
    mixed = ctx.audio_read(0, mix.n_samples)
    assert np.array_equal(left, mixed) and np.array_equal(right, mixed)


@pytest.mark.parametrize("enc,ch,rate", [("s24", 2, 44100), ("f32", 3, 48000), ("ulaw", 2, 8000)])
def test_several_workgroups_with_a_ragged_last_one(enc, ch, rate):
    """About 1.5 s: tens of workgroups, the last one partly filled."""
    n = int(1.5 * rate) + 7
    up, down = ratio(rate)
    n_out = -(-n * up // down)
    assert n_out > 20 * 1024 and n_out % 1024 not in (0, 1023)
    vals = random_values(np.random.default_rng(rate + ch), enc, n, ch)
    _check(_ctx(), wav_bytes(enc, encode(enc, vals), ch, rate), (enc, ch, rate, n))


@pytest.mark.parametrize("enc,ch,rate,seconds", [("s16", 32, 44100, 0.2), ("s24", 7, 48000, 0.2)])
def test_more_channels_than_one_workgroup_stages(enc, ch, rate, seconds):
    """32 channels at 44.1 kHz: at the smallest block a channel's span is about 760 frames of
    8 bytes, so 32 planes need about 190 KiB, more LDS than a CU has: whatever the grouping
    rule, the channels are spread over several groups.  7 channels of 24 bits: an odd count
    and 21-byte frames, so samples start at every dword phase."""
    n = int(seconds * rate) + 3
    vals = random_values(np.random.default_rng(ch), enc, n, ch)
    data = wav_bytes(enc, encode(enc, vals), ch, rate)
    _check(_ctx(), data, (enc, ch, rate))
    _check(_ctx(), data, (enc, ch, rate, "reversed"), channels=list(range(ch))[::-1])


@pytest.mark.parametrize("rate", [16000, 44100])
def test_s24_every_byte_phase(rate):
    ctx = _ctx()
    rng = np.random.default_rng(240 + rate)
    for ch in (2, 3):
        for n in range(1, 10):
            vals = random_values(rng, "s24", n, ch)
            vals[-1, -1] = -(1 << 23)  # the last bytes are 00 00 80: what follows them must not leak in
            _check(ctx, wav_bytes("s24", encode("s24", vals), ch, rate), ("s24", rate, n, ch))


@pytest.mark.parametrize("enc", ["f32", "f64"])
@pytest.mark.parametrize("rate", [16000, 48000])
def test_float_edge_values_stay_in_their_channel(enc, rate):
    rng = np.random.default_rng(70)
    x = rng.uniform(-1.0, 1.0, (4001, 2))
    noise = x[:, 1].copy()
    edges = [np.nan, np.inf, -np.inf, 1e30, -1e30, 256.5, -256.5]
    at = rng.choice(len(x), 40 * len(edges), replace=False)
    x[at, 0] = np.tile(edges, 40)
    data = wav_bytes(enc, encode(enc, x), 2, rate)
    segs = _check(_ctx(), data, (enc, rate))
    # the noise channel is what it is in a file without the edge values
    clean = np.stack([rng.uniform(-1.0, 1.0, len(x)), noise], axis=1)
    want = _host_rows(wav_bytes(enc, encode(enc, clean), 2, rate))[1]
    assert np.isfinite(want).all()
    assert np.array_equal(_ctx().audio_read(segs[1].offset, segs[1].n_samples), want)


# ---------------------------------------------------------------- FLAC
def _flac_rows(stream):
    from whisper.audio import pcm_to_waveform
    from whisper.backend_hip import decode_flac
    pcm, rate, bits = decode_flac(stream)
    return [pcm_to_waveform(pcm[:, [c]], rate, bits) for c in range(pcm.shape[1])]


@pytest.mark.parametrize("bps,ch", [(16, 2), (24, 3)])
def test_flac_split_on_the_device(bps, ch):
    pcm = tone(5000, ch, bps, seed=bps + ch)
    stream, _ = write_stream(pcm, bps, rate=44100, blocks=576, sub={"type": "fixed", "order": 2})
    ctx = _ctx()
    segs = ctx.flac_ingest(stream, channels=list(range(ch)))
    assert all(s.decoded_on == "device" for s in segs)
    _check_segments(ctx, segs, _flac_rows(stream), ("flac", bps, ch))


def test_flac_split_through_the_host_decoder():
    from whisper.audio import pcm_to_waveform
    pcm = tone(1700, 2, 16, seed=3)
    stream, _ = write_stream(pcm, 16, rate=44100, blocks=256, sub={"type": "fixed", "order": 2}, total=0)
    ctx = _ctx()
    segs = ctx.flac_ingest(stream, channels=[1, 0])
    assert all(s.decoded_on == "host" for s in segs)
    _check_segments(ctx, segs, [pcm_to_waveform(pcm[:, [c]], 44100, 16) for c in (1, 0)], "flac host")


# ---------------------------------------------------------------- segments
def test_split_segments_behind_a_mixed_file_feed_the_resident_mel():
    rng = np.random.default_rng(77)
    first = wav_bytes("s16", encode("s16", random_values(rng, "s16", 20003, 2)), 2, 8000)
    stereo = wav_bytes("s24", encode("s24", random_values(rng, "s24", 30011, 2)), 2, 48000, extensible=True)
    from whisper.audio import pcm_to_waveform, wav_info, wav_samples
    info = wav_info(first)
    pcm, bits = wav_samples(first, info)
    host = [pcm_to_waveform(pcm, info.sample_rate, bits)] + _host_rows(stereo)
    ref = _ctx()
    want_mel = []
    for h in host:  # each waveform uploaded alone
        nf = ref.log_mel(h, 80, padding=PAD)
        want_mel.append(ref.mel_read(80, 0, nf))
    ctx = _fresh_ctx()
    try:
        a = ctx.wav_ingest(first)
        segs = ctx.wav_ingest(stereo, dst_offset=a.n_samples, channels=[0, 1])  # reserve = 0: the buffer grows
        assert np.array_equal(ctx.audio_read(0, a.n_samples), host[0])
        _check_segments(ctx, segs, host[1:], "behind", base=a.n_samples)
        base = ctx.log_mel_batch_resident([a.n_samples, segs[0].n_samples, segs[1].n_samples], 80, padding=PAD)
        for i in range(3):
            assert np.array_equal(ctx.mel_read(80, int(base[i]), int(base[i + 1] - base[i])), want_mel[i]), i
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals
def test_refused_split_calls_leave_the_context_alone():
    from whisper.audio import resample_filter
    from whisper.backend_hip import WH_PCM_F32, WH_PCM_S16, HipBackendError, _ptr
    ctx = _fresh_ctx()
    try:
        rng = np.random.default_rng(9)
        vals = random_values(rng, "s16", 9000, 3)
        data = wav_bytes("s16", encode("s16", vals), 3, 48000)
        buf = np.frombuffer(data, np.uint8)
        pcm = np.ascontiguousarray(vals, dtype=np.int16)
        d = ctx.wav_ingest(data)
        nf = ctx.log_mel_resident(d.n_samples, 80, padding=PAD)
        samples, mel = ctx.audio_read(0, d.n_samples), ctx.mel_read(80, 0, nf)
        up, down, taps = resample_filter(48000)
        n_out = ctypes.c_int64(-1)
        good = np.array([2, 0], dtype=np.int32)

        def sel(*ids):
            return np.array(ids, dtype=np.int32)

        def wav(ptr=_ptr(buf), n=len(buf), up=up, down=down, taps=_ptr(taps), n_taps=len(taps), select=good,
                n_select=None, dst=0, reserve=0, out=ctypes.byref(n_out)):
            ctx._check(ctx.lib.wh_wav_ingest_split(
                ctx.h, ptr, n, up, down, taps, n_taps, None if select is None else _ptr(select),
                (0 if select is None else len(select)) if n_select is None else n_select, dst, reserve, out),
                "wh_wav_ingest_split")

        def raw(ptr=_ptr(pcm), fmt=WH_PCM_S16, n=len(pcm), ch=3, bits=16, up=up, down=down, taps=_ptr(taps),
                n_taps=len(taps), select=good, n_select=None, dst=0, reserve=0, out=ctypes.byref(n_out)):
            ctx._check(ctx.lib.wh_audio_ingest_split(
                ctx.h, ptr, fmt, n, ch, bits, up, down, taps, n_taps, None if select is None else _ptr(select),
                (0 if select is None else len(select)) if n_select is None else n_select, dst, reserve, out),
                "wh_audio_ingest_split")

        def untouched():
            assert n_out.value == -1
            assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
            assert np.array_equal(ctx.mel_read(80, 0, nf), mel)
            assert ctx.log_mel_resident(d.n_samples, 80, padding=PAD) == nf  # still the one segment
            with pytest.raises(HipBackendError):
                ctx.audio_read(d.n_samples, 1)  # and nothing behind it

        selection = ((dict(select=None, n_select=2), "null select"), (dict(n_select=0), "n_select"),
                     (dict(select=sel(0, 1, 2, 0), n_select=4), "n_select"), (dict(select=sel(0, 3)), r"select\[1\]"),
                     (dict(select=sel(-1)), r"select\[0\]"), (dict(select=sel(1, 2, 1)), r"select\[2\].*repeats"))
        shared = ((dict(n_taps=len(taps) - 2), "n_taps"), (dict(taps=None), "n_taps"), (dict(dst=5), "dst_offset"),
                  (dict(dst=d.n_samples + 1), "dst_offset"), (dict(out=None), "n_out"), (dict(up=0), "up"),
                  (dict(down=0), "down"), (dict(reserve=-1), "reserve"))
        for call, own in ((wav, ((dict(n=30), "runs past the end"), (dict(n=11), "not a RIFF/WAVE"),
                                 (dict(ptr=None), "null data"))),
                          (raw, ((dict(ptr=None), "null pcm"), (dict(n=0), "n_frames"), (dict(ch=0), "channels"),
                                 (dict(fmt=7), "format"), (dict(bits=17), "bits")))):
            for kw, msg in selection + shared + own:
                with pytest.raises(HipBackendError, match=msg):
                    call(**kw)
                untouched()
        # a mono float32 waveform has nothing to split
        wave = np.zeros(100, np.float32)
        with pytest.raises(HipBackendError, match="WH_PCM_F32"):
            raw(ptr=_ptr(wave), fmt=WH_PCM_F32, n=100, ch=1, bits=32, up=1, down=1, taps=None, n_taps=0, select=sel(0))
        untouched()
        # FLAC: the selection is checked against the stream's channels on both decoders' paths
        with open(JFK, "rb") as f:
            flac = np.frombuffer(f.read(), np.uint8)
        path = ctypes.c_int(-1)
        fup, fdown, ftaps = resample_filter(44100)  # the golden file is 44.1 kHz stereo
        for select, msg in ((sel(0, 1, 1), "n_select"), (sel(2), r"select\[0\]"), (sel(1, 1), "repeats"),
                            (None, "null select")):
            with pytest.raises(HipBackendError, match=msg):
                ctx._check(ctx.lib.wh_flac_ingest_split(
                    ctx.h, _ptr(flac), len(flac), fup, fdown, _ptr(ftaps), len(ftaps), None if select is None else _ptr(select),
                    1 if select is None else len(select), 0, 0, ctypes.byref(n_out), ctypes.byref(path)),
                    "wh_flac_ingest_split")
            untouched()
            assert path.value == -1
        # a good call still works: appended behind the segment
        wav(dst=d.n_samples)
        rows = _host_rows(data, [2, 0])
        assert n_out.value == len(rows[0])
        for k in range(2):
            assert np.array_equal(ctx.audio_read(d.n_samples + k * n_out.value, n_out.value), rows[k])
        assert np.array_equal(ctx.audio_read(0, d.n_samples), samples)
    finally:
        ctx.close()


# ---------------------------------------------------------------- stage counters
def test_split_counters():
    ctx = _fresh_ctx()
    try:
        rng = np.random.default_rng(5)
        for enc, rate in (("s24", 48000), ("ulaw", 8000), ("f32", 16000)):
            data = wav_bytes(enc, encode(enc, random_values(rng, enc, 9000, 2)), 2, rate)
            before = ctx.stats()
            ctx.wav_ingest(data, channels=[0, 1])
            after = ctx.stats()
            print(enc, {k: (before[k], after[k]) for k in after if after[k] != before[k]})
            for k in after:
                if k in ("ingest_copy_ms", "ingest_kernel_ms"):
                    assert after[k] > before[k], (enc, k, before[k], after[k])
                else:
                    assert after[k] == before[k], (enc, k, before[k], after[k])
        stream, _ = write_stream(tone(5000, 2, 16, seed=1), 16, rate=44100, blocks=576, sub={"type": "fixed", "order": 2})
        before = ctx.stats()
        segs = ctx.flac_ingest(stream, channels=[0, 1])
        after = ctx.stats()
        assert segs[0].decoded_on == "device"
        print("flac", {k: (before[k], after[k]) for k in after if after[k] != before[k]})
        for k in ("flac_upload_ms", "flac_parse_ms", "flac_restore_ms", "flac_gather_ms", "flac_resample_ms"):
            assert after[k] > before[k], (k, before[k], after[k])
        assert after["ingest_kernel_ms"] == before["ingest_kernel_ms"]
    finally:
        ctx.close()


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


def _s24(a):
    return np.clip(np.round(np.asarray(a, np.float64) * (1 << 23)), -(1 << 23), (1 << 23) - 1).astype(np.int64)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """``stereo``: a 24-bit 48 kHz stereo WAV of two different signals, 6 s.  ``halves``: one
    channel silent in its first half, the other in its second.  ``mono``: a mono 16-bit FLAC."""
    from whisper import synthetic as S
    root = tmp_path_factory.mktemp("split")
    # every 16 kHz sample three times: 6 s at 48 kHz
    left, right = (np.repeat(S.synthetic_audio(6.0, seed=seed), 3) for seed in (31, 32))
    out = {}
    out["stereo"] = str(root / "stereo_s24_48k.wav")
    with open(out["stereo"], "wb") as f:
        f.write(wav_bytes("s24", encode("s24", np.stack([_s24(left), _s24(right)], axis=1)), 2, 48000, extensible=True))
    a, b = left.copy(), right.copy()
    a[: len(a) // 2] = 0.0
    b[len(b) // 2:] = 0.0
    out["halves"] = str(root / "halves_s24_48k.wav")
    with open(out["halves"], "wb") as f:
        f.write(wav_bytes("s24", encode("s24", np.stack([_s24(a), _s24(b)], axis=1)), 2, 48000, extensible=True))
    mono = np.clip(np.round(S.synthetic_audio(4.0, seed=33) * 32768), -32768, 32767).astype(np.int64)
    out["mono"] = str(root / "mono_16k.flac")
    with open(out["mono"], "wb") as f:
        f.write(write_stream(mono.reshape(-1, 1), 16, rate=16000, blocks=4096, sub={"type": "fixed", "order": 2})[0])
    return out


SEG_KEYS = ("seek", "tokens", "start", "end", "temperature", "text")


def _same(got, ref):
    """The comparison tests/test_gpu_multifile.py uses for lanes."""
    assert got["language"] == ref["language"] and got["text"] == ref["text"]
    assert len(got["segments"]) == len(ref["segments"])
    for a, b in zip(got["segments"], ref["segments"]):
        for k in SEG_KEYS:
            assert a[k] == b[k], (k, a[k], b[k])


def _same_merged(got, refs, names=None):
    import whisper
    want = whisper.merge_channels(refs, names)
    assert len(got["channels"]) == len(refs)
    for g, r in zip(got["channels"], refs):
        _same(g, r)
    assert got["text"] == want["text"] and got["language"] == want["language"]
    assert len(got["segments"]) == len(want["segments"])
    for a, b in zip(got["segments"], want["segments"]):
        for k in SEG_KEYS + ("id", "channel", "channel_index"):
            assert a[k] == b[k], (k, a[k], b[k])


@pytest.fixture(scope="module")
def stereo_refs(micro32, paths):
    """``transcribe`` of each channel's host waveform of the stereo file: computed once."""
    import whisper
    rows = whisper.load_audio_channels(paths["stereo"])
    return [whisper.transcribe(micro32, row, temperature=0.0, language="en") for row in rows]


def test_transcribe_split_equals_the_channel_waveforms(micro32, paths, stereo_refs):
    got = micro32.transcribe(paths["stereo"], channels="split", temperature=0.0, language="en")
    assert all(len(r["segments"]) >= 1 for r in stereo_refs)
    _same_merged(got, stereo_refs)
    assert {s["channel"] for s in got["segments"]} == {"0", "1"}
    named = micro32.transcribe(paths["stereo"], channels=[1, 0], channel_names=["customer", "agent"],
                               temperature=0.0, language="en")
    _same_merged(named, stereo_refs[::-1], ["customer", "agent"])


def test_transcribe_split_with_skip_silence(micro32, paths):
    import whisper
    kw = dict(temperature=0.0, language="en", skip_silence=True)
    refs = [whisper.transcribe(micro32, row, **kw) for row in whisper.load_audio_channels(paths["halves"])]
    got = whisper.transcribe(micro32, paths["halves"], channels="split", **kw)
    for g, r in zip(got["channels"], refs):
        assert g["speech_spans"] == r["speech_spans"]
    assert refs[0]["speech_spans"] != refs[1]["speech_spans"]
    _same_merged(got, refs)


def test_mixed_batch_of_split_and_mixed_files(micro32, paths, stereo_refs):
    import whisper
    from whisper import synthetic as S
    kw = dict(temperature=0.0, language="en")
    one = S.synthetic_audio(5.0, seed=41)
    two = np.stack([S.synthetic_audio(4.0, seed=42), S.synthetic_audio(4.0, seed=43)]).astype(np.float32)
    with pytest.raises(ValueError, match="channels"):
        whisper.transcribe_batch(micro32, [two], **kw)
    batch = whisper.transcribe_batch(micro32, [paths["stereo"], paths["mono"], one, two],
                                     channels=["split", None, None, "split"], **kw)
    assert len(batch) == 4
    _same_merged(batch[0], stereo_refs)
    _same(batch[1], whisper.transcribe(micro32, paths["mono"], **kw))
    _same(batch[2], whisper.transcribe(micro32, one, **kw))
    _same_merged(batch[3], [whisper.transcribe(micro32, row, **kw) for row in two])


def test_a_small_mel_budget_never_cuts_a_files_channels(micro32, paths, stereo_refs, monkeypatch):
    import whisper
    from whisper import multifile
    from whisper import synthetic as S
    kw = dict(temperature=0.0, language="en")
    one = S.synthetic_audio(5.0, seed=41)
    seen = []
    real = multifile.split_groups

    def spy(frames, budget, units=None):
        groups = real(frames, budget, units)
        seen.append((list(units), groups))
        return groups

    monkeypatch.setattr(multifile, "split_groups", spy)
    # lanes: array, stereo.0, stereo.1, array; one lane's frames are 3500 or 3600, so 7500 holds two lanes
    batch = whisper.transcribe_batch(micro32, [one, paths["stereo"], one], channels=[None, "split", None],
                                     mel_budget_frames=7500, **kw)
    units, groups = seen[0]
    assert units == [0, 1, 1, 2] and groups == [[0], [1, 2], [3]]
    ref_one = whisper.transcribe(micro32, one, **kw)
    _same(batch[0], ref_one)
    _same_merged(batch[1], stereo_refs)
    _same(batch[2], ref_one)


def test_load_audio_device_split_and_a_stereo_flac_call(micro32, tmp_path):
    """The README's case: a stereo FLAC with one party per channel, each silent while the other
    speaks, through ``load_audio_device(channels=)`` and ``transcribe(channels="split",
    skip_silence=True)``."""
    import whisper
    from whisper import synthetic as S
    a, b = S.synthetic_audio(3.0, seed=51), S.synthetic_audio(3.0, seed=52)
    a[len(a) // 2:] = 0.0
    b[: len(b) // 2] = 0.0
    pcm = np.clip(np.round(np.stack([a, b], axis=1) * 32768), -32768, 32767).astype(np.int64)
    path = str(tmp_path / "call.flac")
    with open(path, "wb") as f:
        f.write(write_stream(pcm, 16, rate=16000, blocks=4096, sub={"type": "fixed", "order": 2})[0])
    rows = whisper.load_audio_channels(path)
    segs = whisper.load_audio_device(micro32, path, channels="split")
    assert [s.decoded_on for s in segs] == ["device", "device"]
    _check_segments(micro32.ctx, segs, list(rows), "call.flac")
    only = whisper.load_audio_device(micro32, path, channels=[1])
    _check_segments(micro32.ctx, only, [rows[1]], "call.flac [1]")
    kw = dict(temperature=0.0, language="en", skip_silence=True)
    refs = [whisper.transcribe(micro32, row, **kw) for row in rows]
    got = micro32.transcribe(path, channels="split", channel_names=["agent", "customer"], **kw)
    _same_merged(got, refs, ["agent", "customer"])
    for g, r in zip(got["channels"], refs):
        assert g["speech_spans"] == r["speech_spans"]
