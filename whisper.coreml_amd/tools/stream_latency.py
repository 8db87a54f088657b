"""What a stream costs: the device time of one append, and the wall time of one update.

  python whisper.coreml_amd/tools/stream_latency.py [--models turbo,large-v3] [--seconds 12]

1. Append: 100 ms chunks of mu-law 8 kHz and s16 48 kHz into a resident stream; the device
   milliseconds per append come from the WH_STAT_INGEST_* counters (HIP events around the upload
   and around k_pcm_resample_stream), the wall milliseconds from the host clock around the call.
2. Update: ``StreamingTranscriber`` at ``min_chunk = 1.0`` on synthetic audio with the seeded
   synthetic weights, greedy and beam 5, fp16: p50 / p95 of ``StreamUpdate.wall_ms``, printed
   with the tokens each update decoded, because the synthetic weights never choose
   end-of-text: every decode runs to its token limit, which real speech does not.

With ``--pool`` the same two questions for the stream pool (``wh_pool_*``, ``StreamingPool``)
against the single-stream path, in one process:

3. Tick: S mu-law 8 kHz packets of 20 ms, one per stream, through one ``pool_append``, against
   S ``stream_append`` calls of the same packets (S = 1, 16, 64, 256).
4. Round: the wall time of one ``StreamingPool.feed`` in which S streams are due (one second of
   audio each, so the feed is one append, one batched decode, one trim), against the sum of the
   ``wall_ms`` of the same updates of S lone ``StreamingTranscriber``s run one after another on
   the same model (S up to ``--windows``).

With ``--vad`` the cost and the saving of the streams' speech detector (``open(vad=...)``):

5. Tick: S mu-law 8 kHz packets of 20 ms through one ``pool_append`` (S = 1, 16, 64, 256) with a
   detector on every slot and on none, ``--runs`` times each: ``ingest_kernel_ms`` (HIP events
   around the ingest kernel and, behind it, the detector's) and the wall p50 / p95 per tick.
6. Saving: the 12.7 s composite of the tests (silence, speech, a pause, speech, silence, cut from
   ``--audio``) as one pool stream at ``min_chunk = 1.0``, with and without ``vad``: the decode
   rounds, their lanes and the summed ``wall_ms``.  The round and lane counts follow from the
   samples alone; the wall time is that of synthetic weights, whose decodes run to the token limit.

One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def append_cost(rate, encoding, chunks=200):
    import whisper
    from whisper.audio import _mel_context
    ctx = _mel_context(0)
    frames = rate // 10
    width = dict(ulaw=1, s16=2)[encoding]
    data = [bytes(c) for c in np.random.default_rng(0).integers(0, 256, (chunks, frames * width), dtype=np.uint8)]
    s = whisper.AudioStream(ctx, rate, encoding)
    s.append(data[0])  # first-touch costs (allocations, the filter upload) stay out
    before, wall = ctx.stats(), []
    for k in range(1, chunks):
        t = time.perf_counter()
        s.append(data[k])
        wall.append((time.perf_counter() - t) * 1e3)
    after = ctx.stats()
    n = chunks - 1
    return dict(measure="append", rate=rate, encoding=encoding, chunk_ms=100, appends=n,
                copy_ms=round((after["ingest_copy_ms"] - before["ingest_copy_ms"]) / n, 4),
                kernel_ms=round((after["ingest_kernel_ms"] - before["ingest_kernel_ms"]) / n, 4),
                wall_ms_p50=round(float(np.percentile(wall, 50)), 4), wall_ms_p95=round(float(np.percentile(wall, 95)), 4))


def update_cost(model, name, seconds, **decode):
    import whisper
    from whisper import synthetic as S
    audio = S.synthetic_audio(seconds, seed=5)
    pcm = np.clip(np.round(audio * 32768.0), -32768, 32767).astype(np.int16)
    t = whisper.StreamingTranscriber(model, 16000, "s16", 1, language="en", min_chunk=1.0, temperature=0.0, **decode)
    ups = []
    for at in range(0, len(pcm), 1600):  # 100 ms packets
        ups += t.feed(pcm[at:at + 1600])
    ups.append(t.finish())
    ups = [u for u in ups if u.result is not None][1:]  # the first decode captures the step graphs
    wall = [u.wall_ms for u in ups]
    tokens = [sum(len(s["tokens"]) for s in u.result["segments"]) for u in ups]
    return dict(measure="update", model=name, decode=decode or dict(greedy=True), min_chunk=1.0, updates=len(ups),
                wall_ms_p50=round(float(np.percentile(wall, 50)), 1), wall_ms_p95=round(float(np.percentile(wall, 95)), 1),
                tokens_per_update_p50=int(np.percentile(tokens, 50)), tokens_per_update_max=int(max(tokens)),
                buffer_s_max=round(max(u.span[1] - u.span[0] for u in ups) / 16000, 2))


def pool_tick_cost(n_streams, ticks=200):
    """One tick of ``n_streams`` 20 ms mu-law packets: one pool_append against that many stream_appends."""
    from whisper.audio import WAV_ENCODINGS, _mel_context
    ctx = _mel_context(0)
    frames, enc = 160, WAV_ENCODINGS.index("ulaw")
    data = np.random.default_rng(0).integers(0, 256, (ticks, n_streams, frames), dtype=np.uint8)
    slots, counts = list(range(n_streams)), [frames] * n_streams
    ctx.pool_create(n_streams, 2 * frames * ticks + 64)
    for s in slots:
        ctx.pool_open(s, enc, 1, 8000)
    ctx.stream_begin(enc, 1, 8000, reserve=2 * frames * ticks * n_streams + 64)
    # first-touch costs (allocations, the filter upload) stay out
    ctx.pool_append(slots, list(data[0]), counts)
    for s in slots:
        ctx.stream_append(data[0][s], frames)
    out = dict(measure="pool_tick", streams=n_streams, packet_ms=20, ticks=ticks - 1)
    for name in ("pool", "single"):
        before, wall = ctx.stats(), []
        for k in range(1, ticks):
            packets = list(data[k])
            t = time.perf_counter()
            if name == "pool":
                ctx.pool_append(slots, packets, counts)
            else:
                for p in packets:
                    ctx.stream_append(p, frames)
            wall.append((time.perf_counter() - t) * 1e3)
        after = ctx.stats()
        out[name] = dict(copy_ms=round((after["ingest_copy_ms"] - before["ingest_copy_ms"]) / (ticks - 1), 4),
                         kernel_ms=round((after["ingest_kernel_ms"] - before["ingest_kernel_ms"]) / (ticks - 1), 4),
                         wall_ms_p50=round(float(np.percentile(wall, 50)), 4),
                         wall_ms_p95=round(float(np.percentile(wall, 95)), 4))
    ctx.pool_destroy()
    return out


def vad_tick_cost(n_streams, ticks=200, runs=3):
    """One tick of ``n_streams`` 20 ms mu-law packets through ``pool_append``: no slot detecting
    against every slot detecting, ``runs`` times each in turn."""
    from whisper.audio import WAV_ENCODINGS, _mel_context
    from whisper.vad import resolve_stream_options
    ctx = _mel_context(0)
    frames, enc = 160, WAV_ENCODINGS.index("ulaw")
    data = np.random.default_rng(0).integers(0, 256, (ticks, n_streams, frames), dtype=np.uint8)
    slots, counts = list(range(n_streams)), [frames] * n_streams
    params = resolve_stream_options()
    out = dict(measure="vad_tick", streams=n_streams, packet_ms=20, ticks=ticks - 1, none=[], vad=[])
    for _ in range(runs):
        for name in ("none", "vad"):
            ctx.pool_create(n_streams, 2 * frames * ticks + 64)
            for s in slots:
                ctx.pool_open(s, enc, 1, 8000)
                if name == "vad":
                    ctx.pool_vad_enable(s, params)
            ctx.pool_append(slots, list(data[0]), counts)  # first-touch costs stay out
            before, wall = ctx.stats(), []
            for k in range(1, ticks):
                packets = list(data[k])
                t = time.perf_counter()
                ctx.pool_append(slots, packets, counts)
                wall.append((time.perf_counter() - t) * 1e3)
            after = ctx.stats()
            out[name].append(dict(kernel_ms=round((after["ingest_kernel_ms"] - before["ingest_kernel_ms"]) / (ticks - 1), 4),
                                  copy_ms=round((after["ingest_copy_ms"] - before["ingest_copy_ms"]) / (ticks - 1), 4),
                                  wall_ms_p50=round(float(np.percentile(wall, 50)), 4),
                                  wall_ms_p95=round(float(np.percentile(wall, 95)), 4)))
            ctx.pool_destroy()
    return out


def vad_saving(model, name, audio_path, **decode):
    """The composite stream through a pool, without and with a detector."""
    import whisper
    from whisper.audio import load_audio
    w = load_audio(audio_path)
    z = lambda sec: np.zeros(int(round(sec * 16000)), np.float32)
    comp = np.concatenate([z(1.5), w[:72000], z(2.5), w[84800:128000], z(1.5)])
    pcm = np.clip(np.round(comp * 32768.0), -32768, 32767).astype(np.int16)
    out = dict(measure="vad_saving", model=name, decode=decode or dict(greedy=True), seconds=round(len(pcm) / 16000, 2),
               min_chunk=1.0)
    for key, vad in (("none", None), ("vad", True)):
        with whisper.StreamingPool(model, slots=1, temperature=0.0, **decode) as pool:
            h = pool.open(16000, "s16", 1, language="en", min_chunk=1.0, vad=vad)
            ups = []
            for at in range(0, len(pcm), 1600):  # 100 ms packets
                ups += pool.feed({h: pcm[at:at + 1600]})[h]
            ups.append(pool.finish([h])[h])
            decoded = [u for u in ups if u.result is not None]
            out[key] = dict(updates=len(ups), rounds=len(pool.rounds), lanes=sum(len(r) for r in pool.rounds),
                            idle=sum(u.idle for u in ups), endpoints=sum(u.endpoint for u in ups),
                            wall_ms_sum=round(sum(u.wall_ms for u in ups), 1),
                            # the first decode captures the step graphs
                            wall_ms_sum_after_first=round(sum(u.wall_ms for u in decoded[1:]), 1),
                            buffer_s_max=round(max(u.span[1] - u.span[0] for u in decoded) / 16000, 2))
    return out


def pool_round_cost(model, name, n_streams, seconds, **decode):
    """One round with ``n_streams`` due streams against that many lone updates of the same buffers."""
    import whisper
    from whisper import synthetic as S
    pcm = [np.clip(np.round(S.synthetic_audio(seconds, seed=5 + k) * 32768.0), -32768, 32767).astype(np.int16)
           for k in range(n_streams)]
    rounds = int(seconds)
    lone = np.zeros(rounds)
    tokens = []
    for k in range(n_streams):
        t = whisper.StreamingTranscriber(model, 16000, "s16", 1, language="en", min_chunk=1.0, temperature=0.0, **decode)
        ups = t.feed(pcm[k][:rounds * 16000])
        lone += [u.wall_ms for u in ups]
        tokens += [sum(len(s["tokens"]) for s in u.result["segments"]) for u in ups[1:]]
    wall = []
    with whisper.StreamingPool(model, slots=n_streams, temperature=0.0, **decode) as pool:
        handles = [pool.open(16000, "s16", 1, language="en", min_chunk=1.0) for _ in range(n_streams)]
        for r in range(rounds):
            packets = {h: pcm[k][r * 16000:(r + 1) * 16000] for k, h in enumerate(handles)}
            t = time.perf_counter()
            ups = pool.feed(packets)
            wall.append((time.perf_counter() - t) * 1e3)
            assert all(len(u) == 1 for u in ups.values()) and pool.rounds[-1] == handles
    # the first round captures the step graphs
    return dict(measure="pool_round", model=name, decode=decode or dict(greedy=True), streams=n_streams,
                rounds=rounds - 1, pool_ms_p50=round(float(np.percentile(wall[1:], 50)), 1),
                pool_ms_max=round(float(max(wall[1:])), 1), lone_sum_ms_p50=round(float(np.percentile(lone[1:], 50)), 1),
                lone_sum_ms_max=round(float(max(lone[1:])), 1), tokens_per_update_p50=int(np.percentile(tokens, 50)),
                tokens_per_update_max=int(max(tokens)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=None, help="default: turbo,large-v3 (turbo with --pool)")
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--pool", action="store_true", help="the stream pool against the single-stream path")
    ap.add_argument("--vad", action="store_true", help="the streams' speech detector: the tick with and without it, the decodes it saves")
    ap.add_argument("--runs", type=int, default=3, help="--vad: repetitions of every tick measurement")
    ap.add_argument("--audio", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests", "golden",
                                                    "jfk.flac"), help="--vad: the recording the composite is cut from")
    ap.add_argument("--windows", type=int, default=8, help="--pool: max_windows of the model, the most streams per round")
    args = ap.parse_args()
    import whisper
    if args.vad:
        for n in (1, 16, 64, 256):
            print(json.dumps(vad_tick_cost(n, runs=args.runs)), flush=True)
        for name in [m for m in (args.models or "turbo").split(",") if m]:
            model = whisper.load_model(name, device=0, dtype="fp16", max_windows=1, max_group=5, synthetic=True)
            print(json.dumps(vad_saving(model, name, args.audio)), flush=True)
            model.close()
        return
    if args.pool:
        for n in (1, 16, 64, 256):
            print(json.dumps(pool_tick_cost(n)), flush=True)
        for name in [m for m in (args.models or "turbo").split(",") if m]:
            model = whisper.load_model(name, device=0, dtype="fp16", max_windows=args.windows, max_group=5,
                                       synthetic=True)
            for decode in ({}, dict(beam_size=5)):
                n = 1
                while n <= args.windows:
                    print(json.dumps(pool_round_cost(model, name, n, min(args.seconds, 6.0), **decode)), flush=True)
                    n *= 2
            model.close()
        return
    args.models = args.models or "turbo,large-v3"
    for rate, enc in ((8000, "ulaw"), (48000, "s16")):
        print(json.dumps(append_cost(rate, enc)), flush=True)
    for name in [m for m in args.models.split(",") if m]:
        model = whisper.load_model(name, device=0, dtype="fp16", max_windows=1, max_group=5, synthetic=True)
        for decode in ({}, dict(beam_size=5)):
            print(json.dumps(update_cost(model, name, args.seconds, **decode)), flush=True)
        model.close()


if __name__ == "__main__":
    main()
