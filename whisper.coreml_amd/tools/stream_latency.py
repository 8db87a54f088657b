"""What a stream costs: the device time of one append, and the wall time of one update.

  python whisper.coreml_amd/tools/stream_latency.py [--models turbo,large-v3] [--seconds 12]

1. Append: 100 ms chunks of mu-law 8 kHz and s16 48 kHz into a resident stream; the device
   milliseconds per append come from the WH_STAT_INGEST_* counters (HIP events around the upload
   and around k_pcm_resample_stream), the wall milliseconds from the host clock around the call.
2. Update: ``StreamingTranscriber`` at ``min_chunk = 1.0`` on synthetic audio with the seeded
   synthetic weights, greedy and beam 5, fp16: p50 / p95 of ``StreamUpdate.wall_ms``, printed
   with the tokens each update decoded, because the synthetic weights never choose
   end-of-text: every decode runs to its token limit, which real speech does not.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="turbo,large-v3")
    ap.add_argument("--seconds", type=float, default=12.0)
    args = ap.parse_args()
    import whisper
    for rate, enc in ((8000, "ulaw"), (48000, "s16")):
        print(json.dumps(append_cost(rate, enc)), flush=True)
    for name in [m for m in args.models.split(",") if m]:
        model = whisper.load_model(name, device=0, dtype="fp16", max_windows=1, max_group=5, synthetic=True)
        for decode in ({}, dict(beam_size=5)):
            print(json.dumps(update_cost(model, name, args.seconds, **decode)), flush=True)
        model.close()


if __name__ == "__main__":
    main()
