"""Host against device preparation of a long file's waveform (PCM ingest).

For 600 s of 48 kHz stereo 16-bit and 600 s of 44.1 kHz stereo 24-bit PCM (seeded, made
in memory):
  host    pcm_to_waveform (channel mean, resample_poly, quantise; one CPU thread) +
          audio_upload of the float32 waveform                 -- wall time
  device  audio_ingest: upload the PCM, k_pcm_resample         -- wall time, and the copy
          and the kernel each between HIP events (wh_stats [6], [7])
One warm-up then 5 repetitions of each, the median reported; both results are compared
for equality.  Kernel bytes = PCM read + float32 written, over the kernel's event time,
against the achievable HBM rate.
    python profiles/ingest_timing.py [--seconds 600] [--out profiles/ingest/ingest_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper.coreml_amd"))

from whisper.audio import _mel_context, pcm_to_waveform  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s, MI355X streaming rate (8 TB/s peak)
REPS = 5

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=600.0)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ingest", "ingest_timing.json"))
args = ap.parse_args()

ctx = _mel_context(0)
rng = np.random.default_rng(0)
cases = []
for name, rate, bits, dtype in (("48k_stereo_s16", 48000, 16, np.int16), ("44k1_stereo_s24", 44100, 24, np.int32)):
    n = int(args.seconds * rate)
    lim = 1 << (bits - 1)
    pcm = rng.integers(-lim, lim, (n, 2), dtype=dtype)

    def host():
        t0 = time.perf_counter()
        w = pcm_to_waveform(pcm, rate, bits)
        t1 = time.perf_counter()
        ctx.audio_upload(w)  # returns after the copy's stream synchronise
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, len(w)

    def device():
        s0 = ctx.stats()
        t0 = time.perf_counter()
        d = ctx.audio_ingest(pcm, rate, bits)  # returns after the stream synchronise
        wall = time.perf_counter() - t0
        s1 = ctx.stats()
        return (wall, (s1["ingest_copy_ms"] - s0["ingest_copy_ms"]) * 1e-3,
                (s1["ingest_kernel_ms"] - s0["ingest_kernel_ms"]) * 1e-3, d.n_samples)

    host()
    h = [host() for _ in range(REPS)]
    want = ctx.audio_read(0, h[0][2])
    device()
    d = [device() for _ in range(REPS)]
    got = ctx.audio_read(0, d[0][3])
    med = statistics.median
    kernel_s = med(x[2] for x in d)
    kernel_bytes = pcm.nbytes + 4 * d[0][3]
    rec = dict(case=name, seconds=args.seconds, rate=rate, channels=2, bits=bits, frames=n, samples_out=d[0][3],
               pcm_bytes=int(pcm.nbytes), identical_to_host=bool(np.array_equal(got, want)),
               host_wall_s=med(x[0] for x in h), host_pcm_to_waveform_s=med(x[1] for x in h),
               host_wall_all_s=[x[0] for x in h],
               device_wall_s=med(x[0] for x in d), device_wall_all_s=[x[0] for x in d],
               device_copy_event_s=med(x[1] for x in d), device_kernel_event_s=kernel_s,
               kernel_bytes=int(kernel_bytes), kernel_bytes_per_s=kernel_bytes / kernel_s,
               kernel_share_of_achievable_hbm=kernel_bytes / kernel_s / HBM_ACHIEVABLE,
               host_over_device_wall=med(x[0] for x in h) / med(x[0] for x in d))
    cases.append(rec)
    print(json.dumps(rec))

out = dict(script="profiles/ingest_timing.py", repetitions=REPS, statistic="median",
           hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, cases=cases)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
