"""Host against device decoding of a long FLAC file (FLAC on the device).

The stream is tests/golden/jfk.flac (44.1 kHz stereo 24-bit) made about --seconds long: its
metadata kept, STREAMINFO's total scaled and its MD5 zeroed, its frame bytes repeated
verbatim.  The frame headers and both CRCs stay valid; the frame numbers repeat, which neither
decoder reads.
  host    read_pcm(path) (wh_flac_decode on one CPU thread) then audio_ingest(pcm): the path
          before flac_ingest existed                                       -- wall time
  device  flac_ingest(bytes): index, upload, k_flac_parse, chain, k_flac_restore,
          k_flac_gather, k_pcm_resample                                    -- wall time, and
          every stage between HIP events or host timers (wh_stats [8]..[13])
One warm-up then 5 repetitions of each; median, minimum and maximum reported; the two
waveforms are compared for equality.
    python profiles/flac_timing.py [--seconds 600] [--out profiles/flac/flac_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper.coreml_amd"))

from whisper.audio import _mel_context, read_pcm  # noqa: E402
from whisper.backend_hip import flac_index, flac_info  # noqa: E402

REPS = 5
STAGES = ("flac_index_ms", "flac_upload_ms", "flac_parse_ms", "flac_restore_ms", "flac_gather_ms", "flac_resample_ms")

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=600.0)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flac", "flac_timing.json"))
args = ap.parse_args()

with open(os.path.join(REPO, "tests", "golden", "jfk.flac"), "rb") as f:
    jfk = f.read()
rate, channels, bits, total = flac_info(jfk)
first = int(flac_index(jfk)[0][0])
copies = max(1, round(args.seconds * rate / total))
head = bytearray(jfk[:first])
# STREAMINFO: 4 (fLaC) + 4 (block header) + 34 bytes; the total is the low 36 bits of bytes 21..25, the MD5 follows
info = 8
packed = int.from_bytes(head[info + 13:info + 18], "big")
packed = (packed >> 36 << 36) | (total * copies)
head[info + 13:info + 18] = packed.to_bytes(5, "big")
head[info + 18:info + 34] = bytes(16)
stream = bytes(head) + jfk[first:] * copies
assert flac_info(stream) == (rate, channels, bits, total * copies)
seconds = total * copies / rate

ctx = _mel_context(0)
tmp = tempfile.NamedTemporaryFile(suffix=".flac", delete=False)
tmp.write(stream)
tmp.close()


def host():
    t0 = time.perf_counter()
    pcm, r, b = read_pcm(tmp.name)
    t1 = time.perf_counter()
    d = ctx.audio_ingest(pcm, r, b)
    return time.perf_counter() - t0, t1 - t0, d.n_samples


def device():
    s0 = ctx.stats()
    t0 = time.perf_counter()
    d = ctx.flac_ingest(stream)
    wall = time.perf_counter() - t0
    s1 = ctx.stats()
    assert d.decoded_on == "device"
    return wall, {k[:-3] + "_s": (s1[k] - s0[k]) * 1e-3 for k in STAGES}, d.n_samples


def spread(xs):
    xs = list(xs)
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


try:
    host()
    h = [host() for _ in range(REPS)]
    want = ctx.audio_read(0, h[0][2])
    device()
    d = [device() for _ in range(REPS)]
    got = ctx.audio_read(0, d[0][2])
finally:
    os.unlink(tmp.name)
parse_s = statistics.median(x[1]["flac_parse_s"] for x in d)
rec = dict(script="profiles/flac_timing.py", repetitions=REPS, seconds=seconds, rate=rate, channels=channels, bits=bits,
           stream_bytes=len(stream), frames=int(total * copies), candidates=int(len(flac_index(stream)[0])),
           description="jfk.flac's frames repeated verbatim behind its metadata (total scaled, MD5 zeroed); "
                       "frame numbers repeat, which neither decoder reads",
           identical_to_host=bool(np.array_equal(got, want)),
           host_wall_s=spread(x[0] for x in h), host_decode_s=spread(x[1] for x in h),
           device_wall_s=spread(x[0] for x in d),
           device_stage_s={k: spread(x[1][k] for x in d) for k in d[0][1]},
           device_slowest_faster_than_host_fastest=max(x[0] for x in d) < min(x[0] for x in h),
           parse_compressed_bytes_per_s=len(stream) / parse_s,
           parse_samples_per_s=total * copies * channels / parse_s)
print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
