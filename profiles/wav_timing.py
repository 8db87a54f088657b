"""WAV bytes read by the resampling kernel against the host unpack they replace (DESIGN.md,
WAV ingest).

Two files of 600 s, made in memory from a seed:
  44k1_stereo_s24  44.1 kHz stereo 24-bit packed: the audio of profiles/ingest_timing.py's case
                   of that name (the same generator state), written as a WAV
  8k_mono_ulaw     8 kHz mono mu-law
and two routes, one per run (--route):
  tree    HipContext.wav_ingest(file bytes): header parse, upload of the data chunk as it is,
          k_pcm_resample reading the encoding
  parent  what a caller did before wav_ingest existed: the numpy expansion (24-bit -> int32,
          mu-law -> int16) and HipContext.audio_ingest of the array.  This route calls nothing
          the parent commit's library lacks, so it can be timed with that library
          (WHISPER_HIP_LIB).
One warm-up then 5 repetitions: wall time of the whole route, and the copy and the kernel each
between HIP events (wh_stats [6], [7]).  The result is compared with the host twin.
    python profiles/wav_timing.py --route tree|parent [--seconds 600]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper.coreml_amd"))

from whisper import backend_hip  # noqa: E402
from whisper.audio import WAV_S24, WAV_ULAW, _mel_context, pcm_to_waveform, wav_samples  # noqa: E402

REPS = 5
ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=("tree", "parent"), required=True)
ap.add_argument("--seconds", type=float, default=600.0)
args = ap.parse_args()

if args.route == "parent":  # a library without the wh_wav_* symbols: bind what it has
    for name in [k for k in backend_hip._EXPORTS if k.startswith("wh_wav_")]:
        del backend_hip._EXPORTS[name]


def header(tag, channels, rate, container, data_bytes):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * container, channels * container, 8 * container)
    fmt += b"" if tag == 1 else struct.pack("<H", 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", data_bytes)
    return b"RIFF" + struct.pack("<I", len(body) + data_bytes) + body


ctx = _mel_context(0)
rng = np.random.default_rng(0)
rng.integers(-32768, 32768, (int(args.seconds * 48000), 2), dtype=np.int16)  # ingest_timing.py's first case
n24 = int(args.seconds * 44100)
pcm24 = rng.integers(-(1 << 23), 1 << 23, (n24, 2), dtype=np.int32)
pay24 = pcm24.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
n8 = int(args.seconds * 8000)
payu = rng.integers(0, 256, (n8, 1), dtype=np.uint8).tobytes()
del pcm24

for name, enc, rate, ch, container, tag, payload, n in (
        ("44k1_stereo_s24", WAV_S24, 44100, 2, 3, 1, pay24, n24), ("8k_mono_ulaw", WAV_ULAW, 8000, 1, 1, 7, payu, n8)):
    head = header(tag, ch, rate, container, len(payload))
    data = head + payload
    info = backend_hip.WavInfo(enc, ch, rate, 8 * container, len(head), n)
    pcm, bits = wav_samples(data, info)
    want = pcm_to_waveform(pcm, rate, bits)
    del pcm

    def run():
        s0 = ctx.stats()
        t0 = time.perf_counter()
        if args.route == "tree":
            d = ctx.wav_ingest(data)  # returns after the stream synchronise
            uploaded = n * ch * container
        else:
            expanded, b = wav_samples(data, info)
            d = ctx.audio_ingest(expanded, rate, b)
            uploaded = expanded.size * (4 if b > 16 else 2)
        wall = time.perf_counter() - t0
        s1 = ctx.stats()
        return (wall, (s1["ingest_copy_ms"] - s0["ingest_copy_ms"]) * 1e-3,
                (s1["ingest_kernel_ms"] - s0["ingest_kernel_ms"]) * 1e-3, d.n_samples, uploaded)

    run()
    r = [run() for _ in range(REPS)]
    got = ctx.audio_read(0, r[0][3])
    med = statistics.median
    copy_s, kernel_s = med(x[1] for x in r), med(x[2] for x in r)
    print(json.dumps(dict(
        script="profiles/wav_timing.py", route=args.route, case=name, seconds=args.seconds, rate=rate, channels=ch,
        frames=n, samples_out=r[0][3], file_bytes=len(data), bytes_uploaded=int(r[0][4]),
        identical_to_host=bool(np.array_equal(got, want)), wall_s=med(x[0] for x in r), wall_all_s=[x[0] for x in r],
        copy_event_s=copy_s, kernel_event_s=kernel_s, copy_plus_kernel_event_s=med(x[1] + x[2] for x in r),
        copy_event_all_s=[x[1] for x in r], kernel_event_all_s=[x[2] for x in r],
        kernel_below_copy=bool(kernel_s < copy_s))), flush=True)
