"""The split resampling kernel against the mixing one (Channels as files).

Two files of 600 s, made in memory from a seed:
  44k1_stereo_s24  44.1 kHz stereo 24-bit packed: the file of profiles/wav_timing.py's case of
                   that name (the same generator state)
  8k_stereo_ulaw   8 kHz stereo mu-law, the telephony case
and, per file, the routes
  mix      HipContext.wav_ingest(file): k_pcm_resample.  Calls nothing the parent commit's
           library lacks, so with WHISPER_HIP_LIB it times that library (--routes mix)
  split    wav_ingest(file, channels=[0, 1]): one launch of k_pcm_resample_split
  two      wav_ingest(file, channels=[0]) then wav_ingest(file, channels=[1]) behind it: two
           uploads and two launches, the sum is reported
One warm-up then 5 repetitions; the copy and the kernel are timed between HIP events (wh_stats
[6], [7]).  The first second of every split channel is compared with the host twin.
    python profiles/split_timing.py [--routes mix,split,two] [--seconds 600]
"""
import argparse
import json
import os
import statistics
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper.coreml_amd"))

from whisper import backend_hip  # noqa: E402

REPS = 5
ap = argparse.ArgumentParser()
ap.add_argument("--routes", default="mix,split,two")
ap.add_argument("--seconds", type=float, default=600.0)
args = ap.parse_args()
routes = args.routes.split(",")

if routes == ["mix"]:  # possibly a library without the split symbols: bind what it has
    for name in [k for k in backend_hip._EXPORTS if k.endswith("_ingest_split")]:
        del backend_hip._EXPORTS[name]

from whisper.audio import _mel_context, pcm_to_waveform, wav_info, wav_samples  # noqa: E402


def header(tag, channels, rate, container, data_bytes):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * container, channels * container, 8 * container)
    fmt += b"" if tag == 1 else struct.pack("<H", 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", data_bytes)
    return b"RIFF" + struct.pack("<I", len(body) + data_bytes) + body


ctx = _mel_context(0)
rng = np.random.default_rng(0)
rng.integers(-32768, 32768, (int(args.seconds * 48000), 2), dtype=np.int16)  # wav_timing.py's generator state
n24 = int(args.seconds * 44100)
pcm24 = rng.integers(-(1 << 23), 1 << 23, (n24, 2), dtype=np.int32)
pay24 = pcm24.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
del pcm24
n8 = int(args.seconds * 8000)
payu = rng.integers(0, 256, (n8, 2), dtype=np.uint8).tobytes()

for name, rate, container, tag, payload, n in (("44k1_stereo_s24", 44100, 3, 1, pay24, n24),
                                              ("8k_stereo_ulaw", 8000, 1, 7, payu, n8)):
    head = header(tag, 2, rate, container, len(payload))
    data = head + payload
    # the host twin of the file's first 3 s: its first second is out of the filter's reach of the cut
    short = header(tag, 2, rate, container, 3 * rate * 2 * container) + payload[:3 * rate * 2 * container]
    pcm, bits = wav_samples(short, wav_info(short))
    want = [pcm_to_waveform(pcm[:, [c]], rate, bits)[:16000] for c in (0, 1)]

    def run(route):
        s0 = ctx.stats()
        if route == "mix":
            segs = [ctx.wav_ingest(data)]
        elif route == "split":
            segs = ctx.wav_ingest(data, channels=[0, 1])
        else:
            segs = ctx.wav_ingest(data, channels=[0])
            segs += ctx.wav_ingest(data, channels=[1], dst_offset=segs[0].n_samples)
        s1 = ctx.stats()
        return (s1["ingest_copy_ms"] - s0["ingest_copy_ms"], s1["ingest_kernel_ms"] - s0["ingest_kernel_ms"], segs)

    for route in routes:
        run(route)
        r = [run(route) for _ in range(REPS)]
        segs = r[-1][2]
        same = None if route == "mix" else bool(all(
            np.array_equal(ctx.audio_read(s.offset, 16000), want[c]) for c, s in enumerate(segs)))
        kernel = sorted(x[1] for x in r)
        print(json.dumps(dict(
            script="profiles/split_timing.py", lib=os.path.basename(backend_hip.lib_path()), case=name, route=route,
            seconds=args.seconds, frames=n, samples_out=segs[0].n_samples, segments=len(segs),
            first_second_identical_to_host=same, kernel_event_ms=statistics.median(kernel),
            kernel_event_all_ms=[round(x, 4) for x in kernel],
            spread_pct=round(100 * (kernel[-1] - kernel[0]) / statistics.median(kernel), 2),
            copy_event_ms=statistics.median(x[0] for x in r))), flush=True)
