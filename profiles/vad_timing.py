"""What the speech-span detector costs and what skipping silence saves ("Speech
spans on the device").

(a) the detector on 600 s and 3600 s of resident 16 kHz audio (the zeros + jfk.flac + zeros
    fixture, tiled): k_frame_energy and k_speech_spans each between HIP events on the
    context's stream (wh_stats [14], [15]), the call's wall time (it returns after the stream
    synchronise), and the log_mel stage time of the same resident file for scale;
(b) large-v3, seeded synthetic weights, fp16, beam 5, temperature 0,
    condition_on_previous_text=False, on the 600 s file: wall time (ending in a synchronise)
    and windows encoded for transcribe() as it is, over the 30 s clip grid bench.py uses,
    and with skip_silence=True.
One warm-up then --reps repetitions of each, medians reported.
    python profiles/vad_timing.py [--reps 5] [--skip-model] [--out profiles/vad/vad_timing.json]
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

import whisper  # noqa: E402
from whisper import vad  # noqa: E402
from whisper.audio import N_SAMPLES, _mel_context, load_audio  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s, MI355X streaming rate

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-model", action="store_true", help="part (a) only")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vad", "vad_timing.json"))
args = ap.parse_args()
med = statistics.median

jfk = load_audio(os.path.join(REPO, "tests", "golden", "jfk.flac"))
unit = np.concatenate([np.zeros(48000, np.float32), jfk, np.zeros(80000, np.float32)])  # 19 s, 11 s of speech


def tiled(seconds):
    n = int(seconds * 16000)
    return np.tile(unit, -(-n // len(unit)))[:n]


# ---------------------------------------------------------------- (a) the detector alone
ctx = _mel_context(0)
params = vad.resolve_options()
detector = []
for seconds in (600, 3600):
    x = tiled(seconds)
    want, want_t = vad.speech_frames_host(x)
    ctx.audio_upload(x)

    def detect():
        s0 = ctx.stats()
        t0 = time.perf_counter()
        (spans, thr), = ctx.speech_spans(params, 1, cap=256)  # returns after the stream synchronise
        wall = time.perf_counter() - t0
        s1 = ctx.stats()
        return (wall, s1["vad_energy_ms"] - s0["vad_energy_ms"], s1["vad_spans_ms"] - s0["vad_spans_ms"],
                [(int(a), int(b)) for a, b in spans], thr)

    def mel():
        s0 = ctx.stats()
        ctx.log_mel_resident(len(x), 80, padding=N_SAMPLES)
        return ctx.stats()["mel_ms"] - s0["mel_ms"]

    detect()
    d = [detect() for _ in range(args.reps)]
    mel()
    m = [mel() for _ in range(args.reps)]
    energy_ms = med(r[1] for r in d)
    rec = dict(seconds=seconds, samples=len(x), frames=-(-len(x) // 160), spans=len(d[0][3]),
               equal_to_host=bool(d[0][3] == want and d[0][4] == want_t),
               wall_ms=med(r[0] for r in d) * 1e3, wall_all_ms=[r[0] * 1e3 for r in d],
               k_frame_energy_ms=energy_ms, k_frame_energy_all_ms=[r[1] for r in d],
               k_speech_spans_ms=med(r[2] for r in d), k_speech_spans_all_ms=[r[2] for r in d],
               k_frame_energy_share_of_achievable_hbm=len(x) * 4 / (energy_ms * 1e-3) / HBM_ACHIEVABLE,
               log_mel_ms=med(m), log_mel_all_ms=m)
    detector.append(rec)
    print(json.dumps(rec), flush=True)

out = dict(script="profiles/vad_timing.py", repetitions=args.reps, statistic="median", detector=detector)

# ---------------------------------------------------------------- (b) what skipping saves
if not args.skip_model:
    model = whisper.load_model("large-v3", device=0, dtype="fp16", max_windows=20, max_group=5, synthetic=True)
    x = tiled(600)
    kw = dict(beam_size=5, temperature=0.0, condition_on_previous_text=False, language="en")
    variants = (("plain", dict()),
                ("clip_grid_30s", dict(clip_timestamps=",".join(f"{30 * i},{30 * (i + 1)}" for i in range(20)))),
                ("skip_silence", dict(skip_silence=True)))
    runs = []
    for name, extra in variants:
        def run():
            w0 = model.ctx.stats()["encode_windows"]
            t0 = time.perf_counter()
            r = whisper.transcribe(model, x, **kw, **extra)
            model.ctx.sync()
            return time.perf_counter() - t0, int(model.ctx.stats()["encode_windows"] - w0), len(r["segments"])

        run()
        t = [run() for _ in range(args.reps)]
        rec = dict(variant=name, wall_s=med(r[0] for r in t), wall_all_s=[r[0] for r in t], windows_encoded=t[0][1],
                   segments=t[0][2])
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    out["transcribe_600s_large_v3_fp16_beam5"] = runs
    model.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
