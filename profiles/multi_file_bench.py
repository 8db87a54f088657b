#!/usr/bin/env python
"""A list of files: the loop of transcribe() calls against transcribe_batch().

Model: large-v3 with seeded synthetic weights, fp16, beam 5, temperature 0, every other
option at its default (so the prompt of a window depends on the previous one and
transcribe() walks a file one window at a time; the language is detected per file).
Workloads: (a) 40 files of 10 s, (b) 20 files of 120 s, seeded synthetic audio.

Both arms run in this process on the same context.  Each workload is warmed up with one
pass of each arm (every shape and step graph the timed passes use), then the arms
alternate for --repeats rounds; a pass is timed with the host clock around the call,
which returns host results and so ends synchronised.  Reported: every time, the median
and the min-max spread per arm, audio-seconds per second, the ratio of the medians, the
windows and tokens each arm decoded and how many files came out token-identical (fp16:
the arms batch differently, so equality is not required here; fp32 equality is what
tests/test_gpu_multifile.py pins).

    python profiles/multi_file_bench.py --out profiles/r07/multi_file.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "whisper.coreml_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKLOADS = {"a_40x10s": (40, 10.0), "b_20x120s": (20, 120.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--max-windows", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07", "multi_file.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (the spread is part of the result)")

    import whisper
    from bench import seeded_state_dict
    from whisper import synthetic as S

    dims = S.MODEL_DIMS[args.model]
    model = whisper.Whisper(whisper.ModelDimensions(**dims), args.model, device=0, dtype=args.dtype,
                            max_windows=args.max_windows, max_group=args.beam)
    model.load_state_dict(seeded_state_dict(dims, 0))
    if args.model in whisper._ALIGNMENT_HEADS:
        model.set_alignment_heads(whisper._ALIGNMENT_HEADS[args.model])
    kw = dict(temperature=0.0, beam_size=args.beam)

    def loop_arm(files):
        return [whisper.transcribe(model, f, **kw) for f in files]

    def batch_arm(files):
        return whisper.transcribe_batch(model, files, **kw)

    def timed(arm, files):
        model.ctx.sync()
        s0 = model.ctx.stats()
        t = time.perf_counter()
        out = arm(files)
        model.ctx.sync()
        dt = time.perf_counter() - t
        s1 = model.ctx.stats()
        return dt, out, {k: round(s1[k] - s0[k], 3) for k in s1 if isinstance(s1[k], (int, float))}

    def summary(times, audio_s):
        med = statistics.median(times)
        return dict(seconds=[round(t, 4) for t in times], median_s=round(med, 4), min_s=round(min(times), 4),
                    max_s=round(max(times), 4), xrt_median=round(audio_s / med, 1))

    def shape(out):
        segs = [s for r in out for s in r["segments"]]
        return dict(windows=len({(i, s["seek"]) for i, r in enumerate(out) for s in r["segments"]}),
                    segments=len(segs), tokens=sum(len(s["tokens"]) for s in segs))

    result = dict(model=args.model, dtype=args.dtype, beam=args.beam, max_windows=args.max_windows,
                  options="temperature=0, beam_size=%d, otherwise transcribe() defaults" % args.beam,
                  repeats=args.repeats, data="seeded synthetic audio and weights", workloads={})
    for name in args.workloads.split(","):
        n_files, seconds = WORKLOADS[name]
        files = [S.synthetic_audio(seconds, seed=2000 + i) for i in range(n_files)]
        audio_s = n_files * seconds
        _, ref_loop, _ = timed(loop_arm, files)    # warm-up, and the outputs that are compared
        _, ref_batch, _ = timed(batch_arm, files)
        t_loop, t_batch, st_loop, st_batch = [], [], None, None
        for _ in range(args.repeats):
            dt, _, st_loop = timed(loop_arm, files)
            t_loop.append(dt)
            dt, _, st_batch = timed(batch_arm, files)
            t_batch.append(dt)
        same = sum([s["tokens"] for s in a["segments"]] == [s["tokens"] for s in b["segments"]]
                   for a, b in zip(ref_loop, ref_batch))
        rec = dict(files=n_files, seconds_per_file=seconds, audio_seconds=audio_s,
                   loop=dict(summary(t_loop, audio_s), **shape(ref_loop), stage_ms_last_pass=st_loop),
                   batch=dict(summary(t_batch, audio_s), **shape(ref_batch), stage_ms_last_pass=st_batch),
                   files_token_identical=same,
                   languages_equal=[a["language"] for a in ref_loop] == [b["language"] for b in ref_batch])
        rec["speedup_median"] = round(rec["loop"]["median_s"] / rec["batch"]["median_s"], 3)
        result["workloads"][name] = rec
        print(name, json.dumps(rec), flush=True)
    model.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
