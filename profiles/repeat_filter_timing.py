"""What the repetition filter costs a decoder step (repetition controls).

large-v3 fp16 (seeded weights, seeded audio), eot suppressed so no window finishes: the step
graph (wh_time_stage 0) at 1 window greedy, 1 window beam 5, 20 windows x beam 5 and 20
windows x 5 sampled rows (temperature 0.7: the rows keep their own K/V slots, so the step's
self-attention reads do not depend on which tokens were chosen, as they do under beam
search, where the two arms decode different tokens and so different beam ancestries), with
no_repeat_ngram_size=3 + repetition_penalty=1.1 and with both off.  Each measurement: a
decode begun with the options, 64 steps decoded (so 64 sampled positions feed the masks),
then 3 x 50 timed steps, the median per step reported.  The two option sets alternate,
REPS times, so drift of the machine shows as spread.
    python profiles/repeat_filter_timing.py [--out profiles/repeat_filter/timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper.coreml_amd"))

import whisper  # noqa: E402
from whisper import synthetic as S  # noqa: E402
from whisper.audio import N_FRAMES  # noqa: E402
from whisper.decoding import DecodingTask  # noqa: E402

REPS = 3

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="large-v3")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "repeat_filter", "timing.json"))
args = ap.parse_args()

m = whisper.load_model(args.model, device=0, dtype="fp16", max_windows=20, max_group=5, synthetic=True)
audio = S.synthetic_audio(30.0, seed=1)
mel = whisper.pad_or_trim(whisper.log_mel_spectrogram(audio, m.dims.n_mels, padding=whisper.audio.N_SAMPLES)[:, :3000],
                          3000)
eot = DecodingTask(m, whisper.DecodingOptions(language="en")).tokenizer.eot


def step_us(n_win, beam, filt, sampled=False):
    kw = dict(no_repeat_ngram_size=3, repetition_penalty=1.1) if filt else {}
    if sampled:
        kw.update(temperature=0.7, best_of=beam)
    else:
        kw.update(beam_size=beam)
    task = DecodingTask(m, whisper.DecodingOptions(language="en", suppress_tokens=f"-1,{eot}", **kw))
    m.ctx.mel_write(np.concatenate([mel] * n_win, axis=1))
    m.ctx.encode([i * N_FRAMES for i in range(n_win)], [N_FRAMES] * n_win)
    m.ctx.decode_begin(task.wh_opts(seed=7), [task.initial_tokens] * n_win, [task.sot_index] * n_win)
    m.ctx.decode_steps(64)
    return statistics.median(m.ctx.time_stage(0, 50) for _ in range(3)) * 1e3


out = {"model": args.model, "dtype": "fp16", "unit": "us per step", "cases": []}
for n_win, beam, sampled in ((1, None, False), (1, 5, False), (20, 5, False), (20, 5, True)):
    off, on = [], []
    step_us(n_win, beam, False, sampled)  # warm-up: graph capture of both option sets
    step_us(n_win, beam, True, sampled)
    for _ in range(REPS):
        off.append(step_us(n_win, beam, False, sampled))
        on.append(step_us(n_win, beam, True, sampled))
    c = dict(windows=n_win, rows=beam or 1, decoder="sampling T=0.7" if sampled else "beam" if beam else "greedy",
             off_us=[round(x, 2) for x in off], on_us=[round(x, 2) for x in on],
             off_median=round(statistics.median(off), 2), on_median=round(statistics.median(on), 2))
    c["delta_us"] = round(c["on_median"] - c["off_median"], 2)
    c["delta_pct"] = round(100.0 * c["delta_us"] / c["off_median"], 2)
    print(json.dumps(c), flush=True)
    out["cases"].append(c)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
m.close()
