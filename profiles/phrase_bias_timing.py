"""What the phrase table costs the selection launch (phrase biasing).

large-v3 fp16 (seeded weights, seeded audio), eot suppressed so no window finishes: the
selection launch alone (wh_time_stage 4: k_logit_part on the current logits) at 1 window x 5
rows and 20 windows x 5 rows (beam 5), after a decode begun with no table and no repetition
controls (the unfiltered instantiations), with no_repeat_ngram_size=3 + repetition_penalty=1.1,
and with a 512-entry table (32 phrases of 16 tokens, start 0.5, so 32 heads fire at every
update) on top of nothing.  Each measurement: decode_begin, 64 steps decoded, then 3 x 200
timed launches, the median per launch reported; the three arms alternate REPS times.  The
timed launches repeat the in-place penalty / add on the same logits, which changes values and
not the time.
    python profiles/phrase_bias_timing.py [--out profiles/phrase_bias/timing.json]
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
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "phrase_bias", "timing.json"))
args = ap.parse_args()

m = whisper.load_model(args.model, device=0, dtype="fp16", max_windows=20, max_group=5, synthetic=True)
audio = S.synthetic_audio(30.0, seed=1)
mel = whisper.pad_or_trim(whisper.log_mel_spectrogram(audio, m.dims.n_mels, padding=whisper.audio.N_SAMPLES)[:, :3000],
                          3000)
eot = DecodingTask(m, whisper.DecodingOptions(language="en")).tokenizer.eot
rng = np.random.default_rng(3)
TABLE = [[int(t) for t in rng.choice(eot, 16, replace=False)] for _ in range(32)]  # 512 entries

ARMS = {"none": {}, "repeat": dict(no_repeat_ngram_size=3, repetition_penalty=1.1),
        "table512": dict(hotwords=TABLE, hotword_boost=2.0, hotword_start=0.5)}


def select_us(n_win, arm):
    task = DecodingTask(m, whisper.DecodingOptions(language="en", suppress_tokens=f"-1,{eot}", beam_size=5, **ARMS[arm]))
    m.ctx.mel_write(np.concatenate([mel] * n_win, axis=1))
    m.ctx.encode([i * N_FRAMES for i in range(n_win)], [N_FRAMES] * n_win)
    m.ctx.set_phrase_bias(*task.phrase_bias) if task.phrase_bias else m.ctx.set_phrase_bias(None)
    m.ctx.decode_begin(task.wh_opts(seed=7), [task.initial_tokens] * n_win, [task.sot_index] * n_win)
    m.ctx.set_phrase_bias(None)
    m.ctx.decode_steps(64)
    return statistics.median(m.ctx.time_stage(4, 200) for _ in range(3)) * 1e3


out = {"model": args.model, "dtype": "fp16", "unit": "us per selection launch", "cases": []}
for n_win in (1, 20):
    t = {a: [] for a in ARMS}
    for a in ARMS:
        select_us(n_win, a)  # warm-up
    for _ in range(REPS):
        for a in ARMS:
            t[a].append(select_us(n_win, a))
    c = dict(windows=n_win, rows=5)
    for a in ARMS:
        c[a + "_us"] = [round(x, 2) for x in t[a]]
        c[a + "_median"] = round(statistics.median(t[a]), 2)
    print(json.dumps(c), flush=True)
    out["cases"].append(c)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
m.close()
