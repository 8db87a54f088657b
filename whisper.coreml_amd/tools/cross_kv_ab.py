"""A/B of the decoder step over the fp16 cross-KV and over its 8-bit copy (cross_kv="fp8"):
large-v3 dimensions, one encoder layer, synthetic weights, two contexts in one process.  Per
batch shape (beam 5 at 1, 2, 15 and 20 windows) the step's cross-attention launch
(time_stage 3) and the whole step graph (time_stage 0) are timed alternately, native / fp8 /
native / fp8, PAIRS times; one JSON line per shape with each median and spread (max - min).
The first line is the encode time per window of each context (the fp8 one includes the
quantiser).  Run once, as one process, under a time limit."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "whisper.coreml_amd"), REPO]
import whisper  # noqa: E402
from whisper import synthetic as S  # noqa: E402
from whisper.decoding import DecodingTask  # noqa: E402

PAIRS, WINDOWS = 7, 20
dims = dict(S.MODEL_DIMS["large-v3"], n_audio_layer=1)
sd = S.synthetic_state_dict(dims, 0)
audio = S.synthetic_audio(30.0 * WINDOWS, seed=1000)
ctxs = {}
for fmt in ("native", "fp8"):
    m = whisper.Whisper(whisper.ModelDimensions(**dims), "large-v3-1enc", device=0, dtype="fp16", max_windows=WINDOWS,
                        max_group=5, cross_kv=None if fmt == "native" else "fp8")
    m.load_state_dict(sd)
    m.ctx.log_mel(audio, dims["n_mels"], padding=whisper.audio.N_SAMPLES)
    m.ctx.encode([3000 * i for i in range(WINDOWS)], [3000] * WINDOWS)
    ctxs[fmt] = (m, DecodingTask(m, whisper.DecodingOptions(language="en", beam_size=5)))


def stat(xs):
    return dict(median=round(statistics.median(xs), 5), spread=round(max(xs) - min(xs), 5))


enc = {fmt: [] for fmt in ctxs}
for _ in range(PAIRS):
    for fmt, (m, _) in ctxs.items():
        enc[fmt].append(m.ctx.time_stage(1, 3))
print(json.dumps(dict(encode_ms_per_window={f: stat(v) for f, v in enc.items()})), flush=True)
for nw in (1, 2, 15, 20):
    t = {(fmt, what): [] for fmt in ctxs for what in (3, 0)}
    for fmt, (m, task) in ctxs.items():
        m.ctx.decode_begin(task.wh_opts(), [task.initial_tokens] * nw, [task.sot_index] * nw)
    for _ in range(PAIRS):
        for what, iters in ((3, 5), (0, 10)):
            for fmt, (m, _) in ctxs.items():
                t[fmt, what].append(m.ctx.time_stage(what, iters))
    print(json.dumps(dict(windows=nw, beam=5, xattn=ctxs["fp8"][0].ctx.step_kernels(nw, 5)["xattn"],
                          xattn_ms={f: stat(t[f, 3]) for f in ctxs}, step_ms={f: stat(t[f, 0]) for f in ctxs})),
          flush=True)
for m, _ in ctxs.values():
    m.close()
