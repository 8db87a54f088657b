"""A/B of the encoder with its block GEMMs in fp16 (native) and on the 8-bit path
(encoder="fp8"): large-v3 dimensions cut to LAYERS encoder and 4 decoder layers, synthetic
weights, ONE context switched between the formats (wh_set_encoder_format), native / fp8 /
native / fp8, PAIRS times.  One JSON line per measurement with each median and spread
(max - min): the encode per window at 1 window (time_stage 1, device events) and at 20
windows (wall time of wh_encode, which returns synchronised), then one whisper.score call and
one whisper.align window end to end (wall time).  Run once, as one process, under a time limit."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "whisper.coreml_amd"), REPO]
import whisper  # noqa: E402
from whisper import synthetic as S  # noqa: E402
from whisper.backend_hip import WH_ENC_FP8_E4M3, WH_ENC_NATIVE  # noqa: E402

PAIRS, WINDOWS, LAYERS = 7, 20, 8
FORMATS = {"native": WH_ENC_NATIVE, "fp8": WH_ENC_FP8_E4M3}
dims = dict(S.MODEL_DIMS["large-v3"], n_audio_layer=LAYERS, n_text_layer=4)
m = whisper.Whisper(whisper.ModelDimensions(**dims), f"large-v3-{LAYERS}enc", device=0, dtype="fp16", max_windows=WINDOWS,
                    max_group=5)
m.load_state_dict(S.synthetic_state_dict(dims, 0))
audio = S.synthetic_audio(30.0 * WINDOWS, seed=1000)
m.ctx.log_mel(audio, dims["n_mels"], padding=whisper.audio.N_SAMPLES)


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), spread=round(max(xs) - min(xs), 4))


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def ab(what, fn):
    """fn() -> ms, alternated over the formats (one unmeasured call of each first)."""
    t = {f: [] for f in FORMATS}
    for i in range(PAIRS + 1):
        for f, code in FORMATS.items():
            m.ctx.set_encoder_format(code)
            v = fn()
            if i:
                t[f].append(v)
    kern = {}
    for f, code in FORMATS.items():
        m.ctx.set_encoder_format(code)
        kern[f] = m.ctx.encoder_kernels(what.get("windows", 1))
    print(json.dumps(dict(what, encoder_layers=LAYERS, kernels=kern, ms={f: stat(v) for f, v in t.items()})), flush=True)


ab(dict(measure="encode_ms_per_window", windows=1), lambda: m.ctx.time_stage(1, 3))
seeks = [3000 * i for i in range(WINDOWS)]
ab(dict(measure="encode_ms_per_window", windows=WINDOWS),
   lambda: wall_ms(lambda: m.ctx.encode(seeks, [3000] * WINDOWS)) / WINDOWS)
clip = audio[:30 * 16000]
ab(dict(measure="score_call_ms"), lambda: wall_ms(lambda: whisper.score(m, clip, ["hello world", "goodbye"], language="en")))
ab(dict(measure="align_window_ms"), lambda: wall_ms(lambda: whisper.align(m, clip, "hello world again", language="en")))
m.ctx.set_encoder_format(WH_ENC_NATIVE)
m.close()
