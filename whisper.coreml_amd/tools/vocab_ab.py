"""A/B of the single-window step's vocabulary projection over the fp16 token embedding (k_vocab1
at n_text_state 1280) and over its 8-bit copy (vocab="fp8", k_vocab1_w8): large-v3 and turbo
dimensions with one encoder layer, synthetic weights, beam 5, one window, one context per model
whose formats are switched between decodes.  Each round sets the formats, begins the decode anew
(a format serves the batches begun after it) and times the vocabulary launch back to back
(time_stage 10) and the whole step graph (0); native and fp8 alternate, PAIRS rounds each, with
decoder= native and fp8.  One JSON line per model and decoder format with each median and spread
(max - min), and the embedding bytes a token reads.  Run once, as one process, under a time limit."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(REPO, "whisper.coreml_amd"), REPO]
import whisper  # noqa: E402
from whisper import synthetic as S  # noqa: E402
from whisper.decoding import DecodingTask  # noqa: E402

PAIRS = 7
STAGES = ((10, 50, "vocab_ms"), (0, 20, "step_ms"))


def stat(xs):
    return dict(median=round(statistics.median(xs), 5), spread=round(max(xs) - min(xs), 5))


for name in sys.argv[1:] or ("large-v3", "turbo"):
    dims = dict(S.MODEL_DIMS[name], n_audio_layer=1)
    m = whisper.Whisper(whisper.ModelDimensions(**dims), name + "-1enc", device=0, dtype="fp16", max_windows=1, max_group=5)
    m.load_state_dict(S.synthetic_state_dict(dims, 0))
    m.ctx.log_mel(S.synthetic_audio(30.0, seed=1000), dims["n_mels"], padding=whisper.audio.N_SAMPLES)
    m.ctx.encode([0], [3000])
    task = DecodingTask(m, whisper.DecodingOptions(language="en", beam_size=5))
    for dec in ("native", "fp8"):
        m.ctx.set_decoder_format(dec)
        t = {(fmt, key): [] for fmt in ("native", "fp8") for _, _, key in STAGES}
        kern = {}
        for _ in range(PAIRS + 1):  # the first round of each format warms its kernels and is dropped
            for fmt in ("native", "fp8"):
                m.ctx.set_vocab_format(fmt)
                m.ctx.decode_begin(task.wh_opts(), [task.initial_tokens], [task.sot_index])
                kern[fmt] = m.ctx.step_kernels(1, 5)["tail"]
                for what, iters, key in STAGES:
                    t[fmt, key].append(m.ctx.time_stage(what, iters))
        n, V = dims["n_text_state"], dims["n_vocab"]
        print(json.dumps(dict(model=name, n_text_layer=dims["n_text_layer"], windows=1, beam=5, decoder=dec, tail=kern,
                              embedding_mb_per_token={"native": round(V * n * 2 / 1e6, 1), "fp8": round(V * (n + 4) / 1e6, 1)},
                              **{key: {f: stat(t[f, key][1:]) for f in ("native", "fp8")} for _, _, key in STAGES})),
              flush=True)
    m.close()
