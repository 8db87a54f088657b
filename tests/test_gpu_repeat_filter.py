"""The repetition controls of the device decode loop (no_repeat_ngram_size /
repetition_penalty: k_logit_part's RF instantiations) against the reference's own host loop.

The construction of test_gpu_tail.py: `oracle.ref_whisper.decode` drives the per-step ABI
(HipInference: wh_prefill / wh_step / wh_reorder_kv), here wrapped by the numpy restatement
of the filter (tests/repeat_filter_ref.py), which acts on each step's raw logits ahead of
the oracle's own filters.  Both paths see the same logits, so the tokens must be equal and
avg_logprob must agree to that file's bound (abs 1e-4: the device normaliser is summed per
slice).  Every case also asserts that the restatement banned or penalised something, so it
fails on a build that ignores the options, and that no n-gram ending in a text token repeats
in the device result (the unfiltered micro goldens repeat trigrams 207 times).

Micro fp32, one window of micro.npz's audio, sample_len 96: sampled positions cross the
wave boundaries of the 512-thread workgroup, the prompted case starts sampling at 44."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from repeat_filter_ref import FilteredInference, repeats

pytestmark = pytest.mark.gpu

SAMPLE_LEN = 96


@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def window_mel():
    import whisper
    from whisper import synthetic as S
    g = np.load(os.path.join(GOLDEN, "micro.npz"))
    audio = S.synthetic_audio(30.0, seed=int(g["audio_seed"]))
    mel = whisper.log_mel_spectrogram(audio, 80, padding=whisper.audio.N_SAMPLES)
    return whisper.pad_or_trim(mel[:, :3000], 3000)


def _eot():
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    return R.SpecialTokens.for_model(S.MODEL_DIMS["micro"]).eot


def _host_loop(m, name, mel, opts, n, p, sample_len):
    """The oracle's decode loop over the per-step ABI with the filter restated on the host."""
    import whisper
    from oracle import ref_whisper as R
    from types import SimpleNamespace
    from whisper import synthetic as S
    from whisper.decoding import DecodingTask
    from whisper.inference import HipInference
    dims = S.MODEL_DIMS[name]
    st = R.SpecialTokens.for_model(dims)
    task = DecodingTask(m, whisper.DecodingOptions(language="en", sample_len=sample_len, **opts))
    m.ctx.mel_write(mel)
    m.ctx.encode([0], [3000])
    hip = HipInference(m, task.sample_begin, group=opts.get("beam_size", 1), sot_index=task.sot_index)
    inf = FilteredInference(hip, task.sample_begin, st.eot, n=n, p=p)
    ref = R.decode(SimpleNamespace(dims=dims), None, R.Options(sample_len=sample_len, **opts), st, inference=inf)
    return ref, inf, st


CASES = {
    "greedy": dict(),
    "greedy_prompt": dict(prompt=list(range(1000, 1040))),
    "notime": dict(without_timestamps=True),
    "beam": dict(beam_size=5),
}


@pytest.mark.parametrize("n,p", [(3, 1.0), (0, 1.3), (2, 1.2)])
@pytest.mark.parametrize("case", list(CASES))
def test_filtered_decode_equals_host_loop(micro32, window_mel, case, n, p):
    import whisper
    opts = CASES[case]
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=SAMPLE_LEN, no_repeat_ngram_size=n, repetition_penalty=p, **opts))
    ref, inf, st = _host_loop(micro32, "micro", window_mel, opts, n, p, SAMPLE_LEN)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    print(f"{case} n={n} p={p}: {len(a)} tokens (host loop {len(b)}), avg_logprob {got.avg_logprob:.6f} vs "
          f"{ref.avg_logprob:.6f}; host loop banned {inf.n_banned}, penalised {inf.n_penalised}")
    assert inf.n_banned + inf.n_penalised >= 1
    np.testing.assert_array_equal(a, b)
    assert got.avg_logprob == pytest.approx(ref.avg_logprob, abs=1e-4)
    if n:
        assert repeats(a, n, st.eot) == []


def test_large_v3_beam_real_vocabulary():
    """The real vocabulary (51866 ids: 1625-id text slices), fp16, beam 5, eot suppressed so
    the decode runs its whole length, as test_gpu_tail.py's beam_fixed."""
    import whisper
    from conftest import full_model, golden_window
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    m = full_model("large-v3", "fp16")
    st = R.SpecialTokens.for_model(S.MODEL_DIMS["large-v3"])
    opts = dict(beam_size=5, suppress_tokens=f"-1,{st.eot}")
    mel = golden_window("large-v3")
    n, p, sample_len = 3, 1.1, 48
    got = whisper.decode(m, mel, whisper.DecodingOptions(language="en", sample_len=sample_len, no_repeat_ngram_size=n,
                                                         repetition_penalty=p, **opts))
    ref, inf, _ = _host_loop(m, "large-v3", mel, opts, n, p, sample_len)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    print(f"large-v3 fp16 beam: {len(a)} tokens, avg_logprob {got.avg_logprob:.6f} vs {ref.avg_logprob:.6f}; "
          f"host loop banned {inf.n_banned}, penalised {inf.n_penalised}")
    assert inf.n_banned + inf.n_penalised >= 1
    np.testing.assert_array_equal(a, b)
    assert got.avg_logprob == pytest.approx(ref.avg_logprob, abs=1e-4)
    assert repeats(a, n, st.eot) == []


@pytest.mark.parametrize("beam", [None, 5])
def test_three_windows_equal_each_alone(micro32, window_mel, beam):
    """Three windows in one batch (the 16-slice kernels), a different prompt each: every
    window's tokens equal the same window decoded alone (32 slices) with the same options."""
    import whisper
    from whisper.audio import N_FRAMES
    from whisper.decoding import run_windows
    options = whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN, beam_size=beam, no_repeat_ngram_size=3,
                                      repetition_penalty=1.2)
    prompts = [None, list(range(1000, 1040)), list(range(2000, 2007))]
    alone = [whisper.decode(micro32, window_mel, options, prompt=pr) for pr in prompts]
    micro32.ctx.mel_write(np.concatenate([window_mel] * 3, axis=1))
    micro32.ctx.encode([i * N_FRAMES for i in range(3)], [N_FRAMES] * 3)
    res = run_windows(micro32, options, prompts)
    eot = _eot()
    for w, (r, a) in enumerate(zip(res, alone)):
        np.testing.assert_array_equal(np.asarray(r.tokens), np.asarray(a.tokens), err_msg=f"window {w}")
        assert repeats(r.tokens, 3, eot) == [], f"window {w}"
    assert len({tuple(r.tokens) for r in res}) > 1  # the prompts made the windows differ


def test_sampling_rows_obey_the_invariant(micro32, window_mel):
    import whisper
    from whisper.decoding import DecodingTask
    task = DecodingTask(micro32, whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN, temperature=0.7,
                                                         best_of=3, no_repeat_ngram_size=3))
    ctx = micro32.ctx
    ctx.mel_write(window_mel)
    ctx.encode([0], [3000])
    ctx.decode_begin(task.wh_opts(seed=1234), [task.initial_tokens], [task.sot_index])
    ctx.decode_steps(task.sample_len)
    raw = ctx.decode_read(0, 3)
    sb, L = task.sample_begin, raw["length"]
    assert L - sb > 8
    rows = [raw["tokens"][j, sb:L] for j in range(3)]
    for j, row in enumerate(rows):
        assert repeats(row, 3, task.tokenizer.eot) == [], f"row {j}"
    assert len({tuple(int(t) for t in row) for row in rows}) > 1  # it did sample


def test_options_do_not_leak_between_decodes(micro32, window_mel):
    """One context, the step graph re-captured per option set: a filtered decode, a default
    one (micro.npz's greedy tokens, bit for bit), and the filtered one again."""
    import whisper
    g = np.load(os.path.join(GOLDEN, "micro.npz"))
    on = whisper.DecodingOptions(language="en", no_repeat_ngram_size=3, repetition_penalty=1.2)
    off = whisper.DecodingOptions(language="en")
    a = whisper.decode(micro32, window_mel, on)
    b = whisper.decode(micro32, window_mel, off)
    c = whisper.decode(micro32, window_mel, on)
    d = whisper.decode(micro32, window_mel, off)
    np.testing.assert_array_equal(np.asarray(b.tokens), g["greedy_tokens"])
    np.testing.assert_array_equal(np.asarray(d.tokens), g["greedy_tokens"])
    assert b.avg_logprob == d.avg_logprob
    assert list(a.tokens) != list(b.tokens)
    assert repeats(a.tokens, 3, _eot()) == []
    np.testing.assert_array_equal(np.asarray(c.tokens), np.asarray(a.tokens))
    assert c.avg_logprob == a.avg_logprob


@pytest.mark.parametrize("field,value", [("no_repeat_ngram", 17), ("no_repeat_ngram", -1), ("repetition_penalty", -1.0),
                                         ("repetition_penalty", float("nan")), ("repetition_penalty", float("inf"))])
def test_abi_refusals(micro32, window_mel, field, value):
    import whisper
    from whisper.backend_hip import HipBackendError
    from whisper.decoding import DecodingTask
    g = np.load(os.path.join(GOLDEN, "micro.npz"))
    task = DecodingTask(micro32, whisper.DecodingOptions(language="en"))
    ctx = micro32.ctx
    ctx.mel_write(window_mel)
    ctx.encode([0], [3000])
    w = task.wh_opts()
    setattr(w, field, value)
    with pytest.raises(HipBackendError, match=rf"wh_decode_begin failed \(-\d+\): .*{field}"):
        ctx.decode_begin(w, [task.initial_tokens], [task.sot_index])
    # the context is as it was: a default decode straight afterwards gives the golden tokens
    res = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en"))
    np.testing.assert_array_equal(np.asarray(res.tokens), g["greedy_tokens"])


def test_transcribe_passes_the_option(micro32):
    import whisper
    from whisper import synthetic as S
    audio = S.synthetic_audio(60.0, seed=5)
    out = whisper.transcribe(micro32, audio, language="en", no_repeat_ngram_size=3, condition_on_previous_text=False)
    assert out["segments"]
    eot = _eot()
    windows = {}
    for s in out["segments"]:
        windows.setdefault(s["seek"], []).extend(s["tokens"])
    assert len(windows) >= 2
    for seek, toks in windows.items():
        assert repeats(toks, 3, eot) == [], f"window at seek {seek}"
