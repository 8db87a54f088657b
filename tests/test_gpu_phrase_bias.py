"""Phrase biasing in the device decode loop (DecodingOptions.hotwords; wh_set_phrase_bias;
k_logit_part's history-filter instantiations) against the reference's own host loop.

The construction of test_gpu_repeat_filter.py: `oracle.ref_whisper.decode` drives the per-step
ABI (HipInference: wh_prefill / wh_step / wh_reorder_kv, which apply nothing), wrapped by the
numpy restatement of the bias (tests/phrase_bias_ref.py) and, where the case has them, of the
repetition controls, in the stated order.  Both paths see the same logits, so the tokens must
be equal and avg_logprob must agree to that file's bound (abs 1e-4).  The forced cycle, the
prompt boundary, the no-leak sequence and the refusals do not depend on the host loop.

Micro fp32, one window of micro.npz's audio, sample_len 96: sampled positions cross the wave
boundaries of the 512-thread workgroup, the prompted case starts sampling at 44."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from phrase_bias_ref import (FORCED, FORCED_BOOST, FORCED_START, MAX_RULE, MODERATE, MODERATE_B, BiasedInference,
                             is_cycle, text_tokens)
from repeat_filter_ref import FilteredInference

pytestmark = pytest.mark.gpu

SAMPLE_LEN = 96
EOT = 50257  # micro and large-v3 share the multilingual ids below the language tokens


def _hot(table):
    """DecodingOptions keywords of a (phrases, boosts, start) table."""
    return dict(hotwords=[list(p) for p in table[0]], hotword_boost=list(table[1]), hotword_start=table[2])


FORCED_TABLE = ((FORCED,), (FORCED_BOOST,), FORCED_START)


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


@pytest.fixture(scope="module")
def golden_greedy():
    return np.load(os.path.join(GOLDEN, "micro.npz"))["greedy_tokens"]


def _host_loop(m, name, mel, opts, table, n, p, sample_len):
    """The oracle's decode loop over the per-step ABI with the filters restated on the host."""
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
    inner = HipInference(m, task.sample_begin, group=opts.get("beam_size", 1), sot_index=task.sot_index)
    if n or p != 1.0:
        inner = FilteredInference(inner, task.sample_begin, st.eot, n=n, p=p)
    inf = BiasedInference(inner, task.sample_begin, st.eot, *table)
    ref = R.decode(SimpleNamespace(dims=dims), None, R.Options(sample_len=sample_len, **opts), st, inference=inf)
    return ref, inf, st


CASES = {
    "greedy": dict(),
    "greedy_prompt": dict(prompt=list(range(1000, 1040))),
    "notime": dict(without_timestamps=True),
    "beam": dict(beam_size=5),
}


@pytest.fixture(scope="module")
def unbiased(micro32, window_mel):
    """The unbiased device decode of every case, computed once."""
    import whisper
    return {c: whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN, **o))
            for c, o in CASES.items()}


# ---------------------------------------------------------------- 1. device loop = host loop
@pytest.mark.parametrize("n,p", [(0, 1.0), (3, 1.2)])
@pytest.mark.parametrize("case", list(CASES))
def test_biased_decode_equals_host_loop(micro32, window_mel, unbiased, case, n, p):
    import whisper
    opts = CASES[case]
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=SAMPLE_LEN, no_repeat_ngram_size=n, repetition_penalty=p, **_hot(MODERATE), **opts))
    ref, inf, st = _host_loop(micro32, "micro", window_mel, opts, MODERATE, n, p, SAMPLE_LEN)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    print(f"{case} n={n} p={p}: {len(a)} tokens (host loop {len(b)}), avg_logprob {got.avg_logprob:.6f} vs "
          f"{ref.avg_logprob:.6f}; host loop fired {inf.n_fired} continuation bonuses")
    assert inf.n_fired >= 1
    np.testing.assert_array_equal(a, b)
    assert got.avg_logprob == pytest.approx(ref.avg_logprob, abs=1e-4)
    assert list(a) != list(unbiased[case].tokens)
    assert micro32.ctx.phrase_bias is None  # nothing stays installed


@pytest.mark.parametrize("beam", [None, 5])
def test_max_rule_and_overlapping_phrase_equal_host_loop(micro32, window_mel, beam):
    """MAX_RULE: two phrases with a shared prefix name the same continuation (the larger bonus
    counts, not the sum) and [a, a, b] fires k = 1 and k = 2 at once; a kernel that summed, or
    dropped one of the overlapping matches, misses the avg_logprob bound (phrase_bias_ref.py)."""
    import whisper
    opts = dict(beam_size=beam) if beam else {}
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN,
                                                                      **_hot(MAX_RULE), **opts))
    ref, inf, st = _host_loop(micro32, "micro", window_mel, opts, MAX_RULE, 0, 1.0, SAMPLE_LEN)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    text = text_tokens(a, st.eot)
    print(f"beam {beam}: avg_logprob {got.avg_logprob:.6f} vs {ref.avg_logprob:.6f}; fired {inf.n_fired}")
    assert inf.n_fired >= 1
    assert any(text[i] == text[i + 1] == 10496 for i in range(len(text) - 1))  # the overlap did occur
    np.testing.assert_array_equal(a, b)
    assert got.avg_logprob == pytest.approx(ref.avg_logprob, abs=1e-4)


# ---------------------------------------------------------------- 2. the forced cycle
@pytest.mark.parametrize("beam", [None, 5])
def test_forced_cycle(micro32, window_mel, beam):
    import whisper
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=SAMPLE_LEN, beam_size=beam, **_hot(FORCED_TABLE)))
    text = text_tokens(got.tokens, EOT)
    print(f"beam {beam}: {len(text)} text tokens of {len(got.tokens)}")
    assert len(text) >= SAMPLE_LEN - 8
    assert is_cycle(text, FORCED)
    assert np.isfinite(got.avg_logprob)


# ---------------------------------------------------------------- 3. the prompt boundary
def test_no_match_reaches_into_the_prompt(micro32, window_mel):
    """prompt = p[:2], start = 0: nothing of the phrase is sampled, so nothing fires and the
    tokens are those of the unbiased decode with that prompt.  A kernel matching into the
    prompt would add 40 to p[2] at the first update."""
    import whisper
    prompt = list(FORCED[:2])
    plain = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN,
                                                                        prompt=prompt))
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=SAMPLE_LEN, prompt=prompt, hotwords=[list(FORCED)], hotword_boost=FORCED_BOOST,
        hotword_start=0.0))
    assert FORCED[2] not in plain.tokens
    np.testing.assert_array_equal(np.asarray(got.tokens), np.asarray(plain.tokens))
    assert got.avg_logprob == plain.avg_logprob


def test_no_match_reaches_into_the_prefix(micro32, window_mel):
    """The same with prefix = p[:2]: a prefix lies directly below sample_begin (a prompt is
    followed by the SOT sequence, whose specials no table may name), so here a kernel without
    the k <= len - sample_begin bound would match p[:2] and add 40 to p[2] at the first update."""
    import whisper
    prefix = list(FORCED[:2])
    plain = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN,
                                                                        prefix=prefix))
    got = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=SAMPLE_LEN, prefix=prefix, hotwords=[list(FORCED)], hotword_boost=FORCED_BOOST,
        hotword_start=0.0))
    assert FORCED[2] not in plain.tokens and FORCED[2] not in got.tokens
    np.testing.assert_array_equal(np.asarray(got.tokens), np.asarray(plain.tokens))
    assert got.avg_logprob == plain.avg_logprob
    # once p[:2] is sampled instead (start > 0 forces it), p[2] does follow
    forced = whisper.decode(micro32, window_mel, whisper.DecodingOptions(
        language="en", sample_len=8, hotwords=[list(FORCED)], hotword_boost=FORCED_BOOST, hotword_start=FORCED_START))
    assert text_tokens(forced.tokens, EOT)[:3] == list(FORCED[:3])


# ---------------------------------------------------------------- 4. large-v3 width
def test_large_v3_beam_real_vocabulary():
    """The real vocabulary (51866 ids: 1625-id text slices), fp16, beam 5, eot suppressed so the
    decode runs its whole length, as test_gpu_repeat_filter.py's: phrases whose ids lie in the
    first and in the last text slice."""
    import whisper
    from conftest import full_model, golden_window
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    m = full_model("large-v3", "fp16")
    st = R.SpecialTokens.for_model(S.MODEL_DIMS["large-v3"])
    opts = dict(beam_size=5, suppress_tokens=f"-1,{st.eot}")
    mel = golden_window("large-v3")
    # ids below 1624 (first slice) and from 48740 (last text slice, up to eot - 1)
    # (boosts far above any logit span, so that heads are chosen and continuations fire)
    table = (((100, 49000, 200, 50256), (300, 50000, 1623), (48740, 400)), (200.0, 180.0, 190.0), 0.5)
    sample_len = 48
    got = whisper.decode(m, mel, whisper.DecodingOptions(language="en", sample_len=sample_len, **_hot(table), **opts))
    ref, inf, _ = _host_loop(m, "large-v3", mel, opts, table, 0, 1.0, sample_len)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    print(f"large-v3 fp16 beam: {len(a)} tokens, avg_logprob {got.avg_logprob:.6f} vs {ref.avg_logprob:.6f}; "
          f"host loop fired {inf.n_fired}; text {text_tokens(a, st.eot)[:12]}")
    assert inf.n_fired >= 1
    np.testing.assert_array_equal(a, b)
    assert got.avg_logprob == pytest.approx(ref.avg_logprob, abs=1e-4)
    assert m.ctx.phrase_bias is None


# ---------------------------------------------------------------- 5. batching
@pytest.mark.parametrize("beam", [None, 5])
def test_three_windows_equal_each_alone(micro32, window_mel, beam):
    """Three windows in one batch (the 16-slice kernels), a different prompt each: every
    window's tokens equal the same window decoded alone (32 slices) with the same table."""
    import whisper
    from whisper.audio import N_FRAMES
    from whisper.decoding import run_windows
    options = whisper.DecodingOptions(language="en", sample_len=SAMPLE_LEN, beam_size=beam, no_repeat_ngram_size=3,
                                      repetition_penalty=1.2, **_hot(MODERATE))
    prompts = [None, list(range(1000, 1040)), [10496, 300]]  # the last one ends inside a phrase
    alone = [whisper.decode(micro32, window_mel, options, prompt=pr) for pr in prompts]
    micro32.ctx.mel_write(np.concatenate([window_mel] * 3, axis=1))
    micro32.ctx.encode([i * N_FRAMES for i in range(3)], [N_FRAMES] * 3)
    res = run_windows(micro32, options, prompts)
    for w, (r, a) in enumerate(zip(res, alone)):
        np.testing.assert_array_equal(np.asarray(r.tokens), np.asarray(a.tokens), err_msg=f"window {w}")
    assert len({tuple(r.tokens) for r in res}) > 1  # the prompts made the windows differ
    assert set(text_tokens(res[0].tokens, EOT)) & {300, 400, 500}  # and the table acted


# ---------------------------------------------------------------- 6. no leak, graph replay
def test_tables_do_not_leak_and_a_replayed_graph_follows_the_new_table(micro32, window_mel, golden_greedy):
    import whisper
    on = whisper.DecodingOptions(language="en", **_hot(MODERATE))
    on_b = whisper.DecodingOptions(language="en", **_hot(MODERATE_B))
    off = whisper.DecodingOptions(language="en")
    a = whisper.decode(micro32, window_mel, on)
    a2 = whisper.decode(micro32, window_mel, on_b)  # the same entry count: the captured graph is replayed
    b = whisper.decode(micro32, window_mel, off)
    c = whisper.decode(micro32, window_mel, on)
    d = whisper.decode(micro32, window_mel, off)
    np.testing.assert_array_equal(np.asarray(b.tokens), golden_greedy)
    np.testing.assert_array_equal(np.asarray(d.tokens), golden_greedy)
    assert b.avg_logprob == d.avg_logprob
    assert list(a.tokens) != list(b.tokens)
    np.testing.assert_array_equal(np.asarray(c.tokens), np.asarray(a.tokens))
    assert c.avg_logprob == a.avg_logprob
    # the second table's tails appear, the first one's do not
    ta, tb = set(text_tokens(a.tokens, EOT)), set(text_tokens(a2.tokens, EOT))
    assert ta & {300, 400, 500} and not ta & {600, 700, 800}
    assert tb & {600, 700, 800} and not tb & {300, 400, 500}
    assert micro32.ctx.phrase_bias is None


# ---------------------------------------------------------------- 7. refusals
def _raw_set(ctx, n, tokens, offsets, boost, start):
    """wh_set_phrase_bias itself, with whatever arrays (or None) the case gives."""
    from whisper.backend_hip import _ptr
    arr = [None if v is None else np.asarray(v, dtype=dt) for v, dt in
           ((tokens, np.int32), (offsets, np.int32), (boost, np.float32))]
    rc = ctx.lib.wh_set_phrase_bias(ctx.h, n, *[None if v is None else _ptr(v) for v in arr], float(start))
    return rc, ctx.lib.wh_last_error().decode(errors="replace")


REFUSALS = {
    "null_tokens": (1, None, [0, 1], [1.0], 0.5, None),
    "null_offsets": (1, [5], None, [1.0], 0.5, None),
    "null_boost": (1, [5], [0, 1], None, 0.5, None),
    "offsets_not_from_0": (1, [5, 6], [1, 2], [1.0], 0.5, 0),
    "offsets_not_increasing": (2, [5, 6], [0, 2, 2], [1.0, 1.0], 0.5, 1),
    "offsets_decreasing": (2, [5, 6], [0, 2, 1], [1.0, 1.0], 0.5, 1),
    "phrase_of_17": (2, list(range(100, 118)), [0, 1, 18], [1.0, 1.0], 0.5, 1),
    "total_513": (33, list(range(100, 613)), list(range(0, 513, 16)) + [513], [1.0] * 33, 0.5, 32),
    "too_many_phrases": (129, list(range(100, 229)), list(range(130)), [1.0] * 129, 0.5, None),
    "negative_count": (-1, [5], [0, 1], [1.0], 0.5, None),
    "id_negative": (2, [5, -1], [0, 1, 2], [1.0, 1.0], 0.5, 1),
    "id_past_vocabulary": (3, [5, 6, 51865], [0, 1, 2, 3], [1.0] * 3, 0.5, 2),
    "boost_zero": (2, [5, 6], [0, 1, 2], [1.0, 0.0], 0.5, 1),
    "boost_negative": (1, [5], [0, 1], [-2.0], 0.5, 0),
    "boost_nan": (1, [5], [0, 1], [float("nan")], 0.5, 0),
    "boost_inf": (2, [5, 6], [0, 1, 2], [1.0, float("inf")], 0.5, 1),
    "start_negative": (1, [5], [0, 1], [1.0], -0.25, None),
    "start_above_1": (1, [5], [0, 1], [1.0], 1.5, None),
    "start_nan": (1, [5], [0, 1], [1.0], float("nan"), None),
}


@pytest.fixture(scope="module")
def forced_tokens(micro32, window_mel):
    import whisper
    return list(whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en", **_hot(FORCED_TABLE))).tokens)


def _decode_with_installed_table(m, mel):
    """A default-option decode begun over whatever table the context holds (run_windows would
    replace it): the per-window calls themselves."""
    import whisper
    from whisper.decoding import DecodingTask
    task = DecodingTask(m, whisper.DecodingOptions(language="en"))
    ctx = m.ctx
    ctx.mel_write(mel)
    ctx.encode([0], [3000])
    ctx.decode_begin(task.wh_opts(), [task.initial_tokens], [task.sot_index])
    ctx.decode_steps(task.sample_len)
    return task.finalize(ctx.decode_read(0, 1))[0]


@pytest.mark.parametrize("case", list(REFUSALS))
def test_set_phrase_bias_refusals(micro32, window_mel, golden_greedy, forced_tokens, case):
    import whisper
    n, tokens, offsets, boost, start, phrase = REFUSALS[case]
    ctx = micro32.ctx
    ctx.set_phrase_bias(*FORCED_TABLE)  # the previous table
    try:
        rc, msg = _raw_set(ctx, n, tokens, offsets, boost, start)
        print(case, rc, msg)
        assert rc < 0 and "phrase_bias" in msg
        if phrase is not None:
            assert f"phrase {phrase}" in msg
        # a refused set leaves the old table working
        assert _decode_with_installed_table(micro32, window_mel) == forced_tokens
    finally:
        ctx.set_phrase_bias(None)
    # and a default decode gives the golden tokens
    res = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en"))
    np.testing.assert_array_equal(np.asarray(res.tokens), golden_greedy)


def test_decode_begin_refuses_a_table_id_from_eot(micro32, window_mel, golden_greedy, forced_tokens):
    """The vocabulary admits the id, the decode's eot does not: wh_decode_begin refuses, the
    decode state and the table stay as they were."""
    import whisper
    from whisper.backend_hip import HipBackendError
    from whisper.decoding import DecodingTask
    task = DecodingTask(micro32, whisper.DecodingOptions(language="en"))
    ctx = micro32.ctx
    ctx.mel_write(window_mel)
    ctx.encode([0], [3000])
    try:
        for bad in (EOT, 50364, 51864):
            ctx.set_phrase_bias([[5, 6], [7, bad]], [2.0, 2.0], 0.5)
            with pytest.raises(HipBackendError, match=r"wh_decode_begin failed \(-11\): .*phrase_bias.*phrase 1"):
                ctx.decode_begin(task.wh_opts(), [task.initial_tokens], [task.sot_index])
        # with a lower eot in the options the forced table's last id (50256) is refused too
        ctx.set_phrase_bias(*FORCED_TABLE)
        w = task.wh_opts()
        w.eot = 50256
        with pytest.raises(HipBackendError, match=r"wh_decode_begin failed \(-11\): .*phrase_bias"):
            ctx.decode_begin(w, [task.initial_tokens], [task.sot_index])
        assert _decode_with_installed_table(micro32, window_mel) == forced_tokens
    finally:
        ctx.set_phrase_bias(None)
    res = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en"))
    np.testing.assert_array_equal(np.asarray(res.tokens), golden_greedy)


def test_clearing_and_the_wrapper_remember_what_is_installed(micro32, window_mel, golden_greedy):
    import whisper
    ctx = micro32.ctx
    assert ctx.phrase_bias is None
    ctx.set_phrase_bias(*MODERATE)
    assert ctx.phrase_bias == MODERATE
    rc, _ = _raw_set(ctx, 0, None, None, None, 0.0)  # n_phrases == 0: null pointers are allowed
    assert rc == 0
    assert _decode_with_installed_table(micro32, window_mel) == list(golden_greedy)
    ctx.set_phrase_bias(*MODERATE)
    # run_windows clears a table somebody else left when its options carry none
    res = whisper.decode(micro32, window_mel, whisper.DecodingOptions(language="en"))
    np.testing.assert_array_equal(np.asarray(res.tokens), golden_greedy)
    assert ctx.phrase_bias is None


# ---------------------------------------------------------------- 8. option reach
def _windows(result):
    out = {}
    for s in result["segments"]:
        out.setdefault(s["seek"], []).extend(s["tokens"])
    return out


def _occurrences(text, phrase):
    """How often ``phrase`` occurs contiguously in ``text``."""
    n = len(phrase)
    return sum(1 for i in range(len(text) - n + 1) if tuple(text[i:i + n]) == tuple(phrase))


def test_transcribe_and_transcribe_batch_pass_the_options(micro32):
    """Temperature 0 (one rung, deterministic): the text of every window is the forced cycle.
    Then the ladder (0.0, 0.4): the cycle's text compresses past the threshold, so every window
    is decoded again at T = 0.4, with the table.  There the test asks for the phrase to occur,
    not for a strict cycle: the sampler's uniform draw is 1.0 once in 2^24 draws (Gumbel noise
    +inf), about 0.7 stray tokens per window over 50k ids x 223 updates, with or without a
    table; each costs one cycle of the 13 a window holds."""
    import whisper
    from whisper import synthetic as S
    kw = dict(language="en", condition_on_previous_text=False, hotwords=[list(FORCED)], hotword_boost=FORCED_BOOST,
              hotword_start=FORCED_START)
    audio = S.synthetic_audio(60.0, seed=5)
    out = whisper.transcribe(micro32, audio, temperature=0.0, **kw)
    win = _windows(out)
    assert len(win) >= 2
    for seek, toks in win.items():
        text = text_tokens(toks, EOT)
        assert len(text) >= 16 and is_cycle(text, FORCED), f"window at seek {seek}"
    out = whisper.transcribe(micro32, audio, temperature=(0.0, 0.4), **kw)
    assert len(_windows(out)) >= 2
    assert {s["temperature"] for s in out["segments"]} == {0.4}
    for seek, toks in _windows(out).items():
        assert _occurrences(text_tokens(toks, EOT), FORCED) >= 4, f"window at seek {seek} (T = 0.4)"
    files = [S.synthetic_audio(30.0, seed=6), S.synthetic_audio(45.0, seed=7)]
    outs = whisper.transcribe_batch(micro32, files, temperature=0.0, **kw)
    assert len(outs) == 2
    for i, o in enumerate(outs):
        win = _windows(o)
        assert win, f"file {i}"
        for seek, toks in win.items():
            text = text_tokens(toks, EOT)
            assert len(text) >= 16 and is_cycle(text, FORCED), f"file {i}, window at seek {seek}"
    assert micro32.ctx.phrase_bias is None
    with pytest.raises(ValueError, match="hotword_boost"):
        whisper.transcribe(micro32, audio, language="en", hotwords=["x"])
