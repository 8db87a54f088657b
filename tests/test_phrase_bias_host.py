"""Phrase biasing of the device decode loop (DecodingOptions.hotwords / hotword_boost /
hotword_start; wh_set_phrase_bias), host side: the numpy restatement of the definition
(tests/phrase_bias_ref.py, include/whisper_hip.h) on hand-made rows, the options' validation
and the encoding of text phrases, the ABI struct left as it was, and the definition run on the
CPU oracle's micro model.  CPU only."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from phrase_bias_ref import (FORCED, FORCED_BOOST, FORCED_START, MAX_RULE, MODERATE, MODERATE_B, BiasedInference,
                             apply_phrase_bias, is_cycle, text_tokens)
from repeat_filter_ref import FilteredInference, OracleInference, apply_repeat_filter

EOT, TS = 100, 110  # a toy vocabulary: text ids < 100, specials 100..109, timestamps from 110
V = 128
f32 = np.float32


def _x(fill=1.0):
    return np.full(V, fill, dtype=np.float32)


def _changed(x, fill=1.0):
    return {int(i): float(x[i] - f32(fill)) for i in np.where(x != f32(fill))[0]}


# ---------------------------------------------------------------- the restatement
def test_max_rule_for_a_shared_prefix():
    # [1, 2, 3] boost 4 and [1, 2, 3, 9] boost 6 after "... 1 2": 3 is named twice, B(3) = 6
    x = _x()
    fired = apply_phrase_bias(x, [1, 2], 0, EOT, [[1, 2, 3], [1, 2, 3, 9]], [4.0, 6.0], 0.5)
    assert fired == 2
    assert _changed(x) == {1: 3.0, 3: 6.0}  # the head: max(4 * 0.5, 6 * 0.5); a max, not the sum 10
    # the same with the phrases the other way round
    y = _x()
    apply_phrase_bias(y, [1, 2], 0, EOT, [[1, 2, 3, 9], [1, 2, 3]], [6.0, 4.0], 0.5)
    np.testing.assert_array_equal(x, y)
    # different continuations of a shared prefix both get their own boost
    x = _x()
    assert apply_phrase_bias(x, [1, 2], 0, EOT, [[1, 2, 3], [1, 2, 4]], [4.0, 6.0], 0.0) == 2
    assert _changed(x) == {3: 4.0, 4: 6.0}


def test_overlapping_phrase():
    # [a, a, b] after "... a a": k = 1 (next a) and k = 2 (next b) both fire
    x = _x()
    assert apply_phrase_bias(x, [9, 7, 7], 0, EOT, [[7, 7, 8]], [5.0], 0.0) == 2
    assert _changed(x) == {7: 5.0, 8: 5.0}
    # after one a only k = 1
    x = _x()
    assert apply_phrase_bias(x, [9, 7], 0, EOT, [[7, 7, 8]], [5.0], 0.0) == 1
    assert _changed(x) == {7: 5.0}
    # an abandoned phrase retracts nothing and fires nothing
    x = _x()
    assert apply_phrase_bias(x, [7, 7, 3], 0, EOT, [[7, 7, 8]], [5.0], 0.0) == 0
    assert _changed(x) == {}


def test_no_match_reaches_below_sample_begin():
    hist = [90, 1, 2]  # 1 2 would continue [1, 2, 3]
    x = _x()
    assert apply_phrase_bias(x, hist, 2, EOT, [[1, 2, 3]], [5.0], 0.0) == 0  # the 1 is prompt
    assert _changed(x) == {}
    x = _x()
    assert apply_phrase_bias(x, hist, 1, EOT, [[1, 2, 3]], [5.0], 0.0) == 1  # the same history, the 1 sampled
    assert _changed(x) == {3: 5.0}
    x = _x()
    assert apply_phrase_bias(x, hist, 3, EOT, [[1, 2, 3]], [5.0], 0.5) == 0  # nothing sampled: the head only
    assert _changed(x) == {1: 2.5}


def test_timestamp_breaks_a_match_and_specials_are_untouched():
    x = _x()
    assert apply_phrase_bias(x, [1, TS + 2, 2], 0, EOT, [[1, 2, 3]], [5.0], 0.0) == 0
    assert _changed(x) == {}
    # ids >= eot are never touched, as head or as continuation (the ABI refuses such a table
    # at decode time; the restatement shows the rule)
    x = _x()
    apply_phrase_bias(x, [1], 0, EOT, [[1, EOT], [TS, 4], [1, TS + 1]], [5.0, 5.0, 5.0], 1.0)
    assert _changed(x) == {1: 5.0}


def test_start_zero_leaves_the_head_alone():
    x = _x()
    assert apply_phrase_bias(x, [], 0, EOT, [[1, 2]], [5.0], 0.0) == 0
    assert _changed(x) == {}
    x = _x()
    apply_phrase_bias(x, [], 0, EOT, [[1, 2]], [5.0], 0.3)
    assert x[1] == f32(1.0) + f32(f32(5.0) * f32(0.3))  # fl32(b * start), then one fp32 add
    # a product that underflows to zero does not fire
    x = _x(0.0)
    apply_phrase_bias(x, [], 0, EOT, [[1, 2]], [1e-30], 1e-30)
    assert _changed(x, 0.0) == {}


def test_order_with_penalty_and_ban():
    # history 5 6 5: penalty 2 on {5, 6}, phrase [5, 6] boost 3 (k = 1 fires: +3 on 6),
    # ban n = 2 (suffix [5], earlier 5 -> 6: banned)
    hist = [5, 6, 5]
    x = _x(4.0)
    apply_repeat_filter(x, hist, 0, EOT, n=0, p=2.0)
    apply_phrase_bias(x, hist, 0, EOT, [[5, 6], [7, 8]], [3.0, 1.0], 0.5)
    assert x[5] == 2.0 + 1.5 and x[6] == 2.0 + 3.0 and x[7] == 4.5  # penalty first, then the bias
    apply_repeat_filter(x, hist, 0, EOT, n=2, p=1.0)
    assert np.isneginf(x[6])  # a banned id stays at -inf
    # BiasedInference(FilteredInference(.)) runs penalty, ban, bias: the same row
    y = _x(4.0)
    apply_repeat_filter(y, hist, 0, EOT, n=2, p=2.0)
    apply_phrase_bias(y, hist, 0, EOT, [[5, 6], [7, 8]], [3.0, 1.0], 0.5)
    np.testing.assert_array_equal(x, y)
    # the penalty after the bias is something else
    z = _x(4.0)
    apply_phrase_bias(z, hist, 0, EOT, [[5, 6], [7, 8]], [3.0, 1.0], 0.5)
    apply_repeat_filter(z, hist, 0, EOT, n=0, p=2.0)
    assert z[5] != x[5]


def test_the_shared_tables_obey_the_limits():
    assert len(FORCED) == 16 and len(set(FORCED)) == 16
    assert {0, 1624, 1625, 50256} <= set(FORCED)
    assert sum(len(p) for p in MODERATE[0]) == sum(len(p) for p in MODERATE_B[0])
    assert [len(p) for p in MODERATE[0]] == [len(p) for p in MODERATE_B[0]]


# ---------------------------------------------------------------- options
def _shell(name="micro"):
    import whisper
    from whisper import synthetic as S
    dims = whisper.ModelDimensions(**S.MODEL_DIMS[name])
    ml = dims.n_vocab >= 51865
    return SimpleNamespace(dims=dims, is_multilingual=ml, num_languages=dims.n_vocab - 51765 - int(ml))


def _task(**kw):
    import whisper
    from whisper.decoding import DecodingTask
    return DecodingTask(_shell(), whisper.DecodingOptions(language="en", **kw))


@pytest.mark.parametrize("bad,name", [
    (dict(hotwords=["Kubernetes"]), "hotword_boost"),                                  # no default boost
    (dict(hotwords=["a", "b"], hotword_boost=[1.0]), "hotword_boost"),                 # one per phrase
    (dict(hotwords=["a"], hotword_boost=0.0), "hotword_boost"),
    (dict(hotwords=["a"], hotword_boost=-1.0), "hotword_boost"),
    (dict(hotwords=["a"], hotword_boost=math.nan), "hotword_boost"),
    (dict(hotwords=["a"], hotword_boost=math.inf), "hotword_boost"),
    (dict(hotwords=["a"], hotword_boost=2.0, hotword_start=1.5), "hotword_start"),
    (dict(hotwords=["a"], hotword_boost=2.0, hotword_start=-0.1), "hotword_start"),
    (dict(hotwords=["a"], hotword_boost=2.0, hotword_start=math.nan), "hotword_start"),
    (dict(hotwords="Kubernetes", hotword_boost=2.0), "hotwords"),                      # one string, not a list
    (dict(hotwords=["  "], hotword_boost=2.0), "hotwords"),
    (dict(hotwords=[[]], hotword_boost=2.0), "hotwords"),
    (dict(hotwords=[list(range(100, 117))], hotword_boost=2.0), "hotwords"),           # 17 tokens
    (dict(hotwords=[[i] for i in range(129)], hotword_boost=2.0), "hotwords"),         # 129 phrases
    (dict(hotwords=[list(range(100, 116))] * 33, hotword_boost=2.0), "hotwords"),      # 528 tokens
    (dict(hotwords=[[50257]], hotword_boost=2.0), "hotwords"),                         # eot
    (dict(hotwords=[[5, 50364]], hotword_boost=2.0), "hotwords"),                      # a timestamp
    (dict(hotwords=[[-1]], hotword_boost=2.0), "hotwords"),
    (dict(hotwords=["supercalifragilisticexpialidocious antidisestablishmentarianism x y z"], hotword_boost=2.0),
     "hotwords"),                                                                      # text longer than 16 tokens
])
def test_options_refused(bad, name):
    with pytest.raises(ValueError, match=name):
        _task(**bad)


def test_options_accepted_and_text_is_encoded_like_text_after_a_timestamp():
    assert _task().phrase_bias is None
    assert _task(hotwords=[]).phrase_bias is None
    assert _task(hotword_boost=3.0).phrase_bias is None  # a boost alone means nothing
    t = _task(hotwords=["Kubernetes", "  mitochondria ", [11, 12, 13]], hotword_boost=4.0, hotword_start=0.25)
    ph, bo, start = t.phrase_bias
    tok = t.tokenizer
    assert ph[0] == tuple(tok.encode(" Kubernetes")) and ph[1] == tuple(tok.encode(" mitochondria"))
    assert tok.decode(list(ph[0])) == " Kubernetes"
    assert ph[2] == (11, 12, 13)
    assert bo == (4.0, 4.0, 4.0) and start == 0.25
    t = _task(hotwords=["a", "b"], hotword_boost=[1.5, 2.5])
    assert t.phrase_bias[1] == (1.5, 2.5) and t.phrase_bias[2] == 0.5  # hotword_start's default
    # the limits themselves are accepted
    t = _task(hotwords=[list(range(100, 116))] * 32, hotword_boost=1.0, hotword_start=1.0)
    assert sum(len(p) for p in t.phrase_bias[0]) == 512
    t = _task(hotwords=[[i] for i in range(128)], hotword_boost=1.0, hotword_start=0.0)
    assert len(t.phrase_bias[0]) == 128
    assert _task(hotwords=[FORCED], hotword_boost=FORCED_BOOST).phrase_bias[0] == (FORCED,)
    # every rung of a temperature ladder keeps the options (dataclasses.replace)
    from dataclasses import replace
    o = replace(t.options, temperature=0.4)
    assert o.hotwords is t.options.hotwords and o.hotword_boost == 1.0


def test_abi_struct_is_as_it_was_and_the_entry_point_is_bound():
    import re
    from whisper import backend_hip
    from conftest import REPO
    names = [f[0] for f in backend_hip.WhDecodeOpts._fields_]
    assert names[-2:] == ["no_repeat_ngram", "repetition_penalty"]  # the table is context state, not an option
    assert "wh_set_phrase_bias" in backend_hip._EXPORTS
    hdr = open(os.path.join(REPO, "include", "whisper_hip.h")).read()
    assert re.search(r"\bint\s+wh_set_phrase_bias\s*\(", hdr)
    w = _task(hotwords=[FORCED], hotword_boost=FORCED_BOOST).wh_opts()
    assert w.no_repeat_ngram == 0  # wh_opts carries nothing of the table


def test_library_exports_the_entry_point_and_version_3():
    import ctypes
    from whisper import backend_hip
    lib = ctypes.CDLL(backend_hip.lib_path())
    assert hasattr(lib, "wh_set_phrase_bias")
    lib.wh_version.restype = ctypes.c_int
    assert lib.wh_version() == 3


# ---------------------------------------------------------------- on the oracle's micro model
@pytest.fixture(scope="module")
def micro():
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    g = np.load(os.path.join(GOLDEN, "micro.npz"))
    dims = S.MODEL_DIMS["micro"]
    model = R.OracleWhisper(dims, S.synthetic_state_dict(dims, int(g["seed"])))
    audio = S.synthetic_audio(30.0, seed=int(g["audio_seed"]))
    mel = R.pad_or_trim(R.log_mel_spectrogram(audio, 80, padding=R.N_SAMPLES)[:, :3000])
    model.set_audio(model.encode(mel))
    return model, R.SpecialTokens.for_model(dims)


class _Span:
    """Records the largest max - min of the raw logit rows that pass through."""

    def __init__(self, inner):
        self.inner, self.span = inner, 0.0

    def logits(self, tokens, audio_features=None):
        out = self.inner.logits(tokens, audio_features)
        lg = np.asarray(out[0])[:, -1]
        self.span = max(self.span, float((lg.max(axis=1) - lg.min(axis=1)).max()))
        return out

    def rearrange_kv_cache(self, source_indices):
        self.inner.rearrange_kv_cache(source_indices)


@pytest.mark.parametrize("beam", [None, 5])
def test_forced_decode_on_the_oracle(micro, beam):
    """One phrase of 16 distinct ids, boost 40, start 0.5, sample_len 40: the text tokens are
    the phrase repeated cyclically, because +40 (next token) and +20 (head) exceed the span of
    the micro logits."""
    from oracle import ref_whisper as R
    from whisper.decoding import DecodingTask
    model, st = micro
    sup = set(_task().suppress_list()) | set(_task().tokenizer.encode(" "))
    assert not sup & set(FORCED) and max(FORCED) == st.eot - 1
    sb = len(st.sot_sequence)
    span = _Span(OracleInference(model))
    inf = BiasedInference(span, sb, st.eot, [FORCED], [FORCED_BOOST], FORCED_START)
    res = R.decode(model, None, R.Options(beam_size=beam, sample_len=40), st, inference=inf)
    text = text_tokens(res.tokens, st.eot)
    print(f"beam {beam}: {len(text)} text tokens of {len(res.tokens)}, logit span {span.span:.3f}, fired {inf.n_fired}")
    assert span.span < FORCED_BOOST * FORCED_START  # what forces the cycle
    assert len(text) >= 32 and is_cycle(text, FORCED)
    assert math.isfinite(res.avg_logprob)


def test_moderate_table_changes_the_oracle_decode(micro):
    """What the GPU parity test relies on, on the CPU: with MODERATE continuation bonuses
    fire and the tokens differ from the unbiased decode; composed with the repetition
    controls in the stated order as well."""
    from oracle import ref_whisper as R
    model, st = micro
    sb = len(st.sot_sequence)
    plain = R.decode(model, None, R.Options(sample_len=64), st, inference=OracleInference(model))
    for n, p in ((0, 1.0), (3, 1.2)):
        inner = FilteredInference(OracleInference(model), sb, st.eot, n=n, p=p) if n else OracleInference(model)
        inf = BiasedInference(inner, sb, st.eot, *MODERATE)
        res = R.decode(model, None, R.Options(sample_len=64), st, inference=inf)
        assert inf.n_fired >= 1 and list(res.tokens) != list(plain.tokens)
        assert math.isfinite(res.avg_logprob)
        assert set(text_tokens(res.tokens, st.eot)) & {300, 400, 500}  # tails the unbiased decode never emits


def test_max_rule_table_tells_a_sum_from_a_max(micro, monkeypatch):
    """What the GPU case with MAX_RULE relies on: a restatement that sums the bonuses of the
    pairs naming one id moves avg_logprob far past the parity bound of 1e-4."""
    import phrase_bias_ref
    from oracle import ref_whisper as R
    model, st = micro
    sb = len(st.sot_sequence)

    def summing(x, tokens, sample_begin, eot, phrases, boosts, start):
        fired = 0
        for p, b in zip(phrases, boosts):
            fired += apply_phrase_bias(x, tokens, sample_begin, eot, [p], [b], start)
        return fired

    def run():
        inf = BiasedInference(OracleInference(model), sb, st.eot, *MAX_RULE)
        return R.decode(model, None, R.Options(sample_len=96), st, inference=inf), inf

    a, inf = run()
    monkeypatch.setattr(phrase_bias_ref, "apply_phrase_bias", summing)
    b, _ = run()
    text = text_tokens(a.tokens, st.eot)
    assert inf.n_fired >= 1 and any(text[i] == text[i + 1] == 10496 for i in range(len(text) - 1))
    assert abs(a.avg_logprob - b.avg_logprob) > 0.1
