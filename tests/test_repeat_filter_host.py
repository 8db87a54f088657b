"""The repetition controls of the device decode loop (DecodingOptions.no_repeat_ngram_size /
repetition_penalty), host side: the numpy restatement of the definition
(tests/repeat_filter_ref.py, include/whisper_hip.h wh_decode_opts) on hand-made sequences,
the options' validation and their way into the ABI struct, and the definition run on the CPU
oracle's micro model (finite, and no n-gram ending in a text token repeats).  CPU only."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from repeat_filter_ref import FilteredInference, OracleInference, apply_repeat_filter, repeats

EOT, TS = 100, 110  # a toy vocabulary: text ids < 100, specials 100..109, timestamps from 110
V = 128


def _x(fill=1.0):
    return np.full(V, fill, dtype=np.float32)


def _killed(x):
    return sorted(int(i) for i in np.where(np.isneginf(x))[0])


# ---------------------------------------------------------------- the n-gram ban
def test_overlapping_match():
    # a a a, n = 2: suffix [a]; windows at q = 0 and q = 1 (the second overlaps the suffix)
    x = _x()
    _, ban = apply_repeat_filter(x, [7, 7, 7], 0, EOT, n=2)
    assert ban == [7] and _killed(x) == [7]
    # a a, n = 2: q = 0 only; its window [a] is the suffix's own predecessor
    x = _x()
    apply_repeat_filter(x, [7, 7], 0, EOT, n=2)
    assert _killed(x) == [7]
    # one token: len(seq) < n, nothing
    x = _x()
    apply_repeat_filter(x, [7], 0, EOT, n=2)
    assert _killed(x) == []


def test_window_starting_at_sample_begin():
    prompt = [90, 91, 92]
    seq = [1, 2, 3, 9, 1, 2]  # suffix [1, 2] matches q = 0: ban 3
    x = _x()
    apply_repeat_filter(x, prompt + seq, len(prompt), EOT, n=3)
    assert _killed(x) == [3]


def test_match_reaching_into_the_prompt_does_not_ban():
    # history ... 1 | 2 3 9 1 2 with sample_begin after the first 1: the window [1, 2]
    # would start one token inside the prompt
    hist = [90, 1, 2, 3, 9, 1, 2]
    x = _x()
    apply_repeat_filter(x, hist, 2, EOT, n=3)
    assert _killed(x) == []
    x = _x()
    apply_repeat_filter(x, hist, 1, EOT, n=3)  # the same history, the 1 now sampled
    assert _killed(x) == [3]


def test_timestamp_and_eot_are_never_banned():
    x = _x()
    apply_repeat_filter(x, [5, TS + 3, 5], 0, EOT, n=2)  # 5 -> timestamp: not banned
    assert _killed(x) == []
    x = _x()
    apply_repeat_filter(x, [5, EOT, 5], 0, EOT, n=2)
    assert _killed(x) == []
    # timestamps take part in the match: [ts, 5] -> 6
    x = _x()
    apply_repeat_filter(x, [TS + 1, 5, 6, TS + 1, 5], 0, EOT, n=3)
    assert _killed(x) == [6]
    # n = 1 bans every text id sampled so far, nothing else
    x = _x()
    apply_repeat_filter(x, [90, 4, TS + 2, 4, 8, EOT + 1], 1, EOT, n=1)
    assert _killed(x) == [4, 8]


# ---------------------------------------------------------------- the penalty
def test_penalty_signs_and_once_per_id():
    x = _x()
    x[1], x[2], x[3], x[4] = 3.0, -3.0, 0.0, 0.7
    x[EOT], x[TS] = 5.0, 5.0
    p = 1.3
    pen, _ = apply_repeat_filter(x, [1, 2, 3, 4, 4, 4, 4, 4, EOT, TS], 0, EOT, p=p)
    assert pen == [1, 2, 3, 4]
    f = np.float32
    assert x[1] == f(3.0) / f(p) and x[2] == f(-3.0) * f(p) and x[3] == 0.0
    assert x[4] == f(0.7) / f(p)  # once, though the id occurs five times
    assert x[EOT] == 5.0 and x[TS] == 5.0 and x[5] == 1.0
    for off in (0.0, 1.0):
        y = _x()
        assert apply_repeat_filter(y, [1, 2, 1], 0, EOT, p=off) == ([], [])
        assert (y == 1.0).all()


def test_penalty_then_ban_and_prompt_excluded():
    x = _x(2.0)
    apply_repeat_filter(x, [50, 51, 1, 2, 1], 2, EOT, n=2, p=2.0)
    assert x[1] == 1.0 and np.isneginf(x[2])  # 2: penalised, then banned
    assert x[50] == 2.0 and x[51] == 2.0       # the prompt's ids are untouched


def test_repeats_helper():
    assert repeats([1, 2, 3, 1, 2, 3], 3, EOT) == [(0, 3)]
    assert repeats([1, 2, TS, 1, 2, TS], 3, EOT) == []
    assert repeats([1, 2, 3, 4], 2, EOT) == []


# ---------------------------------------------------------------- options
def _shell(name="micro"):
    import whisper
    from whisper import synthetic as S
    dims = whisper.ModelDimensions(**S.MODEL_DIMS[name])
    ml = dims.n_vocab >= 51865
    return SimpleNamespace(dims=dims, is_multilingual=ml, num_languages=dims.n_vocab - 51765 - int(ml))


@pytest.mark.parametrize("bad", [dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=17),
                                 dict(repetition_penalty=-0.5), dict(repetition_penalty=math.nan),
                                 dict(repetition_penalty=math.inf)])
def test_options_refused(bad):
    import whisper
    from whisper.decoding import DecodingTask
    with pytest.raises(ValueError, match=next(iter(bad))):
        DecodingTask(_shell(), whisper.DecodingOptions(language="en", **bad))


def test_wh_opts_carries_the_values():
    import whisper
    from whisper.decoding import DecodingTask
    w = DecodingTask(_shell(), whisper.DecodingOptions(language="en")).wh_opts()
    assert w.no_repeat_ngram == 0 and w.repetition_penalty in (0.0, 1.0)
    w = DecodingTask(_shell(), whisper.DecodingOptions(language="en", no_repeat_ngram_size=3,
                                                       repetition_penalty=1.25)).wh_opts()
    assert w.no_repeat_ngram == 3 and w.repetition_penalty == 1.25
    w = DecodingTask(_shell(), whisper.DecodingOptions(language="en", beam_size=5, no_repeat_ngram_size=16)).wh_opts()
    assert w.no_repeat_ngram == 16 and w.beam == 1
    from whisper.backend_hip import WhDecodeOpts
    z = WhDecodeOpts()  # zero-initialised: off
    assert z.no_repeat_ngram == 0 and z.repetition_penalty == 0.0
    names = [f[0] for f in WhDecodeOpts._fields_]
    assert names[-2:] == ["no_repeat_ngram", "repetition_penalty"]  # appended: the old layout is a prefix


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


@pytest.mark.parametrize("n,p", [(3, 1.0), (0, 1.3)])
@pytest.mark.parametrize("beam", [None, 5])
def test_oracle_micro_stays_finite_and_obeys_the_invariant(micro, n, p, beam):
    from oracle import ref_whisper as R
    model, st = micro
    sb = len(st.sot_sequence)
    inf = FilteredInference(OracleInference(model), sb, st.eot, n=n, p=p)
    res = R.decode(model, None, R.Options(beam_size=beam, sample_len=64), st, inference=inf)
    assert math.isfinite(res.avg_logprob) and math.isfinite(res.sum_logprob)
    assert len(res.tokens) > 8
    assert inf.n_banned + inf.n_penalised > 0
    if n:
        assert repeats(res.tokens, n, st.eot) == []
    else:
        # the unfiltered decode loops; the penalty must have changed the result
        plain = R.decode(model, None, R.Options(beam_size=beam, sample_len=64), st,
                         inference=OracleInference(model))
        assert list(plain.tokens) != list(res.tokens)
