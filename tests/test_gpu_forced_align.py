"""Forced alignment on the GPU: wh_dtw_open / wh_align_batch_open (csrc/wh_align.hip) and
whisper.align / align_batch (whisper/align.py), micro synthetic model, fp32.

* dtw_open against tests/dtw_open_ref.py: path, end row and scores bit-exact (the cost
  cells are one fp64 add rounded to fp32 and the score one more; every comparison is fp32).
* align_batch_open against the oracle pipeline (its cross-QK -> alignment_matrix ->
  dtw_open_ref): end rows and paths equal, probabilities rtol 1e-3, the bar of
  tests/test_gpu_words.py; closed windows of a mixed call equal ctx.align_batch exactly in
  path, to rtol 1e-5 in probability (batched against single first passes, as there).
* whisper.align on the golden window's audio against the reference's find_alignment words
  (micro_words.json), a multi-window file, and align_batch against lone align calls."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dtw_open_ref import dtw_open_ref, dtw_tables, planted_matrix

pytestmark = pytest.mark.gpu

ROW_PENALTY = 4.0


@pytest.fixture(scope="module")
def words_golden():
    with open(os.path.join(GOLDEN, "micro_words.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def micro32():
    import whisper
    m = whisper.load_model("micro", device=0, dtype="fp32", max_windows=4, max_group=5, synthetic=True)
    yield m
    m.close()


def _matrix(shape, kind):
    n, m = shape
    rng = np.random.default_rng(n * 10007 + m * 31 + len(kind))
    if kind == "zeros":
        return np.zeros(shape, dtype=np.float32)
    if kind == "ints":
        return rng.integers(0, 3, shape).astype(np.float32)
    if kind == "randn":
        return rng.standard_normal(shape).astype(np.float32)
    spoken = max(1, min(2 * n // 3, m // 3))
    return planted_matrix(n, m, spoken, 0.2, n + m, min_frames=3 if 3 * spoken <= m else 1)[0]


SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (17, 5), (5, 300), (40, 150), (220, 1500)]
# (600, 1500): the 2-bit trace no longer fits LDS, so the kernel keeps it in global memory
DTW_CASES = [(s, k) for s in SHAPES for k in ("zeros", "ints", "randn", "planted")] + [((600, 1500), "ints"),
                                                                                      ((600, 1500), "planted")]


@pytest.mark.parametrize("shape,kind", DTW_CASES)
def test_dtw_open_matches_the_definition(micro32, shape, kind):
    x = _matrix(shape, kind)
    n = shape[0]
    tables = dtw_tables(x)
    for min_rows in sorted({1, max(1, n // 2), n}):
        for pen in (0.0, ROW_PENALTY):
            path, e, scores = micro32.ctx.dtw_open(x, min_rows, pen)
            rpath, re, rscores = dtw_open_ref(x, min_rows, pen, tables)
            assert e == re, (min_rows, pen)
            np.testing.assert_array_equal(scores, rscores, err_msg=str((min_rows, pen)))
            np.testing.assert_array_equal(path, rpath, err_msg=str((min_rows, pen)))
            assert path.shape[1] <= e + shape[1]
    closed = micro32.ctx.dtw(x)
    path, e, scores = micro32.ctx.dtw_open(x, 0, ROW_PENALTY)
    np.testing.assert_array_equal(path, closed)
    np.testing.assert_array_equal(scores, dtw_open_ref(x, 0, ROW_PENALTY, tables)[2])
    assert e == n
    if kind == "zeros":
        assert micro32.ctx.dtw_open(x, 1, 0.0)[1] == 1  # all ties: the smallest admissible row wins


def _window0(m, gw, slots=1):
    """tests/test_gpu_words.py's recipe: window 0 of the golden audio, here in ``slots`` slots
    (windows that share a first pass need a slot each: it writes the slot's self-KV rows)."""
    import whisper
    from whisper import synthetic as S
    audio = S.synthetic_audio(gw["audio_seconds"], seed=gw["audio_seed"])
    mel = whisper.log_mel_spectrogram(audio, m.dims.n_mels, padding=whisper.audio.N_SAMPLES)
    seg = whisper.pad_or_trim(mel[:, :3000], 3000)
    m.ctx.mel_write(seg)
    m.ctx.encode([0] * slots, [3000] * slots)
    m._last_windows = ([0] * slots, [3000] * slots)


def test_align_batch_open_matches_oracle_pipeline(micro32, words_golden):
    from oracle import ref_timing as RT
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    from whisper.timing import _alignment_head_ids
    m = micro32
    _window0(m, words_golden, slots=3)
    xa = m.ctx.audio_features(0)
    np.testing.assert_array_equal(m.ctx.audio_features(2), xa)
    dims = S.MODEL_DIMS["micro"]
    om = R.OracleWhisper(dims, S.synthetic_state_dict(dims, 0))
    om.set_audio(torch.from_numpy(xa))
    st = R.SpecialTokens.for_model(dims)
    n_sot = len(st.sot_sequence)
    heads = _alignment_head_ids(m)
    cases = list(words_golden["find_alignment"].items())
    refs = {}
    for key, case in cases:
        rp, _, _, matrix = RT.find_alignment_path(om, st.sot_sequence, st.no_timestamps, st.eot, case["text_tokens"],
                                                  case["num_frames"])
        refs[key] = (rp, (-matrix).numpy().astype(np.float32))
    # open and closed windows mixed in one call: window k of a call is golden case k with
    # min_rows 1, 0 (closed) or half its rows, rotating over three calls
    half = {key: max(1, (len(case["text_tokens"]) + 1) // 2) for key, case in cases}
    plan, got, closed = [], [], []
    for rot in range(3):
        part = [(key, case, (1, 0, half[key])[(k + rot) % 3]) for k, (key, case) in enumerate(cases)]
        seqs = [[*st.sot_sequence, st.no_timestamps, *case["text_tokens"], st.eot] for _, case, _ in part]
        nfs = [case["num_frames"] for _, case, _ in part]
        slots = list(range(len(part)))
        got += m.ctx.align_batch_open(slots, seqs, n_sot, nfs, heads, [mr for _, _, mr in part], ROW_PENALTY)
        closed += m.ctx.align_batch(slots, seqs, n_sot, nfs, heads)
        plan += part
    assert len(cases) == 3 and sorted(mr == 0 for _, _, mr in plan) == [False] * 6 + [True] * 3
    ends = {}
    for (key, case, mr), (probs, ti, tm, e), (cp, cti, ctm) in zip(plan, got, closed):
        rp, x = refs[key]
        rpath, re, _ = dtw_open_ref(x, mr, ROW_PENALTY)
        assert e == re, (key, mr)
        np.testing.assert_array_equal(ti, rpath[0], err_msg=f"{key} {mr}")
        np.testing.assert_array_equal(tm, rpath[1], err_msg=f"{key} {mr}")
        np.testing.assert_allclose(probs, rp, rtol=1e-3, err_msg=key)
        assert len(ti) <= e + case["num_frames"] // 2
        if mr == 0:
            assert e == len(case["text_tokens"]) + 1
            np.testing.assert_array_equal(ti, cti)
            np.testing.assert_array_equal(tm, ctm)
            np.testing.assert_array_equal(probs, cp)  # the same batched first pass: the same bits
        ends[(key, mr)] = e
    # a lone open window gives what it gave in the batch
    key, case, mr = plan[0]
    one = m.ctx.align_batch_open([0], [[*st.sot_sequence, st.no_timestamps, *case["text_tokens"], st.eot]], n_sot,
                                 [case["num_frames"]], heads, [mr], ROW_PENALTY)[0]
    assert one[3] == ends[(key, mr)]
    np.testing.assert_array_equal(one[1], got[0][1])
    np.testing.assert_array_equal(one[2], got[0][2])
    np.testing.assert_allclose(one[0], got[0][0], rtol=1e-5)


def test_align_single_closed_window_matches_reference(micro32, words_golden):
    """whisper.align on the golden window's audio with a golden case's tokens as the text is
    one closed window: its words equal the reference's find_alignment output (which is
    before add_word_timestamps' segment-level refinements)."""
    import whisper
    from whisper import synthetic as S
    audio = S.synthetic_audio(words_golden["audio_seconds"], seed=words_golden["audio_seed"])[:30 * 16000]
    case = words_golden["find_alignment"]["a"]
    assert case["num_frames"] == 3000
    r = whisper.align(micro32, audio, [case["text_tokens"]], language="en")
    assert r["windows"] == [(0, 3000, len(case["text_tokens"]), len(case["text_tokens"]) + 1, len(case["words"]))]
    assert r["unaligned"] == [] and len(r["segments"]) == 1 and r["segments"][0]["tokens"] == case["text_tokens"]
    got, ref = r["segments"][0]["words"], case["words"]
    assert [w["word"] for w in got] == [w["word"] for w in ref]
    assert [w["tokens"] for w in got] == [w["tokens"] for w in ref]
    np.testing.assert_allclose([w["start"] for w in got], [w["start"] for w in ref], rtol=0, atol=1e-9)
    np.testing.assert_allclose([w["end"] for w in got], [w["end"] for w in ref], rtol=0, atol=1e-9)
    np.testing.assert_allclose([w["probability"] for w in got], [w["probability"] for w in ref], rtol=1e-3)


def _timeline(result):
    return [(w["word"], tuple(w["tokens"]), w["start"], w["end"]) for s in result["segments"] for w in s["words"]]


def test_align_multi_window_and_batch(micro32):
    import whisper
    from whisper import synthetic as S
    from whisper.tokenizer import get_tokenizer
    m = micro32
    tok = get_tokenizer(m.is_multilingual, num_languages=m.num_languages, language="en", task="transcribe")
    rng = np.random.default_rng(21)
    long_text = [[int(t) for t in rng.integers(0, tok.eot, 30)] for _ in range(5)]  # 150 tokens in 5 lines
    short_text = [[int(t) for t in rng.integers(0, tok.eot, 12)]]
    long_audio = S.synthetic_audio(65.0, seed=7)
    short_audio = S.synthetic_audio(10.0, seed=8)
    lone = whisper.align(m, long_audio, long_text, language="en")
    assert len(lone["windows"]) >= 3
    words = _timeline(lone)
    assert len(words) > 0
    n_words = sum(len(tok.split_to_word_tokens(line)[0]) for line in long_text)
    kept = sum(len(w[1]) for w in words) + sum(len(u["tokens"]) for u in lone["unaligned"])
    assert kept == 150 and len(words) + len(lone["unaligned"]) <= n_words
    starts = [w[2] for w in words]
    assert starts == sorted(starts)
    assert all(0.0 <= w[2] <= w[3] <= 65.0 for w in words)
    for (seek, seg, n_cand, e, acc), nxt in zip(lone["windows"], lone["windows"][1:]):
        assert nxt[0] > seek or acc > 0
    short = whisper.align(m, short_audio, short_text, language="en")
    assert short["windows"] == [(0, 1000, 12, 13, len(_timeline(short)))]
    batch = whisper.align_batch(m, [long_audio, short_audio, long_audio], [long_text, short_text, long_text],
                                language="en")

    def same(got, want):
        assert _timeline(got) == _timeline(want) and got["windows"] == want["windows"]
        assert got["language"] == want["language"] == "en"
        assert [u["tokens"] for u in got["unaligned"]] == [u["tokens"] for u in want["unaligned"]]
        gp = [w["probability"] for s in got["segments"] for w in s["words"]]
        wp = [w["probability"] for s in want["segments"] for w in s["words"]]
        np.testing.assert_allclose(gp, wp, rtol=1e-5)

    same(batch[0], lone)
    same(batch[1], short)
    same(batch[2], lone)
    same(batch[2], batch[0])
    # lanes run longest file first, so above the 10 s file holds the last slot and nobody moves
    # when it ends.  Here the first 65 s file has the short text and ends rounds before the
    # second, whose lane then moves from slot 1 to slot 0.
    early = whisper.align(m, long_audio, short_text, language="en")
    assert len(early["windows"]) < len(lone["windows"])
    moved = whisper.align_batch(m, [long_audio, long_audio, short_audio], [short_text, long_text, short_text],
                                language="en")
    same(moved[0], early)
    same(moved[1], lone)
    same(moved[2], short)


def test_align_detects_the_language_of_the_first_window(micro32):
    """language=None: the language is transcribe's for the same audio (the first window's
    <|startoftranscript|> pass), per file of a batch, and the result is that of an align call
    given that language."""
    import whisper
    from whisper import synthetic as S
    m = micro32
    rng = np.random.default_rng(22)
    text = [[int(t) for t in rng.integers(0, 50000, 20)]]
    audio = S.synthetic_audio(12.0, seed=9)
    detected = whisper.transcribe(m, audio, temperature=0.0, without_timestamps=True, sample_len=2)["language"]
    assert detected in whisper.tokenizer.LANGUAGES
    lone = whisper.align(m, audio, text)
    assert lone["language"] == detected
    given = whisper.align(m, audio, text, language=detected)
    assert _timeline(lone) == _timeline(given) and lone["windows"] == given["windows"]
    batch = whisper.align_batch(m, [audio, audio], [text, text], language=[None, "en"])
    assert batch[0]["language"] == detected and batch[1]["language"] == "en"
    assert _timeline(batch[0]) == _timeline(lone)
    with pytest.raises(ValueError, match="no text token"):  # refused before the detection runs
        whisper.align(m, audio, [[51000, 1 << 20]])


def test_abi_refusals_leave_the_context_usable(micro32, words_golden):
    from whisper import HipBackendError
    from whisper.timing import _alignment_head_ids
    from whisper.tokenizer import get_tokenizer
    m = micro32
    x = np.random.default_rng(0).standard_normal((7, 20)).astype(np.float32)
    want = m.ctx.dtw(x)
    with pytest.raises(HipBackendError, match="min_rows"):
        m.ctx.dtw_open(x, 8, ROW_PENALTY)
    with pytest.raises(HipBackendError, match="min_rows"):
        m.ctx.dtw_open(x, -1, ROW_PENALTY)
    for pen in (float("nan"), float("inf"), -1.0):
        with pytest.raises(HipBackendError, match="row_penalty"):
            m.ctx.dtw_open(x, 1, pen)
    with pytest.raises(HipBackendError, match="n_rows"):
        m.ctx.dtw_open(np.zeros((1024, 4), dtype=np.float32), 1, ROW_PENALTY)
    np.testing.assert_array_equal(m.ctx.dtw(x), want)
    np.testing.assert_array_equal(m.ctx.dtw_open(x, 0, ROW_PENALTY)[0], want)

    _window0(m, words_golden)
    tok = get_tokenizer(m.is_multilingual, num_languages=m.num_languages, language="en", task="transcribe")
    text = words_golden["find_alignment"]["c"]["text_tokens"]
    seq = [*tok.sot_sequence, tok.no_timestamps, *text, tok.eot]
    heads, n_sot = _alignment_head_ids(m), len(tok.sot_sequence)
    good = m.ctx.align_batch_open([0], [seq], n_sot, [800], heads, [1], ROW_PENALTY)
    with pytest.raises(HipBackendError, match="min_rows"):
        m.ctx.align_batch_open([0], [seq], n_sot, [800], heads, [len(text) + 2], ROW_PENALTY)
    with pytest.raises(HipBackendError, match="row_penalty"):
        m.ctx.align_batch_open([0], [seq], n_sot, [800], heads, [1], float("nan"))
    with pytest.raises(HipBackendError, match="n_rows"):
        m.ctx.align_batch_open([0], [[*seq[:-1], *([text[0]] * 1100), tok.eot]], n_sot, [800], heads, [1], ROW_PENALTY)
    with pytest.raises(HipBackendError, match="num_frames"):
        m.ctx.align_batch_open([0], [seq], n_sot, [1], heads, [1], ROW_PENALTY)  # what wh_align_batch refuses
    again = m.ctx.align_batch_open([0], [seq], n_sot, [800], heads, [1], ROW_PENALTY)
    assert again[0][3] == good[0][3]
    np.testing.assert_array_equal(again[0][1], good[0][1])
    np.testing.assert_array_equal(again[0][2], good[0][2])
