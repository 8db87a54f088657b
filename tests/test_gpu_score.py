"""whisper.score: the fused vocabulary scoring kernel (csrc/wh_score.hip) against numpy fp64,
its row independence, wh_score_batch / whisper.score against the CPU oracle, and the refusals.

The error bar is the project's own (tests/test_gpu_batch.py TAU): a logit is held to
tau * (the reference row's top-32 logit range), lse moves by at most the largest logit error,
so every log-probability is held to 2 * tau * range of its row.  The worst observed share of
that bar goes to the margin log (conftest.record_margin).

Kernel data.  E is N(0, 0.1^2) as in the synthetic checkpoints; a row is N(0, 1) noise plus
PLANT * E[p] / |E[p]| for a random id p, the peaked shape of a trained model's rows (iid normal
logits have a top-2 gap under the fp16 bar in ~9 % of rows, which says nothing about a kernel).
SEED = 21: in the fp64 reference alone, the rows whose top-2 gap is under 2 * tau * range
are 0 of the 1-, 17- and row-block + 1 calls and at most 3 of 257 (1.2 %) in every case, inside
the 2 % that may be left out of the argmax comparison (checked on the CPU with numpy; of
seeds 11..23, 11, 14, 17, 20 and 23 put such a row among the first 17 at width 128 in fp16).
"""
import numpy as np
import pytest

from conftest import record_margin

pytestmark = pytest.mark.gpu

TAU = {"fp32": 2e-5, "fp16": 1e-2}
SEED, PLANT, VMAX, PASS = 21, 6.0, 51866, 256
# rows a workgroup keeps in LDS (csrc/wh_score.hip: the most 16-row tiles, at most 4, with
# 16 * tiles * (K * sizeof + 16 + 256) <= 160 KB)
ROW_BLOCK = {(128, "fp32"): 64, (128, "fp16"): 64, (1280, "fp16"): 48, (1280, "fp32"): 16}
_CACHE = {}


def _operands(width):
    """(E [VMAX][width], rows [PASS + 1][width], state dict without E) of one width, made once."""
    if width not in _CACHE:
        from whisper import synthetic as S
        rng = np.random.default_rng([SEED, width])
        E = (0.1 * rng.standard_normal((VMAX, width), dtype=np.float32)).astype(np.float32)
        p = rng.integers(0, 51864, PASS + 1)
        X = rng.standard_normal((PASS + 1, width), dtype=np.float32)
        X += (PLANT * E[p] / np.linalg.norm(E[p], axis=1, keepdims=True)).astype(np.float32)
        dims = dict(S.MODEL_DIMS["micro"], n_audio_state=width, n_text_state=width, n_audio_head=width // 64,
                    n_text_head=width // 64, n_audio_layer=1, n_text_layer=1)
        sd = S.synthetic_state_dict(dict(dims, n_vocab=8), 0)
        _CACHE[width] = (E, X, dims, sd)
    return _CACHE[width]


def _held(a, dtype):
    """The operand as a context of ``dtype`` holds it, in fp64."""
    return (a.astype(np.float16) if dtype == "fp16" else a).astype(np.float64)


def _case(width, dtype, V):
    """Rows, targets and the fp64 logits of one case.  Rows 3 and 5 are c * E[V - 1] and c * E[0]:
    the argmax in the ragged tail and in the first column.  Targets 0 and 1 are V - 1 and 0."""
    E, X, _, _ = _operands(width)
    key = (width, dtype)
    if key not in _CACHE:
        _CACHE[key] = _held(X, dtype) @ _held(E, dtype).T
    X = X.copy()
    X[3], X[5] = 3.0 * E[V - 1], 3.0 * E[0]
    z = _CACHE[key][:, :V].copy()
    z[[3, 5]] = _held(X[[3, 5]], dtype) @ _held(E[:V], dtype).T
    tgt = np.random.default_rng([SEED, V]).integers(0, V, len(X)).astype(np.int32)
    tgt[0], tgt[1] = V - 1, 0
    return X, tgt, z


def _reference(z, tgt, tau):
    """fp64 log-softmax: (logprob, argmax, top logprob, bar, decisive) per row."""
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    top = np.sort(np.partition(z, -32, axis=1)[:, -32:], axis=1)
    bar = 2 * tau * (top[:, -1] - top[:, 0])
    return z[np.arange(len(z)), tgt] - lse, z.argmax(axis=1), m - lse, bar, (top[:, -1] - top[:, -2]) >= bar


def _context(width, dtype, V):
    import whisper
    E, _, dims, sd = _operands(width)
    m = whisper.Whisper(whisper.ModelDimensions(**dict(dims, n_vocab=V)), "score", device=0, dtype=dtype,
                        max_windows=1, max_group=1)
    m.load_state_dict(dict(sd, **{"decoder.token_embedding.weight": E[:V]}))
    return m


@pytest.mark.parametrize("V", [51864, 51865, 51866])
@pytest.mark.parametrize("width,dtype", list(ROW_BLOCK))
def test_vocab_score_matches_fp64(width, dtype, V):
    """wh_vocab_score at 1, 17, one row block + 1 and one pass + 1 rows against numpy fp64."""
    X, tgt, z = _case(width, dtype, V)
    want_lp, want_top, want_tlp, bar, decisive = _reference(z, tgt, TAU[dtype])
    m = _context(width, dtype, V)
    try:
        for n in (1, 17, ROW_BLOCK[width, dtype] + 1, PASS + 1):
            lp, top, tlp = m.ctx.vocab_score(X[:n], tgt[:n])
            share = float(max((np.abs(lp - want_lp[:n]) / bar[:n]).max(), (np.abs(tlp - want_tlp[:n]) / bar[:n]).max()))
            record_margin("vocab_score", width=width, dtype=dtype, vocab=V, rows=n, share_of_bar=share,
                          indecisive=int((~decisive[:n]).sum()))
            print(f"width {width} {dtype} V {V} rows {n}: worst share of the bar {share:.3g}")
            assert share <= 1.0
            assert (~decisive[:n]).sum() <= 0.02 * n
            np.testing.assert_array_equal(top[decisive[:n]], want_top[:n][decisive[:n]])
            if n > 5:
                assert top[3] == V - 1 and top[5] == 0
    finally:
        m.close()


@pytest.mark.parametrize("width,dtype", [(1280, "fp16"), (128, "fp32")])
def test_vocab_score_row_independence(width, dtype):
    """A row's outputs are bit-identical alone, among 17 rows and among a row block + 1."""
    V, rb = VMAX, ROW_BLOCK[width, dtype]
    X, tgt, _ = _case(width, dtype, V)
    m = _context(width, dtype, V)
    try:
        for row, p17, pblock in ((7, 16, rb), (40, 2, 20)):
            alone = m.ctx.vocab_score(X[[row]], tgt[[row]])
            for n, pos in ((17, p17), (rb + 1, pblock)):
                idx = np.arange(100, 100 + n)
                idx[pos] = row
                among = m.ctx.vocab_score(X[idx], tgt[idx])
                for a, b in zip(alone, among):
                    assert np.array_equal(a, b[[pos]]), (row, n, pos, a, b[pos])
    finally:
        m.close()


# ------------------------------------------------------------------ end to end against the oracle
@pytest.fixture(scope="module", params=["fp32", "fp16"])
def micro(request):
    import torch

    import whisper
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = S.MODEL_DIMS["micro"]
    sd = S.synthetic_state_dict(dims, 0)
    m = whisper.Whisper(whisper.ModelDimensions(**dims), "micro", device=0, dtype=request.param, max_windows=2,
                        max_group=1)
    m.load_state_dict(sd)
    om = R.OracleWhisper(dims, sd)
    audios = [S.synthetic_audio(12.0, seed=31), S.synthetic_audio(7.0, seed=32)]
    xa = []
    for a in audios:
        mel = R.log_mel_spectrogram(a, dims["n_mels"], padding=R.N_SAMPLES)
        xa.append(om.encode(R.pad_or_trim(mel[:, :len(a) // 160])))

    def oracle(file, seq, n_ctx):
        """fp64 log-softmax of the oracle's teacher-forced logits: (logprob, bar) per scored position."""
        om.set_audio(xa[file])
        z = om.decoder_forward(torch.tensor([seq[:-1]]), 0, None)[0][0].double().numpy()[n_ctx - 1:]
        return _reference(z, np.asarray(seq[n_ctx:]), TAU[request.param])

    yield m, request.param, audios, oracle
    m.close()


def _sequence(m, text, prompt=None):
    from whisper.score import context_tokens
    from whisper.tokenizer import get_tokenizer
    tok = get_tokenizer(m.is_multilingual, num_languages=m.num_languages, language="en", task="transcribe")
    head = context_tokens(tok, prompt, m.dims.n_text_ctx)
    return [*head, *text, tok.eot], len(head)


def _check(m, dtype, res, file, texts, oracle, prompt=None, what=""):
    worst = 0.0
    for c, text in zip(res["candidates"], texts):
        seq, n_ctx = _sequence(m, text, prompt)
        want_lp, _, want_tlp, bar, _ = oracle(file, seq, n_ctx)
        got = np.asarray(c["token_logprobs"] + [c["eot_logprob"]])
        assert c["tokens"] == list(text) and len(got) == len(text) + 1 == len(c["top_tokens"])
        worst = max(worst, (np.abs(got - want_lp) / bar).max(), (np.abs(c["top_logprobs"] - want_tlp) / bar).max())
        total = 0.0
        for x in got:
            total += float(x)
        assert c["sum_logprob"] == total and c["avg_logprob"] == total / (len(text) + 1)
    avg = [c["avg_logprob"] for c in res["candidates"]]
    assert res["best"] == avg.index(max(avg))
    record_margin("score_oracle", dtype=dtype, what=what, file=file, share_of_bar=float(worst))
    print(f"{what} {dtype} file {file}: worst share of the bar {worst:.3g}")
    assert worst <= 1.0


def test_score_matches_oracle(micro):
    """Three candidates of different lengths share one encoder slot; two recordings go through
    score_batch, one with a prompt; score() of each file stays within the bar as well."""
    import whisper
    m, dtype, audios, oracle = micro
    rng = np.random.default_rng(41)
    cands = [[[int(t) for t in rng.integers(0, 50000, n)] for n in (5, 12, 1)],
             [[int(t) for t in rng.integers(0, 50000, n)] for n in (9, 3)]]
    prompts = [None, "a prompt of a few words"]
    batch = whisper.score_batch(m, audios, cands, language="en", initial_prompt=prompts)
    for i in range(2):
        _check(m, dtype, batch[i], i, cands[i], oracle, prompts[i], "score_batch")
        lone = whisper.score(m, audios[i], cands[i], language="en", initial_prompt=prompts[i])
        _check(m, dtype, lone, i, cands[i], oracle, prompts[i], "score")
    text = whisper.score(m, audios[0], ["the quick brown fox", "the quick brown box"], language="en")
    assert [c["text"] for c in text["candidates"]] == ["the quick brown fox", "the quick brown box"]
    from whisper.tokenizer import get_tokenizer
    tok = get_tokenizer(m.is_multilingual, num_languages=m.num_languages, language="en", task="transcribe")
    assert text["candidates"][1]["tokens"] == tok.encode(" the quick brown box")


BAD = [  # (what, keyword of the wh_score_batch call to change, value, the field the error names)
    ("n_seq", "n_seq", 0, "n_seq"), ("slot", "slots", [2], r"slots\[0\]"), ("short", "tokens", [[50258]], r"n_tokens\[0\]"),
    ("long", "tokens", [[50258] * 449], r"n_tokens\[0\]"), ("ctx0", "n_ctx", [0], r"n_ctx\[0\]"),
    ("ctx_all", "n_ctx", [6], r"n_ctx\[0\]"), ("id", "tokens", [[50258, 50259, 50359, 50363, 51865, 50257]], r"tokens\[4\]"),
    ("null", "null", 3, "n_tokens"), ("target", "target", 51865, r"targets\[1\]"), ("rows", "rows", 4097, "n_rows"),
    ("audio", "audio", 31.0, "audio 0"), ("sequence", "sequence", 445, "candidate 1 of audio 0"),
    ("finalize", "finalize", None, "not finalized"),
]


@pytest.mark.parametrize("what,field,value,names", BAD, ids=[b[0] for b in BAD])
def test_refusals(micro, what, field, value, names):
    """Every refusal names its field and leaves a following valid call's results unchanged."""
    import whisper
    from whisper import HipBackendError
    from whisper import synthetic as S
    from whisper.backend_hip import _ptr
    m, _, audios, _ = micro
    good = whisper.score(m, audios[1], [[11, 12, 13]], language="en")
    x = np.ones((2, 128), np.float32)
    if field == "audio":
        with pytest.raises(ValueError, match=names):
            whisper.score(m, S.synthetic_audio(value, seed=1), [[11]], language="en")
    elif field == "sequence":
        with pytest.raises(ValueError, match=names):
            whisper.score(m, audios[1], [[11], [11] * value], language="en")
    elif field == "target":
        with pytest.raises(HipBackendError, match=names):
            m.ctx.vocab_score(x, [0, value])
    elif field == "rows":
        with pytest.raises(HipBackendError, match=names):
            m.ctx.vocab_score(np.ones((value, 128), np.float32), np.zeros(value, np.int32))
    elif field == "null":
        z, f = np.zeros(8, np.int32), np.zeros(8, np.float32)
        assert m.ctx.lib.wh_score_batch(m.ctx.h, 1, _ptr(z), _ptr(z), None, _ptr(z), _ptr(f), _ptr(z), _ptr(f)) < 0
        assert names in m.ctx.lib.wh_last_error().decode()
    elif field == "finalize":
        raw = whisper.Whisper(m.dims, "micro", device=0, dtype="fp32", max_windows=1, max_group=1)
        try:
            with pytest.raises(HipBackendError, match=names):
                raw.ctx.score_batch([0], [[50258, 11]], [1])
            with pytest.raises(HipBackendError, match=names):
                raw.ctx.vocab_score(x[:1], [0])
        finally:
            raw.close()
    else:
        kw = dict(slots=[0], tokens=[[50258, 50259, 50359, 50363, 11, 50257]], n_ctx=[4])
        if field != "n_seq":
            kw[field] = value
        with pytest.raises(HipBackendError, match=names):
            if field == "n_seq":
                z = np.zeros(8, np.int32)
                m.ctx._check(m.ctx.lib.wh_score_batch(m.ctx.h, value, *[_ptr(z)] * 4, _ptr(np.zeros(8, np.float32)), _ptr(z),
                                                      _ptr(np.zeros(8, np.float32))), "wh_score_batch")
            else:
                m.ctx.score_batch(kw["slots"], kw["tokens"], kw["n_ctx"])
    assert whisper.score(m, audios[1], [[11, 12, 13]], language="en") == good
