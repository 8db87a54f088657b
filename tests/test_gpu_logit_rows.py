"""Every vocabulary column of the step logits, at every kernel of the vocabulary projection.

The parity tests score a step's logits at the reference's top-32 columns and by argmax: 32 of
51865 columns.  A vocabulary kernel that writes a wrong value, a stale one or nothing into any
other column, drops a 16-column tile at a workgroup boundary, gets the ragged last tile wrong or
reads a per-column scale of the wrong tile passes all of that, while the log-softmax and the
timestamp rule downstream read the whole row.  Here every column is held to the bar the top-32
already is: |logit - oracle| <= TAU[dtype] x (the row's top-32 range), every value finite
(test_gpu_batch.score_whole_row), at the first pass, steps 1 and 2 (two consecutive steps: an
unwritten column shows as the previous step's value) and the last of 8 steps.

Part 1, on the CPU: the old score is blind to six such corruptions of a micro-oracle row and the
whole-row score names the column of each.  Part 2, on the GPU: one case per instantiation of the six
kernels (csrc/wh_vocab_pick.h), each asserting step_kernels()["vocab"] first.  Models: the five
widths cut to 1 + 2 layers (test_gpu_decoder_w8._dims) and turbo1 (test_gpu_cross_kv8._dims), real
V, seeded weights, audio seeds 3 and 4, a seeded random trajectory with reorders.  The reference is
the fp32 CPU oracle; where an 8-bit option is set, the oracle computes the steps with the device's
code * scale, as test_gpu_vocab_w8 / test_gpu_decoder_w8 / test_gpu_cross_kv8 build it.
"""
import copy
import functools

import numpy as np
import pytest

import test_gpu_cross_kv8 as CK
import test_gpu_decoder_w8 as DW
from test_gpu_batch import TAU, _teacher_force, check_whole_rows, score_top32, score_whole_row, whole_row_passes
from test_gpu_widths import TOPK, _micro_oracle, random_trajectory

gpu = pytest.mark.gpu
SEEDS = (3, 4)
N_STEPS = 8
KEEP = whole_row_passes(N_STEPS + 1)
MAX_WINDOWS, MAX_GROUP = 14, 8
EMB = "decoder.token_embedding.weight"


# ------------------------------------------------------------------ 1. the scorer, on the CPU
@functools.lru_cache(maxsize=None)
def _micro_rows():
    om, _, st = _micro_oracle()
    t = random_trajectory(om, list(st.sot_sequence), 5, 4, np.random.default_rng(7), keep=range(5))
    return t


def _scores(dev, t, s):
    """(old top-32 share, old top-1, whole-row share, its column) per row of pass s."""
    out = [score_top32(dev[r], t["topv"][s, r], t["topi"][s, r], TAU["fp32"]) +
           score_whole_row(dev[r], t["full"][s][r], t["topv"][s, r]) for r in range(len(dev))]
    return [np.asarray(x) for x in zip(*out)]


def _corruptions(t, s, r):
    """name -> (corrupted copy of pass s's rows, the column the whole-row score must name): each
    outside row r's top 32, each below its maximum, each moving its column by more than the fp16 bar."""
    ref = t["full"][s]
    row, topv, top = ref[r], t["topv"][s, r], set(int(i) for i in t["topi"][s, r])
    V, bar = len(row), TAU["fp16"] * (topv[0] - topv[-1])
    assert row.max() == topv[0] > 0 > row.min() and bar > 0
    lo = int(np.argmin(row))                                   # the lowest logit: far from the median, negative
    tile = next(k for k in range(V // 16) if not top & set(range(16 * k, 16 * k + 16))
                and np.abs(row[16 * k:16 * k + 16]).max() > bar
                and np.abs(row[16 * k:16 * k + 16] - t["full"][s - 1][r, 16 * k:16 * k + 16]).max() > bar
                and t["full"][s - 1][r, 16 * k:16 * k + 16].max() < topv[0])
    cols = slice(16 * tile, 16 * tile + 16)
    assert lo not in top and V - 1 not in top and abs(row[V - 1] - row[V - 2]) > bar and row[V - 2] < topv[0]
    assert abs(row[lo] - np.median(row)) > bar and abs(row[lo]) > bar
    out = {}

    def put(name, col, change):
        dev = ref.copy()
        change(dev[r])
        out[name] = (dev, col)

    put("median", lo, lambda x: x.__setitem__(lo, np.median(row)))
    put("tile zeroed", 16 * tile + int(np.argmax(np.abs(row[cols]))), lambda x: x.__setitem__(cols, 0))
    put("last column", V - 1, lambda x: x.__setitem__(V - 1, row[V - 2]))
    prev = t["full"][s - 1][r, cols]
    put("stale tile", 16 * tile + int(np.argmax(np.abs(row[cols] - prev))), lambda x: x.__setitem__(cols, prev))
    put("scaled by 2", lo, lambda x: x.__setitem__(lo, 2 * row[lo]))
    put("NaN", lo, lambda x: x.__setitem__(lo, np.nan))
    return out


@pytest.mark.parametrize("s,r", [(2, 0), (4, 3)])
def test_whole_row_score_sees_what_top32_cannot(s, r):
    """The micro oracle's own rows stand for the device's.  Untouched, both scores pass.  Corrupted
    outside the top 32 and below the maximum, the old score (top-32 share + argmax, held to the
    tighter fp32 bar) passes all but the NaN; the whole-row score fails each at the looser fp16 bar,
    in the row and at the column that was changed, and leaves the other rows alone."""
    t = _micro_rows()
    rel, top1, rel_all, _ = _scores(t["full"][s].copy(), t, s)
    assert rel.max() == 0 and top1.all() and rel_all.max() == 0
    cases = _corruptions(t, s, r)
    assert list(cases) == ["median", "tile zeroed", "last column", "stale tile", "scaled by 2", "NaN"]
    for name, (dev, col) in cases.items():
        rel, top1, rel_all, col_all = _scores(dev, t, s)
        if name != "NaN":
            assert rel.max() <= TAU["fp32"] and top1.all(), f"{name}: the top-32 score was expected to miss it"
        assert rel_all[r] > TAU["fp16"] and int(col_all[r]) == col, (name, rel_all[r], int(col_all[r]), col)
        assert (np.delete(rel_all, r) == 0).all(), name
    assert np.isinf(_scores(cases["NaN"][0], t, s)[2][r])


def test_recorder_keeps_whole_rows_only_where_asked():
    """full = {} by default (every existing trajectory unchanged); kept rows carry the recorded top-32."""
    om, _, st = _micro_oracle()
    assert random_trajectory(om, list(st.sot_sequence), 2, 2, np.random.default_rng(7))["full"] == {}
    t = _micro_rows()
    assert sorted(t["full"]) == [0, 1, 2, 3, 4] and t["full"][3].shape == (5, om.n_vocab) and t["full"][3].dtype == np.float32
    for s in t["full"]:
        np.testing.assert_array_equal(np.take_along_axis(t["full"][s], t["topi"][s], axis=1), t["topv"][s])
    assert whole_row_passes(9) == {0, 1, 2, 8} and whole_row_passes(2) == {0, 1}


# ------------------------------------------------------------------ 2. the kernels, on the GPU
def _dims(model, V):
    d = CK._dims(model) if isinstance(model, str) else DW._dims(model)
    return dict(d, n_vocab=V) if V else d


def _name(model):
    return model if isinstance(model, str) else DW.MODEL_OF[model]


@functools.lru_cache(maxsize=1)
def _oracle(model, V):
    """One model's oracle: (dims, weights, OracleWhisper, sot, {seed: its cross K / V})."""
    import torch

    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = _dims(model, V)
    sd = S.synthetic_state_dict(dims, 0)
    om = R.OracleWhisper(dims, sd)
    ckv = {}
    for seed in SEEDS:
        om.set_audio(om.encode(torch.from_numpy(DW._mel(seed, dims["n_mels"]))))
        ckv[seed] = (om.cross_k, om.cross_v)
    return dims, sd, om, list(R.SpecialTokens.for_model(dims).sot_sequence), ckv


_CTX = {}


def _model(model, V, dtype, vocab=None, decoder=None, cross_kv=None):
    """One context alive at a time; the cases are listed so that neighbours share theirs."""
    import whisper
    key = (model, V, dtype, vocab, decoder, cross_kv)
    if key not in _CTX:
        for k in list(_CTX):
            _CTX.pop(k).close()
        dims, sd = _oracle(model, V)[:2]
        m = whisper.Whisper(whisper.ModelDimensions(**dims), _name(model), device=0, dtype=dtype, max_windows=MAX_WINDOWS,
                            max_group=MAX_GROUP, vocab=vocab, decoder=decoder, cross_kv=cross_kv)
        m.load_state_dict(sd)
        _CTX[key] = m
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k in list(_CTX):
        _CTX.pop(k).close()
    _reference.cache_clear()
    _oracle.cache_clear()
    _micro_rows.cache_clear()


def _trajectory(om, om_step, sot, group, V, rng):
    """A seeded random trajectory as test_gpu_widths.random_trajectory draws it (a reorder with
    repeats before every step at group > 1, tokens uniform over the vocabulary), the first pass
    over `om`, the steps over `om_step`, whose last V logit columns count."""
    import torch
    lg, cache, _ = om.decoder_forward(torch.tensor([sot] * group), 0, None)
    tok, topv, topi, src, full = [np.full(group, sot[-1])], [], [], [], {}
    for s in range(N_STEPS + 1):
        row = lg[:, -1, -V:]
        v, i = torch.topk(row, TOPK)
        topv.append(v.numpy()), topi.append(i.numpy())
        if s in KEEP:
            full[s] = row.numpy().copy()
        if s == N_STEPS:
            break
        if group > 1:
            src.append(rng.integers(0, group, group))
            cache = [[c[0][src[-1]], c[1][src[-1]]] for c in cache]
        tok.append(rng.integers(0, V, group))
        lg, cache, _ = om_step.decoder_forward(torch.from_numpy(tok[-1])[:, None], len(sot) + s, cache)
    return dict(tok=np.stack(tok), topv=np.stack(topv), topi=np.stack(topi), src=np.stack(src) if src else None, full=full)


@functools.lru_cache(maxsize=8)
def _reference(model, V, seed, group):
    """The native formats: the oracle's own weights throughout; shared by both dtypes and every batch."""
    dims, _, om, sot, ckv = _oracle(model, V)
    om.cross_k, om.cross_v = ckv[seed]
    return _trajectory(om, om, sot, group, dims["n_vocab"], np.random.default_rng([36, seed, group]))


def _reference8(m, model, V, seed, group, decoder, cross_kv):
    """vocab="fp8" (and the other two options): the first pass over the oracle's own weights, the
    steps over the device's code * scale: the embedding below the original one (2V rows: the
    token lookup keeps the original, the last V logit columns count), the decoder linears, and
    slot 0's cross K / V of the encode just done."""
    import torch
    dims, _, om, sot, ckv = _oracle(model, V)
    om8 = copy.copy(om)
    om8.sd = dict(om.sd)
    codes, scale = m.ctx.vocab_w8()
    om8.sd[EMB] = torch.cat([om.sd[EMB], torch.from_numpy(DW._e4m3(codes) * scale[:, None])])
    for layer in range(dims["n_text_layer"] if decoder else 0):
        for which, (names, _) in enumerate(DW.PARTS):
            codes, scale = m.ctx.decoder_w8(layer, which)
            parts = torch.from_numpy(DW._e4m3(codes) * scale[:, None]).chunk(len(names))
            om8.sd.update({f"decoder.blocks.{layer}.{k}": p for k, p in zip(names, parts)})
    om.cross_k, om.cross_v = om8.cross_k, om8.cross_v = ckv[seed]
    if cross_kv:
        n = dims["n_text_state"]
        as_rows = lambda x: torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(1, 1500, n))
        deq = [CK._dequant(m, 0, l) for l in range(dims["n_text_layer"])]
        om8.cross_k, om8.cross_v = [as_rows(k) for k, _ in deq], [as_rows(v) for _, v in deq]
    return _trajectory(om, om8, sot, group, dims["n_vocab"], np.random.default_rng([37, seed, group]))


def _encode(m, seeds):
    m.ctx.mel_write(np.concatenate([DW._mel(s, m.dims.n_mels) for s in seeds], axis=1))
    m.ctx.encode([3000 * w for w in range(len(seeds))], [3000] * len(seeds))


F8 = dict(vocab="fp8")
# (kernel, model, V, dtype, windows, rows per window, options), grouped by context; the row counts are the
# smallest that reach each instantiation (wh_vocab_pick.h; k_vocab_small / k_vocab_2p / k_gemv_x: one per
# count of 16-row tiles), none past 112 rows
CASES = (
    # k_vocab1_w8: every store form of the last tile (8, 9, 10 columns) at 384, both ends of the widths
    [("k_vocab1_w8", 384, 51864, "fp16", 1, 8, F8), ("k_vocab1_w8", 384, 51866, "fp16", 1, 5, F8)] +
    [("k_vocab1_w8", 384, None, "fp16", 1, g, F8) for g in (1, 5, 8)] +
    # k_vocab_small with the LayerNorm prologue (one window), then over plain rows
    [("k_vocab_small", 384, None, dt, 1, g, {}) for dt in ("fp16", "fp32") for g in (1, 8)] +
    [("k_vocab1_w8", 512, None, "fp16", 1, 5, dict(vocab="fp8", decoder="fp8", cross_kv="fp8"))] +
    [("k_vocab_small", 512, None, "fp16", 1, g, {}) for g in (1, 8)] +
    [("k_vocab_small", 512, None, "fp16", 2, 5, {}), ("k_vocab_small", 512, None, "fp16", 4, 8, {}),
     ("k_gemv_x", 512, None, "fp16", 7, 5, {}),
     ("k_vocab_small", 512, None, "fp32", 2, 8, {}), ("k_gemv_rows", 512, None, "fp32", 4, 5, {})] +
    [("k_vocab_small", w, None, "fp16", 1, g, {}) for w in (768, 1024) for g in (1, 8)] +
    [("k_vocab1_w8", 1280, None, "fp16", 1, g, F8) for g in (1, 5, 8)] +
    [("k_vocab1", 1280, None, "fp16", 1, g, {}) for g in (1, 5, 8)] +
    [("k_vocab_small", 1280, None, "fp16", 2, 5, {}), ("k_vocab_small", 1280, None, "fp16", 4, 8, {})] +
    [("k_vocab_small", 1280, None, "fp32", 1, g, {}) for g in (1, 8)] +
    [("k_vocab_small", 1280, None, "fp32", 2, 8, {}), ("k_gemv_rows", 1280, None, "fp32", 4, 5, {}),
     ("k_gemv_x", 1280, None, "fp32", 7, 5, {})] +
    # k_vocab_2p: MTV 3, 5 and 7 (the top edge, 112 rows)
    [("k_vocab_2p", "turbo1", None, "fp16", nw, g, {}) for nw, g in ((7, 5), (13, 5), (14, 8))])


def _id(c):
    return f"{c[0]}-{_name(c[1])}{'-V' + str(c[2]) if c[2] else ''}-{c[3]}-{c[4]}x{c[5]}" + "".join(f"-{k}8" for k in c[6])


@gpu
@pytest.mark.parametrize("kernel,model,V,dtype,n_win,group,opts", CASES, ids=[_id(c) for c in CASES])
def test_whole_rows(kernel, model, V, dtype, n_win, group, opts):
    m = _model(model, V, dtype, **opts)
    kern = m.ctx.step_kernels(n_win, group)
    assert kern["vocab"] == kernel, kern
    assert kern["tail"] == ("vocab<w8>+k_logit_part" if opts else "vocab+k_logit_part"), kern
    assert n_win * group <= 112
    sot = _oracle(model, V)[3]
    # one window: each audio seed in turn; more: the two seeds cycled over the windows
    batches = [[s] for s in SEEDS] if n_win == 1 else [[SEEDS[w % 2] for w in range(n_win)]]
    res = []
    for seeds in batches:
        _encode(m, seeds)
        if opts:
            trajs = [_reference8(m, model, V, seeds[0], group, opts.get("decoder"), opts.get("cross_kv"))]
        else:
            trajs = [_reference(model, V, s, group) for s in seeds]
        res.append(_teacher_force(m, trajs, sot, whole=True))
    rel, top1, rel_all, col_all = (np.stack(x) for x in zip(*res))
    check_whole_rows("logit_rows", rel, rel_all, col_all, dtype, kernel, model=_name(model), n_vocab=m.dims.n_vocab,
                     windows=n_win, rows=n_win * group, options="+".join(sorted(opts)))
    assert rel.max() <= TAU[dtype], f"top-32 max rel err {rel.max():.3e} > {TAU[dtype]}"
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"
