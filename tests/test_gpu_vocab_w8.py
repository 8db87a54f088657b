"""vocab="fp8": the single-window step's logits over an 8-bit (E4M3) copy of the token embedding
(k_vocab1_w8).  Seeded synthetic weights cut to 1 audio and 2 text layers, embedding row ZERO
zeroed.  The reference is the fp32 CPU oracle whose logits use the DEVICE's code * scale while its
token lookup keeps the original embedding: it gets 2V embedding rows, the original on top and the
dequantised copy below, and the last V logit columns count.  The bar is the fp16 bar, unchanged."""
import copy
import functools

import numpy as np
import pytest

from conftest import record_margin
from test_gpu_batch import TAU, _teacher_force, check_whole_rows, whole_row_passes
from test_gpu_decoder_w8 import MODEL_OF, N_STEPS, PARTS, SEEDS, _drive, _e4m3, _encode, _loop, _mel
from test_gpu_widths import NONDECISIVE_CAP, TOPK, nondecisive

gpu = pytest.mark.gpu
EMB = "decoder.token_embedding.weight"
ZERO = 51000     # a timestamp token: never teacher-forced (tokens < eot), never in the sot sequence
V_OF = {w: (51866 if w == 1280 else 51865) for w in MODEL_OF}


@functools.lru_cache(maxsize=1)
def _oracle(width, V):
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = dict(S.MODEL_DIMS[MODEL_OF[width]], n_audio_layer=1, n_text_layer=2, n_vocab=V)
    sd = S.synthetic_state_dict(dims, 0)
    sd[EMB][ZERO] = 0
    st = R.SpecialTokens.for_model(dims)
    return dims, sd, R.OracleWhisper(dims, sd), list(st.sot_sequence), st.eot


_CTX = {}


def _model(width, V=None, vocab="fp8", decoder=None, dtype="fp16", **over):
    import whisper
    from whisper import synthetic as S
    V = V or V_OF[width]
    key = (width, V, vocab, decoder, dtype, tuple(over))
    if key not in _CTX:
        for k in [k for k in _CTX if k[:2] != (width, V)]:
            _CTX.pop(k).close()
        dims, sd = _oracle(width, V)[:2]
        if over:
            dims, sd = dict(dims, **over), S.synthetic_state_dict(dict(dims, **over), 0)
        m = whisper.Whisper(whisper.ModelDimensions(**dims), MODEL_OF[width], device=0, dtype=dtype, max_windows=2,
                            max_group=8, vocab=vocab, decoder=decoder)
        m.load_state_dict(sd)
        _CTX[key] = m
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k in list(_CTX):
        _CTX.pop(k).close()


@gpu
@pytest.mark.parametrize("width", [384, 1280])
def test_quantiser_format(width):
    """test_gpu_decoder_w8's format checks (its derived bound) and the zero row; the codes come
    back in logical order, so the host un-permutes the kernel's tile-major layout."""
    m, sd = _model(width), _oracle(width, V_OF[width])[1]
    w = sd[EMB].astype(np.float16).astype(np.float32)
    codes, scale = m.ctx.vocab_w8()
    want = (np.abs(w).max(axis=-1) / np.float32(448)).astype(np.float32)
    live = want > 0
    assert (np.abs(scale - want)[live] / np.spacing(want[live])).max() <= 2
    assert not live[ZERO] and scale[ZERO] == 0 and not codes[ZERO].any() and live.sum() == len(w) - 1
    assert not np.isin(codes, (0x7F, 0xFF)).any()
    err = np.abs(_e4m3(codes) * scale[:, None] - w)
    bound = np.maximum(np.abs(w) * 2.0 ** -4, scale[:, None] * 2.0 ** -10) * (1 + 1e-5)
    print(f"{width}: worst err / bound {float((err[live] / bound[live]).max()):.3f}")
    assert (err <= bound).all()


@functools.lru_cache(maxsize=1)
def _oracle8(width, V, decoder):
    """The oracle with the device's code * scale under its embedding (and as its decoder linears)."""
    import torch
    dims, _, om = _oracle(width, V)[:3]
    ctx = _model(width, V, decoder=decoder).ctx
    om8 = copy.copy(om)
    om8.sd = dict(om.sd)
    codes, scale = ctx.vocab_w8()
    om8.sd[EMB] = torch.cat([om.sd[EMB], torch.from_numpy(_e4m3(codes) * scale[:, None])])
    for layer in range(dims["n_text_layer"] if decoder else 0):
        for which, (names, _) in enumerate(PARTS):
            codes, scale = ctx.decoder_w8(layer, which)
            parts = torch.from_numpy(_e4m3(codes) * scale[:, None]).chunk(len(names))
            om8.sd.update({f"decoder.blocks.{layer}.{k}": p for k, p in zip(names, parts)})
    return om8


@functools.lru_cache(maxsize=2)
def _cross_kv(width, V, seed):
    import torch
    dims, _, om = _oracle(width, V)[:3]
    om.set_audio(om.encode(torch.from_numpy(_mel(seed, dims["n_mels"]))))
    return om.cross_k, om.cross_v


def _reference(width, V, decoder, seed, group):
    """One window: the first pass over the oracle's own weights, the steps' logits over om8's."""
    import torch
    _, _, om, sot, eot = _oracle(width, V)
    om8 = _oracle8(width, V, decoder)
    om.cross_k, om.cross_v = om8.cross_k, om8.cross_v = _cross_kv(width, V, seed)
    rng = np.random.default_rng([34, seed, group])
    lg, cache, _ = om.decoder_forward(torch.tensor([sot] * group), 0, None)
    tok, topv, topi, full = [np.full(group, sot[-1])], [], [], {}
    for s in range(N_STEPS + 1):
        v, i = torch.topk(lg[:, -1, -V:], TOPK)
        topv.append(v.numpy()), topi.append(i.numpy())
        if s in whole_row_passes(N_STEPS + 1):
            full[s] = lg[:, -1, -V:].numpy().copy()
        if s == N_STEPS:
            break
        tok.append(rng.integers(0, eot, group))
        lg, cache, _ = om8.decoder_forward(torch.from_numpy(tok[-1])[:, None], len(sot) + s, cache)
    return dict(tok=np.stack(tok), topv=np.stack(topv), topi=np.stack(topi), src=None, full=full)


# every width at 1, 5, 8 rows; at 384 a last tile of 8, 9, 10 columns (whole stores, scalar tails); one over decoder="fp8"
CASES = [(w, None, g, None) for w in sorted(MODEL_OF) for g in (1, 5, 8)] + \
        [(384, 51864, 8, None), (384, 51866, 5, None), (512, None, 5, "fp8")]


@gpu
@pytest.mark.parametrize("width,V,group,decoder", CASES)
def test_teacher_forced_step_logits(width, V, group, decoder):
    V = V or V_OF[width]
    m = _model(width, V, decoder=decoder)
    kern = m.ctx.step_kernels(1, group)
    assert kern["tail"] == "vocab<w8>+k_logit_part" and kern["proj"] == ("k_proj1<w8>" if decoder else "k_proj1"), kern
    trajs = [_reference(width, V, decoder, seed, group) for seed in SEEDS]
    skipped = nondecisive(trajs, TAU["fp16"])
    res = []
    for seed, t in zip(SEEDS, trajs):
        _encode(m, [seed])
        res.append(_teacher_force(m, [t], _oracle(width, V)[3], whole=True))
    rel, top1, rel_all, col_all = (np.stack(x) for x in zip(*res))
    print(f"{width} V {V} vocab w8 1 x {group} decoder {decoder}: max rel err {rel.max():.3e} "
          f"({rel.max() / TAU['fp16']:.3f} TAU), top-1 agreement {top1.mean():.4f}, non-decisive {skipped:.4f}; {kern}")
    record_margin("vocab_w8_teacher_forced", width=width, n_vocab=V, rows=group, decoder=decoder, worst_rel=float(rel.max()),
                  frac_of_tau=float(rel.max() / TAU["fp16"]), tau=TAU["fp16"], top1_agreement=float(top1.mean()),
                  nondecisive=skipped, tail=kern["tail"])
    assert skipped <= NONDECISIVE_CAP, f"the top-1 check would skip {skipped:.3f} of the (step, row) pairs"
    assert rel.max() <= TAU["fp16"], f"max rel err {rel.max():.3e} > {TAU['fp16']}"
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"
    # (seed, pass, row): every column, the ragged last tile included, of the first pass, steps 1, 2 and the last
    assert kern["vocab"] == "k_vocab1_w8", kern
    check_whole_rows("vocab_w8_teacher_forced", rel, rel_all, col_all, "fp16", kern["vocab"], width=width, n_vocab=V,
                     rows=group, decoder=decoder)


@gpu
def test_other_paths_bit_equal_to_native():
    """Two-window steps, the first pass and scoring read the fp16 embedding; set back: the native step."""
    sot = _oracle(512, 51865)[3]
    m8, mn = _model(512), _model(512, vocab="native")
    assert m8.ctx.step_kernels(2, 5)["tail"] == mn.ctx.step_kernels(1, 5)["tail"] == "vocab+k_logit_part"
    cand = sot + [400, 500, 600]
    got = [(_drive(m, 2, 5), m.ctx.prefill_logits(1, sot)[0], m.ctx.score_batch([0], [cand], [len(sot)])) for m in (m8, mn)]
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert all(np.array_equal(a, b) for a, b in zip(got[0][2][0], got[1][2][0]))
    single = _drive(mn, 1, 5)
    assert not np.array_equal(_drive(m8, 1, 5), single)     # the 8-bit embedding is what the step read
    m8.ctx.set_vocab_format("native")
    try:
        assert np.array_equal(_drive(m8, 1, 5), single)
    finally:
        m8.ctx.set_vocab_format("fp8")


@gpu
def test_format_change_between_graph_decodes():
    """Device loop: a format set while a batch is in flight serves the next batch, both directions."""
    m8, mn = _model(512), _model(512, vocab="native")
    want8, wantn = _loop(m8), _loop(mn)
    assert not np.array_equal(want8[1], wantn[1])
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    try:
        assert same(_loop(m8, lambda: m8.ctx.set_vocab_format("native")), want8)   # in flight: still fp8
        assert same(_loop(m8), wantn)                                              # the next batch: native
        assert same(_loop(m8, lambda: m8.ctx.set_vocab_format("fp8")), wantn)
        assert same(_loop(m8), want8)
    finally:
        m8.ctx.set_vocab_format("fp8")


@gpu
def test_refusals():
    from whisper.backend_hip import WH_VOCAB_NATIVE, HipBackendError
    m = _model(512, vocab="native", dtype="fp32")
    with pytest.raises(HipBackendError, match="fp16 context"):
        m.ctx.set_vocab_format("fp8")
    m = _model(512, vocab="native")
    with pytest.raises(HipBackendError, match="unknown format"):
        m.ctx.set_vocab_format(7)
    with pytest.raises(HipBackendError, match="WH_VOCAB_NATIVE"):
        m.ctx.vocab_w8()
    m.ctx.set_vocab_format(WH_VOCAB_NATIVE)    # the format it has: fine
    assert m.ctx.step_kernels(1, 5)["tail"] == "vocab+k_logit_part" and _drive(m, 1, 5).shape[0] == 4
    odd = _model(512, vocab="native", n_audio_state=256, n_audio_head=4, n_text_state=256, n_text_head=4)
    with pytest.raises(HipBackendError, match="n_text_state"):
        odd.ctx.set_vocab_format("fp8")
    assert odd.ctx.vocab_format == "native" and _drive(odd, 1, 5).shape[0] == 4
