"""decoder="fp8": the single-window decoder step over 8-bit (E4M3) copies of the decoder weights.

Seeded synthetic weights (seed 0), every model cut to 1 audio layer and 2 text layers (the
pending deferred residual crosses a layer boundary), at the five model widths.  The step's
reference is the CPU oracle in fp32 whose six decoder linears per layer are, for the step
calls, the DEVICE's code * scale (decoder_w8): what the device computes with; the first pass
runs over the model's own weights, as on the device.  The bar is the project's fp16 bar,
unchanged.  On random weights; accuracy on real speech is unmeasured (off by default).
"""
import copy
import functools

import numpy as np
import pytest

from conftest import record_margin
from test_gpu_batch import TAU, _teacher_force, check_whole_rows, whole_row_passes
from test_gpu_widths import NONDECISIVE_CAP, TOPK, nondecisive

gpu = pytest.mark.gpu
SEEDS = (3, 4)
N_STEPS = 16
MODEL_OF = {384: "tiny", 512: "base", 768: "small", 1024: "medium", 1280: "turbo"}
# which -> the oracle's weights it holds, each `rows` rows of n
PARTS = [(("attn.query.weight", "attn.key.weight", "attn.value.weight"), 1), (("attn.out.weight",), 1),
         (("cross_attn.query.weight",), 1), (("cross_attn.out.weight",), 1), (("mlp.0.weight",), 4), (("mlp.2.weight",), 1)]


def _dims(width, **over):
    from whisper import synthetic as S
    return dict(S.MODEL_DIMS[MODEL_OF[width]], n_audio_layer=1, n_text_layer=2, **over)


@functools.lru_cache(maxsize=None)
def _mel(seed, n_mels):
    import whisper
    from whisper import synthetic as S
    mel = whisper.log_mel_spectrogram(S.synthetic_audio(30.0, seed=seed), n_mels, padding=whisper.audio.N_SAMPLES)
    return whisper.pad_or_trim(mel[:, :3000], 3000)


@functools.lru_cache(maxsize=1)
def _oracle(width):
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = _dims(width)
    sd = S.synthetic_state_dict(dims, 0)
    st = R.SpecialTokens.for_model(dims)
    return dims, sd, R.OracleWhisper(dims, sd), list(st.sot_sequence), st.eot


_CTX = {}


def _model(width, decoder="fp8", dtype="fp16", **over):
    import whisper
    from whisper import synthetic as S
    key = (width, decoder, dtype, tuple(over))
    if key not in _CTX:
        for k in [k for k in _CTX if k[0] != width]:
            _CTX.pop(k).close()
        dims = _dims(width, **over)
        sd = S.synthetic_state_dict(dims, 0) if over else _oracle(width)[1]
        m = whisper.Whisper(whisper.ModelDimensions(**dims), MODEL_OF[width], device=0, dtype=dtype, max_windows=2,
                            max_group=8, decoder=decoder)
        m.load_state_dict(sd)
        _CTX[key] = m
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k in list(_CTX):
        _CTX.pop(k).close()
    _reference.cache_clear()      # the kept whole rows


def _encode(m, seeds):
    m.ctx.mel_write(np.concatenate([_mel(s, m.dims.n_mels) for s in seeds], axis=1))
    m.ctx.encode([3000 * w for w in range(len(seeds))], [3000] * len(seeds))


def _e4m3(codes):
    import torch
    return torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()


def _fp16_weight(sd, layer, which):
    """The fp16 weight the device quantised: the checkpoint's rows, the query's 64^-0.5 folded in."""
    names, _ = PARTS[which]
    w = [sd[f"decoder.blocks.{layer}.{k}"] * np.float32(0.125 if "query" in k else 1) for k in names]
    return np.concatenate(w).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------ 1. the quantiser
@gpu
@pytest.mark.parametrize("width", [384, 1280])
def test_quantiser_format(width):
    """Scales = amax / 448 (2 fp32 ulps), no NaN code, |code * scale - w| within half an E4M3
    step of w (2^-4 |w| in a normal binade, scale * 2^-10 below 2^-6): derived, not measured."""
    m, sd = _model(width), _oracle(width)[1]
    for layer, which in ((0, 0), (0, 4), (1, 2), (1, 5)):
        w = _fp16_weight(sd, layer, which)
        codes, scale = m.ctx.decoder_w8(layer, which)
        want = (np.abs(w).max(axis=-1) / np.float32(448)).astype(np.float32)
        ulps = np.abs(scale - want) / np.spacing(want)
        assert ulps.max() <= 2, (layer, which, float(ulps.max()))
        assert not np.isin(codes, (0x7F, 0xFF)).any(), (layer, which)
        err = np.abs(_e4m3(codes) * scale[:, None] - w)
        bound = np.maximum(np.abs(w) * 2.0 ** -4, scale[:, None] * 2.0 ** -10) * (1 + 1e-5)
        print(f"{width} layer {layer} which {which}: worst err / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (layer, which)


# ------------------------------------------------------------------ 2. the step against the oracle
@functools.lru_cache(maxsize=1)
def _oracle8(width):
    """The oracle with the device's code * scale as its six decoder linears per layer."""
    import torch
    dims, _, om = _oracle(width)[:3]
    om8 = copy.copy(om)
    om8.sd = dict(om.sd)
    for layer in range(dims["n_text_layer"]):
        for which, (names, _) in enumerate(PARTS):
            codes, scale = _model(width).ctx.decoder_w8(layer, which)
            parts = torch.from_numpy(_e4m3(codes) * scale[:, None]).chunk(len(names))
            om8.sd.update({f"decoder.blocks.{layer}.{k}": w for k, w in zip(names, parts)})
    return om8


@functools.lru_cache(maxsize=2)
def _cross_kv(width, seed):
    import torch
    dims, _, om = _oracle(width)[:3]
    om.set_audio(om.encode(torch.from_numpy(_mel(seed, dims["n_mels"]))))
    return om.cross_k, om.cross_v


@functools.lru_cache(maxsize=None)
def _reference(width, seed, group):
    """The oracle's trajectory of one window: the first pass over its own weights, the steps
    over the device's dequantised decoder linears."""
    import torch
    _, _, om, sot, eot = _oracle(width)
    om8 = _oracle8(width)
    om.cross_k, om.cross_v = om8.cross_k, om8.cross_v = _cross_kv(width, seed)
    rng = np.random.default_rng([32, seed, group])
    lg, cache, _ = om.decoder_forward(torch.tensor([sot] * group), 0, None)
    tok, topv, topi, full = [np.full(group, sot[-1])], [], [], {}
    for s in range(N_STEPS + 1):
        v, i = torch.topk(lg[:, -1], TOPK)
        topv.append(v.numpy()), topi.append(i.numpy())
        if s in whole_row_passes(N_STEPS + 1):
            full[s] = lg[:, -1].numpy().copy()
        if s == N_STEPS:
            break
        tok.append(rng.integers(0, eot, group))
        lg, cache, _ = om8.decoder_forward(torch.from_numpy(tok[-1])[:, None], len(sot) + s, cache)
    return dict(tok=np.stack(tok), topv=np.stack(topv), topi=np.stack(topi), src=None, full=full)


@gpu
@pytest.mark.parametrize("group", [1, 5, 8])
@pytest.mark.parametrize("width", sorted(MODEL_OF))
def test_teacher_forced_step_logits(width, group):
    """Every p1_width_launch row (1280: the 32-column fc1) at 1, 5 and P1_RMAX = 8 rows; layer
    1's QKV prologue adds layer 0's deferred fc2 residual."""
    m = _model(width)
    kern = m.ctx.step_kernels(1, group)
    assert kern["proj"] == "k_proj1<w8>", kern
    trajs = [_reference(width, seed, group) for seed in SEEDS]
    skipped = nondecisive(trajs, TAU["fp16"])
    res = []
    for seed, t in zip(SEEDS, trajs):
        _encode(m, [seed])
        res.append(_teacher_force(m, [t], _oracle(width)[3], whole=True))
    rel, top1, rel_all, col_all = (np.stack(x) for x in zip(*res))
    print(f"{width} w8 1 x {group}: max rel err {rel.max():.3e} ({rel.max() / TAU['fp16']:.3f} TAU), top-1 agreement "
          f"{top1.mean():.4f}, non-decisive {skipped:.4f}; {kern}")
    record_margin("decoder_w8_teacher_forced", width=width, rows=group, worst_rel=float(rel.max()),
                  frac_of_tau=float(rel.max() / TAU["fp16"]), tau=TAU["fp16"], top1_agreement=float(top1.mean()),
                  nondecisive=skipped, proj=kern["proj"])
    assert skipped <= NONDECISIVE_CAP, f"the top-1 check would skip {skipped:.3f} of the (step, row) pairs"
    assert rel.max() <= TAU["fp16"], f"max rel err {rel.max():.3e} > {TAU['fp16']}"
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"
    # (seed, pass, row): every column of the first pass, steps 1, 2 and the last, the same bar
    check_whole_rows("decoder_w8_teacher_forced", rel, rel_all, col_all, "fp16", kern["vocab"], width=width, rows=group)


# ------------------------------------------------------------------ 3. nothing else moved
def _drive(m, n_win, group, steps=4):
    sot, eot = _oracle(512)[3:]
    _encode(m, [SEEDS[w % 2] for w in range(n_win)])
    m.ctx.prefill([sot] * n_win, group, [0] * n_win)
    rng = np.random.default_rng(33)
    return np.stack([m.ctx.step(rng.integers(0, eot, n_win * group), text_offsets=[len(sot) + s] * n_win)
                     for s in range(steps)])


@gpu
def test_other_paths_bit_equal_to_native():
    """Steps of two windows, the first pass and scoring read the fp16 weights; set back to
    native, the single-window step is the native one."""
    sot = _oracle(512)[3]
    m8, mn = _model(512), _model(512, "native")
    assert m8.ctx.step_kernels(2, 5)["proj"] == "k_proj" and mn.ctx.step_kernels(1, 5)["proj"] == "k_proj1"
    cand = sot + [400, 500, 600]
    got = [(_drive(m, 2, 5), m.ctx.prefill_logits(1, sot)[0], m.ctx.score_batch([0], [cand], [len(sot)])) for m in (m8, mn)]
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
    for a, b in zip(got[0][2][0], got[1][2][0]):
        assert np.array_equal(a, b)
    single = _drive(mn, 1, 5)
    assert not np.array_equal(_drive(m8, 1, 5), single)     # the 8-bit weights are what the step read
    m8.ctx.set_decoder_format("native")
    try:
        assert m8.ctx.step_kernels(1, 5)["proj"] == "k_proj1"
        assert np.array_equal(_drive(m8, 1, 5), single)
    finally:
        m8.ctx.set_decoder_format("fp8")
    assert m8.ctx.step_kernels(1, 5)["proj"] == "k_proj1<w8>"


# ------------------------------------------------------------------ 4. refusals
@gpu
def test_refusals():
    from whisper.backend_hip import WH_DEC_NATIVE, HipBackendError
    with pytest.raises(ValueError, match="fp8.*fp32|fp32.*fp8"):
        _model(512, "fp8", "fp32")
    m = _model(512, "native", "fp32")
    with pytest.raises(HipBackendError, match="fp16 context"):
        m.ctx.set_decoder_format("fp8")
    m = _model(512, "native")
    with pytest.raises(HipBackendError, match="unknown format"):
        m.ctx.set_decoder_format(7)
    with pytest.raises(HipBackendError, match="WH_DEC_NATIVE"):
        m.ctx.decoder_w8(0, 0)
    m.ctx.set_decoder_format(WH_DEC_NATIVE)    # the format it has: fine
    assert m.ctx.step_kernels(1, 5)["proj"] == "k_proj1" and _drive(m, 1, 5).shape[0] == 4
    odd = _model(512, "native", n_audio_state=256, n_audio_head=4, n_text_state=256, n_text_head=4)
    with pytest.raises(HipBackendError, match="n_text_state"):
        odd.ctx.set_decoder_format("fp8")
    assert odd.ctx.step_kernels(1, 5)["proj"] == "k_proj"


# ------------------------------------------------------------------ 5. the captured step graph
def _loop(m, before=None, steps=6):
    """A one-window beam-5 decode through the device loop (the captured step graph): its rows'
    tokens and sum_logprobs.  `before`: called between the first two steps and the rest."""
    import whisper
    from whisper.decoding import DecodingTask
    task = DecodingTask(m, whisper.DecodingOptions(language="en", beam_size=5))
    _encode(m, [SEEDS[0]])
    m.ctx.decode_begin(task.wh_opts(), [task.initial_tokens], [task.sot_index])
    m.ctx.decode_steps(2)
    if before:
        before()
    m.ctx.decode_steps(steps - 2)
    r = m.ctx.decode_read(0, 5)
    return r["tokens"].copy(), r["sum_logprobs"].copy()


@gpu
def test_format_change_between_graph_decodes():
    """A format set while a batch is in flight leaves that batch (and its graph) alone and
    serves the next one, whose options and group, hence graph key, are the same."""
    m8, mn = _model(512), _model(512, "native")
    want8, wantn = _loop(m8), _loop(mn)
    assert not np.array_equal(want8[1], wantn[1])
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    try:
        assert same(_loop(m8, lambda: m8.ctx.set_decoder_format("native")), want8)   # in flight: still fp8
        assert same(_loop(m8), wantn)                                                # the next batch: native
        assert same(_loop(m8, lambda: m8.ctx.set_decoder_format("fp8")), wantn)
        assert same(_loop(m8), want8)
    finally:
        m8.ctx.set_decoder_format("fp8")
