"""encoder="fp8": the four GEMMs of every encoder block on the 8-bit (E4M3) matrix path.

Format (include/whisper_hip.h "Encoder formats"): x rounded to fp16, one fp32 scale per row,
scale = amax / 448, code = e4m3(clamp(x / scale, +-448)), zero rows scale 0 and codes 0.  The
GEMM is checked against float64 over the DEVICE's codes and scales, so only its accumulation and
the fp16 store are under test; the block against a float64 emulation with the same quantiser.
Seeded synthetic weights: nothing here says anything about real speech.
"""
import functools

import numpy as np
import pytest

from conftest import record_margin
from test_gpu_cross_kv8 import SEEDS, _dims, _mel

gpu = pytest.mark.gpu
_CTX = {}


def _model(model, encoder="fp8"):
    import whisper
    from whisper import synthetic as S
    if (model, encoder) not in _CTX:
        dims = _dims(model)
        m = whisper.Whisper(whisper.ModelDimensions(**dims), model, device=0, dtype="fp16", max_windows=3, max_group=5,
                            encoder=encoder)
        m.load_state_dict(S.synthetic_state_dict(dims, 0))
        _CTX[(model, encoder)] = m
    return _CTX[(model, encoder)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k in list(_CTX):
        _CTX.pop(k).close()


def _features(m, n_win):
    m.ctx.mel_write(np.concatenate([_mel(SEEDS[w % 2], m.dims.n_mels) for w in range(n_win)], axis=1))
    m.ctx.encode([3000 * w for w in range(n_win)], [3000] * n_win)
    return [m.ctx.audio_features(w) for w in range(n_win)]


def _quant(x):
    """The format rule on rows of x (float32 / float64): (codes as float32 values, scales)."""
    import torch
    h = torch.as_tensor(x).to(torch.float16).to(torch.float32)
    s = h.abs().amax(-1, keepdim=True) / np.float32(448)
    q = torch.where(s > 0, h / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(h)).clamp(-448, 448)
    return q.to(torch.float8_e4m3fn), s[..., 0]


def _e4m3(codes):
    import torch
    return torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float64)


# ------------------------------------------------------------------ 1. the quantisers, bit-exact
@gpu
def test_quantisers_bit_exact():
    import torch
    rng = np.random.default_rng(40)
    K = 256

    def rows(n):
        x = rng.standard_normal((n, K)).astype(np.float32) * np.exp2(rng.integers(-12, 12, (n, 1))).astype(np.float32)
        x[1] = 0.0                                                       # an all-zero row
        x[2] = rng.integers(-40, 41, K) * np.float32(2.0 ** -24)        # amax an fp16 subnormal
        x[3, ::7], x[3, 3::7] = 65504.0, -65504.0                        # the fp16 extremes
        return x
    x, w = rows(9), rows(64)
    _, xc, xs, wc, ws = _model("base3").ctx.fp8_linear(x, w, tile=128)
    for name, src, codes, scales in (("x", x, xc, xs), ("w", w, wc, ws)):
        q, s = _quant(src)
        assert np.array_equal(scales, s.numpy()), name
        assert np.array_equal(codes, q.view(torch.uint8).numpy()), name
        assert not np.isin(codes, (0x7F, 0xFF)).any() and not codes[1].any() and scales[1] == 0, name


# ------------------------------------------------------------------ 2. the GEMM against float64
TILES = {256: 128, 128: 64}   # tile selector -> its columns


@gpu
@pytest.mark.parametrize("mode", ["plain", "bias_gelu"])
@pytest.mark.parametrize("K", [128, 256, 384, 1280, 5120])
@pytest.mark.parametrize("ntiles", [1, 3])
@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1500])
def test_gemm8_against_float64(M, tile, ntiles, K, mode):
    """|y - ref| <= K 2^-23 sum_k |x^ w^| sa sw (fp32 accumulation in any order, the two scale
    and the bias roundings inside its slack) + half an fp16 ulp of the result; with GELU the
    pre-activation bound times its Lipschitz constant 1.13 plus 8 fp32 ulps of |pre| for the
    fp32 erf evaluation (0.5 x (1 + erf): a few-ulp erff and three roundings)."""
    import torch
    N = ntiles * TILES[tile]
    rng = np.random.default_rng([41, M, N, K])
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if mode == "bias_gelu" else None
    y, xc, xs, wc, ws = _model("base3").ctx.fp8_linear(x, w, bias, gelu=mode == "bias_gelu", tile=tile)
    xh, wh = _e4m3(xc), _e4m3(wc)
    sc = torch.from_numpy(xs).double()[:, None] * torch.from_numpy(ws).double()[None, :]
    ref = (xh @ wh.T) * sc
    tol = K * 2.0 ** -23 * (xh.abs() @ wh.abs().T) * sc
    if bias is not None:
        ref = ref + torch.from_numpy(bias).double()
        tol = 1.13 * tol + 8 * 2.0 ** -24 * ref.abs()
        ref = 0.5 * ref * (1 + torch.erf(ref / np.sqrt(2.0)))
    ref, tol = ref.numpy(), tol.numpy()
    tol = tol + 0.5 * np.spacing((np.abs(ref) + tol).astype(np.float16)).astype(np.float64)
    worst = float((np.abs(y - ref) / tol).max())
    print(f"M={M} N={N} K={K} tile={tile} {mode}: worst err / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 3. one encoder block
def _encode64(sd, dims, mel, quant):
    """The oracle's encoder arithmetic (oracle/ref_whisper.py encode) in float64, one block;
    quant: the format's quantiser on the four GEMM inputs and the four weights."""
    import torch
    import torch.nn.functional as F
    s = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items() if k.startswith("encoder.")}

    def deq(t):
        if not quant:
            return t
        q, sc = _quant(t)
        return q.to(torch.float64) * sc.double()[..., None]

    def lin(h, name, bias=True):
        return F.linear(deq(h), deq(s[name + ".weight"]), s[name + ".bias"] if bias else None)
    x = F.gelu(F.conv1d(torch.from_numpy(mel).double()[None], s["encoder.conv1.weight"], s["encoder.conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(x, s["encoder.conv2.weight"], s["encoder.conv2.bias"], stride=2, padding=1))
    x = x.permute(0, 2, 1) + s["encoder.positional_embedding"]
    n, H, p = x.shape[-1], dims["n_audio_head"], "encoder.blocks.0."
    ln = lambda t, name: F.layer_norm(t, (n,), s[name + ".weight"], s[name + ".bias"], 1e-7)
    h = ln(x, p + "attn_ln")
    q, k, v = lin(h, p + "attn.query"), lin(h, p + "attn.key", False) * 64 ** -0.5, lin(h, p + "attn.value")
    heads = lambda t: t.view(1, 1500, H, 64).permute(0, 2, 1, 3)
    o = ((heads(q) @ heads(k).transpose(-1, -2)).softmax(-1) @ heads(v)).permute(0, 2, 1, 3).reshape(1, 1500, n)
    x = x + lin(o, p + "attn.out")
    x = x + lin(F.gelu(lin(ln(x, p + "mlp_ln"), p + "mlp.0")), p + "mlp.2")
    return ln(x, "encoder.ln_post")[0].numpy()


@gpu
@pytest.mark.parametrize("model", ["base3", "turbo1"])
def test_encoder_block_against_emulation(model):
    """||dev - emul|| / ||emul|| <= 0.5 E_q, E_q = ||emul - unquantised|| / ||unquantised||:
    the device's fp16 LayerNorm / GELU values differ from float64 by ~2^-11, so ~2^-8 of the
    codes fall across a rounding boundary by one E4M3 step: rms 0.06 step against the
    quantisation's own 0.29 step, a ratio of ~0.2; 0.5 leaves a factor of two and stays far
    under the >= 1 of a wrong or missing scale."""
    from whisper import synthetic as S
    dims = _dims(model)
    sd = S.synthetic_state_dict(dims, 0)
    mel = _mel(SEEDS[0], dims["n_mels"])
    emul, plain = _encode64(sd, dims, mel, True), _encode64(sd, dims, mel, False)
    e_q = float(np.linalg.norm(emul - plain) / np.linalg.norm(plain))
    m = _model(model)
    assert m.ctx.encoder_kernels(1)["qkv"].startswith("k_gemm8"), m.ctx.encoder_kernels(1)
    dev = _features(m, 1)[0].reshape(emul.shape)
    rel = float(np.linalg.norm(dev - emul) / np.linalg.norm(emul))
    print(f"{model}: dev-emul {rel:.3e}, E_q {e_q:.3e}, ratio {rel / e_q:.3f}")
    record_margin("encoder_fp8_block", model=model, rel_dev_emul=rel, e_q=e_q, ratio=rel / e_q)
    assert rel <= 0.5 * e_q


# ------------------------------------------------------------------ 4. / 5. invariance, switching
@gpu
def test_batch_invariance():
    m = _model("turbo1")
    two, three = _features(m, 2), _features(m, 3)
    assert all(np.array_equal(a, b) for a, b in zip(two, three))
    assert not np.array_equal(two[0], two[1])


@gpu
def test_switching_back_is_bit_identical():
    from whisper.backend_hip import WH_ENC_FP8_E4M3, WH_ENC_NATIVE
    never, m = _features(_model("base3", "native"), 2), _model("base3")
    fp8 = _features(m, 2)
    m.ctx.set_encoder_format(WH_ENC_NATIVE)
    assert m.ctx.encoder_kernels(2)["encoder"] == "native"
    back = _features(m, 2)
    m.ctx.set_encoder_format(WH_ENC_FP8_E4M3)
    assert all(np.array_equal(a, b) for a, b in zip(never, back))
    assert not np.array_equal(fp8[0], never[0])
    assert all(np.array_equal(a, b) for a, b in zip(fp8, _features(m, 2)))


# ------------------------------------------------------------------ 6. recorded, not asserted
@gpu
@pytest.mark.parametrize("model", ["base3", "turbo1"])
def test_quantisation_effect_recorded(model):
    """2 windows x 5 beams, 16 teacher-forced steps of seeded tokens in an fp8-encoder and a
    native context: worst |logit difference| over the native top-32 as a share of its range."""
    from oracle import ref_whisper as R
    st = R.SpecialTokens.for_model(_dims(model))
    sot, lg = list(st.sot_sequence), {}
    for enc in ("fp8", "native"):
        m, rng = _model(model, enc), np.random.default_rng(42)
        _features(m, 2)
        m.ctx.prefill([sot] * 2, 5, [0] * 2)
        lg[enc] = [np.array(m.ctx.step([int(t) for t in rng.integers(0, st.eot, 10)], text_offsets=[len(sot) + s] * 2))
                   for s in range(16)]
    share = 0.0
    for a, b in zip(lg["fp8"], lg["native"]):
        top = np.argsort(b, axis=1)[:, -32:]
        ref = np.take_along_axis(b, top, 1)
        share = max(share, float((np.abs(np.take_along_axis(a, top, 1) - ref).max(1) / (ref.max(1) - ref.min(1))).max()))
    print(f"{model}: fp8 against native encoder, worst share of the top-32 range {share:.4e}")
    record_margin("encoder_fp8_quantisation_effect", model=model, windows=2, rows=10, steps=16, worst_share_of_range=share)
