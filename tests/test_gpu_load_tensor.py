"""wh_load_tensor / wh_finalize at the raw ABI: every refusal by its code and text, and a load
that does not depend on the order the tensors arrive in.  Micro model, a fresh context per case.
"""
import numpy as np
import pytest

from test_gpu_cross_kv8 import _mel

gpu = pytest.mark.gpu
SOT = [50258, 50259, 50359]


def _dims():
    from whisper import synthetic as S
    return S.MODEL_DIMS["micro"]


# the tensors a micro checkpoint holds: 11 outside the blocks, 15 per encoder and 24 per decoder block
N_TENSORS = 5 + 2 * 15 + 2 + 2 + 2 * 24 + 2


@pytest.fixture
def ctx():
    from whisper.backend_hip import HipContext
    c = HipContext(_dims(), dtype="fp16", max_windows=1, max_group=1)
    yield c
    c.close()


def _refused(call, code, text):
    from whisper.backend_hip import HipBackendError
    with pytest.raises(HipBackendError) as e:
        call()
    assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)


@gpu
def test_wrong_rank_is_refused_by_name(ctx):
    _refused(lambda: ctx.load_tensor("encoder.conv1.bias", np.zeros((128, 1), np.float32)), -4,
             "encoder.conv1.bias: bad rank")
    _refused(lambda: ctx.load_tensor("decoder.blocks.1.attn.key.weight", np.zeros(128, np.float32)), -4,
             "decoder.blocks.1.attn.key.weight: bad rank")


@gpu
def test_wrong_dimension_is_refused(ctx):
    _refused(lambda: ctx.load_tensor("decoder.blocks.0.mlp.0.weight", np.zeros((128, 128), np.float32)), -4,
             "decoder.blocks.0.mlp.0.weight: bad shape")
    _refused(lambda: ctx.load_tensor("encoder.conv1.weight", np.zeros((128, 80, 2), np.float32)), -4,
             "encoder.conv1.weight: bad shape")
    _refused(lambda: ctx.load_tensor("decoder.token_embedding.weight", np.zeros((51864, 128), np.float32)), -4,
             "decoder.token_embedding.weight: bad shape")


@gpu
def test_unknown_block_tensor_is_refused(ctx):
    _refused(lambda: ctx.load_tensor("encoder.blocks.0.nope", np.zeros(128, np.float32)), -5,
             "unknown tensor encoder.blocks.0.nope")
    # the cross-attention exists in the decoder only
    _refused(lambda: ctx.load_tensor("encoder.blocks.0.cross_attn.out.bias", np.zeros(128, np.float32)), -5,
             "unknown tensor encoder.blocks.0.cross_attn.out.bias")


@gpu
def test_layer_out_of_range_is_refused(ctx):
    _refused(lambda: ctx.load_tensor("decoder.blocks.2.attn.out.bias", np.zeros(128, np.float32)), -5,
             "layer out of range decoder.blocks.2.attn.out.bias")


@gpu
def test_unknown_name_outside_the_blocks_is_refused(ctx):
    _refused(lambda: ctx.load_tensor("decoder.ln.gain", np.zeros(128, np.float32)), -5, "unknown tensor decoder.ln.gain")


@gpu
def test_finalize_counts_a_withheld_tensor(ctx):
    from whisper import synthetic as S
    sd = S.synthetic_state_dict(_dims(), 0)
    assert len(sd) == N_TENSORS
    for k, v in sd.items():
        if k != "decoder.blocks.1.cross_attn.value.bias":
            ctx.load_tensor(k, v)
    _refused(ctx.finalize, -6, f"loaded {N_TENSORS - 1} of {N_TENSORS} tensors")


@gpu
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_load_order_does_not_matter(dtype):
    from whisper import synthetic as S
    from whisper.backend_hip import HipContext
    sd = S.synthetic_state_dict(_dims(), 0)
    got = []
    for keys in (list(sd), list(sd)[::-1]):
        c = HipContext(_dims(), dtype=dtype, max_windows=1, max_group=1)
        try:
            for k in keys:
                c.load_tensor(k, sd[k])
            c.finalize()
            c.mel_write(_mel(3, 80))
            c.encode([0], [3000])
            got.append((c.audio_features(0), c.prefill_logits(0, SOT)[0]))
        finally:
            c.close()
    assert np.isfinite(got[0][1]).all() and np.abs(got[0][0]).max() > 0
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1])
