"""A wh_load_tensor after wh_finalize: the context is unfinalized until the next wh_finalize,
which rebuilds what it derives from the weights (the fragment-ordered W_q, the encoder's 8-bit
weights), so a reloaded context computes what a fresh one with the same weights does.
"""
import numpy as np
import pytest

from test_gpu_cross_kv8 import _mel

gpu = pytest.mark.gpu
SOT = [50258, 50259, 50359]


def _dims():
    from whisper import synthetic as S
    return S.MODEL_DIMS["micro"]


def _context(sd, encoder="native"):
    from whisper.backend_hip import HipContext
    c = HipContext(_dims(), dtype="fp16", max_windows=1, max_group=1, encoder=encoder)
    for k, v in sd.items():
        c.load_tensor(k, v)
    c.finalize()
    return c


def _changed(name):
    from whisper import synthetic as S
    sd = S.synthetic_state_dict(_dims(), 0)
    new = dict(sd)
    new[name] = (sd[name][::-1] * np.float32(0.5)).copy()
    assert not np.array_equal(new[name], sd[name])
    return sd, new


def _refused_unfinalized(c):
    from whisper.backend_hip import HipBackendError, WhDecodeOpts
    c.mel_write(_mel(3, 80))
    with pytest.raises(HipBackendError, match=r"\(-9\): weights not finalized"):
        c.encode([0], [3000])
    opts = WhDecodeOpts(group=1, sample_len=4, eot=50257, no_speech=50362, no_timestamps=50363, timestamp_begin=50364)
    with pytest.raises(HipBackendError, match=r"\(-9\): weights not finalized"):
        c.decode_begin(opts, [SOT], [0])


def _greedy_logits(c, steps=4):
    c.mel_write(_mel(3, 80))
    c.encode([0], [3000])
    rows = [c.prefill([SOT], 1, [0])[0, 1].copy()]
    for _ in range(steps):
        rows.append(c.step([int(rows[-1].argmax())])[0].copy())
    return np.stack(rows)


@gpu
def test_reloaded_cross_query_weight_needs_finalize_and_matches_a_fresh_context():
    name = "decoder.blocks.0.cross_attn.query.weight"
    sd, new = _changed(name)
    c = _context(sd)
    try:
        before = _greedy_logits(c)
        c.load_tensor(name, new[name])
        _refused_unfinalized(c)
        c.finalize()
        got = _greedy_logits(c)
    finally:
        c.close()
    f = _context(new)
    try:
        want = _greedy_logits(f)
    finally:
        f.close()
    assert np.isfinite(want).all() and not np.array_equal(before, want)
    assert np.array_equal(got, want)


@gpu
def test_reloaded_encoder_weight_is_quantised_again_for_fp8():
    from whisper.backend_hip import WH_ENC_FP8_E4M3, WH_ENC_NATIVE
    name = "encoder.blocks.0.mlp.0.weight"
    sd, new = _changed(name)

    def features(c):
        c.mel_write(_mel(3, 80))
        c.encode([0], [3000])
        return c.audio_features(0)

    c = _context(sd, encoder="fp8")
    try:
        before = features(c)
        c.set_encoder_format(WH_ENC_NATIVE)
        c.load_tensor(name, new[name])
        _refused_unfinalized(c)
        c.finalize()
        c.set_encoder_format(WH_ENC_FP8_E4M3)
        got = features(c)
    finally:
        c.close()
    f = _context(new, encoder="fp8")
    try:
        want = features(f)
    finally:
        f.close()
    assert np.isfinite(want).all() and not np.array_equal(before, want)
    assert np.array_equal(got, want)
