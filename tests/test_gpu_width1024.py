"""The decoder step at the medium models' width (n_text_state 1024), two windows.

Two windows of one row each is the smallest batch that takes the split-K step: k_proj
writes partial slabs (fp16 in fp16 contexts) and k_resid_ln sums them into the residual
and normalises it for the next projection (one window takes the k_proj1 layers instead).
At widths 772..1024 k_resid_ln's block is 256 threads, the size that once also meant "the
two-float4 form, fp32 slabs only": fp16 slabs were then read as fp32.  This is the narrow
regression test of that defect; tests/test_gpu_widths.py runs widths 512, 768 and 1024 over
every step path (the golden-trajectory teacher-forced tests cover 128, 384 and 1280).

Synthetic medium dimensions with 1 encoder and 2 decoder layers (both forms of the
residual launch: the next layer's LayerNorm and the final one), seeded weights, two copies
of one synthetic 30 s window.  wh_prefill of the sot sequence, then 8 wh_step calls, each
fed the argmax of the CPU oracle's own logits (the oracle teacher-forces); prefill and
every step are held to tests/test_gpu_batch.py's bound, per window:
    max |logit - oracle| over the oracle's top-32  <=  TAU[dtype] * (top-32 range).
fp32 is the control: its slabs are fp32 at every width.
"""
import functools

import numpy as np
import pytest

from test_gpu_batch import TAU

pytestmark = pytest.mark.gpu

N_WIN, N_STEPS = 2, 8


def _dims():
    from whisper import synthetic as S
    return dict(S.MODEL_DIMS["medium"], n_audio_layer=1, n_text_layer=2)


@functools.lru_cache(maxsize=None)
def _reference():
    """(mel, sot, per pass: the token fed to it and the oracle's top-32 values / ids); pass 0
    is the prefill of the sot sequence, pass s >= 1 step s.  Computed once, for both dtypes."""
    import torch

    import whisper
    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = _dims()
    sd = S.synthetic_state_dict(dims, 0)
    audio = S.synthetic_audio(30.0, seed=3)
    mel = whisper.log_mel_spectrogram(audio, dims["n_mels"], padding=whisper.audio.N_SAMPLES)
    mel = whisper.pad_or_trim(mel[:, :3000], 3000)
    om = R.OracleWhisper(dims, sd)
    om.set_audio(om.encode(torch.from_numpy(mel)))
    sot = list(R.SpecialTokens.for_model(dims).sot_sequence)
    logits, cache, _ = om.decoder_forward(torch.tensor([sot]), 0, None)
    passes = []
    for s in range(N_STEPS + 1):
        row = logits[0, -1]
        topv, topi = torch.topk(row, 32)
        passes.append((sot[-1] if s == 0 else tok, topv.numpy(), topi.numpy()))
        tok = int(torch.argmax(row))
        if s < N_STEPS:
            logits, cache, _ = om.decoder_forward(torch.tensor([[tok]]), len(sot) + s, cache)
    return mel, sot, sd, passes


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_medium_width_two_window_steps(dtype):
    import whisper
    mel, sot, sd, passes = _reference()
    m = whisper.Whisper(whisper.ModelDimensions(**_dims()), "medium-2layer", device=0, dtype=dtype,
                        max_windows=N_WIN, max_group=1)
    try:
        m.load_state_dict(sd)
        m.ctx.mel_write(np.concatenate([mel] * N_WIN, axis=1))
        m.ctx.encode([3000 * w for w in range(N_WIN)], [3000] * N_WIN)
        rel = np.zeros((N_STEPS + 1, N_WIN))
        for s, (tok, topv, topi) in enumerate(passes):
            if s == 0:
                rows = m.ctx.prefill([sot] * N_WIN, 1, [0] * N_WIN)[:, 1]
            else:
                rows = m.ctx.step([tok] * N_WIN, text_offsets=[len(sot) + s - 1] * N_WIN)
            for w in range(N_WIN):
                rel[s, w] = np.abs(rows[w][topi] - topv).max() / (topv[0] - topv[-1])
        kern = m.ctx.step_kernels(N_WIN, 1)
    finally:
        m.close()
    print(f"medium width {dtype} {N_WIN} windows: max rel err per pass {rel.max(axis=1).tolist()}, "
          f"per window {rel.max(axis=0).tolist()} (bound {TAU[dtype]}) {kern}")
    assert kern["proj"] == "k_proj", kern  # the split-K step, not the single-window layers
    assert (rel.max(axis=0) <= TAU[dtype]).all(), f"max rel err per window {rel.max(axis=0)} > {TAU[dtype]}"
