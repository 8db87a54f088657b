"""Parity at the base, small and medium widths (n_state 512, 768, 1024; 8, 12, 16 heads).

The library builds code paths chosen by the model width: k_proj1's template instantiations
(CPL 2 / 3 / 4) with their in-launch split-K and deferred fc2 residual, k_proj's K splits
picked from (N, K) (z = 4 / 4 / 8; z = 16 for fc2, at 1024 through the last-resort 8-step tile:
its K = 4096 used to fit no configuration and fell to k_gemv_rows / k_gemv_x<EPI_PARTIAL>, chosen
by row count), the separate cross-attention query launch (k_xattn_seg projects it in-kernel at 1280
only), k_vocab_small / k_gemv_x for the vocabulary (k_vocab1 / k_vocab_2p are K = 1280 only),
head counts that do not divide by the 8 XCDs, and the encoder's k_gemm_256 / k_gemm_tile cut by
tile count.  The other parity tests run widths 128, 384 and 1280.

Models: MODEL_DIMS["base" | "small" | "medium"] cut to 1 encoder and 3 decoder layers (the
k_proj1 deferred residual ping-pongs both ways and still ends in the final-layer form), the
real vocabulary, synthetic_state_dict(dims, 0), two distinct 30 s windows (audio seeds 3, 4).
The reference is oracle.ref_whisper.OracleWhisper on the CPU, computed once per width and
shared by both dtypes and every shape; trajectories are recorded by OracleRecorder, an object
with the reference's Inference interface (test_trajectory_recorder_* pin it without a GPU).

Bars:
  * teacher-forced step logits along a seeded random trajectory (136 steps after the prefill,
    random source rows through wh_reorder_kv at 5 beams): test_gpu_batch.py's
        max |logit - oracle| over the oracle's top-32  <=  TAU[dtype] * (top-32 range)
    per (step, row), top-1 equal wherever the oracle's top-2 margin exceeds 2 TAU range;
  * batch invariance: the same two windows' step logits in batches of 2 and 7 windows,
    bit-identical;
  * encoder output, every element: 2e-3 (fp32) / 6e-2 (fp16) max abs; cross K / V, every
    element: 2e-3 / 2e-2 of the tensor's max abs; slots of one 16-window chunk that hold the
    same audio window: bit-identical;
  * the device loop (whisper.decode, fixed work, 48 tokens): fp32 tokens equal the oracle's and
    avg_logprob within 1e-3; fp16 tokens equal through the decisive prefix.
"""
import functools

import numpy as np
import pytest

from conftest import record_margin
from test_gpu_batch import TAU, _teacher_force

gpu = pytest.mark.gpu

MODEL_OF = {512: "base", 768: "small", 1024: "medium"}
WIDTHS = sorted(MODEL_OF)
DTYPES = ["fp32", "fp16"]
SEEDS = (3, 4)             # the two distinct audio windows; slot / window w holds SEEDS[w % 2]
N_STEPS = 136              # steps after the prefill: contexts cross the 64- and the 128-key pass cuts
TOPK = 32
MAX_WINDOWS, MAX_GROUP = 17, 5
NONDECISIVE_CAP = 0.15
XA_TOL = {"fp32": 2e-3, "fp16": 6e-2}      # encoder output, max abs (test_gpu_micro.py's bars)
CKV_RTOL = {"fp32": 2e-3, "fp16": 2e-2}    # cross K / V, max abs error over the tensor's max abs
SAMPLE_LEN = 48


# ------------------------------------------------------------------ the trajectory recorder
class OracleRecorder:
    """The reference's Inference interface (``logits`` / ``rearrange_kv_cache``) over an
    OracleWhisper whose audio is set, recording per pass the token fed to every row, the
    top-32 of the raw last-position logits and the reorder source rows: the
    dict(tok, topv, topi, src) that test_gpu_batch._teacher_force replays.  Pass 0 is the
    first pass over the initial tokens; src[s - 1] is applied between passes s - 1 and s."""

    def __init__(self, om):
        self.om = om
        self.cache, self.offset = None, 0
        self.tok, self.topv, self.topi, self.src = [], [], [], []

    def logits(self, tokens, audio_features=None):
        import torch
        tokens = torch.as_tensor(tokens)
        inp = tokens if self.cache is None else tokens[:, -1:]
        lg, self.cache, _ = self.om.decoder_forward(inp, self.offset, self.cache)
        self.offset += inp.shape[1]
        v, i = torch.topk(lg[:, -1], TOPK)
        self.tok.append(inp[:, -1].numpy().copy())
        self.topv.append(v.numpy())
        self.topi.append(i.numpy())
        return lg, None

    def rearrange_kv_cache(self, source_indices):
        src = [int(s) for s in source_indices]
        self.cache = [[c[0][src], c[1][src]] for c in self.cache]
        self.src.append(src)

    def trajectory(self):
        assert not self.src or len(self.src) >= len(self.tok) - 1
        return dict(tok=np.stack(self.tok), topv=np.stack(self.topv), topi=np.stack(self.topi),
                    src=np.asarray(self.src[:len(self.tok) - 1]) if self.src else None)


def random_trajectory(om, sot, group, n_steps, rng):
    """A seeded random trajectory through the recorder: after the first pass over ``sot``,
    every step reorders the rows by a source vector drawn uniformly with repeats (group > 1)
    and feeds every row a token drawn uniformly from the vocabulary."""
    import torch
    rec = OracleRecorder(om)
    rec.logits(torch.tensor([list(sot)] * group))
    for _ in range(n_steps):
        if group > 1:
            rec.rearrange_kv_cache(rng.integers(0, group, group))
        rec.logits(torch.from_numpy(rng.integers(0, om.n_vocab, group))[:, None])
    return rec.trajectory()


def nondecisive(trajs, tau):
    """Share of (step, row) pairs whose oracle top-2 margin is within 2 tau (top-32 range)."""
    topv = np.concatenate([t["topv"].reshape(-1, TOPK) for t in trajs])
    return float(((topv[:, 0] - topv[:, 1]) <= 2 * tau * (topv[:, 0] - topv[:, -1])).mean())


def recorded_decisive_prefix(topv, tau):
    """test_gpu_batch.decisive_prefix from a recorded trajectory's top-32 values."""
    topv = topv[:, 0]
    close = (topv[:, 0] - topv[:, 1]) <= 2 * tau * (topv[:, 0] - topv[:, -1])
    return int(np.argmax(close)) if close.any() else len(topv)


# ------------------------------------------------------------------ the CPU reference
def _dims(width):
    from whisper import synthetic as S
    return dict(S.MODEL_DIMS[MODEL_OF[width]], n_audio_layer=1, n_text_layer=3)


@functools.lru_cache(maxsize=None)
def _mel(seed):
    import whisper
    from whisper import synthetic as S
    mel = whisper.log_mel_spectrogram(S.synthetic_audio(30.0, seed=seed), 80, padding=whisper.audio.N_SAMPLES)
    return whisper.pad_or_trim(mel[:, :3000], 3000)


class _Oracle:
    """One width's oracle: weights, the two windows' encoder output and cross K / V."""

    def __init__(self, width):
        import torch

        from oracle import ref_whisper as R
        from whisper import synthetic as S
        self.dims = _dims(width)
        self.sd = S.synthetic_state_dict(self.dims, 0)
        self.om = R.OracleWhisper(self.dims, self.sd)
        self.st = R.SpecialTokens.for_model(self.dims)
        self.sot = list(self.st.sot_sequence)
        self.xa, self.ckv = {}, {}
        for seed in SEEDS:
            self.xa[seed] = self.om.encode(torch.from_numpy(_mel(seed)))
            self.om.set_audio(self.xa[seed])
            self.ckv[seed] = (self.om.cross_k, self.om.cross_v)

    def audio(self, seed):
        self.om.cross_k, self.om.cross_v = self.ckv[seed]
        return self.om


@functools.lru_cache(maxsize=None)
def _oracle(width):
    return _Oracle(width)


@functools.lru_cache(maxsize=None)
def _random_reference(width, seed, group):
    o = _oracle(width)
    return random_trajectory(o.audio(seed), o.sot, group, N_STEPS, np.random.default_rng([11, seed, group]))


@functools.lru_cache(maxsize=None)
def _decode_reference(width, seed, beam):
    """The oracle's own fixed-work decode of one window: (Result, recorded trajectory)."""
    from oracle import ref_whisper as R
    o = _oracle(width)
    rec = OracleRecorder(o.audio(seed))
    res = R.decode(o.om, None, R.Options(beam_size=beam, suppress_tokens=f"-1,{o.st.eot}", sample_len=SAMPLE_LEN),
                   o.st, inference=rec)
    return res, rec.trajectory()


# ------------------------------------------------------------------ the GPU contexts
_CTX = {}


def _model(width, dtype):
    """One context per (width, dtype), 17 windows x 5 beams; one alive at a time."""
    import whisper
    key = (width, dtype)
    if key not in _CTX:
        for k in list(_CTX):
            _CTX.pop(k).close()
        o = _oracle(width)
        m = whisper.Whisper(whisper.ModelDimensions(**o.dims), f"{MODEL_OF[width]}-3layer", device=0, dtype=dtype,
                            max_windows=MAX_WINDOWS, max_group=MAX_GROUP)
        m.load_state_dict(o.sd)
        _CTX[key] = m
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for k in list(_CTX):
        _CTX.pop(k).close()


def _encode(m, n_win):
    m.ctx.mel_write(np.concatenate([_mel(SEEDS[w % 2]) for w in range(n_win)], axis=1))
    m.ctx.encode([3000 * w for w in range(n_win)], [3000] * n_win)


# ------------------------------------------------------------------ 1. teacher-forced steps
SHAPES = [(1, 1), (1, 5), (2, 5), (7, 5)]   # windows x rows per window: 1, 5, 10, 35 rows


@gpu
@pytest.mark.parametrize("width,dtype,n_win,group",
                         [(w, d, nw, g) for w in WIDTHS for d in DTYPES for nw, g in SHAPES])
def test_teacher_forced_step_logits(width, dtype, n_win, group):
    """A seeded random trajectory per distinct window through wh_prefill / wh_reorder_kv /
    wh_step.  1 x 1 and 1 x 5: the k_proj1 layers of this width (deferred fc2 residual both
    ways over 3 layers), k_vocab_small with the LayerNorm prologue, beams and ancestry;
    2 x 5: split-K k_proj at one row tile, k_resid_ln, the separate cross-q launch;
    7 x 5: three row tiles, the k_gemv_x vocabulary in fp16 (33 - 112 rows)."""
    m = _model(width, dtype)
    kern = m.ctx.step_kernels(n_win, group)
    assert kern["proj"] == ("k_proj1" if n_win == 1 else "k_proj"), kern
    assert "<qproj>" not in kern["xattn"], kern   # the in-kernel cross-q serves n = 1280 only
    trajs = [_random_reference(width, SEEDS[w % 2], group) for w in range(n_win)]
    sot = _oracle(width).sot
    skipped = nondecisive(trajs, TAU[dtype])
    _encode(m, n_win)
    rel, top1 = _teacher_force(m, trajs, sot)
    assert rel.shape == (N_STEPS + 1, n_win * group)
    worst = np.unravel_index(int(np.argmax(rel)), rel.shape)
    print(f"width {width} {dtype} {n_win} x {group}: max rel err {rel.max():.3e} ({rel.max() / TAU[dtype]:.3f} TAU) at "
          f"step {worst[0]} row {worst[1]}, p99 {np.quantile(rel, 0.99):.3e}, mean {rel.mean():.3e}; top-1 "
          f"agreement {top1.mean():.4f}, non-decisive {skipped:.4f}; {kern}")
    record_margin("widths_teacher_forced", model=MODEL_OF[width], width=width, dtype=dtype, windows=n_win,
                  rows=int(rel.shape[1]), worst_rel=float(rel.max()), worst_step=int(worst[0]),
                  worst_row=int(worst[1]), p99_rel=float(np.quantile(rel, 0.99)), mean_rel=float(rel.mean()),
                  tau=TAU[dtype], frac_of_tau=float(rel.max() / TAU[dtype]), top1_agreement=float(top1.mean()),
                  nondecisive=skipped, proj=kern["proj"], xattn=kern["xattn"])
    assert skipped <= NONDECISIVE_CAP, f"the top-1 check would skip {skipped:.3f} of the (step, row) pairs"
    assert rel.max() <= TAU[dtype], f"max rel err {rel.max():.3e} > {TAU[dtype]} at step {worst[0]} row {worst[1]}"
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"


INVARIANCE_STEPS = 40


@gpu
@pytest.mark.parametrize("width,dtype", [(w, d) for w in WIDTHS for d in DTYPES])
def test_step_batch_invariance(width, dtype):
    """DESIGN.md §2 "batch invariance" at these widths: the step logits of the same two
    windows (5 rows each, the random trajectories above, prefill + 40 steps) are bit-identical
    in a batch of 2 windows (10 rows) and of 7 (35 rows).  Every split-K projection must take
    its tiling from the weight shape alone; 35 rows also move the fp16 vocabulary projection
    from k_vocab_small to k_gemv_x, which sum a row's k-steps in the same order.  Width 1024
    failed this from the first step on (max |diff| 2.0e-5 fp32, 8.4e-3 fp16) while fc2, K = 4096,
    fitted no k_proj configuration: k_gemv_rows with 4 slabs up to 32 rows, k_gemv_x<EPI_PARTIAL>
    with 16 from 33 rows on (wh_proj.hip CFGS, the last-resort entry)."""
    m = _model(width, dtype)
    sot, group, keep = _oracle(width).sot, 5, 10
    got = {}
    for n_win in (2, 7):
        trajs = [_random_reference(width, SEEDS[w % 2], group) for w in range(n_win)]
        _encode(m, n_win)
        out = [np.repeat(m.ctx.prefill([sot] * n_win, group, [0] * n_win)[:2, 1], group, axis=0)]
        for s in range(1, INVARIANCE_STEPS + 1):
            m.ctx.reorder_kv([w * group + int(x) for w in range(n_win) for x in trajs[w]["src"][s - 1]])
            lg = m.ctx.step([int(x) for w in range(n_win) for x in trajs[w]["tok"][s]],
                            text_offsets=[len(sot) + s - 1] * n_win)
            out.append(lg[:keep].copy())
        got[n_win] = np.stack(out)
    diff = np.abs(got[7] - got[2])
    first = int(np.argmax(diff.max(axis=(1, 2)) > 0)) if diff.max() > 0 else -1
    print(f"width {width} {dtype} batch invariance 2 vs 7 windows: max |diff| {diff.max():.3e}, first differing pass {first}")
    record_margin("widths_batch_invariance", model=MODEL_OF[width], width=width, dtype=dtype,
                  max_abs_diff=float(diff.max()), first_differing_pass=first)
    assert np.array_equal(got[7], got[2]), \
        f"logits differ between 2 and 7 windows from pass {first} on, max |diff| {diff.max():.3e}"


# ------------------------------------------------------------------ 2. encoder and cross K / V
def _heads(t, n_head):
    """[1, 1500, n] -> [H, 1500, 64], wh_read_cross_kv's layout."""
    return t[0].reshape(t.shape[1], n_head, 64).permute(1, 0, 2).numpy()


@gpu
@pytest.mark.parametrize("width,dtype", [(w, d) for w in WIDTHS for d in DTYPES])
def test_encoder_and_cross_kv_whole_tensors(width, dtype):
    """encode at 1 window (half tiles, KZ = 2 in fp16), 3 windows (k_gemm_tile) and 17 windows
    (a full 16-window chunk: k_gemm_256 from 256 tiles on, a ragged last row tile; then a chunk
    of one window inside a multi-window encode).  Every slot's audio features, element-wise,
    against the oracle's encoder; cross K / V of every decoder layer at slots 0, 1, 15, 16
    (K unscaled: the library, like the oracle, folds 0.125 into the decoder query)."""
    m = _model(width, dtype)
    o = _oracle(width)
    H, L = o.dims["n_text_head"], o.dims["n_text_layer"]
    xa_ref = {s: o.xa[s].numpy() for s in SEEDS}
    kv_ref = {s: [(_heads(o.ckv[s][0][l], H), _heads(o.ckv[s][1][l], H)) for l in range(L)] for s in SEEDS}
    fails = []
    for n_win in (1, 3, 17):
        _encode(m, n_win)
        xa = [m.ctx.audio_features(w) for w in range(n_win)]
        err = np.stack([np.abs(xa[w] - xa_ref[SEEDS[w % 2]]) for w in range(n_win)])
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        kv_worst, kv_at = 0.0, None
        for slot in (s for s in (0, 1, 15, 16) if s < n_win):
            for l in range(L):
                for name, got, ref in zip("kv", m.ctx.cross_kv(slot, l), kv_ref[SEEDS[slot % 2]][l]):
                    e = float(np.abs(got - ref).max() / np.abs(ref).max())
                    if e > kv_worst:
                        kv_worst, kv_at = e, (slot, l, name)
        print(f"width {width} {dtype} encode {n_win} windows: xa max abs err {err.max():.3e} at (slot, row, col) "
              f"{tuple(map(int, at))}, per slot {err.max(axis=(1, 2)).tolist()}; cross K/V worst {kv_worst:.3e} of "
              f"max abs at (slot, layer, k/v) {kv_at}")
        record_margin("widths_encoder", model=MODEL_OF[width], width=width, dtype=dtype, windows=n_win,
                      xa_max_abs_err=float(err.max()), slot=int(at[0]), row=int(at[1]), col=int(at[2]),
                      xa_tol=XA_TOL[dtype], ckv_worst_rel=kv_worst, ckv_at=str(kv_at), ckv_rtol=CKV_RTOL[dtype])
        if err.max() > XA_TOL[dtype]:
            fails.append(f"{n_win} windows: xa max abs err {err.max():.3e} > {XA_TOL[dtype]} at {tuple(map(int, at))}")
        if kv_worst > CKV_RTOL[dtype]:
            fails.append(f"{n_win} windows: cross {kv_at} err {kv_worst:.3e} > {CKV_RTOL[dtype]} of max abs")
        if n_win == 17:
            # no tolerance: the 16-window chunk's slots with the same audio, bit for bit
            for w in range(2, 16):
                if not np.array_equal(xa[w], xa[w % 2]):
                    d = np.abs(xa[w] - xa[w % 2])
                    fails.append(f"17 windows: slot {w} differs from slot {w % 2} (same audio, same chunk), max "
                                 f"{d.max():.3e} at {tuple(map(int, np.unravel_index(int(np.argmax(d)), d.shape)))}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ 3. the device loop
@gpu
@pytest.mark.parametrize("width,dtype,beam,n_win",
                         [(w, d, b, nw) for w in WIDTHS for d in DTYPES for b in (None, 5) for nw in (1, 3)])
def test_device_loop_tokens(width, dtype, beam, n_win):
    """whisper.decode (the loop on the device: token selection, k_merge writing the next
    step's E[tok] + P[pos] rows at this width), fixed work, 48 tokens, greedy and beam 5, one
    window and three (audio seeds 3, 4, 3) in one batch, against the oracle's decode of each
    window.  fp16: through the steps before the first whose recorded top-2 margin (row 0, as
    test_gpu_batch.decisive_prefix takes it) is within 2 TAU of the top-32 range."""
    import whisper
    m = _model(width, dtype)
    o = _oracle(width)
    seeds = [SEEDS[w % 2] for w in range(n_win)]
    res = whisper.decode(m, np.stack([_mel(s) for s in seeds]),
                         whisper.DecodingOptions(language="en", beam_size=beam, suppress_tokens=f"-1,{o.st.eot}",
                                                 sample_len=SAMPLE_LEN))
    assert len(res) == n_win
    for w, (seed, r) in enumerate(zip(seeds, res)):
        ref, traj = _decode_reference(width, seed, beam)
        got, want = np.asarray(r.tokens), np.asarray(ref.tokens)
        n = min(len(got), len(want))
        agree = int(np.argmax(got[:n] != want[:n])) if np.any(got[:n] != want[:n]) else n
        need = min(recorded_decisive_prefix(traj["topv"], TAU[dtype]), len(want))
        dlp = abs(float(r.avg_logprob) - float(ref.avg_logprob))
        print(f"width {width} {dtype} beam {beam} window {w}/{n_win} (seed {seed}): agreement {agree}/{len(want)} "
              f"(decisive prefix {need}), avg_logprob diff {dlp:.2e}")
        record_margin("widths_device_loop", model=MODEL_OF[width], width=width, dtype=dtype, beam=beam or 1,
                      windows=n_win, window=w, agree_steps=agree, ref_steps=int(len(want)), decisive_prefix=need,
                      avg_logprob_diff=dlp)
        assert len(want) == SAMPLE_LEN
        if dtype == "fp32":
            np.testing.assert_array_equal(got, want, err_msg=f"window {w} (audio seed {seed})")
            assert dlp <= 1e-3, f"window {w}: avg_logprob {r.avg_logprob} vs {ref.avg_logprob}"
        else:
            assert len(got) == len(want)
            assert agree >= need, f"window {w}: tokens differ at step {agree}, inside the decisive prefix {need}"


# ------------------------------------------------------------------ 4. the harness, on the CPU
@functools.lru_cache(maxsize=None)
def _micro_oracle():
    import torch

    from oracle import ref_whisper as R
    from whisper import synthetic as S
    dims = S.MODEL_DIMS["micro"]
    om = R.OracleWhisper(dims, S.synthetic_state_dict(dims, 0))
    mel = R.pad_or_trim(R.log_mel_spectrogram(S.synthetic_audio(30.0, seed=3), dims["n_mels"],
                                              padding=R.N_SAMPLES)[:, :3000])
    xa = om.encode(mel)
    om.set_audio(xa)
    return om, xa, R.SpecialTokens.for_model(dims)


@pytest.mark.parametrize("beam", [None, 5])
def test_trajectory_recorder_reproduces_oracle_decode(beam):
    """The recorder passed as inference= leaves R.decode's result unchanged, and what it
    recorded is that decode: one pass per token, fed the tokens the loop chose."""
    from oracle import ref_whisper as R
    om, xa, st = _micro_oracle()
    opts = R.Options(beam_size=beam, suppress_tokens=f"-1,{st.eot}", sample_len=SAMPLE_LEN)
    want = R.decode(om, None, opts, st, xa=xa)
    rec = OracleRecorder(om)
    got = R.decode(om, None, opts, st, inference=rec)
    assert got.tokens == want.tokens and len(want.tokens) == SAMPLE_LEN
    assert got.avg_logprob == want.avg_logprob
    t = rec.trajectory()
    G = beam or 1
    assert t["tok"].shape == (SAMPLE_LEN, G) and t["topv"].shape == (SAMPLE_LEN, G, TOPK)
    assert (t["tok"][0] == st.sot_sequence[-1]).all()
    assert (t["src"] is None) if beam is None else (t["src"].shape == (SAMPLE_LEN - 1, G))
    if beam is None:  # greedy feeds its choice back
        assert [int(x) for x in t["tok"][1:, 0]] == want.tokens[:-1]
    assert np.isfinite(t["topv"]).all() and (np.diff(t["topv"], axis=-1) <= 0).all()


def test_trajectory_recorder_random_replay_matches_full_prefix():
    """The reorder bookkeeping the GPU tests rest on: along a random 5-row trajectory the
    recorder's cached logits of a late step equal a fresh decoder_forward over every row's
    whole prefix, rebuilt here from (tok, src) alone.  Both are the oracle's fp32 arithmetic
    in a different association, so the bar is the fp32 one the library is held to."""
    import torch
    om, _, st = _micro_oracle()
    sot, G, S = list(st.sot_sequence), 5, 40
    t = random_trajectory(om, sot, G, S, np.random.default_rng(5))
    assert t["tok"].shape == (S + 1, G) and t["src"].shape == (S, G)
    assert len({tuple(r) for r in t["src"]}) > S // 2 and (t["src"].max(), t["src"].min()) == (G - 1, 0)
    prefix = [list(sot) for _ in range(G)]
    for s in range(1, S + 1):
        prefix = [prefix[int(t["src"][s - 1, r])] + [int(t["tok"][s, r])] for r in range(G)]
        if s in (S - 1, S):
            assert len({tuple(p) for p in prefix}) > 1      # rows really differ
            full, _, _ = om.decoder_forward(torch.tensor(prefix), 0, None)
            for r in range(G):
                topv, topi = t["topv"][s, r], t["topi"][s, r]
                rel = np.abs(full[r, -1].numpy()[topi] - topv).max() / (topv[0] - topv[-1])
                assert rel <= TAU["fp32"], (s, r, rel)
