"""Parity at decoder contexts 228 to 448, and the stop at the context limit.

transcribe() conditions every window after a file's first one on the previous text: the
window starts from <|startofprev|> + up to 223 prompt tokens + the SOT sequence (227 tokens
multilingual), its steps run at positions 227 to 447, and a window that does not reach EOT
ends because the context is full (`len + 1 > n_ctx`), not because sample_len ran out.  The
other parity files start from the bare SOT sequence (contexts up to about 228) or from 40
prompt tokens; this one starts where they end.  What runs here and nowhere else against a
reference: k_self_attn_qkv at 4 to 7 key passes, sv[] / slot_of[] beyond 256 entries,
k_self_attn at first-pass rows 64 to 446 in fp16 (the coalesced-K branch), merge_window
staging up to MG_MAXCTX history words, the stop rule in the greedy and the beam branch,
pmax = CTX - 1 in merge_embed, positional rows above 268, and begin_batch splitting a first
pass over several prefill() calls.

Models, all synthetic_state_dict(dims, 0), one 30 s window per audio seed (3, 4): "micro";
"base3" = test_gpu_widths._dims(512) (k_proj1 / k_proj, k_vocab_small / k_gemv_x); "turbo1"
= turbo with one encoder layer and its 4 decoder layers, 128 mels, 51866 ids (K = 1280:
k_vocab1; one window runs k_proj1, whose step_kernels reports no in-kernel cross-query).
The reference is oracle.ref_whisper.OracleWhisper on the CPU, once per model, shared by both
dtypes.  The window's log-mel is the oracle's own (CPU) and is written to the device with
mel_write, so the harness tests below see the very trajectories the GPU tests replay.

1. test_teacher_forced_to_last_position: [sot_prev] + 223 uniform ids in [0, eot) + SOT
   sequence, then n_text_ctx - 227 = 221 steps of uniform tokens with uniform source rows at
   5 beams through wh_prefill / wh_reorder_kv / wh_step; the last step feeds position 447.
   The project's bar: per (step, row) max |logit - oracle| over the oracle's top-32 <=
   TAU[dtype] * (top-32 range), top-1 equal where the oracle's margin exceeds 2 TAU range,
   at most NONDECISIVE_CAP of the pairs non-decisive.  The worst error per 64-position bucket
   of the context goes to the margin log: recorded, not asserted.
2. test_device_loop_stops_at_context_limit / test_filtered_... / test_three_windows_...:
   whisper.decode (graph path, selection and merge on the device) against
   oracle.ref_whisper.decode over HipInference on the same logits: tokens equal in fp32 and
   fp16, avg_logprob within 1e-4 (test_gpu_tail.py's bound).  EOT suppressed, 223 prompt ids,
   the default sample_len 224: the oracle stops on `tokens.shape[-1] > n_text_ctx` after 222
   tokens, and the case fails unless that count is below sample_len.
3. test_first_pass_split_over_prefill_calls: 4 windows with 300, 300, 227, 300 initial
   tokens in a 4-window context: 1127 rows > the 1024-row prefill buffer.
4. test_stale_cache_content_does_not_matter: exact.  A short run's logits are bit-identical
   before and after runs that fill the cache up to position 447.

What the tolerance tests can and cannot see.  Measured on the oracle at context 447: when the
last step reads the cached K / V row of one position from its neighbour, the top-32 logits
move by 2.3e-3 to 8.3e-3 of their range on micro and by 1.0e-2 to 2.0e-2 on the 512-wide
model.  The fp32 bar (2e-5) catches a single mis-read key with more than 100x to spare
(test_fp32_bar_catches_one_misread_key keeps a 10x floor).  The fp16 bar (1e-2) does NOT
reliably catch a single key: on the 512-wide model one key moves the logits by 1.0 to 2.0
TAU and a 64-key pass read one row off by 0.7 to 1.9 TAU, while honest fp16 error already
takes a good part of one TAU.  In fp16 the exact checks of parts 2 and 4 carry that weight.
"""
import functools

import numpy as np
import pytest

from conftest import record_margin
from repeat_filter_ref import FilteredInference, repeats
from test_gpu_batch import TAU
from test_gpu_widths import NONDECISIVE_CAP, TOPK, OracleRecorder, _dims, _model, nondecisive, random_trajectory
import test_gpu_widths as _widths

gpu = pytest.mark.gpu

DTYPES = ["fp32", "fp16"]
SEEDS = (3, 4)              # the two distinct audio windows; window w holds SEEDS[w % 2]
N_PROMPT = 223              # n_text_ctx // 2 - 1: what transcribe() keeps of the previous text
MAX_GROUP = 5
MICRO_WINDOWS = 4           # part 3 needs exactly the 1024-row prefill buffer
N_VARIANTS = {"micro": 1, "base3": 4, "turbo1": 1}   # distinct trajectories per audio seed (7 x 5: 4 + 3)
BUCKET = 64


def _model_dims(model):
    from whisper import synthetic as S
    if model == "micro":
        return dict(S.MODEL_DIMS["micro"])
    if model == "base3":
        return _dims(512)
    assert model == "turbo1"
    return dict(S.MODEL_DIMS["turbo"], n_audio_layer=1)


# ------------------------------------------------------------------ the CPU reference
class _LongOracle:
    """test_gpu_widths._Oracle for any of the three models, from the oracle's own log-mel:
    weights, special tokens, and per audio seed the window's mel, encoder output and cross K / V."""

    def __init__(self, model):
        from oracle import ref_whisper as R
        from whisper import synthetic as S
        self.model = model
        self.dims = _model_dims(model)
        self.sd = S.synthetic_state_dict(self.dims, 0)
        self.om = R.OracleWhisper(self.dims, self.sd)
        self.st = R.SpecialTokens.for_model(self.dims)
        self.sot = list(self.st.sot_sequence)
        self.n_ctx = self.dims["n_text_ctx"]
        self._mel, self.xa, self.ckv = {}, {}, {}

    def mel(self, seed):
        from oracle import ref_whisper as R
        from whisper import synthetic as S
        if seed not in self._mel:
            mel = R.log_mel_spectrogram(S.synthetic_audio(30.0, seed=seed), self.dims["n_mels"], padding=R.N_SAMPLES)
            self._mel[seed] = R.pad_or_trim(mel[:, :3000]).numpy()
        return self._mel[seed]

    def audio(self, seed):
        """The oracle with this window's cross K / V set (encoded on first use)."""
        import torch
        if seed not in self.ckv:
            self.xa[seed] = self.om.encode(torch.from_numpy(self.mel(seed)))
            self.om.set_audio(self.xa[seed])
            self.ckv[seed] = (self.om.cross_k, self.om.cross_v)
        self.om.cross_k, self.om.cross_v = self.ckv[seed]
        return self.om

    def prompted(self, rng, n_init=None):
        """[sot_prev] + uniform ids in [0, eot) + the SOT sequence, n_init tokens in all."""
        n = N_PROMPT if n_init is None else n_init - 1 - len(self.sot)
        return [self.st.sot_prev] + [int(t) for t in rng.integers(0, self.st.eot, n)] + self.sot


@functools.lru_cache(maxsize=None)
def _long_oracle(model):
    return _LongOracle(model)


def random_trajectories(om, inits, group, n_steps, rngs):
    """random_trajectory for several windows of ONE audio window in a single oracle batch
    (the CPU oracle streams its weights once per pass whatever the row count): window k's
    rows are k * group ..., its draws come from rngs[k] in random_trajectory's order (source
    rows, then tokens), so each returned trajectory is what random_trajectory(om, inits[k],
    group, n_steps, rngs[k]) records.  All inits have one length.  The first pass, whose
    logits at all 227 positions are most of a trajectory's cost, runs one row per window: a
    window's rows share it, as they do on the device."""
    import torch
    n = len(inits)
    assert len(rngs) == n and len({len(i) for i in inits}) == 1
    rec = OracleRecorder(om)
    rec.logits(torch.tensor([list(i) for i in inits]))
    if group > 1:
        rows = [k for k in range(n) for _ in range(group)]
        rec.cache = [[c[0][rows], c[1][rows]] for c in rec.cache]
        rec.tok, rec.topv, rec.topi = [rec.tok[0][rows]], [rec.topv[0][rows]], [rec.topi[0][rows]]
    for _ in range(n_steps):
        src, tok = [], []
        for k, rng in enumerate(rngs):
            src.append(k * group + (rng.integers(0, group, group) if group > 1 else np.zeros(1, dtype=np.int64)))
            tok.append(rng.integers(0, om.n_vocab, group))
        if group > 1:
            rec.rearrange_kv_cache(np.concatenate(src))
        rec.logits(torch.from_numpy(np.concatenate(tok))[:, None])
    t = rec.trajectory()
    rows = [slice(k * group, (k + 1) * group) for k in range(n)]
    return [dict(tok=t["tok"][:, r], topv=t["topv"][:, r], topi=t["topi"][:, r],
                 src=None if t["src"] is None else t["src"][:, r] - k * group) for k, r in enumerate(rows)]


@functools.lru_cache(maxsize=None)
def _long_reference(model, seed, group):
    """The part-1 trajectories of one audio seed: N_VARIANTS[model] of (initial tokens,
    trajectory), each from default_rng([17, seed, group, variant]): first the 223 prompt ids,
    then the steps up to position n_text_ctx - 1."""
    o = _long_oracle(model)
    rngs = [np.random.default_rng([17, seed, group, v]) for v in range(N_VARIANTS[model])]
    inits = [o.prompted(rng) for rng in rngs]
    trajs = random_trajectories(o.audio(seed), inits, group, o.n_ctx - len(inits[0]), rngs)
    return list(zip(inits, trajs))


def _windows(model, n_win, group):
    """Per window (audio seeds alternate, every window a trajectory of its own): (inits, trajs)."""
    per = [_long_reference(model, SEEDS[w % 2], group)[w // 2] for w in range(n_win)]
    return [p[0] for p in per], [p[1] for p in per]


# ------------------------------------------------------------------ the replay
def teacher_force(m, trajs, inits, sot_index=None):
    """test_gpu_batch._teacher_force with per-window initial tokens (any lengths) and hence
    per-window text_offsets: wh_prefill of inits[w], then per step the reorder (5 rows) and
    wh_step with trajs[w]'s tokens.  Returns the per-(pass, row) relative errors, the top-1
    agreement where the reference's margin is decisive, and wh_prefill's [n_win][2][V]
    logits (rows sot_index[w], default 0, and last)."""
    n_win = len(trajs)
    S, G = trajs[0]["tok"].shape
    for t, init in zip(trajs, inits):
        assert t["tok"].shape == (S, G) and init[-1] == int(t["tok"][0, 0])
    two = m.ctx.prefill(inits, G, [0] * n_win if sot_index is None else sot_index)
    rel = np.zeros((S, n_win * G))
    top1 = np.ones((S, n_win * G), dtype=bool)

    def score(s, rows):
        for r in range(n_win * G):
            w, b = divmod(r, G)
            topv, topi = trajs[w]["topv"][s, b], trajs[w]["topi"][s, b]
            rng = topv[0] - topv[-1]
            rel[s, r] = np.abs(rows[r][topi] - topv).max() / rng
            if topv[0] - topv[1] > 2 * TAU[m.dtype] * rng:
                top1[s, r] = int(np.argmax(rows[r])) == int(topi[0])

    score(0, np.repeat(two[:, 1], G, axis=0))
    for s in range(1, S):
        if trajs[0]["src"] is not None:
            m.ctx.reorder_kv([w * G + int(x) for w in range(n_win) for x in trajs[w]["src"][s - 1]])
        lg = m.ctx.step([int(x) for w in range(n_win) for x in trajs[w]["tok"][s]],
                        text_offsets=[len(init) + s - 1 for init in inits])
        score(s, lg)
    return rel, top1, two


def context_buckets(rel, n_init, group):
    """Worst relative error per 64-position bucket of the context: pass s of a window with
    n_init initial tokens feeds position n_init - 1 + s.  {"0-63": ..., "384-447": ...},
    None where no pass of the run falls."""
    S = rel.shape[0]
    worst = {}
    for w, n in enumerate(n_init):
        pos = n - 1 + np.arange(S)
        per_pass = rel[:, w * group:(w + 1) * group].max(axis=1)
        for b in np.unique(pos // BUCKET):
            worst[int(b)] = max(worst.get(int(b), 0.0), float(per_pass[pos // BUCKET == b].max()))
    top = max((max(n_init) - 1 + S - 1) // BUCKET, 6)
    return {f"{b * BUCKET}-{b * BUCKET + BUCKET - 1}": worst.get(b) for b in range(top + 1)}


# ------------------------------------------------------------------ the GPU contexts
_CTX = {}


def _context(model, dtype):
    """One context per (model, dtype); the 512-wide one is test_gpu_widths' (17 x 5)."""
    if model == "base3":
        for k in list(_CTX):
            _CTX.pop(k).close()
        m = _model(512, dtype)
        assert m.dims.__dict__ == _long_oracle(model).dims      # the same seeded weights
        return m
    import whisper
    key = (model, dtype)
    if key not in _CTX:
        for k in list(_CTX):
            _CTX.pop(k).close()
        for k in list(_widths._CTX):
            _widths._CTX.pop(k).close()
        o = _long_oracle(model)
        m = whisper.Whisper(whisper.ModelDimensions(**o.dims), model, device=0, dtype=dtype,
                            max_windows=MICRO_WINDOWS if model == "micro" else 1, max_group=MAX_GROUP)
        m.load_state_dict(o.sd)
        _CTX[key] = m
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctxs in (_CTX, _widths._CTX):
        for k in list(ctxs):
            ctxs.pop(k).close()


def _encode(m, model, n_win):
    o = _long_oracle(model)
    m.ctx.mel_write(np.concatenate([o.mel(SEEDS[w % 2]) for w in range(n_win)], axis=1))
    m.ctx.encode([3000 * w for w in range(n_win)], [3000] * n_win)


# ------------------------------------------------------------------ 1. teacher-forced steps
SHAPES = [("micro", 1, 1), ("micro", 1, 5), ("base3", 1, 1), ("base3", 1, 5), ("base3", 2, 5), ("base3", 7, 5),
          ("turbo1", 1, 1), ("turbo1", 1, 5)]


@gpu
@pytest.mark.parametrize("model,n_win,group,dtype",
                         [s + (d,) for mo in ("micro", "base3", "turbo1") for d in DTYPES for s in SHAPES if s[0] == mo])
def test_teacher_forced_to_last_position(model, n_win, group, dtype):
    """A 227-token first pass (in fp16 k_self_attn's coalesced-K branch from row 64 on), then
    221 steps at positions 227 to 447.  One window: k_proj1 and k_self_attn; 2 x 5 and 7 x 5:
    k_proj and k_self_attn_qkv at 4 to 7 key passes, every window on a trajectory of its own."""
    m = _context(model, dtype)
    o = _long_oracle(model)
    kern = m.ctx.step_kernels(n_win, group)
    assert kern["proj"] == ("k_proj1" if n_win == 1 else "k_proj"), kern
    inits, trajs = _windows(model, n_win, group)
    assert all(len(i) == 1 + N_PROMPT + len(o.sot) == 227 for i in inits)
    assert len({tuple(i) for i in inits}) == n_win                    # every window its own trajectory
    skipped = nondecisive(trajs, TAU[dtype])
    assert skipped <= NONDECISIVE_CAP, f"the top-1 check would skip {skipped:.3f} of the (step, row) pairs"
    _encode(m, model, n_win)
    rel, top1, _ = teacher_force(m, trajs, inits)
    assert rel.shape == (o.n_ctx - 227 + 1, n_win * group)           # the last pass feeds position 447
    worst = np.unravel_index(int(np.argmax(rel)), rel.shape)
    buckets = context_buckets(rel, [len(i) for i in inits], group)
    print(f"{model} {dtype} {n_win} x {group}: max rel err {rel.max():.3e} ({rel.max() / TAU[dtype]:.3f} TAU) at "
          f"step {worst[0]} (position {226 + worst[0]}) row {worst[1]}, p99 {np.quantile(rel, 0.99):.3e}; per "
          f"bucket {buckets}; top-1 agreement {top1.mean():.4f}, non-decisive {skipped:.4f}; {kern}")
    record_margin("longctx_teacher_forced", model=model, dtype=dtype, windows=n_win, rows=int(rel.shape[1]),
                  worst_rel=float(rel.max()), worst_step=int(worst[0]), worst_position=int(226 + worst[0]),
                  worst_row=int(worst[1]), p99_rel=float(np.quantile(rel, 0.99)), mean_rel=float(rel.mean()),
                  tau=TAU[dtype], frac_of_tau=float(rel.max() / TAU[dtype]), top1_agreement=float(top1.mean()),
                  nondecisive=skipped, worst_rel_by_context=buckets, proj=kern["proj"], xattn=kern["xattn"],
                  self_attn=kern["self_attn"])
    assert rel.max() <= TAU[dtype], \
        f"max rel err {rel.max():.3e} > {TAU[dtype]} at step {worst[0]} row {worst[1]}; per bucket {buckets}"
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"


# ------------------------------------------------------------------ 2. the device loop into the limit
def _prompt(model, n, key=0):
    o = _long_oracle(model)
    return [int(t) for t in np.random.default_rng([23, n, key]).integers(0, o.st.eot, n)] if n else None


def _host_loop(m, model, seed, opts, n=0, p=1.0):
    """oracle.ref_whisper.decode over the per-step ABI for one window (test_gpu_tail.py),
    the repeat filter restated on the host when asked for (test_gpu_repeat_filter.py)."""
    from types import SimpleNamespace

    import whisper
    from oracle import ref_whisper as R
    from whisper.decoding import DecodingTask
    from whisper.inference import HipInference
    o = _long_oracle(model)
    task = DecodingTask(m, whisper.DecodingOptions(language="en", **opts))
    m.ctx.mel_write(o.mel(seed))
    m.ctx.encode([0], [3000])
    inf = HipInference(m, task.sample_begin, group=opts.get("beam_size") or 1, sot_index=task.sot_index)
    if n or p != 1.0:
        inf = FilteredInference(inf, task.sample_begin, o.st.eot, n=n, p=p)
    ref = R.decode(SimpleNamespace(dims=o.dims), None, R.Options(**opts), o.st, inference=inf)
    return ref, inf, task


def _into_the_limit(model, dtype, beam, without_timestamps, n=0, p=1.0):
    import whisper
    m = _context(model, dtype)
    o = _long_oracle(model)
    opts = dict(suppress_tokens=f"-1,{o.st.eot}", prompt=_prompt(model, N_PROMPT), beam_size=beam,
                without_timestamps=without_timestamps)
    got = whisper.decode(m, o.mel(3), whisper.DecodingOptions(language="en", no_repeat_ngram_size=n,
                                                              repetition_penalty=p, **opts))
    ref, inf, task = _host_loop(m, model, 3, opts, n, p)
    a, b = np.asarray(got.tokens), np.asarray(ref.tokens)
    dlp = abs(float(got.avg_logprob) - float(ref.avg_logprob))
    print(f"{model} {dtype} beam {beam} without_timestamps {without_timestamps} n={n} p={p}: {len(a)} tokens (host "
          f"loop {len(b)}, sample_len {task.sample_len}, {task.sample_begin} initial), avg_logprob diff {dlp:.2e}")
    # the host loop stopped on tokens.shape[-1] > n_text_ctx, not on sample_len: its last pass fed position 447
    assert task.sample_begin == 227 + int(without_timestamps) and task.sample_len == 224
    assert len(b) == o.n_ctx + 1 - task.sample_begin < task.sample_len
    assert len(a) == len(b)
    np.testing.assert_array_equal(a, b)
    assert dlp <= 1e-4
    return a, inf


@gpu
@pytest.mark.parametrize("model,dtype,beam,without_timestamps",
                         [(mo, d, b, wt) for mo in ("micro", "turbo1") for d in DTYPES for b in (None, 5)
                          for wt in (False, True)])
def test_device_loop_stops_at_context_limit(model, dtype, beam, without_timestamps):
    _into_the_limit(model, dtype, beam, without_timestamps)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_filtered_device_loop_stops_at_context_limit(dtype):
    """no_repeat_ngram_size 3 and repetition_penalty 1.1 over 222 sampled tokens (the
    repeat-filter tests stop at 96), with that file's assertions."""
    a, inf = _into_the_limit("micro", dtype, None, False, n=3, p=1.1)
    assert inf.n_banned + inf.n_penalised >= 1
    assert repeats(a, 3, _long_oracle("micro").st.eot) == []


@gpu
@pytest.mark.parametrize("dtype,beam", [(d, b) for d in DTYPES for b in (None, 5)])
def test_three_windows_finish_at_different_steps(dtype, beam):
    """Prompts of 223, 100 and 0 tokens in one batch (audio seeds 3, 4, 3): window 0 stops on
    the context after 222 tokens and is re-embedded at pos = min(len - 1, pmax) while the
    others run on to sample_len.  Each window's tokens equal the same window decoded alone,
    in fp32 and in fp16: a batch of one window runs other arithmetic (k_proj1, 32 selection
    slices; DESIGN.md §2 "batch invariance"), so avg_logprob is not compared, and the tokens
    can be because micro's top-2 margins stand far above the fp16 bound (non-decisive share
    0.000 at TAU[fp16] on every micro trajectory of this file)."""
    import whisper
    from whisper.decoding import run_windows
    m = _context("micro", dtype)
    o = _long_oracle("micro")
    options = whisper.DecodingOptions(language="en", beam_size=beam, suppress_tokens=f"-1,{o.st.eot}")
    prompts = [_prompt("micro", N_PROMPT), _prompt("micro", 100), None]
    seeds = [SEEDS[w % 2] for w in range(3)]
    want = [whisper.decode(m, o.mel(seeds[w]), options, prompt=prompts[w]) for w in range(3)]
    m.ctx.mel_write(np.concatenate([o.mel(s) for s in seeds], axis=1))
    m.ctx.encode([0, 3000, 6000], [3000] * 3)
    res = run_windows(m, options, prompts)
    counts = [len(r.tokens) for r in res]
    print(f"micro {dtype} beam {beam}: token counts {counts}")
    assert counts == [o.n_ctx + 1 - 227, 224, 224] and counts[0] < 224
    for w, (r, a) in enumerate(zip(res, want)):
        np.testing.assert_array_equal(np.asarray(r.tokens), np.asarray(a.tokens), err_msg=f"window {w}")
    assert len({tuple(r.tokens[:200]) for r in res}) == 3  # the prompts and the audio made the windows differ


# ------------------------------------------------------------------ 3. a first pass over two prefill() calls
SPLIT_INIT = (300, 300, 227, 300)


def prefill_rows(max_windows):
    """Rows of one prefill() call (wh_runtime.hip: PRE = max(PRE_ROWS, min(Wcap * 240, 8192)))."""
    return max(1024, min(max_windows * 240, 8192))


@functools.lru_cache(maxsize=None)
def _split_reference():
    """Per window (audio seeds alternate): initial tokens of SPLIT_INIT[w] ids, a 5-row
    trajectory until the longest window feeds position 447, and the oracle's top-32 at the
    <|startoftranscript|> row of the first pass (the no-speech row)."""
    import torch
    o = _long_oracle("micro")
    n_steps = o.n_ctx - max(SPLIT_INIT)
    out = []
    for w, n in enumerate(SPLIT_INIT):
        rng = np.random.default_rng([19, w, n])
        init = o.prompted(rng, n)
        assert len(init) == n
        om = o.audio(SEEDS[w % 2])
        traj = random_trajectory(om, init, MAX_GROUP, n_steps, rng)
        si = init.index(o.st.sot)
        lg, _, _ = om.decoder_forward(torch.tensor([init[:si + 1]]), 0, None)   # causal: the prefix suffices
        v, i = torch.topk(lg[0, -1], TOPK)
        out.append((init, traj, si, v.numpy(), i.numpy()))
    return out


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_pass_split_over_prefill_calls(dtype):
    m = _context("micro", dtype)
    ref = _split_reference()
    inits, trajs, sot_index = [r[0] for r in ref], [r[1] for r in ref], [r[2] for r in ref]
    n_win = len(inits)
    # teeth: the first pass does not fit one prefill() call, and no call can hold all four
    assert m.ctx.max_windows == n_win and sum(len(i) for i in inits) == 1127 > prefill_rows(m.ctx.max_windows)
    skipped = nondecisive(trajs, TAU[dtype])
    assert skipped <= NONDECISIVE_CAP, skipped
    _encode(m, "micro", n_win)
    rel, top1, two = teacher_force(m, trajs, inits, sot_index)
    assert rel.shape == (448 - 300 + 1, n_win * MAX_GROUP)
    sot_rel = np.asarray([np.abs(two[w, 0][ti] - tv).max() / (tv[0] - tv[-1]) for w, (_, _, _, tv, ti) in enumerate(ref)])
    per_win = rel.reshape(rel.shape[0], n_win, -1).max(axis=(0, 2))
    first = rel[0].reshape(n_win, -1).max(axis=1)
    buckets = context_buckets(rel, [len(i) for i in inits], MAX_GROUP)
    print(f"micro {dtype} split first pass {SPLIT_INIT}: per window max rel err {per_win.tolist()} (first pass "
          f"{first.tolist()}), sot row {sot_rel.tolist()}; per bucket {buckets}; top-1 agreement {top1.mean():.4f}")
    record_margin("longctx_split_prefill", model="micro", dtype=dtype, windows=n_win, init=list(SPLIT_INIT),
                  worst_rel_per_window=per_win.tolist(), first_pass_rel=first.tolist(), sot_row_rel=sot_rel.tolist(),
                  worst_rel_by_context=buckets, tau=TAU[dtype], frac_of_tau=float(per_win.max() / TAU[dtype]),
                  nondecisive=skipped)
    assert (per_win <= TAU[dtype]).all(), per_win
    assert (sot_rel <= TAU[dtype]).all(), sot_rel
    assert top1.all(), f"top-1 differs at {np.argwhere(~top1)[:5].tolist()} despite a decisive margin"


# ------------------------------------------------------------------ 4. stale cache content
SHORT_STEPS = 40


def _drive(m, init, n_steps, rng, keep):
    """Prefill of ``init`` at 1 x 5, then n_steps of uniform tokens and source rows drawn from
    ``rng``.  keep: returns [1 + n_steps][5][V] logits; otherwise the first pass's last row."""
    V = m.dims.n_vocab
    two = m.ctx.prefill([init], MAX_GROUP, [0])
    out = [np.repeat(two[:1, 1], MAX_GROUP, axis=0)]
    for s in range(n_steps):
        m.ctx.reorder_kv([int(x) for x in rng.integers(0, MAX_GROUP, MAX_GROUP)])
        lg = m.ctx.step([int(x) for x in rng.integers(0, V, MAX_GROUP)], text_offsets=[len(init) + s], logits=keep)
        if keep:
            out.append(lg.copy())
    return np.stack(out) if keep else out[0]


@gpu
@pytest.mark.parametrize("model,dtype", [(mo, d) for mo in ("micro", "base3") for d in DTYPES])
def test_stale_cache_content_does_not_matter(model, dtype):
    """Run A (the bare SOT sequence, 40 steps, 1 x 5), then two runs up to position 447: the
    227-token start of part 1 (first pass rows 0 to 226 in beam slot 0, steps in all five),
    and a bare-SOT start (steps from position 3 on in all five slots); then A again,
    bit-identical.  A kernel that gives weight to a key at or beyond its position, or of
    another slot, reads other cache content in the two A runs, in fp16 too."""
    from whisper.backend_hip import HipBackendError
    m = _context(model, dtype)
    o = _long_oracle(model)
    _encode(m, model, 1)
    first = _drive(m, o.sot, SHORT_STEPS, np.random.default_rng(29), keep=True)
    long_init = o.prompted(np.random.default_rng(31))
    l1 = _drive(m, long_init, o.n_ctx - len(long_init), np.random.default_rng(37), keep=False)
    l2 = _drive(m, o.sot, o.n_ctx - len(o.sot), np.random.default_rng(41), keep=False)
    # teeth: the runs in between were other runs (another first pass), to the end of the context
    assert len(long_init) == 227 and not np.array_equal(l1, first[0])
    with pytest.raises(HipBackendError, match="text context full"):
        m.ctx.step([0] * MAX_GROUP, text_offsets=[o.n_ctx])
    again = _drive(m, o.sot, SHORT_STEPS, np.random.default_rng(29), keep=True)
    assert np.array_equal(l2, first[0])     # the bare-SOT first pass after the 227-token one, too
    diff = np.abs(again - first)
    at = int(np.argmax(diff.max(axis=(1, 2)) > 0)) if diff.max() > 0 else -1
    print(f"{model} {dtype} stale cache: max |diff| {diff.max():.3e}, first differing pass {at}")
    record_margin("longctx_stale_cache", model=model, dtype=dtype, max_abs_diff=float(diff.max()), first_differing_pass=at)
    assert np.isfinite(first).all()
    assert np.array_equal(again, first), f"logits differ from pass {at} on, max |diff| {diff.max():.3e}"


# ------------------------------------------------------------------ 5. the harness, on the CPU
def test_recorder_replay_matches_full_prefix_at_full_context():
    """test_gpu_widths.test_trajectory_recorder_random_replay_matches_full_prefix from a
    227-token start to position 447, through random_trajectories' several windows per batch:
    at the last two steps the recorded top-32 equal a fresh decoder_forward over each row's
    whole prefix, rebuilt from (tok, src) alone."""
    import torch
    o = _long_oracle("micro")
    G = 5
    rngs = [np.random.default_rng([5, k]) for k in range(2)]
    inits = [o.prompted(rng) for rng in rngs]
    S = o.n_ctx - len(inits[0])
    om = o.audio(3)
    trajs = random_trajectories(om, inits, G, S, rngs)
    # a window of the batch is the window on its own: the same draws, the same logits
    alone_rng = np.random.default_rng([5, 1])
    assert o.prompted(alone_rng) == inits[1]
    alone = random_trajectory(om, inits[1], G, S, alone_rng)
    assert np.array_equal(alone["tok"], trajs[1]["tok"]) and np.array_equal(alone["src"], trajs[1]["src"])
    assert np.abs(alone["topv"] - trajs[1]["topv"]).max() <= TAU["fp32"] * (alone["topv"][..., 0] - alone["topv"][..., -1]).min()
    for init, t in zip(inits, trajs):
        assert len(init) == 227 and t["tok"].shape == (S + 1, G) and t["src"].shape == (S, G) and S == 221
        assert (t["src"].max(), t["src"].min()) == (G - 1, 0)
        prefix = [list(init) for _ in range(G)]
        for s in range(1, S + 1):
            prefix = [prefix[int(t["src"][s - 1, r])] + [int(t["tok"][s, r])] for r in range(G)]
            if s in (S - 1, S):
                assert len({tuple(p) for p in prefix}) > 1 and len(prefix[0]) == 227 + s
                full, _, _ = om.decoder_forward(torch.tensor(prefix), 0, None)
                for r in range(G):
                    topv, topi = t["topv"][s, r], t["topi"][s, r]
                    rel = np.abs(full[r, -1].numpy()[topi] - topv).max() / (topv[0] - topv[-1])
                    assert rel <= TAU["fp32"], (s, r, rel)
        assert len(prefix[0]) == o.n_ctx


def test_teacher_force_offsets_and_buckets():
    """teacher_force on a scripted context: per-window initial tokens reach wh_prefill as
    they are, every wh_step carries each window's own offset, rows are scored against their
    own window, and context_buckets files pass s of window w under n_init[w] - 1 + s."""
    V, G, S = 64, 2, 5
    inits = [[7, 8, 9], [1, 2, 3, 4, 5, 6] * 21 + [11]]             # 3 and 127 tokens
    rng = np.random.default_rng(0)
    trajs = []
    for init in inits:
        logits = rng.standard_normal((S, G, V)).astype(np.float32)
        logits[0, 1] = logits[0, 0]
        topi = np.argsort(-logits, axis=-1)[..., :TOPK]
        tok = rng.integers(0, V, (S, G))
        tok[0] = init[-1]
        trajs.append(dict(tok=tok, topi=topi, topv=np.take_along_axis(logits, topi, -1), src=rng.integers(0, G, (S - 1, G)),
                          logits=logits))

    class Ctx:
        calls = []

        def prefill(self, init_tokens, group, sot_index):
            self.calls.append(("prefill", [list(i) for i in init_tokens], group, list(sot_index)))
            self.s = 0
            return np.stack([np.stack([t["logits"][0, 0] * 0, t["logits"][0, 0]]) for t in trajs])

        def reorder_kv(self, src):
            self.calls.append(("reorder", list(src)))

        def step(self, tokens, text_offsets):
            self.s += 1
            self.calls.append(("step", list(tokens), list(text_offsets)))
            lg = np.concatenate([t["logits"][self.s] for t in trajs])
            if self.s == 3:
                lg = lg.copy()
                lg[G + 1, trajs[1]["topi"][3, 1, 4]] -= 0.5            # window 1, row 1, pass 3
            return lg

    class M:
        dtype, ctx = "fp32", Ctx()

    rel, top1, two = teacher_force(M, trajs, inits, [0, 5])
    calls = M.ctx.calls
    assert calls[0] == ("prefill", inits, G, [0, 5]) and two.shape == (2, 2, V)
    assert [c[2] for c in calls if c[0] == "step"] == [[3 + s, 127 + s] for s in range(S - 1)]
    assert [c[1] for c in calls if c[0] == "step"] == [[int(x) for t in trajs for x in t["tok"][s]] for s in range(1, S)]
    assert [c[1] for c in calls if c[0] == "reorder"] == \
        [[w * G + int(x) for w, t in enumerate(trajs) for x in t["src"][s]] for s in range(S - 1)]
    want = np.zeros((S, 2 * G))
    tv = trajs[1]["topv"][3, 1]
    want[3, G + 1] = 0.5 / (tv[0] - tv[-1])
    np.testing.assert_allclose(rel, want, atol=1e-6)
    assert top1.all()
    b = context_buckets(rel, [3, 127], G)
    assert list(b) == ["0-63", "64-127", "128-191", "192-255", "256-319", "320-383", "384-447"]
    # window 0 passes at positions 2..6; window 1 at 126, 127 | 128, 129 (pass 3), 130
    assert b["0-63"] == 0.0 and b["64-127"] == 0.0 and b["128-191"] == pytest.approx(want[3, G + 1]) and b["192-255"] is None


@pytest.mark.parametrize("model", ["micro", "base3"])
def test_long_trajectories_are_decisive(model):
    """The top-1 check of part 1 skips at most NONDECISIVE_CAP of the (step, row) pairs of the
    very trajectories the GPU tests replay, at both TAUs (turbo1: asserted in the GPU test)."""
    shapes = [(n, g) for mo, n, g in SHAPES if mo == model]
    for n_win, group in shapes:
        inits, trajs = _windows(model, n_win, group)
        assert trajs[0]["tok"].shape == (448 - 227 + 1, group)
        for dtype in DTYPES:
            share = nondecisive(trajs, TAU[dtype])
            print(f"{model} {n_win} x {group} {dtype}: non-decisive {share:.4f}")
            assert share <= NONDECISIVE_CAP, (model, n_win, group, dtype, share)
    if model == "micro":
        share = nondecisive([r[1] for r in _split_reference()], TAU["fp16"])
        print(f"micro split first pass: non-decisive {share:.4f}")
        assert share <= NONDECISIVE_CAP


def test_fp32_bar_catches_one_misread_key():
    """The power of the fp32 bar, on the oracle: at context 447 the cached K / V row of one
    position p is overwritten with row p - 1 in every layer; the last step's top-32 must move
    by at least 10 TAU[fp32] of their range (measured 3.5e-3 to 8.3e-3 on this trajectory,
    2.3e-3 or more on others: 11x that floor)."""
    import torch
    o = _long_oracle("micro")
    om = o.audio(3)
    rng = np.random.default_rng([17, 3, 1, 0])
    toks = o.prompted(rng) + [int(t) for t in rng.integers(0, om.n_vocab, o.n_ctx - 227)]
    assert len(toks) == o.n_ctx
    _, cache, _ = om.decoder_forward(torch.tensor([toks[:-1]]), 0, None)
    clean, _, _ = om.decoder_forward(torch.tensor([toks[-1:]]), o.n_ctx - 1, cache)
    topv, topi = torch.topk(clean[0, -1], TOPK)
    span = float(topv[0] - topv[-1])
    for p in (1, 223, 300, 446):
        bad = [[c[0].clone(), c[1].clone()] for c in cache]
        for c in bad:
            c[0][:, p] = c[0][:, p - 1]
            c[1][:, p] = c[1][:, p - 1]
        lg, _, _ = om.decoder_forward(torch.tensor([toks[-1:]]), o.n_ctx - 1, bad)
        moved = float((lg[0, -1][topi] - topv).abs().max()) / span
        print(f"position {p} read from {p - 1}: top-32 move by {moved:.3e} of the range ({moved / TAU['fp32']:.0f} TAU)")
        assert moved >= 10 * TAU["fp32"], (p, moved)
