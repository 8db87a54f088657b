"""The repetition filter of the device decode loop (include/whisper_hip.h, wh_decode_opts:
no_repeat_ngram / repetition_penalty) restated in numpy, and the wrapper that puts it at the
head of the oracle's filter list.  Shared by test_repeat_filter_host.py and
test_gpu_repeat_filter.py."""
import numpy as np


def apply_repeat_filter(x, tokens, sample_begin, eot, n=0, p=1.0):
    """In place on one row of raw fp32 logits ``x``; ``tokens`` is the row's whole history
    (initial tokens + sampled).  Returns (ids penalised, ids banned)."""
    assert x.dtype == np.float32 and x.ndim == 1
    seq = [int(t) for t in tokens[sample_begin:]]
    penalised, banned = [], []
    if p not in (0.0, 1.0):
        pf = np.float32(p)
        for t in sorted(set(seq)):
            if t < eot:
                # fp32 arithmetic, the division correctly rounded (numpy float32 / float32)
                x[t] = x[t] / pf if x[t] > 0 else x[t] * pf
                penalised.append(t)
    if n > 0 and len(seq) >= n:
        suf = seq[len(seq) - (n - 1):] if n > 1 else []
        for q in range(0, len(seq) - n + 1):
            if seq[q:q + n - 1] == suf and seq[q + n - 1] < eot:
                x[seq[q + n - 1]] = -np.inf
                banned.append(seq[q + n - 1])
    return penalised, sorted(set(banned))


def repeats(seq, n, eot):
    """The invariant of no_repeat_ngram n on a sampled sequence: every (i, j), i < j, with
    seq[i:i+n] == seq[j:j+n] whose last token is a text id (< eot).  Empty when it holds."""
    seq = [int(t) for t in seq]
    first, bad = {}, []
    for j in range(len(seq) - n + 1):
        g = tuple(seq[j:j + n])
        if g in first:
            if g[-1] < eot:
                bad.append((first[g], j))
        else:
            first[g] = j
    return bad


class FilteredInference:
    """An Inference (``logits`` / ``rearrange_kv_cache``, reference decoding.py:127-204)
    that applies the filter to the last position's logits of every row of ``inner``'s
    answer: ``oracle.ref_whisper.decode`` hands the full ``tokens`` to ``logits`` at every
    step and applies its own filters afterwards, so this is a LogitFilter at the head of
    the list.  Counts what it did (``n_penalised``, ``n_banned``)."""

    def __init__(self, inner, sample_begin, eot, n=0, p=1.0):
        self.inner, self.sample_begin, self.eot, self.n, self.p = inner, sample_begin, eot, n, p
        self.n_penalised = self.n_banned = 0

    def logits(self, tokens, audio_features=None):
        out = self.inner.logits(tokens, audio_features)
        lg = out[0]
        if hasattr(lg, "detach"):
            lg = lg.detach().cpu().numpy()
        lg = np.array(lg, dtype=np.float32)  # a copy: the inner's buffer stays as it was
        tok = tokens.detach().cpu().numpy() if hasattr(tokens, "detach") else np.asarray(tokens)
        for k in range(tok.shape[0]):
            row = lg[k, -1]
            pen, ban = apply_repeat_filter(row, tok[k], self.sample_begin, self.eot, self.n, self.p)
            self.n_penalised += len(pen)
            self.n_banned += len(ban)
        return (lg,) + tuple(out[1:])

    def rearrange_kv_cache(self, source_indices):
        self.inner.rearrange_kv_cache(source_indices)

    def cleanup_caching(self):
        if hasattr(self.inner, "cleanup_caching"):
            self.inner.cleanup_caching()


class OracleInference:
    """The CPU oracle's decoder (OracleWhisper.decoder_forward with its KV cache) behind the
    Inference interface, for the host tests."""

    def __init__(self, model):
        self.model, self.cache, self.offset = model, None, 0

    def logits(self, tokens, audio_features=None):
        inp = tokens if self.cache is None else tokens[:, -1:]
        lg, self.cache, _ = self.model.decoder_forward(inp, self.offset, self.cache)
        self.offset += inp.shape[1]
        return lg, None

    def rearrange_kv_cache(self, source_indices):
        src = list(source_indices)
        self.cache = [[c[0][src], c[1][src]] for c in self.cache]
