"""The phrase bias of the device decode loop (include/whisper_hip.h, wh_set_phrase_bias)
restated in numpy, the wrapper that puts it into the oracle's filter list, and the phrase
tables the tests use.  Shared by test_phrase_bias_host.py and test_gpu_phrase_bias.py."""
import numpy as np


def apply_phrase_bias(x, tokens, sample_begin, eot, phrases, boosts, start):
    """In place on one row of raw fp32 logits ``x``; ``tokens`` is the row's whole history
    (initial tokens + sampled).  Returns how many continuation pairs (k >= 1) fired."""
    assert x.dtype == np.float32 and x.ndim == 1
    seq = [int(t) for t in tokens[sample_begin:]]
    best, fired = {}, 0  # id -> B(id), the largest bonus among the firing pairs that name it
    for p, b in zip(phrases, boosts):
        p, b = [int(t) for t in p], np.float32(b)
        b0 = np.float32(b * np.float32(start))  # fl32(b * start)
        if b0 > 0:
            best[p[0]] = max(best.get(p[0], np.float32(0)), b0)
        for k in range(1, len(p)):
            if len(seq) >= k and seq[len(seq) - k:] == p[:k]:
                best[p[k]] = max(best.get(p[k], np.float32(0)), b)
                fired += 1
    for t, bonus in best.items():
        if t < eot:  # eot and every id above it are never touched
            x[t] = x[t] + np.float32(bonus)  # one fp32 add
    return fired


class BiasedInference:
    """An Inference shaped like repeat_filter_ref.FilteredInference that applies the phrase
    bias to the last position's logits of every row of ``inner``'s answer.  The stated order
    is penalty, bias, ban: wrap a FilteredInference (``BiasedInference(FilteredInference(x))``).
    Its ban then runs before the bias instead of after it, which gives the same logits: the
    ban's targets come from the history alone, and -inf + bonus is -inf.  The other way round
    (the penalty after the bias) is not the definition.  Counts the continuation pairs that
    fired (``n_fired``)."""

    def __init__(self, inner, sample_begin, eot, phrases, boosts, start):
        self.inner, self.sample_begin, self.eot = inner, sample_begin, eot
        self.phrases, self.boosts, self.start = phrases, boosts, start
        self.n_fired = 0

    def logits(self, tokens, audio_features=None):
        out = self.inner.logits(tokens, audio_features)
        lg = out[0]
        if hasattr(lg, "detach"):
            lg = lg.detach().cpu().numpy()
        lg = np.array(lg, dtype=np.float32)  # a copy: the inner's buffer stays as it was
        tok = tokens.detach().cpu().numpy() if hasattr(tokens, "detach") else np.asarray(tokens)
        for r in range(tok.shape[0]):
            self.n_fired += apply_phrase_bias(lg[r, -1], tok[r], self.sample_begin, self.eot, self.phrases,
                                              self.boosts, self.start)
        return (lg,) + tuple(out[1:])

    def rearrange_kv_cache(self, source_indices):
        self.inner.rearrange_kv_cache(source_indices)

    def cleanup_caching(self):
        if hasattr(self.inner, "cleanup_caching"):
            self.inner.cleanup_caching()


def text_tokens(tokens, eot):
    return [int(t) for t in tokens if int(t) < eot]


def is_cycle(text, phrase):
    """``text`` is ``phrase`` repeated cyclically from its first token."""
    return len(text) > 0 and all(t == phrase[i % len(phrase)] for i, t in enumerate(text))


# ---------------------------------------------------------------- the tables of the tests
# The forced cycle: one phrase of 16 distinct ids over the vocabulary: id 0, eot - 1 (50256),
# the two sides of the first boundary of the 32-slice selection (1624 | 1625), none in the
# default suppress list.  With boost 40 and start 0.5 the next phrase token gets +40 and the
# phrase head +20 against micro logits that span less than 11, so the text is the phrase,
# cyclically.  (start 1.0 would not force it: after p[0] the k = 0 and k = 1 bonuses tie.)
FORCED = (0, 1624, 1625, 3000, 5000, 8000, 11000, 15000, 20000, 25000, 30000, 35000, 40000, 45000, 50000, 50256)
FORCED_BOOST, FORCED_START = 40.0, 0.5

# A moderate table for the micro model, whose unbiased output has two distinct text ids
# (10496 and 22373): heads from those, tails from elsewhere, chosen on the CPU oracle so that
# in every case of the parity test continuation bonuses fire and the tokens change.
MODERATE = (((10496, 300, 400, 500), (22373, 5000), (400, 777), (1624, 1625), (500, 1625, 50256)),
            (14.0, 10.0, 8.0, 3.0, 12.0), 0.1)
# The same entry count (13) as MODERATE, other ids: replays MODERATE's captured step graph.
MODERATE_B = (((10496, 600, 700, 800), (22373, 6000), (700, 888), (1623, 1626), (800, 1626, 50255)),
              (14.0, 10.0, 8.0, 3.0, 12.0), 0.1)

# The max rule and the overlapping phrase on the device: after "... 10496" id 300 is named by
# k = 1 of the first two phrases (a shared prefix; B = 8, a sum would give 16), and after
# "... 10496 10496" the third phrase fires k = 1 and k = 2.  On the CPU oracle a summing
# restatement moves avg_logprob by 0.25 (greedy and beam 5) and changes the beam's tokens, far
# past the parity bound of 1e-4; start 0, so only continuations act.
MAX_RULE = (((10496, 300), (10496, 300, 400), (10496, 10496, 777)), (8.0, 8.0, 12.0), 0.0)
