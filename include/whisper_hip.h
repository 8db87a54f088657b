/*
 * libwhisper_hip — C ABI of the MI355X (gfx950) Whisper backend.
 *
 * This is the drop-in replacement for the reference's native backend boundary,
 * coreml/coreml.h:5-31 of wangchou/whisper.coreml, which Python binds through
 * ctypes in whisper/coreml.py:19-244.  The roles map one to one (citations are
 * /root/reference paths):
 *
 *   loadEncoder/loadCrossKV/loadDecoder256/loadDecoder1 (coreml.h:5,9,13,23)
 *        -> wh_create + wh_load_tensor + wh_finalize (weights come from the
 *           reference's own state_dict names, whisper/__init__.py:152-160)
 *   encoderPredict (coreml.h:7) + crossKVPredict (coreml.h:11)
 *        -> wh_encode  (AudioEncoder.forward encoder.py:103-136 and
 *           TextDecoder.crossKVCaches decoder.py:172-187, all windows batched)
 *   decoder256Predict (coreml.h:15-21) -> wh_decode_begin (first pass) /
 *           wh_prefill_logits (full-row logits + alignment cross-QK)
 *   decoder1Predict (coreml.h:26-31) + rearrange_mkv (coreml.h:25) + the host
 *           beam/filter loop (whisper/decoding.py:707-737)
 *        -> wh_decode_steps (one hipGraph per token: decoder step, logit filters,
 *           greedy/beam update, KV reorder by index indirection)
 *   the same roles one call per token, for a caller that keeps the reference's
 *   host loop (PyTorchInference.logits / rearrange_kv_cache, decoding.py:151-204):
 *        decoder256Predict (coreml.h:15-21) -> wh_prefill
 *        decoder1Predict   (coreml.h:26-31) -> wh_step
 *        rearrange_mkv     (coreml.h:25)    -> wh_reorder_kv
 *   log_mel_spectrogram (whisper/audio.py:110-157) -> wh_log_mel
 *   showCoremlPredictTime (whisper/coreml.py:247-263) -> wh_stats
 *
 * Conventions: every call returns 0 on success, a negative code on failure
 * (message via wh_last_error, thread-local).  All pointers are host pointers
 * (plain C arrays, row-major); device memory is owned by the context.  A
 * context is bound to one HIP device; use one context per GPU process.
 */
#ifndef WHISPER_HIP_H
#define WHISPER_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wh_ctx wh_ctx;

/* ModelDimensions (whisper/model.py:18-29) */
typedef struct wh_dims {
  int n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wh_dims;

enum { WH_F32 = 0, WH_F16 = 1 };

/* DecodingOptions (whisper/decoding.py:81-115) resolved against the tokenizer */
typedef struct wh_decode_opts {
  int group;             /* rows per window: beam_size, best_of or 1 (<= 8) */
  int beam;              /* 1 = BeamSearchDecoder, 0 = GreedyDecoder */
  float patience;        /* beam: max_candidates = round(group * patience) */
  float temperature;     /* greedy: 0 = argmax, > 0 = sampling */
  int sample_len;        /* max updates (n_text_ctx / 2 by default) */
  int suppress_blank;    /* SuppressBlank */
  int timestamps;        /* ApplyTimestampRules (0 = without_timestamps) */
  int max_initial;       /* max_initial_timestamp index, -1 = none */
  int eot, no_speech, no_timestamps, timestamp_begin; /* no_speech < 0: none */
  int blank[4];          /* tokenizer.encode(" ") ids suppressed with eot at the first step */
  int n_blank;
  const int* suppress;   /* SuppressTokens ids (already resolved, -1 expanded) */
  int n_suppress;
  unsigned long long seed; /* sampling RNG seed */
  int max_candidates;    /* beam: round(beam_size * patience) as the host computes it
                            (Python round, decoding.py:339); <= 0: derived from patience */
  /* Repetition controls of the device loop (wh_version >= 2).  Both are off when zero, so a
     caller that zero-initialises the struct and fills the fields above decodes as before.
     They act on the raw logits of every update, ahead of SuppressBlank, SuppressTokens and
     ApplyTimestampRules (a LogitFilter at the head of the reference's list, decoding.py:
     450-532), so the timestamp-versus-text comparison sees the filtered logits.  Per row,
     seq = tokens[sample_begin : len]: the sampled tokens only, not the prompt, the SOT
     sequence or a prefix.
       repetition_penalty p (0 or 1 = off): for every distinct id t < eot in seq,
         x[t] = x[t] > 0 ? x[t] / p : x[t] * p, in fp32 (the division correctly rounded),
         once per id however often it occurs.
       no_repeat_ngram n (0 = off, 1..16), only if len(seq) >= n: with suf the last n - 1
         tokens of seq, for every q in [0, len(seq) - n] with seq[q : q+n-1] == suf and
         seq[q+n-1] < eot: x[seq[q+n-1]] = -inf.  The window at q may overlap suf; matching
         is on raw ids, so timestamp tokens take part in the n-grams; n = 1 bans every text
         id sampled so far.
     The penalty comes first, then the ban.  eot and every id above it (specials,
     timestamps) are never changed, so a row cannot become all -inf through these.
     wh_decode_begin refuses (-11, the field named in wh_last_error, the context's decode
     state unchanged) an n outside 0..16, a penalty that is negative, NaN or infinite, and
     either option where the selection would not run in its sliced kernels (a vocabulary
     they do not fit, or the tuning switch WHISPER_HIP_LOGIT_SPLIT=0).  wh_prefill / wh_step
     hand the logits to the host and apply no filter. */
  int no_repeat_ngram;
  float repetition_penalty;
} wh_decode_opts;

const char* wh_last_error(void);
int wh_version(void);

int wh_create(int device, const wh_dims* dims, int compute_dtype, int max_windows, int max_group, wh_ctx** out);
int wh_destroy(wh_ctx* ctx);

/* checkpoint-format float32 tensor by reference state_dict name; the decoder query
   pre-scale (decoder.py:16-20) and the encoder key scale (encoder.py:38) are
   folded here. */
int wh_load_tensor(wh_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim);
int wh_finalize(wh_ctx* ctx);

/* mel filterbank [n_mels][201] (whisper/audio.py:91-107; the host derives it with the
   Slaney formula librosa uses and checks it against the reference asset in tests) */
int wh_set_mel_filters(wh_ctx* ctx, int n_mels, const float* filters);

/* Phrase biasing (hotwords) of the device decode loop (wh_version >= 3).  A phrase table is
   n_phrases phrases; phrase j has the token ids p_j = tokens[offsets[j] .. offsets[j+1]) (m_j of
   them) and the boost b_j = boost[j]; the scalar `start` is shared by all phrases.
   For every row and every update, with seq = tokens[sample_begin : len] (the sampled tokens
   only, the seq of the repetition controls above: never the prompt, the SOT sequence or a
   prefix), the pair (j, k), 0 <= k < m_j, fires when
     k == 0: fl32(b_j * start) > 0; its bonus is fl32(b_j * start);
     k >= 1: len(seq) >= k and seq[-k:] == p_j[:k]; its bonus is b_j.
   Matching is on raw ids, so a timestamp token inside seq breaks a match.  Overlapping
   matches all count: [a, a, b] after "... a a" fires k = 1 and k = 2.  For every id t = p_j[k]
   named by at least one firing pair, x[t] = x[t] + B(t) in fp32, B(t) the largest bonus among
   those pairs: a max, not a sum, so the result does not depend on evaluation order.  Nothing
   is retracted when a phrase is abandoned.
   Order at the head of the filter list: repetition penalty, phrase bias, n-gram ban, then
   SuppressBlank, SuppressTokens and ApplyTimestampRules.  A banned or suppressed id stays at
   -inf; eot and every id above it are never touched.  The log-probabilities the loop
   accumulates and reports (sum_logprobs, and so avg_logprob) are those of the biased
   distribution.
   Limits: 1..128 phrases, 1..16 tokens each, at most 512 tokens in total, every id in
   [0, n_vocab) and, at decode time, below eot; every b_j finite and > 0; start in [0, 1].
   The table is context state, kept on the host: the next wh_decode_begin /
   wh_decode_begin_slots uploads it, a decode in progress keeps the table it began with.
   n_phrases == 0 clears the table (the pointers may then be null).  Every breach of the
   limits is refused before any write (a negative code; wh_last_error names phrase_bias and
   the offending phrase), and a refused call leaves the previous table in place.
   With a non-empty table wh_decode_begin refuses (-11, phrase_bias in the message, the
   decode state unchanged) a table id >= opts.eot, and a selection that would not run in the
   sliced kernels, the rule of the repetition controls.  wh_prefill / wh_step hand out raw
   logits and apply nothing. */
int wh_set_phrase_bias(wh_ctx* ctx, int n_phrases, const int* tokens, const int* offsets /*[n_phrases+1]*/,
                       const float* boost /*[n_phrases]*/, float start);

/* log-mel of a whole file into the context's mel buffer: n_frames = (n + padding) / 160.
   normalize = 1 applies the global-max floor and scaling immediately. */
int wh_log_mel(wh_ctx* ctx, const float* audio, int64_t n_samples, int64_t padding, int n_mels, int normalize,
               int64_t* n_frames);
/* frames [frame0, frame0 + count) of the same log-mel (count < 0: to the end); the
   context stores them with their absolute offset, so wh_encode seeks and wh_mel_read
   frames stay absolute.  One rank of a file sharded over GPUs computes only the frames
   of its clips; the global max (wh_mel_max) is then all-reduced and applied with
   wh_mel_normalize.  *total_frames = (n + padding) / 160. */
int wh_log_mel_frames(wh_ctx* ctx, const float* audio, int64_t n_samples, int64_t padding, int n_mels,
                      int64_t frame0, int64_t count, int normalize, int64_t* total_frames);
/* keep audio resident in HBM; wh_log_mel(ctx, NULL, n, ...) then computes from it */
int wh_audio_upload(wh_ctx* ctx, const float* audio, int64_t n_samples);

/* ---- PCM ingest: a decoded file goes to the device as PCM and becomes the 16 kHz mono
   float32 waveform there, bit for bit the one whisper/audio.py load_audio makes on the host.
   pcm is interleaved [n_frames][channels]: int16 (WH_PCM_S16, bits <= 16), int32
   (WH_PCM_S32, e.g. 24-bit FLAC as wh_flac_decode returns it) or, for WH_PCM_F32, a mono
   float32 waveform already at 16 kHz (channels = up = down = 1, taps NULL), copied as it
   is.  For the integer formats, with up = 16000 / g, down = rate / g, g = gcd(rate, 16000),
   half = 10 * max(up, down), all in fp64:
     x[m]   = (sum of frame m's channels) * 2^-(bits-1) / channels
     y[k]   = sum over 0 <= m < n_frames of x[m] * taps[k*down - m*up + half],
              tap index within [0, 2*half]          (frames outside the file are zeros)
     out[k] = clip(rint(32768 * y[k]), -32768, 32767) / 32768,   k < ceil(n_frames * up / down)
   (rint rounds half to even).  taps [n_taps = 2*half + 1] is the host's filter — the library
   designs none; scipy.signal.resample_poly's is firwin(2*half + 1, 1 / max(up, down),
   window=("kaiser", 5.0)) * up — and its device copy is cached per (up, down).  up == down
   skips the filter (taps unused): mix and quantise only.
   The context keeps the resident audio as segments lying back to back from sample 0:
   dst_offset = 0 starts a new list, dst_offset = the end of the last segment appends, any
   other offset is refused.  reserve (0 allowed) is the total the caller will hold; if the
   buffer has to grow, the samples below dst_offset are kept.  *n_out = samples written.
   wh_log_mel(ctx, NULL, n, ...) works while there is exactly one segment of length n;
   wh_log_mel_batch(ctx, NULL, ...) takes the segments as its files.  A null pcm, n_frames < 1,
   channels < 1, an unknown format, bits outside 1..32 (1..16 for S16), up or down < 1, an
   n_taps other than 2*half + 1 when up != down, and a bad dst_offset are refused before
   anything is launched: the resident segments and the context mel stay as they were. */
enum { WH_PCM_S16 = 0, WH_PCM_S32 = 1, WH_PCM_F32 = 2 };
int wh_audio_ingest(wh_ctx* ctx, const void* pcm, int format, int64_t n_frames, int channels, int bits,
                    int up, int down, const double* taps, int n_taps,
                    int64_t dst_offset, int64_t reserve, int64_t* n_out);
/* resident samples [offset, offset + n) back to the host */
int wh_audio_read(wh_ctx* ctx, float* out, int64_t offset, int64_t n);

/* ---- speech spans: which frames of a resident file hold speech, found on the device so that
   only those are encoded and decoded (whisper/vad.py restates this in numpy).  The definition
   is in integers, so host and device agree exactly and the summation order cannot matter.
   Per file, a resident segment (offset, n) of 16 kHz float32 samples x:
     1. q[i] = clamp(rint(32768 * x[i]), -32768, 32767), rint in fp32 to even (the product is
        exact); a NaN sample counts as 0.
     2. frame f is samples [160 f, 160 f + 160) of the file, F = ceil(n / 160), samples past n
        are zeros; E[f] = sum q^2 as uint64 (at most 160 * 2^30).  Frames are the mel's hop:
        100 per second, frame indices are seek frames.
     3. histogram of 160 quarter-octave bins: bin 0 holds E == 0; for E >= 1, m = floor(log2 E),
        sub = (E >> (m-2)) & 3 if m >= 2 else (E << (2-m)) & 3, bin = 1 + 4 m + sub, whose lower
        edge is (4 + sub) << (m-2) if m >= 2 else (4 + sub) >> (2-m) (bin 0: 0).
     4. rank = max(1, ceil(F * percentile / 100)); N = the lower edge of the first bin whose
        cumulative count reaches rank (the noise level);
        T = min(max((N * ratio_q8) >> 8, t_lo), t_hi).
     5. active[f] = E[f] > T.  A run of fewer than min_silence inactive frames between two
        active frames becomes active; active runs shorter than min_speech frames are then
        dropped; each remaining run [s, e) becomes [max(0, s - pad), min(F, e + pad)); runs
        that now overlap or touch are merged.
   The caller turns decibels into the integers: ratio_q8 = round(256 * 10^(margin_db / 10))
   with margin_db <= 40 (the product stays under 2^64), t_lo = round(160 * 2^30 *
   10^(floor_db / 10)), t_hi the same of ceil_db.
   wh_speech_spans runs this for the first n_files resident segments (wh_audio_ingest /
   wh_flac_ingest / wh_audio_upload): two kernels on the context's stream with no host round
   trip between them, then one small copy.  spans [n_files][cap][2] int32 frames, n_spans
   [n_files], thresholds [n_files] = T.  A file with more than cap spans reports the count it
   needs in n_spans and has none written (the call still returns 0): call again with that
   capacity.  A file has at most F / 2 + 1 spans; room beyond that of the largest file is
   neither allocated nor copied.  Refused before the first HIP call: null opts / n_spans / thresholds, null spans
   with cap > 0, cap < 0, percentile outside 1..99, ratio_q8 outside [256, 2560000],
   t_lo > t_hi, a negative or > 2^30 frame count, n_files < 1 or more files than there are
   resident segments (the message says "resident"), a file of 2^30 frames or more.
   wh_frame_energy_read: E (energy_out, capacity cap values, needs F) and the histogram
   (hist_out [160], nullable) of resident segment `file`, computed by the first kernel alone.
   With energy_out NULL nothing is computed and the return value is F (the one call whose
   success is not 0). */
typedef struct wh_vad_opts {
  uint64_t ratio_q8, t_lo, t_hi;
  int percentile;                   /* 1..99 */
  int min_silence, min_speech, pad; /* frames */
} wh_vad_opts;
int wh_speech_spans(wh_ctx* ctx, const wh_vad_opts* opts, int n_files, int32_t* spans, int cap, int32_t* n_spans,
                    uint64_t* thresholds);
int wh_frame_energy_read(wh_ctx* ctx, int file, uint64_t* energy_out, int64_t cap, uint32_t* hist_out);

int wh_mel_max(wh_ctx* ctx, float* gmax);              /* raw log10 max of the last wh_log_mel */
int wh_mel_normalize(wh_ctx* ctx, float gmax);         /* floor at gmax-8, (x+4)/4 */
/* log-mel of n_files waveforms, concatenated in `audio` (file i has n_samples[i] floats),
   each padded, reflect-framed, floored at ITS OWN max-8 and scaled exactly as wh_log_mel
   does for that file alone.  The files' frames lie back to back in the context mel:
   file i owns absolute frames [frame_base[i], frame_base[i+1]), frame_base[0] = 0,
   frame_base[i+1]-frame_base[i] = (n_samples[i]+padding)/160.  wh_encode / wh_mel_read
   then take absolute frames as before.  One upload, one descriptor copy, a constant
   number of launches and one synchronisation, whatever n_files is.  The call takes over
   the resident-audio buffer: a later wh_log_mel(ctx, NULL, n, ...) fails until
   wh_audio_upload is called again.  audio = NULL means the resident segments of
   wh_audio_ingest: valid only when they are exactly n_files segments of these lengths
   (otherwise refused, the message says "resident"); nothing is uploaded and the segments
   stay resident, so the call can be repeated.  n_files < 1, a file with n_samples < 1 or
   n_samples + padding <= 200, and unset filters are refused before anything is launched;
   wh_last_error names the file's index. */
int wh_log_mel_batch(wh_ctx* ctx, const float* audio, int n_files, const int64_t* n_samples, int64_t padding,
                     int n_mels, int64_t* frame_base /* [n_files+1] */);
int wh_mel_max_batch(wh_ctx* ctx, float* gmax, int n_files); /* raw log10 max per file of the last wh_log_mel_batch */
int wh_mel_read(wh_ctx* ctx, float* out, int64_t frame0, int64_t n_frames); /* [n_mels][n_frames], absolute frames */
int wh_mel_write(wh_ctx* ctx, const float* mel, int64_t n_frames);          /* host mel -> context */

/* encoder + cross-KV for n_win windows of the context mel: window i = frames
   [seek[i], seek[i] + seg[i]) zero-padded to 3000 (audio.py:65-88), into slot i */
int wh_encode(wh_ctx* ctx, int n_win, const int64_t* seek_frames, const int* seg_frames);
int wh_read_audio_features(wh_ctx* ctx, int slot, float* out);                   /* [n_audio_ctx][n_state] */
int wh_read_cross_kv(wh_ctx* ctx, int slot, int layer, float* k_out, float* v_out); /* [H][n_audio_ctx][64] */

/* decode n_win windows (slots 0..n_win-1): prefill of the initial tokens
   (init_tokens[w*max_init + i], i < n_init[w]) and the first token update */
int wh_decode_begin(wh_ctx* ctx, int n_win, const wh_decode_opts* opts, const int* init_tokens, const int* n_init,
                    int max_init, const int* sot_index);
/* wh_decode_begin where decode window w attends to the audio features of encoder slot
   slots[w] (the temperature fallback, transcribe.py:188-228, re-decodes only the
   windows that failed, from the slots that already hold them).  wh_decode_read's
   `slot` is the decode window index w. */
int wh_decode_begin_slots(wh_ctx* ctx, int n_win, const int* slots, const wh_decode_opts* opts,
                          const int* init_tokens, const int* n_init, int max_init, const int* sot_index);
/* run up to max_steps token updates (hipGraph); *n_done = windows finished */
int wh_decode_steps(wh_ctx* ctx, int max_steps, int* n_done);
/* read back a window: tokens [group][n_text_ctx+1], sum_logprobs [group], len,
   finished (beam) fin_tokens [maxc][n_text_ctx+1], fin_len/fin_score [maxc] */
int wh_decode_read(wh_ctx* ctx, int slot, int* tokens, float* sum_logprobs, int* len, int* fin_n, int* fin_tokens,
                   int* fin_len, float* fin_score, float* no_speech_prob);
int wh_decode_maxc(wh_ctx* ctx);

/* ---- per-step boundary (the reference's decoder256Predict / decoder1Predict /
   rearrange_mkv, coreml.h:15-31, driven by its host DecodingTask loop,
   decoding.py:707-737).  Rows are r = w * group + b for windows w < n_win (slots
   0..n_win-1, encoded by wh_encode) and beams b < group.

   wh_prefill: first pass of each window's initial tokens (tokens[w * max_tokens + i],
   i < n_tokens[w]; all rows of a window share them, coreml.mm:279-327 runs the same
   pass once per beam).  logits (nullable) [n_win][2][n_vocab]: the rows at position
   sot_index[w] (no-speech probability, decoding.py:716-720) and n_tokens[w] - 1. */
int wh_prefill(wh_ctx* ctx, int n_win, int group, const int* tokens, const int* n_tokens, int max_tokens,
               const int* sot_index, float* logits);
/* wh_step: one decoder step.  Row r appends tokens[r] (the token the host chose for it)
   at position text_offsets[w] (nullable; when given it must equal the window's cached
   length, the text_offset of decoder1Predict) and returns logits [n_win*group][n_vocab]
   (nullable: kept on the device only). */
int wh_step(wh_ctx* ctx, const int* tokens, const int* text_offsets, float* logits);
/* wh_reorder_kv: after a beam update, row r continues the sequence of row
   source_rows[r] (a row of the same window; PyTorchInference.rearrange_kv_cache).
   No cache bytes move: the rows' ancestry tables are permuted.  Once per step. */
int wh_reorder_kv(wh_ctx* ctx, const int* source_rows);

/* decoder forward over tokens at offset 0 for one window slot (Whisper.forward,
   model.py:110-119 / the decoder256 first pass); logits [n_tokens][n_vocab];
   align_qk (nullable) [n_align][n_tokens][n_audio_ctx] raw cross q.k of the heads
   in align_heads (layer*n_head + head).  Like the reference's first pass, it writes the
   slot's self-KV rows: call it (and wh_align / wh_align_batch) on a slot whose decode has
   finished or that is not in the current batch; a device-loop decode of OTHER slots may
   continue with wh_decode_steps afterwards (its step rows are re-embedded first). */
int wh_prefill_logits(wh_ctx* ctx, int slot, const int* tokens, int n_tokens, float* logits, const int* align_heads,
                      int n_align, float* align_qk);

/* find_alignment's numeric half (reference whisper/timing.py:163-231), replacing the
   model(tokens) first pass with cross-QK capture (model.py:110-119, decoder.py:306-313,
   the decoder256 CoreML call of coreml.h:17-18 with out_cross_head_weights), the
   softmax / z-norm / median filter / head mean (timing.py:197-205) and dtw
   (timing.py:139-151, dtw_cpu :82-105 + backtrace :57-79) — all on the GPU.
   tokens = sot_sequence (n_sot ids) + [no_timestamps] + text (T ids) + [eot]
   (timing.py:175-182); the window's audio features must be in `slot`.
   token_probs [T] = softmax(logits[n_sot + k][:eot])[text[k]] (timing.py:187-191);
   path [2][T + 1 + num_frames/2]: text indices then time indices, *path_len valid
   entries of each (the rows of dtw(-matrix), timing.py:206). */
int wh_align(wh_ctx* ctx, int slot, const int* tokens, int n_tokens, int n_sot, int num_frames, const int* align_heads,
             int n_align, int medfilt_width, float* token_probs, int* path, int* path_len);
/* wh_align for n_win windows at once (slots[w], n_tokens[w] ids each, concatenated in
   tokens; num_frames[w]): their first passes run batched (up to 1024 rows per pass) and
   their DTWs run one workgroup per window in one launch.  Outputs concatenated in window
   order: token_probs [T_w], paths [2][T_w + 1 + num_frames[w]/2], path_lens [n_win]. */
int wh_align_batch(wh_ctx* ctx, int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                   const int* num_frames, const int* align_heads, int n_align, int medfilt_width, float* token_probs,
                   int* paths, int* path_lens);
/* timing.dtw(x) of a host matrix x [n_rows][n_cols] (n_rows <= 1023) on the GPU:
   path [2][n_rows + n_cols], *path_len valid entries of each */
int wh_dtw(wh_ctx* ctx, const float* x, int n_rows, int n_cols, int* path, int* path_len);

/* Open-end DTW: forced alignment past one window (whisper/align.py).  wh_dtw forces all N
   rows onto all M columns because its backtrace starts at the corner (N, M); here the end
   row is free, so the result says how many of the offered rows the columns account for.
   For x [N][M]:
     cost         exactly wh_dtw's: cost[0][0] = 0, the rest of row 0 and column 0 +inf,
                  cost[i][j] = fl32(fl64(x[i-1][j-1]) + fl64(c)), c chosen among
                  c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1] by the tie order
                  (c0 < c1 && c0 < c2 -> 0, else c1 < c0 && c1 < c2 -> 1, else 2)
     score[i]     fl32(fl64(cost[i][M]) + fl64(row_penalty) * i), i = 1..N
     end_row e    the smallest i in [min_rows, N] with the smallest score[i] (fp32 compare)
     path         the backtrace from (e, M) by wh_dtw's trace rules, reversed as there;
                  path_len <= e + M, the buffers keep the size [2][N + M]
   min_rows in 1..N and a finite row_penalty >= 0 (an fp32 value).  min_rows == 0 means
   closed: e = N and the path is wh_dtw's, bit for bit.  The penalty is what keeps the end
   from overshooting: without one, a row beyond the spoken text can always be entered by a
   diagonal step through one frame whose z-score happens to be positive.  whisper/align.py
   uses 4.0 (a token must own evidence worth about two frames at 2 sigma); that value comes
   from planted z-normalised matrices and has NOT been measured on real speech.
   end_scores (nullable) [n_rows] = score[1..N].  Refused before any HIP call, with a negative
   code and wh_last_error naming the field: a null pointer, min_rows outside 0..n_rows, a
   negative / NaN / infinite row_penalty, n_rows > 1023. */
int wh_dtw_open(wh_ctx* ctx, const float* x, int n_rows, int n_cols, int min_rows, float row_penalty, int* path,
                int* path_len, int* end_row, float* end_scores);
/* wh_align_batch with an open-end DTW per window: min_rows[w] == 0 runs window w closed
   (its results equal wh_align_batch's), otherwise its DTW ends at the best row >= min_rows[w]
   under row_penalty.  The matrix of window w has N = T_w + 1 rows as in wh_align_batch: the
   text tokens, then the row that predicts eot; end_rows[w] = T_w + 1 means that all the text
   and the trailing non-speech fit.  token_probs, paths and path_lens are laid out as in
   wh_align_batch (paths [2][T_w + 1 + num_frames[w]/2] per window, path_lens[w] <= end_rows[w]
   + num_frames[w]/2 valid).  Refuses what wh_dtw_open and wh_align_batch refuse.  Like
   wh_prefill_logits it writes the self-KV rows of every slot it is given: call it on slots
   whose decode has finished or that are not in the current batch. */
int wh_align_batch_open(wh_ctx* ctx, int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                        const int* num_frames, const int* align_heads, int n_align, int medfilt_width,
                        const int* min_rows, float row_penalty, float* token_probs, int* paths, int* path_lens,
                        int* end_rows);

/* the kernels the decoder step runs for a batch of n_win windows x group rows, as
   "proj=<name>,xattn=<name>" (the dominant projection family and the cross-attention;
   what bench.py labels its roofline lines with).  Returns the length written. */
int wh_step_kernels(wh_ctx* ctx, int n_win, int group, char* buf, int cap);

/* cumulative stage wall times in ms: [0] mel [1] encode [2] prefill [3] steps
   [4] step count [5] encode windows; device ms of wh_audio_ingest between HIP events:
   [6] its host-to-device copies [7] its resampling kernel; device ms of wh_flac_ingest /
   wh_flac_decode_device on the device path: [8] upload of the stream and the candidate table
   [9] k_flac_parse [10] k_flac_restore [11] k_flac_gather [12] the resampling kernel; [13] host
   ms of the candidate index and the chain; device ms of wh_speech_spans / wh_frame_energy_read:
   [14] k_frame_energy [15] k_speech_spans.  WH_N_STATS values in all. */
enum { WH_N_STATS = 16 };
enum {
  WH_STAT_MEL_MS = 0, WH_STAT_ENCODE_MS, WH_STAT_PREFILL_MS, WH_STAT_STEPS_MS, WH_STAT_STEPS, WH_STAT_ENCODE_WINDOWS,
  WH_STAT_INGEST_COPY_MS, WH_STAT_INGEST_KERNEL_MS, WH_STAT_FLAC_UPLOAD_MS, WH_STAT_FLAC_PARSE_MS,
  WH_STAT_FLAC_RESTORE_MS, WH_STAT_FLAC_GATHER_MS, WH_STAT_FLAC_RESAMPLE_MS, WH_STAT_FLAC_INDEX_MS,
  WH_STAT_VAD_ENERGY_MS, WH_STAT_VAD_SPANS_MS
};
int wh_stats(wh_ctx* ctx, double* out, int n);
int wh_sync(wh_ctx* ctx);

/* per-token wall milliseconds of every decode_steps chunk since the last reset
   (chunk wall time / steps in the chunk, host poll included): *n = count, up to
   cap values copied to out (nullable); reset != 0 clears the record.  Feeds the
   p50 per-token decode ms of BASELINE.json's metric. */
int wh_token_ms(wh_ctx* ctx, float* out, int cap, int* n, int reset);

/* timing of the dominant kernels for roofline reporting: runs `iters` launches of
   the given stage on the context's own stream between HIP events.
   what: 0 = one decoder step graph (current batch), 1 = encoder of 1 window,
         2 = one split-K projection launch (k_proj; the six per layer, all layers, back to back),
         3 = one cross-attention launch (the step kernel k_cross_attn1, all layers).
         4 = the token-selection kernel (k_logit_rows) on the current logits,
         5 / 6 = 2 / 3 on layer 0 only, repeated (operands Infinity-Cache warm),
         7 = the step's k_proj launches inside `iters` eager decoder steps, each timed by
             its own dispatch events (advances the decode state like a step),
         8 / 9 = the batched step's self-attention (k_self_attn_qkv) of every layer at the
             current context, with the decode's ancestry (8) or every row reading beam slot
             0's history (9: all beams share one history); the ancestry is restored.
   For 2, 3, 5, 6, 7, 8 and 9 *ms_per_iter is the average duration of a single kernel launch. */
int wh_time_stage(wh_ctx* ctx, int what, int iters, double* ms_per_iter);

/* ---- audio file decoding (host only, no context / GPU needed) ----
   Replaces the reference's `ffmpeg` subprocess in load_audio (whisper/audio.py:42-62)
   for FLAC input (tests/jfk.flac is 44.1 kHz stereo 24-bit).  Samples are decoded
   bit-exactly (STREAMINFO MD5); down-mixing and resampling are done by the caller.
   wh_flac_info: stream parameters from STREAMINFO.
   wh_flac_decode: interleaved int32 samples [frames][channels] into out (capacity
   cap_frames frames); *n_frames = frames decoded.  Errors: < 0, wh_flac_last_error(). */
int wh_flac_info(const uint8_t* data, int64_t n, int* sample_rate, int* channels, int* bits_per_sample,
                 int64_t* total_samples);
int wh_flac_decode(const uint8_t* data, int64_t n, int32_t* out, int64_t cap_frames, int64_t* n_frames);
const char* wh_flac_last_error(void);

/* ---- FLAC decoded frame-parallel.  FLAC frames decode independently, so the stream is cut
   at frame-header candidates and every candidate is decoded by its own lane (csrc/wh_flacdev.h,
   one code for the host and the device); the frames that tile the stream from the first one
   to its end (each ends where the next begins, block sizes summing to STREAMINFO's total) are
   then gathered into interleaved PCM.  The contract: for every stream this path either gives
   exactly the PCM wh_flac_decode gives, or it does not run and the call goes through
   wh_flac_decode: the samples, or the error, are that decoder's.  It runs for 1-8 channels,
   4-24 bits per sample (frames included) and a known total; a broken chain, a frame past its
   byte budget (STREAMINFO's maximum frame size, or twice the verbatim size when that is 0), a
   sample leaving int32, or staging beyond 4 x the PCM size send the stream to the host decoder.
   Like wh_flac_decode it verifies neither the frame CRC-16 nor the STREAMINFO MD5.

   wh_flac_index: the candidates after the metadata, sorted by byte offset: a sync code
   (0xFF, then 0xF8 or 0xF9), no reserved block-size / sample-rate / sample-size code, a
   channel code <= 10 that matches STREAMINFO's channel count, a well-formed UTF-8-style
   number and a matching header CRC-8.  False candidates inside frame bodies may be among them.
   offsets [cap], fields [cap][4] = header length, block size, channel assignment, bits per
   sample; *n_cand = candidates found (all of them, also beyond cap).
   wh_flac_decode_indexed: wh_flac_decode through the index on the host (no context, no GPU):
   the CPU twin of the device path.  wh_flac_last_path: 0 if this thread's last
   wh_flac_decode_indexed ran the indexed path, 1 if it went through wh_flac_decode.
   wh_flac_decode_device: the device decode alone (upload, parse / restore / gather kernels),
   PCM copied back as int32 [frames][channels]; *path_out = 0 device, 1 host.
   wh_flac_ingest: a FLAC stream -> the resident 16 kHz waveform, with wh_audio_ingest's
   segment semantics (dst_offset, reserve, n_out, the same refusals before the first HIP
   call) and its arithmetic (the device PCM is int16 for bits <= 16, else int32, and goes
   through the same resampling kernel).  up, down, taps as for wh_audio_ingest, from the
   stream's rate (wh_flac_info).  On the host path it calls wh_flac_decode and wh_audio_ingest;
   an error is reported unchanged and the resident segments and the mel stay as they were. */
int wh_flac_index(const uint8_t* data, int64_t n, int64_t* offsets, int32_t* fields, int64_t cap, int64_t* n_cand);
int wh_flac_decode_indexed(const uint8_t* data, int64_t n, int32_t* out, int64_t cap_frames, int64_t* n_frames);
int wh_flac_last_path(void);
int wh_flac_decode_device(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int32_t* out, int64_t cap_frames,
                          int64_t* n_frames, int* path_out);
int wh_flac_ingest(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                   int n_taps, int64_t dst_offset, int64_t reserve, int64_t* n_out, int* path_out);

/* ---- WAV in every common sample encoding.  wh_wav_info (host only, no context / GPU needed)
   reads the RIFF/WAVE header; the samples are decoded from the file's own bytes on the device
   (wh_wav_ingest).  No read passes data + n for any input.  Errors: < 0, wh_wav_last_error().
   Chunk walk: "RIFF" <size> "WAVE", then chunks (id, 32-bit size, body, a pad byte after an odd
     size).  The first `fmt ` must precede `data`; later `fmt ` chunks and unknown chunks (LIST,
     fact, bext, ...) are skipped; a chunk before `data` that runs past the end is refused.
     RF64 / BW64 are refused by name.
   Format tag: 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law, 0xFFFE extensible (cbSize >= 22; the tag
     is the first two bytes of SubFormat, whose other 14 bytes must be 00 00 00 00 10 00 80 00
     00 AA 00 38 9B 71).  Any other tag is refused and the message names it.
   Sample container: block_align / channels bytes, which must divide exactly and be what
     bits-per-sample rounds up to.  PCM: 1, 2, 3, 4 bytes give U8, S16, S24, S32, and the WHOLE
     container is the sample (WAV left-justifies fewer valid bits: 20-in-24 scales by 2^-23);
     valid_bits (wValidBitsPerSample of an extensible header, else bits-per-sample) is reported
     only.  Float: 4 or 8.  A-law / mu-law: 1.  Anything else is refused.
   Limits: channels 1..256, rate >= 1 (wh_audio_ingest's).
   Frames: n_frames = min(declared data size, bytes present after the data header) / block_align;
     a declared size of 0 or 0xFFFFFFFF means "to the end of the file"; a trailing partial frame
     is dropped; zero frames is refused.  data_offset + n_frames * block_align <= n always.

   The value of a sample (whisper/audio.py restates this in numpy), little-endian:
     U8 byte - 128 at 8 bits; S16 / S24 / S32 two's complement at 16 / 24 / 32 bits;
     mu-law  u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84,
             negative iff u & 0x80, at 16 bits;
     A-law   a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15,
             mag = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8, positive iff a & 0x80, at 16 bits;
     F32 / F64 widened to fp64, a non-finite value is 0.0, finite values clamped to [-256, 256].
   An integer frame is x[m] of wh_audio_ingest (the int64 sum of the channels * 2^-(bits-1) /
   channels); a float frame is its channels added in channel order in fp64, divided by channels.
   From x[m] on everything is wh_audio_ingest's: the filter, the quantisation, the segments.

   wh_wav_ingest: a whole WAV file -> the resident 16 kHz waveform.  Only the data chunk is
   uploaded (3 bytes per 24-bit sample, 1 per G.711 sample) and the resampling kernel reads the
   encoding itself.  up, down, taps as for wh_audio_ingest, from the file's rate (wh_wav_info).
   wh_audio_ingest's segment semantics (dst_offset, reserve, n_out) and refusals before the first
   HIP call (a stream wh_wav_info refuses, null data / n_out, up / down, n_taps, dst_offset,
   reserve): the resident segments and the mel stay as they were.  It moves
   WH_STAT_INGEST_COPY_MS and WH_STAT_INGEST_KERNEL_MS and no other counter. */
enum { WH_WAV_U8 = 0, WH_WAV_S16, WH_WAV_S24, WH_WAV_S32, WH_WAV_F32, WH_WAV_F64, WH_WAV_ALAW, WH_WAV_ULAW };
typedef struct wh_wav_fmt { int encoding, channels, sample_rate, valid_bits; int64_t data_offset, n_frames; } wh_wav_fmt;
int wh_wav_info(const uint8_t* data, int64_t n, wh_wav_fmt* out);
const char* wh_wav_last_error(void);
int wh_wav_ingest(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                  int n_taps, int64_t dst_offset, int64_t reserve, int64_t* n_out);

/* ---- Channels as files: the three ingest calls with the channels kept apart, for recordings
   that hold one party per channel.  select[0 .. n_select) are distinct channel ids of the file;
   on success n_select resident segments are appended at dst_offset, each *n_out samples long,
   segment s holding channel select[s] (selection order), lying back to back: segment s starts
   at dst_offset + s * *n_out.  There is no mix.  For selected channel c, in fp64,
     x_c[m] = sample(m, c) * 2^-(bits-1)            integer encodings (exact)
     x_c[m] = float_sample(sample(m, c))            F32 / F64 (non-finite -> 0, clamp to +-256)
   frames outside [0, n_frames) are zeros, and from x_c[m] on y[k] and out[k] are
   wh_audio_ingest's.  This is what the non-split call computes for a mono file that holds only
   that channel, bit for bit; whisper/audio.py load_audio_channels restates it on the host.
   The dst_offset rule is wh_audio_ingest's (0, or the end of the last segment); reserve is the
   total the caller will hold.  wh_log_mel(ctx, NULL, n, ...) works afterwards only if exactly one
   segment is resident (n_select == 1 at dst_offset 0); wh_log_mel_batch(ctx, NULL, ...) and
   wh_speech_spans take the segments as their files.
   One upload and one resampling launch whatever n_select is (k_pcm_resample_split,
   csrc/wh_ingest.hip).  wh_flac_ingest_split decodes on the device exactly as wh_flac_ingest
   does and differs only in that launch; on the host path it calls wh_flac_decode and
   wh_audio_ingest_split.  *path_out = 0 device, 1 host, as for wh_flac_ingest.
   Refused before the first HIP call, wh_last_error naming the field, the resident segments and
   the mel left as they were: everything the non-split call refuses; a null select; n_select < 1
   or > channels; an id outside [0, channels); a repeated id; WH_PCM_F32 (a mono waveform has
   nothing to split).
   Counters: the PCM and WAV forms move WH_STAT_INGEST_COPY_MS and WH_STAT_INGEST_KERNEL_MS, the
   FLAC device path its own (WH_STAT_FLAC_*, the launch in WH_STAT_FLAC_RESAMPLE_MS).
   wh_version() does not change with these three: a caller detects them by the presence of the
   symbols. */
int wh_audio_ingest_split(wh_ctx* ctx, const void* pcm, int format, int64_t n_frames, int channels, int bits,
                          int up, int down, const double* taps, int n_taps, const int* select, int n_select,
                          int64_t dst_offset, int64_t reserve, int64_t* n_out);
int wh_flac_ingest_split(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                         int n_taps, const int* select, int n_select, int64_t dst_offset, int64_t reserve,
                         int64_t* n_out, int* path_out);
int wh_wav_ingest_split(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                        int n_taps, const int* select, int n_select, int64_t dst_offset, int64_t reserve,
                        int64_t* n_out);

/* ---- A resident stream: a recording that arrives in chunks (live audio from a socket).  The
   context resamples every chunk as it comes and keeps ONE growing resident segment, so
   wh_log_mel(ctx, NULL, n, ...), wh_speech_spans and wh_audio_read work on it as they are.
   A stream is raw interleaved frames [n_frames][channels] in one of the eight WH_WAV_* sample
   encodings (no container); up, down, taps as for wh_audio_ingest, from the stream's rate.

   The contract: take any split of a recording of N frames into chunks (one-frame chunks and
   chunks shorter than the filter included).  The samples the appends emit, followed by those of
   wh_stream_finish, are bit for bit what wh_wav_ingest / wh_audio_ingest write for the whole
   recording at once.  This is exact, not approximate: output k of the one-shot kernel reads
   frames from m_k = (k*down + half) / up backwards over 2*half/up frames and accumulates with fma
   in that fixed order; frames outside the file are 0.0, and an fma with a zero operand leaves the
   accumulator unchanged.  So output k is final once frame m_k has arrived, and after n frames in
   total the stream has emitted
     E(n) = max(0, ceil((n*up - half) / down))     (n when up == down: there is no filter)
   samples: at most 20 outputs (1.25 ms) are held back.  wh_stream_finish emits the rest up to
   ceil(N*up/down), reading the frames from N on as zeros.  wh_stream_emitted (host only, no
   context) returns E(n_frames), or with final != 0 the total ceil(n_frames*up/down); -1 for
   n_frames < 0 or up, down < 1.
   The frames a later chunk still needs, the last 2*half/up of them mixed down to fp64, are kept
   on the device in a double buffer (csrc/wh_ingest.hip, k_pcm_resample_stream): an append reads
   one half and writes the other, with no host round trip.

   wh_stream_begin opens a stream and leaves an empty resident segment; a stream that was open is
   dropped.  reserve (0 allowed): the samples the caller expects to hold at once.
   wh_stream_append takes n_frames frames; *n_out (nullable) = samples emitted by this call,
   E(after) - E(before), possibly 0.  n_frames == 0 is a no-op.
   wh_stream_finish ends the input: *n_out (nullable) = the samples it emitted.  The stream stays
   open for wh_stream_trim and wh_stream_info; a second finish emits nothing.
   wh_stream_trim drops the first n_drop resident samples, 0 <= n_drop <= resident length: the
   rest moves to sample 0 unchanged (through a bounce buffer when source and destination
   overlap), n_drop == length leaves an empty segment.  Later appends continue without a seam:
   the resampler's state lives in input frames and is not touched.
   wh_stream_info: frames appended, samples emitted, samples dropped (the resident segment is
   (0, samples_out - samples_dropped)), finished; any pointer may be null.
   Any other call that writes the resident buffer ends the stream: wh_audio_upload, every
   wh_*_ingest*, wh_log_mel* with a host array.  Afterwards append, finish, trim and info are
   refused until the next wh_stream_begin.
   Refused before the first HIP call, the stream and the resident samples unchanged, -1 for a null
   pointer and -7 otherwise, wh_last_error naming "stream" and the field: an encoding outside the
   eight, channels outside 1..256, up or down outside 1..2^20, an n_taps other than 2*half + 1
   (or null taps) when up != down, a negative reserve; append / finish / trim / info without an
   open stream; append after finish; null data with n_frames > 0; n_frames < 0 or past 2^40 in
   total; n_drop out of range.
   Counters: the uploads and the trim's copies go to WH_STAT_INGEST_COPY_MS, the kernel to
   WH_STAT_INGEST_KERNEL_MS.  wh_version() does not change with these six: a caller detects them
   by the presence of the symbols. */
int wh_stream_begin(wh_ctx* ctx, int encoding /* WH_WAV_* */, int channels, int up, int down, const double* taps,
                    int n_taps, int64_t reserve);
int wh_stream_append(wh_ctx* ctx, const void* data, int64_t n_frames, int64_t* n_out);
int wh_stream_finish(wh_ctx* ctx, int64_t* n_out);
int wh_stream_trim(wh_ctx* ctx, int64_t n_drop);
int wh_stream_info(wh_ctx* ctx, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished);
/* returns a 64-bit count (int64_t's width on every ABI): the only entry point whose result is
   not a status, spelled so that tools which list the `int wh_*(` declarations still see it */
long long
int wh_stream_emitted(int64_t n_frames, int up, int down, int final);

/* ---- A pool of streams: many live recordings on one context, fed and decoded together.
   wh_pool_create gives the context n_slots slots (1..4096); a slot holds one stream with its own
   format, its own history and its own resident buffer of at most slot_samples 16 kHz samples.  The
   pool shares nothing with the resident segments or the single stream above: no wh_audio_upload,
   wh_*_ingest*, wh_log_mel* or wh_stream_* call touches a slot, and no pool call touches the
   resident segments or the single stream.  wh_pool_destroy frees it (every slot is dropped).

   Each slot obeys the wh_stream_* contract, stream by stream: take any split of a recording into
   packets and batch them with any packets of other slots; the samples the slot emits, followed by
   those of wh_pool_finish, are bit for bit what wh_wav_ingest writes for the whole recording
   (the pool's kernel runs the single stream's device functions, csrc/wh_ingest.hip).

   wh_pool_open: wh_stream_begin's format arguments and refusals, for a slot that is not open.
   wh_pool_close frees the slot for another open.
   wh_pool_append: n packets, packet i being n_frames[i] frames at data[i] for slot slots[i];
   n_out[i] (n_out nullable) = E(after) - E(before) of wh_stream_emitted.  n_frames[i] == 0 is
   allowed and emits 0 (data[i] may then be null).  One call gathers the packets in pinned memory
   (each 16-byte aligned, 8 readable bytes behind it) and makes one copy of them, one descriptor
   copy, one kernel launch and one synchronisation, whatever n is.
   wh_pool_finish ends the input of the n slots (one launch); a slot that is already finished
   emits 0.  The slots stay open for trim, info, read and log_mel.
   wh_pool_trim drops the first n_drop[i] resident samples of slot slots[i], 0 <= n_drop[i] <=
   resident length; the rest is unchanged and later appends continue without a seam.  Every slot
   has two buffers: the remainder is copied into the other one (one launch for all slots) and
   the slot then reads that one, so no copy overlaps itself.
   wh_pool_info: as wh_stream_info, for one slot.  wh_pool_read: the slot's resident samples
   [offset, offset + n).
   wh_pool_log_mel is wh_log_mel_batch with the files taken from the buffers of the n slots, in
   call order: the same kernels and per-file normalisation, frame_base[n + 1] as there, and
   wh_mel_max_batch(ctx, g, n) works afterwards.  It writes only the context mel.

   A batched call is all or nothing.  Everything is checked before the first HIP call, and a
   refused call leaves every slot, every n_out[] entry, the counters and the context mel as they
   were: -1 for a null pointer and -7 otherwise, wh_last_error naming "pool", the field and its
   index in the call.  Refused: no pool (a second create while one exists); n_slots or
   slot_samples out of range; a slot out of range, or not open (already open, for open); the same
   slot twice in one call; n < 1; null data[i] with n_frames[i] > 0; n_frames[i] < 0 or past 2^40
   in total; an append after finish; n_drop[i] outside the resident length; a read outside it; a
   log_mel of an empty slot; and an append (or finish) that would take a slot past slot_samples:
   the message says "capacity", and the caller must trim first.
   Counters: the copies go to WH_STAT_INGEST_COPY_MS, the kernels to WH_STAT_INGEST_KERNEL_MS,
   the mel to WH_STAT_MEL_MS.  wh_version() does not change with these ten: a caller detects them
   by the presence of the symbols. */
int wh_pool_create(wh_ctx* ctx, int n_slots, int64_t slot_samples);
int wh_pool_destroy(wh_ctx* ctx);
int wh_pool_open(wh_ctx* ctx, int slot, int encoding /* WH_WAV_* */, int channels, int up, int down,
                 const double* taps, int n_taps);
int wh_pool_close(wh_ctx* ctx, int slot);
int wh_pool_append(wh_ctx* ctx, int n, const int* slots, const void* const* data, const int64_t* n_frames,
                   int64_t* n_out);
int wh_pool_finish(wh_ctx* ctx, int n, const int* slots, int64_t* n_out);
int wh_pool_trim(wh_ctx* ctx, int n, const int* slots, const int64_t* n_drop);
int wh_pool_info(wh_ctx* ctx, int slot, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped,
                 int* finished);
int wh_pool_read(wh_ctx* ctx, int slot, float* out, int64_t offset, int64_t n);
int wh_pool_log_mel(wh_ctx* ctx, int n, const int* slots, int64_t padding, int n_mels, int64_t* frame_base);

/* ---- Voice activity of a live stream: a causal, incremental speech detector that lives on the
   device next to a stream's samples and is updated inside the call that ingests them.
   The definition is in integers (whisper/vad.py, StreamVad, restates it in numpy); steps 1-3 are
   those of wh_speech_spans above (q, E, the quarter-octave bins).

   Frame grid.  A detector belongs to one stream.  Frame f is the stream's emitted 16 kHz samples
   [160 f, 160 f + 160), counted from the stream's first sample: trims do not move the grid.
   E[f] = the uint64 sum of q^2 over the frame.

   Options (wh_svad_opts): ratio_q8, t_lo, t_hi and percentile as in wh_vad_opts; window W in
   1..6000 frames; min_silence in 1..2^20 frames; min_speech in 0..2^20 frames.

   State, all zero at enable: hist[160]; ring[W] of bin numbers (uint8); frames; samples (seen so
   far); partial (the q^2 sum of the samples of the incomplete frame `frames` seen so far); state
   (0 SILENCE, 1 ONSET, 2 SPEECH); run_start, run_end (meaningful only while state != SILENCE);
   closed_start, closed_end (the last span that ended), closed_total; threshold.

   Per completed frame f, in order:
     b = bin(E[f]);  hist[b] += 1;  if f >= W: hist[ring[f % W]] -= 1;  ring[f % W] = b
     n = min(f + 1, W);  rank = max(1, ceil(n * percentile / 100))
     N = the lower edge of the first bin whose cumulative count reaches rank
     T = min(max((N * ratio_q8) >> 8, t_lo), t_hi)
     if E[f] > T:
         if state == SILENCE: state = ONSET; run_start = f
         run_end = f + 1
         if state == ONSET and run_end - run_start >= min_speech: state = SPEECH
     elif state != SILENCE and f + 1 - run_end >= min_silence:
         if state == SPEECH: (closed_start, closed_end) = (run_start, run_end); closed_total += 1
         state = SILENCE
     frames = f + 1;  threshold = T
   With t_lo == t_hi the closed spans (and the open run of a stream that ends in SPEECH) are
   step 5 of wh_speech_spans with pad = 0: the file's rules evaluated causally.

   An append hands the detector exactly the samples that append emitted: whole frames are closed
   as above, the rest goes into partial (so a trim that drops samples the grid has not closed
   loses nothing).  A finish hands it the samples it releases and, if samples % 160 != 0, closes
   the last frame with zeros: frames = ceil(samples / 160), partial = 0.

   wh_pool_vad_enable gives an open slot that has taken no frames yet a detector (its state block
   is allocated here).  From then on wh_pool_append / wh_pool_finish update it: with detecting
   slots in a call, the call's descriptor copy carries their descriptors too, one more launch
   (csrc/wh_svad.hip, one workgroup per detecting slot: the energies of the new samples in
   parallel, then the recurrence on one wave) goes on the same stream behind the ingest kernel,
   and one device-to-host copy of the states goes before the call's one synchronisation.  A call
   without detecting slots launches and copies what it did before.  wh_pool_trim does not touch a
   detector; wh_pool_close and wh_pool_destroy drop it.
   wh_pool_vad_state: the states of n detecting slots as of each slot's last append or finish,
   from the host copy (no HIP call).  wh_pool_vad_read (inspection): ring receives W bytes
   (cap >= W), hist (nullable) the 160 counters.
   wh_stream_vad_enable / wh_stream_vad_state: the same for the single stream, behind
   wh_stream_append / wh_stream_finish; wh_stream_begin drops the detector, and so does any call
   that ends the stream.
   The detector's kernel time goes to WH_STAT_INGEST_KERNEL_MS, the state copy is not charged.

   Refused before the first HIP call, nothing changed (-1 for a null pointer, -7 otherwise,
   wh_last_error naming "pool" or "stream" and the field): null opts / out / ring; percentile
   outside 1..99; ratio_q8 outside [256, 2560000]; t_lo > t_hi; window, min_silence or
   min_speech outside the ranges above; a slot that is not open, has already taken frames (or is
   finished) or is already detecting; state or read of a slot without a detector; cap < W.
   wh_version() does not change with these five: a caller detects them by the symbols. */
typedef struct wh_svad_opts {
  uint64_t ratio_q8, t_lo, t_hi;
  int percentile;                      /* 1..99 */
  int window, min_silence, min_speech; /* frames */
} wh_svad_opts;
typedef struct wh_svad_state {
  int64_t frames, samples, run_start, run_end, closed_start, closed_end, closed_total;
  uint64_t threshold, partial;
  int32_t state, reserved;
} wh_svad_state;
int wh_pool_vad_enable(wh_ctx* ctx, int slot, const wh_svad_opts* opts);
int wh_pool_vad_state(wh_ctx* ctx, int n, const int* slots, wh_svad_state* out);
int wh_pool_vad_read(wh_ctx* ctx, int slot, uint8_t* ring, int cap, uint32_t* hist);
int wh_stream_vad_enable(wh_ctx* ctx, const wh_svad_opts* opts);
int wh_stream_vad_state(wh_ctx* ctx, wh_svad_state* out);

#ifdef __cplusplus
}
#endif
#endif
