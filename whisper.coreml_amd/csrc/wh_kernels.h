// Kernel launch declarations for libwhisper_hip.
#pragma once
#include "wh_common.h"

namespace wh {

constexpr int TKP = 1536;  // cross-KV keys per (window, head) block: 1500 padded to whole 64-key tiles
// cross-V (V^T) is tile-major: xv_index (wh_common.h)

template <typename T>
void launch_layernorm(const float* x, T* y, const float* g, const float* b, int rows, int n, float eps,
                      const int* rows_in, hipStream_t st);
// Split-K slabs of the decoder-step projections (k_proj EPI_PARTIAL) are fp32, or fp16 in
// fp16 contexts (GemmArgs::slab_half): `part` then points at half_t
// elements and slab_half is 1.  Strides count elements.
template <typename T>
void launch_resid_ln(float* x, const float* part, int nsplit, int64_t part_stride, const float* bias, T* y,
                     const float* g, const float* b, int rows, int n, float eps, hipStream_t st, int slab_half = 0);
template <typename T>
void launch_attn_enc(const T* qkv, int ld, int ns, int H, int Tlen, int nwin, int64_t wsi, const T* vt, int tkp, T* out,
                     int64_t wso, hipStream_t st);
template <typename T>
void launch_self_attn(const T* q, int ldq, const T* kc, const T* vc, const int* rw, const int* rs, const int* rp,
                      const int* anc, int anc_beams, int nbeam, int H, int ctx, T* out, int ldo, int rows,
                      hipStream_t st);
template <typename T>
int launch_self_attn_qkv(const float* part, int nsplit, int64_t part_stride, const float* bqkv, int ns, T* kc, T* vc,
                          const int* rw, const int* rs, const int* rp, const int* anc, int anc_beams, int nbeam, int H,
                          int ctx, T* out, int ldo, int rows, hipStream_t st, int slab_half = 0);
template <typename T>
void launch_reduce_store(const float* part, int nsplit, int64_t part_stride, const float* bias, T* out, int ldo, int M,
                         int N, int gelu, hipStream_t st, int slab_half = 0);
// decoder-step query given as split-K slabs: q = bias + sum_z part[z*stride + row*ldq + c]
// (part == nullptr: q is a T matrix); needs <= 16 rows per window and z in {4, 8, 10}
// (cross_attn_q_slabs(z)).
struct XQPart {
  const float* part = nullptr;  // half_t elements when part_half
  int part_half = 0;
  int64_t stride = 0;
  int z = 0;
  const float* bias = nullptr;
  int max_rows = 0;  // rows per window when known (decoder step: the beam group)
  // step cross-attention records of pairs cut between workgroups, [pair][segment][XREC],
  // one arrival counter per (window, head) pair (zero between launches), and the pair
  // capacity of both; null = the first-pass kernel
  float* split_rec = nullptr;
  int* split_cnt = nullptr;
  int max_pairs = 0;
  // round 6: the query projected inside the step kernel (xattn_fused_q): q = qx W_q^T + bias
  // with qx the LayerNorm'd rows [rows][n] (T) and qwf = W_q [n][n] (T) in fragment order
  // (launch_wq_frag); q / part unused
  const void* qx = nullptr;
  const void* qwf = nullptr;
};
// the shapes the in-kernel query projection serves: fp16, n = 1280 (large-v3, turbo), <= 8
// rows per window; the choice depends on the model and the beam group only, never on the
// window count (a window's step stays batch-invariant)
inline bool xattn_fused_q(int n, int rows_per_window, int elem_size) {
  return elem_size == 2 && n == 1280 && rows_per_window >= 1 && rows_per_window <= 8;
}
// W_q [n][n] (fp16) -> the in-kernel query projection's fragment order: 16-B chunk
// ((((h * 4 + c) * 2 + kh) * (n / 64) + s) * 64 + lane) holds row h * 64 + 16 c + (lane & 15),
// columns kh * n / 2 + 32 s + 8 (lane >> 4) .. + 7 (a wave's k-step s is 1 KB contiguous)
void launch_wq_frag(const void* w, void* f, int n, hipStream_t st);
constexpr int XREC = 16 * 64 + 32;  // floats per segment record: O[16][64], m[16], l[16]
// step cross-attention (k_xattn_seg): one softmax partial per 64-key tile, at most
// XS_NSP tiles per (window, head) pair (Tk <= 1536), at most XS_QP pairs per workgroup
constexpr int XS_NSP = 24;
constexpr int XS_QP = 4;
int xattn_seg_grid(int npair, int nsp, int smax);
inline bool cross_attn_q_slabs(int z) { return z == 4 || z == 8 || z == 10; }
template <typename T>
void launch_cross_attn(const T* q, int ldq, const T* ck, const T* cv, int Tk, int H, int nsplit, int nwin,
                       const int* win_row0, const int* win_nrows, const int* win_slot, int64_t win_stride, float* po,
                       float* pm, float* pl, T* out, int ldo, int rows, float* qk_out, const int* qk_map, int qk_rows,
                       hipStream_t st, XQPart xq = XQPart());
template <typename T>
void launch_embed(const T* E, const T* P, int n, const int* row_tok, int* row_pos, const int* hist,
                  const int* cur_len, int G, int hctx, int pmax, float* x, int rows, hipStream_t st);
template <typename T>
void launch_mel_windows(const float* mel, int64_t ld_mel, int n_mels, const int64_t* seeks, const int* segs, T* melT,
                        int64_t win_stride, int rows_alloc, int nwin, hipStream_t st);
template <typename T>
void launch_zero_rows(T* buf, int64_t ws, int n, int ra, int rb, int nwin, hipStream_t st);

void launch_mel(const float* audio, int64_t n_real, int64_t n_padded, int64_t frame0, int64_t count,
                const float* filters, int n_mels, float* mel, int64_t ld, unsigned* gmax, hipStream_t st);
void launch_mel_norm(float* mel, int64_t count, int64_t ld, int n_mels, const unsigned* gmax, const float* ovr,
                     hipStream_t st);
// one file of a wh_log_mel_batch call: its samples start at audio_off of the concatenated
// audio, its frames at column frame_base of the mel, its frame blocks at block_base
struct MelFile {
  int64_t audio_off, n_real, n_padded, nframes, frame_base, block_base;
};
int mel_blocks(int64_t nframes);  // frame blocks one file takes (whole blocks)
// segmented log-mel of every file, raw values then each file's own max-8 floor and scaling
void launch_mel_seg(const float* audio, const MelFile* files, int n_files, int64_t n_blocks, const float* filters,
                    int n_mels, float* mel, int64_t ld, unsigned* gmax, hipStream_t st);
// wh_audio_ingest's kernel: interleaved PCM [n_frames][channels] in `encoding` (a WH_WAV_* code
// of include/whisper_hip.h; S16 and S32 are what wh_audio_ingest and the FLAC path hold) at
// 2^-(bits-1) per step (bits = 1 for the float encodings) -> n_out mono float32 samples at
// 16 kHz, accumulated in fp64 and quantised to 16-bit steps.  taps [2*10*max(up, down) + 1]
// doubles on the device, or null when up == down (mix and quantise only).  The buffer must be
// allocated 8 bytes past the samples (24-bit samples are read as aligned dwords).  One launch.
void launch_pcm_resample(const void* pcm, int encoding, int64_t n_frames, int channels, int bits, int up, int down,
                         const double* taps, float* out, int64_t n_out, hipStream_t st);
// wh_stream_append / wh_stream_finish's kernel: the chunk `pcm` holds frames [n0, n0 + nc) of a
// recording; outputs [k0, k0 + n_emit) of launch_pcm_resample on the whole recording go to out[0 ..
// n_emit).  Frames before n0 are read from hist_old (`hist` = 2*half/up doubles, frames
// [n0 - hist, n0)), frames from n0 + nc on are zeros; hist_new (another buffer) receives frames
// [n0 + nc - hist, n0 + nc).  The caller guarantees that every output's newest frame is below
// n0 + nc or that the recording has ended.  The chunk buffer is allocated 8 bytes past its samples.
void launch_pcm_resample_stream(const void* pcm, int encoding, int64_t n0, int64_t nc, int channels, int bits, int up,
                                int down, const double* taps, const double* hist_old, double* hist_new, int hist,
                                float* out, int64_t k0, int64_t n_emit, hipStream_t st);
// wh_pool_append / wh_pool_finish's kernel: launch_pcm_resample_stream for n streams in one grid.
// The host fills descriptor i of a pinned array (pool_stream_bytes() each) with the arguments
// that launch would take and the stream's first workgroup; pool_stream_fill returns the
// workgroups the stream takes, which must not be 0 (a stream without work is left out).  The
// device copy of the array is what the launch reads.
size_t pool_stream_bytes();
int64_t pool_stream_fill(void* desc, int i, int64_t block0, const void* pcm, int encoding, int64_t n0, int64_t nc,
                         int channels, int bits, int up, int down, const double* taps, const double* hist_old,
                         double* hist_new, int hist, float* out, int64_t k0, int64_t n_emit);
void launch_pcm_resample_pool(const void* desc, int n, int64_t n_blocks, hipStream_t st);
// wh_pool_trim's kernel: n moves of floats between buffers that do not overlap, one launch
struct PoolMove {
  const float* src;
  float* dst;
  int64_t n;
};
void launch_pool_move(const PoolMove* moves, int n, int64_t longest, hipStream_t st);
// wh_*_ingest_split's kernel: the same input, but no mix: selected channel s (select[s], n_select
// distinct ids in [0, channels), at most 256) becomes a waveform of its own, n_out samples at
// out + s * n_out, with the arithmetic the kernel above has for a mono file of that channel.
// One launch for all selected channels.
void launch_pcm_resample_split(const void* pcm, int encoding, int64_t n_frames, int channels, int bits, int up,
                               int down, const double* taps, const int* select, int n_select, float* out,
                               int64_t n_out, hipStream_t st);

// ------------------------------------------------------------ decode state (device)
// Per window slot w (capacity nw) with G rows (beams / samples) each.
struct DecState {
  int* hist;         // [nw][G][hctx]   token history (initial tokens + sampled)
  int* anc;          // [nw][G][ctx]    KV slot of each position (beam reorder by indirection)
  int* len;          // [nw]            current token count
  int* sample_begin; // [nw]
  int* step;         // [nw]            updates done
  int* done;         // [nw]
  float* sum_lp;     // [nw][G]
  int* fin_n;        // [nw]
  float* fin_score;  // [nw][maxc]
  int* fin_len;      // [nw][maxc]
  int* fin_tok;      // [nw][maxc][hctx]
  float* cand_val;   // [nw*G][KC]
  int* cand_idx;     // [nw*G][KC]
  float* lpart;      // [nw*G][LP_SLICES][LP_REC] per-slice token-selection partials
  int* lp_cnt;       // [nw*G] slice arrival counters of k_logit_part (zero between launches)
  int* lpw_cnt;      // [nw] row arrival counters of the merging k_logit_part (zero between launches)
  unsigned long long* seed;  // [1] sampling seed (device memory: not part of a captured graph)
  int nw, G, ctx, hctx, maxc;
};

// One token of the phrase table: phrase token k of its phrase, so the k records before it
// hold the prefix ids.  bonus is fl32(boost * start) at k = 0 and the boost elsewhere.
struct BiasRec {
  int id, k;
  float bonus;
  int pad;
};
constexpr int BIAS_MAX_ENTRIES = 512;  // one record per thread of k_logit_part's workgroup
constexpr int BIAS_MAX_PHRASES = 128;
constexpr int BIAS_MAX_LEN = 16;

struct DecOpts {
  int V, eot, ts_begin, no_ts;       // vocabulary facts
  int blank[4], n_blank;             // SuppressBlank ids (tokenizer.encode(" ") + eot)
  const unsigned* suppress;          // bitmask [ceil(V/32)] or null
  int suppress_blank, timestamps;    // flags
  int max_initial;                   // max_initial_timestamp index or -1
  int beam;                          // 1 = beam search, 0 = greedy/sampling
  int sample_len;                    // max updates
  int n_ctx;                         // text context (448): stop when len > n_ctx
  float temperature;                 // > 0: Gumbel-max sampling (greedy decoder)
  // repetition filter over the sampled tokens hist[sample_begin, len) of each row, on the raw
  // logits ahead of every other filter (include/whisper_hip.h, wh_decode_opts):
  int no_repeat_ngram;               // 0 = off, 1..16: ban the text ids that would repeat an n-gram
  float repetition_penalty;          // 1 = off (set_opts stores 1 for 0): x > 0 ? x / p : x * p for
                                     // every text id sampled so far
  // phrase bias (include/whisper_hip.h, wh_set_phrase_bias): after the penalty, before the ban.
  // The table's contents are device memory, not part of this struct: a new table of the same
  // size leaves the step graph's key (the bytes of DecOpts) as it was
  int n_bias;                        // table entries (0 = off, <= BIAS_MAX_ENTRIES)
  const BiasRec* bias;               // [n_bias] one record per phrase token, phrases back to back
};
inline bool repeat_filter_on(const DecOpts& o) {
  return o.no_repeat_ngram > 0 || (o.repetition_penalty != 1.f && o.repetition_penalty != 0.f);
}
// the history-filter instantiations of k_logit_part (RF) serve the repetition controls and
// the phrase table alike
inline bool history_filter_on(const DecOpts& o) { return repeat_filter_on(o) || o.n_bias > 0; }

constexpr int LP_SLICES = 32;  // vocabulary slices per row: 31 text slices + [timestamp_begin, V)
constexpr int LP_REC = 32;    // words per slice record
void launch_logit_rows(float* logits, int ldl, const DecState& s, const DecOpts& o, int nwin, hipStream_t st);
// vocabulary slices per row the selection of nwin windows runs with (k_logit_part), 0 where
// it is k_logit_rows; the repetition filter exists in the sliced kernels only
int logit_slices(const DecState& s, const DecOpts& o, int nwin);
// k_merge also writes the NEXT step's decoder input rows (the embedding of each row's
// newest token, k_embed's arithmetic) when em.x is set: the step graph then starts with
// the first layer instead of a separate k_embed launch (round 4)
struct MergeEmbed {
  const void* E = nullptr;  // token embedding [V][n] (T)
  const void* P = nullptr;  // positional embedding [ctx][n] (T)
  float* x = nullptr;       // decoder input rows [rows][n] (fp32)
  int* row_pos = nullptr;   // position of each row's input token
  int n = 0, pmax = 0, half = 0;
};
void launch_merge(const DecState& s, const DecOpts& o, int nwin, hipStream_t st, const MergeEmbed& em = MergeEmbed());
int self_attn_kco_min();  // fp16: the coalesced-K self-attention passes (round 6) run from this many cached keys on
// token selection + candidate merge of one update: one k_logit_part launch whose last
// row combiner of each window runs the merge (round 4), or the selection then k_merge
void launch_select_merge(float* logits, int ldl, const DecState& s, const DecOpts& o, int nwin, hipStream_t st,
                         const MergeEmbed& em);
// per-step ABI (wh_step / wh_reorder_kv): append host-chosen tokens, reorder rows
void launch_append_tokens(const DecState& s, const int* tok, int nwin, hipStream_t st);
void launch_reorder_rows(const DecState& s, const int* src, int nwin, hipStream_t st);
void launch_no_speech(const float* logits, int ldl, int rows, int V, int no_speech, float* out, hipStream_t st);
void launch_broadcast_rows(const float* src, int ld_src, const int* src_rows, float* dst, int ld_dst, int G, int nwin,
                           int V, hipStream_t st);

}  // namespace wh
