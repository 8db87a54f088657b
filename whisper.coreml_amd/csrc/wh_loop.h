// The host side of a context's decode loop and of alignment: the decode options, the step
// graph and its two-deep done-flag poll, the readback, the per-step ABI's checks, the DTW
// driver and the window bookkeeping of wh_align_batch and wh_score_batch.  None of it depends
// on the model's element type, so it is a plain struct compiled once (csrc/wh_loop.hip) and the
// base of wh_ctx; what does depend on it, it reaches through five virtuals of Ctx<T>.
#pragma once
#include <string>
#include <vector>

#include "wh_align.h"
#include "wh_host.h"
#include "wh_kernels.h"
#include "wh_rows.h"
#include "wh_score.h"
#include "whisper_hip.h"

namespace wh {
constexpr int CTX = 448;       // text positions (decoder.py:243, decoding.py:173)
constexpr int HCTX = CTX + 1;  // history capacity (tokens.shape[-1] may reach n_ctx + 1)
}  // namespace wh

struct DecodeLoop {
  // set by Ctx<T>::init (the device pointers lie in its activation arena); ~Ctx releases
  int Ld = 0, nh = 0, V = 0;  // decoder layers, heads, vocabulary
  int Wcap = 0, Gcap = 0, PRE = 0;  // max_windows, max_group, first-pass rows per pass
  bool finalized = false;     // every weight loaded
  hipStream_t st = nullptr;
  Timer tm;
  double stats[WH_N_STATS] = {0};  // WH_STAT_*
  std::vector<float> token_ms;     // per-token wall ms of each decode_steps chunk
  // wh_set_phrase_bias's table; the next wh_decode_begin uploads it
  std::vector<wh::BiasRec> bias_tab;
  int maxc = 5;
  unsigned* suppress = nullptr;
  wh::BiasRec* bias_dev = nullptr;  // [BIAS_MAX_ENTRIES], allocated once: DecOpts::bias never changes
  float* nsp = nullptr;
  int *src_rows = nullptr, *qk_map = nullptr;  // qk_map [Ld][nh]
  int* h_done = nullptr;  // pinned: two poll buffers of Wcap flags
  hipEvent_t poll_ev[2] = {nullptr, nullptr};
  wh::DecState S;  // the current batch
  wh::DecOpts O;
  int cur_nwin = 0, cur_G = 1;
  std::vector<int> h_len;      // host mirror of S.len for the per-step ABI
  std::vector<int> win_slots;  // cross-KV slot of each decode window
  unsigned long long h_seed = 0;
  bool step_api = false;  // the batch was begun by wh_prefill: wh_step / wh_reorder_kv
  // The device loop's step input rows (x_d, row_pos) are written by the previous update's
  // merge.  Any other use of those buffers between two decode_steps calls (a first pass, a
  // timing stage) sets rows_dirty, and the next decode_steps re-embeds them (restore_rows).
  bool rows_dirty = false;
  hipGraph_t graph = nullptr;  // graph cache
  hipGraphExec_t gexec = nullptr;
  std::vector<char> graph_key;
  // grow-only device scratch of the alignment, DTW and prefill-logits calls (one at a time)
  DevBuf<char> scratch;

  int set_opts(const wh_decode_opts* o, int n_win);
  int ensure_graph();
  int launch_step();
  // WHISPER_HIP_EAGER=1: the step kernels launched directly, not through the captured graph
  bool eager() const { const char* e = tune_env("WHISPER_HIP_EAGER"); return e && e[0] == '1'; }
  int decode_steps(int max_steps, int* n_done);
  int decode_read(int slot, int* tokens, float* slp, int* len, int* fin_n, int* fin_tok, int* fin_len,
                  float* fin_score, float* nspo);
  int reorder_kv(const int* src);
  // the checks that open begin_batch (they leave cur_nwin = 0, win_slots filled) and step_tokens
  int begin_check(int n_win, int G, const int* init, const int* n_init, int max_init, const int* sot_index,
                  const int* slots);
  int step_check(const int* tok, const int* offsets);
  // A first pass writes beam slot 0's self-KV rows of its slot: refused on a slot that the
  // live device-loop batch is still decoding (its done flag unset), which it would corrupt.
  // Slots outside the batch, finished windows and the per-step ABI's batch are allowed.
  int check_slot_idle(int slot);
  int ensure_scratch(size_t bytes);
  // timing.dtw (timing.py:82-105, 139-151) of a host cost matrix x [N][M] on the GPU.
  // open == nullptr: wh_dtw, the closed kernel.  Otherwise wh_dtw_open: min_rows == 0 is
  // closed too, run as min_rows = N, which gives wh_dtw's path and still fills the scores
  struct DtwOpen { int min_rows; float row_penalty; int* end_row; float* scores; };
  int dtw(const float* x, int N, int M, int* path, int* plen, const DtwOpen* open);
  // find_alignment's device half (timing.py:163-231): window w is sot_sequence +
  // [no_timestamps] + text + [eot] (n_tokens[w] ids, back to back in tokens) over the audio
  // features of slots[w].  Up to PRE rows of first passes run together with the alignment
  // heads' cross-QK captured, then the text tokens' probabilities, the filtered head-mean
  // matrices and all DTWs of the pass in one launch.  Outputs in window order: probs [T_w],
  // paths [2][T_w+1+F_w], plens [n_win].  min_rows == nullptr: closed (wh_align[_batch]);
  // else per window, 0 = closed, run by the open kernel with min_rows = N.  The windows of
  // one call need a slot each (check_slot_idle).
  int align_windows(int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                    const int* num_frames, const int* ah, int na, int medfilt, const int* min_rows, float row_penalty,
                    float* probs, int* paths, int* plens, int* end_rows);
  // wh_vocab_score / wh_score_batch (whisper_hip.h).  The *_check halves are host code with
  // no HIP call: the entry points run them before the context is entered.
  int vocab_score_check(const float* x, int n_rows, const int* targets, const float* logprob, const int* top_id,
                        const float* top_logprob);
  // n_rows host rows [nh * 64] through the fused kernel, SCORE_PASS rows per pass
  int vocab_score(const float* x, int n_rows, const int* targets, float* logprob, int* top_id, float* top_logprob);
  int score_check(int n_seq, const int* slots, const int* tokens, const int* n_tokens, const int* n_ctx,
                  const float* logprob, const int* top_id, const float* top_logprob);
  // Teacher-forced scoring: sequence s runs as one window of a first pass, its self-KV rows in
  // an idle window (check_slot_idle) that it borrows for the pass, its cross-attention over
  // encoder slot slots[s], so several sequences may name one slot.  Row i - 1 scores tokens[i]
  // for i in [n_ctx, n_tokens); the last token is never fed.  A pass takes consecutive
  // sequences while an idle window and PRE rows are left.
  int score_windows(int n_seq, const int* slots, const int* tokens, const int* n_tokens, const int* n_ctx,
                    float* logprob, int* top_id, float* top_logprob);
  static constexpr int SCORE_PASS = 256;  // rows per pass of vocab_score: 1 MB of records
  // the device operands of one fused scoring launch (wh_score.h ScoreArgs)
  struct ScoreOut { const int* target; void* rec; float* logprob; int* top_id; float* top_logprob; };

 protected:
  ~DecodeLoop() = default;
  // one decoder step for the current batch (the graph's body)
  virtual int step_body() = 0;
  virtual void restore_rows() = 0;
  // one alignment pass: the first pass of p's rows, the alignment heads' cross-QK into d_qk
  // [na][p.R][1500], then probs[k] of ptok[k] at row sel[k] through d_lg (128 logit rows)
  virtual int align_rows(const wh::RowPlan& p, const std::vector<int>& sel, float* d_qk, float* d_lg, int eot,
                         const int* ptok, float* probs) = 0;
  // one scoring pass: the first pass of p's rows, then the fused kernel on rows sel[0..n_sel) of
  // the final LayerNorm's output
  virtual int score_rows(const wh::RowPlan& p, const int* sel, int n_sel, const ScoreOut& o) = 0;
  // n rows of fp32 device rows xf, converted to the context type in xt, through the fused kernel
  virtual int score_host_rows(const float* xf, void* xt, int n, const ScoreOut& o) = 0;
};
