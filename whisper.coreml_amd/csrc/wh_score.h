// Fused vocabulary scoring (csrc/wh_score.hip): log-softmax statistics of LN(x) E^T per row
// without the [rows][V] logits ever existing.  wh_vocab_score / wh_score_batch (whisper_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wh_common.h"

namespace wh {

// The vocabulary is cut into this many slices of whole 16-column tiles, one workgroup per
// (slice, row block): 256 workgroups per row block, one per CU.  A workgroup has 16 waves and
// a wave owns one tile, so a slice holds at most 16 tiles: V <= 256 * 16 * 16 = 65536.
constexpr int SCORE_SLICES = 256;
constexpr int SCORE_WAVES = 16;
// what a workgroup leaves per (slice, row): {max, sum of exp(z - max), target logit or -inf,
// lowest argmax column (int bits)}; laid out [slice][row]
constexpr size_t score_rec_bytes(int rows) { return (size_t)SCORE_SLICES * rows * 16; }

struct ScoreArgs {
  const void* X;       // [rows][ldx] in the context type (rows gathered by x_rows when set)
  const void* E;       // [V][K]
  const int* x_rows;   // nullable
  const int* target;   // [R]
  float4_t* rec;       // [SCORE_SLICES][R]
  float* logprob;      // [R]
  int* top_id;         // [R]
  float* top_logprob;  // [R]
  int64_t ldx;
  int R, V, K;
};

// rows a workgroup keeps resident (a multiple of 16, <= 64): all of K of every row, padded,
// plus the waves' records, within 160 KB of LDS.  Depends on the type and K only.
template <typename T>
int score_row_block(int K);
// k_score_part over every (slice, row block), then k_score_merge.  0, or -1 for a shape the
// kernel does not serve (K % 128, K > 2048, V > 65536, R < 1).
template <typename T>
int launch_vocab_score(const ScoreArgs& a, hipStream_t st);
// fp32 rows -> the context type (fp16: round to nearest even)
template <typename T>
void launch_score_cast(const float* x, T* out, int64_t n, hipStream_t st);

}  // namespace wh
