// 1024 rows at large-v3 dimensions, fp16: the fused scoring kernel (k_score_part +
// k_score_merge, csrc/wh_score.hip) against what alignment does for its token probabilities
// (the vocabulary GEMM into 128 logit rows, then launch_token_probs, 8 times).  Device time
// between HIP events, the two alternated; every sample is printed.
//   make -C whisper.coreml_amd tools/score_bench && ./whisper.coreml_amd/tools/score_bench
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wh_align.h"
#include "wh_gemm.h"
#include "wh_score.h"

using namespace wh;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e = (x);                                                        \
    if (e != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

int main() {
  const int R = 1024, V = 51866, K = 1280, reps = 10;
  half_t *E, *X;
  float *lg, *probs, *lp, *tlp;
  int *rows, *tgt, *top;
  void* rec;
  CK(hipMalloc(&E, (size_t)V * K * 2));
  CK(hipMemset(E, 0x2c, (size_t)V * K * 2));  // every element 0.0652
  CK(hipMalloc(&X, (size_t)R * K * 2));
  CK(hipMemset(X, 0x2c, (size_t)R * K * 2));
  CK(hipMalloc(&lg, (size_t)128 * V * 4));
  CK(hipMalloc(&rec, score_rec_bytes(R)));
  for (void** p : {(void**)&probs, (void**)&lp, (void**)&tlp, (void**)&rows, (void**)&tgt, (void**)&top}) {
    CK(hipMalloc(p, R * 4));
    CK(hipMemset(*p, 0, R * 4));
  }
  std::vector<int> h(R);
  for (int i = 0; i < R; ++i) h[i] = i;
  CK(hipMemcpy(rows, h.data(), R * 4, hipMemcpyHostToDevice));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto fused = [&] {
    ScoreArgs a;
    a.X = X; a.E = E; a.x_rows = rows; a.target = tgt; a.rec = (float4_t*)rec; a.logprob = lp; a.top_id = top;
    a.top_logprob = tlp; a.ldx = K; a.R = R; a.V = V; a.K = K;
    return launch_vocab_score<half_t>(a, st);
  };
  auto loop = [&] {
    for (int r0 = 0; r0 < R; r0 += 128) {
      GemmArgs a;
      a.X = X; a.W = E; a.M = 128; a.N = V; a.K = K; a.ldx = K; a.x_group_rows = 128; a.out_f32 = lg; a.ldo = V;
      a.x_rows = rows + r0;
      if (launch_gemm<half_t>(a, EPI_F32_COLS, st)) return 1;
      launch_token_probs(lg, V, 128, 50257, tgt + r0, probs + r0, st);
    }
    return 0;
  };
  std::vector<float> t[2];
  for (int i = -2; i < reps; ++i)  // two warm-up rounds
    for (int which = 0; which < 2; ++which) {
      CK(hipEventRecord(e0, st));
      if (which ? loop() : fused()) { printf("launch refused\n"); return 1; }
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 0) {
        t[which].push_back(ms);
        printf("round %d %s %.3f ms\n", i, which ? "gemm+token_probs x8" : "fused+merge        ", ms);
      }
    }
  CK(hipGetLastError());
  for (int which = 0; which < 2; ++which) {
    std::sort(t[which].begin(), t[which].end());
    printf("%s: median %.3f ms, min %.3f, max %.3f over %d alternated samples\n", which ? "gemm+token_probs x8" : "fused+merge",
           (t[which][reps / 2 - 1] + t[which][reps / 2]) / 2, t[which].front(), t[which].back(), reps);
  }
  return 0;
}
