// Which kernel computes a vocabulary projection, logits[M][N] = X[M][K] E[N][K]^T in fp32
// (EPI_F32_COLS with no bias).  One pure host function: the skinny launcher (wh_gemm.hip), the
// 8-bit launcher (wh_vocab8.hip), the runtime's vocab() and wh_step_kernels' `vocab=` field all
// ask it, so what is reported is what runs.  Plain C++ with no HIP in it:
// tools/vocab_pick_host_check.cpp pins it at every boundary without a GPU.
//
//   elt  bytes per element of X and E: 2 (fp16) or 4 (fp32)
//   ln   X is the fp32 residual rows and the final LayerNorm runs in the kernel's prologue (the
//        single-window step after the k_proj1 layers)
//   w8   E is the 8-bit copy (vocab="fp8"; the single-window step only)
//   vocab1_on / vocab_small_on: the tuning build's WHISPER_HIP_VOCAB1 / WHISPER_HIP_VOCAB_SMALL
//        switches; the shipped library passes true for both
#pragma once
#include <algorithm>

namespace wh {

enum VocabKernel {
  VK_NONE = 0,     // no kernel serves the shape: the launchers refuse it
  VK_VOCAB1,       // k_vocab1: fp16, K 1280, LayerNorm prologue, <= 8 rows
  VK_VOCAB_SMALL,  // k_vocab_small: the prologue elsewhere; plain rows up to 32 (fp16) / 16 (fp32)
  VK_VOCAB_2P,     // k_vocab_2p: fp16, K 1280, 33..112 plain rows
  VK_GEMV_X,       // k_gemv_x<EPI_F32_COLS>: 3 or more row tiles
  VK_GEMV_ROWS,    // k_gemv_rows<EPI_F32_COLS>: the rest
  VK_VOCAB1_W8,    // k_vocab1_w8: the 8-bit single-window step
};

inline const char* vocab_kernel_name(VocabKernel k) {
  switch (k) {
    case VK_VOCAB1: return "k_vocab1";
    case VK_VOCAB_SMALL: return "k_vocab_small";
    case VK_VOCAB_2P: return "k_vocab_2p";
    case VK_GEMV_X: return "k_gemv_x";
    case VK_GEMV_ROWS: return "k_gemv_rows";
    case VK_VOCAB1_W8: return "k_vocab1_w8";
    default: return "none";
  }
}

// k_vocab_small: the rows in groups of <= 64 that fit LDS with all of K (152 KB)
inline int vocab_small_groups(int elt, int M, int K) {
  const int vrg_max = std::min(64, (152 * 1024) / (K * elt + 16));
  return (M + vrg_max - 1) / vrg_max;
}

inline VocabKernel vocab_kernel(int elt, int M, int N, int K, bool ln, bool w8, bool vocab1_on = true,
                                bool vocab_small_on = true) {
  if (M < 1 || N < 1 || K < 32 || K % 32) return VK_NONE;
  if (w8) {  // (8 B x ldo x rows and 16 K x tiles stay under 2^31: V <= 57344, K <= 1280)
    const bool width = K == 1280 || K == 1024 || K == 768 || K == 512 || K == 384 || K == 128;
    return elt == 2 && ln && M <= 8 && N <= 57344 && width ? VK_VOCAB1_W8 : VK_NONE;
  }
  const bool vocab = N >= 16384;  // below it the plain skinny kernels
  // the LayerNorm prologue exists only in k_vocab_small / k_vocab1
  if (ln && !(vocab_small_on && vocab && M <= 8 && K <= 1280)) return VK_NONE;
  // the single-window step (LayerNorm prologue, fp16, K 1280): k_vocab1, balanced over the chip;
  // (N + 15) / 16 <= 256 x 13: at most 13 tiles per workgroup (TMAX)
  if (elt == 2 && vocab1_on && ln && K == 1280 && M <= 8 && (N + 15) / 16 <= 256 * 13) return VK_VOCAB1;
  // k_vocab_small (<= 32 rows: at 100 rows, 2 groups of 50, it measured 89.2 us against
  // k_gemv_x's 84.6: each CU streams its column block twice, profiles/r03/vocab_groups_ab.txt)
  if (vocab_small_on && vocab && M <= (elt == 2 ? 32 : 16) && K <= 1280 && vocab_small_groups(elt, M, K) <= 4)
    return VK_VOCAB_SMALL;
  // k_vocab_2p: 33..112 fp16 rows resident in LDS, half of K per pass
  if (elt == 2 && vocab_small_on && vocab && M > 32 && M <= 112 && !ln && K == 1280 && M * (K + 16) <= 150 * 1024)
    return VK_VOCAB_2P;
  if ((M + 15) / 16 >= 3 && vocab) return VK_GEMV_X;
  return VK_GEMV_ROWS;
}

}  // namespace wh
