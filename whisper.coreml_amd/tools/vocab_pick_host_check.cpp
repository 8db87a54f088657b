// vocab_kernel (csrc/wh_vocab_pick.h), the choice of the vocabulary projection's kernel, against a
// table written out by hand, under the host sanitizers, without a context, a GPU or Python:
//   make -C whisper.coreml_amd tools/vocab_pick_host_check && ./whisper.coreml_amd/tools/vocab_pick_host_check
// The table walks every boundary of the choice: 8 / 9, 16 / 17 (fp32), 32 / 33 and 112 / 113 rows,
// K = 1280 against the other widths, the LayerNorm prologue against plain rows, the 8-bit step.
// tests/test_vocab_pick.py builds and runs it.
#include <cstdio>

#include "wh_vocab_pick.h"

using namespace wh;

struct Case {
  int elt, M, N, K;
  bool ln, w8;
  VocabKernel want;
};

static const int V = 51865, V3 = 51866;

static const Case CASES[] = {
    // the single-window step, fp16: K 1280 -> k_vocab1, the other widths -> k_vocab_small
    {2, 1, V3, 1280, true, false, VK_VOCAB1},
    {2, 5, V3, 1280, true, false, VK_VOCAB1},
    {2, 8, V3, 1280, true, false, VK_VOCAB1},
    {2, 9, V3, 1280, true, false, VK_NONE},  // the prologue serves 8 rows (P1_RMAX)
    {2, 8, 256 * 13 * 16, 1280, true, false, VK_VOCAB1},
    {2, 8, 256 * 13 * 16 + 1, 1280, true, false, VK_VOCAB_SMALL},  // a 14th tile per workgroup
    {2, 1, V, 384, true, false, VK_VOCAB_SMALL},
    {2, 8, V, 512, true, false, VK_VOCAB_SMALL},
    {2, 8, V, 768, true, false, VK_VOCAB_SMALL},
    {2, 8, V, 1024, true, false, VK_VOCAB_SMALL},
    {2, 8, V, 128, true, false, VK_VOCAB_SMALL},
    {2, 9, V, 512, true, false, VK_NONE},
    {2, 8, V, 1312, true, false, VK_NONE},   // the prologue holds K <= 1280
    {2, 8, 16383, 512, true, false, VK_NONE},
    // the single-window step, fp32: k_vocab_small at every width
    {4, 1, V, 384, true, false, VK_VOCAB_SMALL},
    {4, 8, V3, 1280, true, false, VK_VOCAB_SMALL},
    {4, 9, V3, 1280, true, false, VK_NONE},
    // plain rows, fp16, K 1280: small to 32, 2p to 112, then k_gemv_x
    {2, 9, V3, 1280, false, false, VK_VOCAB_SMALL},
    {2, 10, V3, 1280, false, false, VK_VOCAB_SMALL},
    {2, 32, V3, 1280, false, false, VK_VOCAB_SMALL},
    {2, 33, V3, 1280, false, false, VK_VOCAB_2P},
    {2, 35, V3, 1280, false, false, VK_VOCAB_2P},
    {2, 65, V3, 1280, false, false, VK_VOCAB_2P},
    {2, 112, V3, 1280, false, false, VK_VOCAB_2P},
    {2, 113, V3, 1280, false, false, VK_GEMV_X},
    {2, 128, V3, 1280, false, false, VK_GEMV_X},
    // plain rows, fp16, the other widths: k_vocab_2p is K 1280 only
    {2, 10, V, 512, false, false, VK_VOCAB_SMALL},
    {2, 32, V, 512, false, false, VK_VOCAB_SMALL},
    {2, 33, V, 512, false, false, VK_GEMV_X},
    {2, 35, V, 512, false, false, VK_GEMV_X},
    {2, 35, V, 1024, false, false, VK_GEMV_X},
    {2, 112, V, 384, false, false, VK_GEMV_X},
    // plain rows, fp32: small to 16, k_gemv_rows on two row tiles, k_gemv_x from three
    {4, 10, V, 512, false, false, VK_VOCAB_SMALL},
    {4, 16, V, 512, false, false, VK_VOCAB_SMALL},
    {4, 16, V3, 1280, false, false, VK_VOCAB_SMALL},
    {4, 17, V, 512, false, false, VK_GEMV_ROWS},
    {4, 17, V3, 1280, false, false, VK_GEMV_ROWS},
    {4, 20, V, 512, false, false, VK_GEMV_ROWS},
    {4, 32, V3, 1280, false, false, VK_GEMV_ROWS},
    {4, 33, V3, 1280, false, false, VK_GEMV_X},
    {4, 35, V, 512, false, false, VK_GEMV_X},
    {4, 112, V3, 1280, false, false, VK_GEMV_X},
    {4, 113, V3, 1280, false, false, VK_GEMV_X},
    // K past 1280 or a small N: the plain skinny kernels
    {2, 10, V, 1312, false, false, VK_GEMV_ROWS},
    {2, 35, V, 1312, false, false, VK_GEMV_X},
    {2, 10, 16383, 512, false, false, VK_GEMV_ROWS},
    {2, 35, 16383, 1280, false, false, VK_GEMV_ROWS},
    {2, 10, 16384, 512, false, false, VK_VOCAB_SMALL},
    // the 8-bit step: fp16, the prologue, <= 8 rows, the k_proj1 widths, V <= 57344
    {2, 1, V, 384, true, true, VK_VOCAB1_W8},
    {2, 8, V3, 1280, true, true, VK_VOCAB1_W8},
    {2, 8, 51864, 384, true, true, VK_VOCAB1_W8},
    {2, 8, V, 128, true, true, VK_VOCAB1_W8},
    {2, 8, 57344, 1024, true, true, VK_VOCAB1_W8},
    {2, 8, 57345, 1024, true, true, VK_NONE},
    {2, 9, V, 512, true, true, VK_NONE},
    {2, 8, V, 256, true, true, VK_NONE},
    {2, 8, V, 512, false, true, VK_NONE},
    {4, 8, V, 512, true, true, VK_NONE},
    // no rows, a K that is no multiple of 32
    {2, 0, V, 512, false, false, VK_NONE},
    {2, 8, V, 500, false, false, VK_NONE},
};

int main() {
  int failures = 0;
  for (const Case& c : CASES) {
    const VocabKernel got = vocab_kernel(c.elt, c.M, c.N, c.K, c.ln, c.w8);
    if (got == c.want) continue;
    ++failures;
    fprintf(stderr, "FAIL elt %d M %d N %d K %d ln %d w8 %d: %s, want %s\n", c.elt, c.M, c.N, c.K, c.ln, c.w8,
            vocab_kernel_name(got), vocab_kernel_name(c.want));
  }
  // the tuning build's switches: without k_vocab1 the step runs k_vocab_small; without
  // k_vocab_small (and with it k_vocab_2p) plain rows run the k_gemv kernels and the prologue has none
  struct Sw { int M; bool ln, v1, vs; VocabKernel want; };
  const Sw sws[] = {{8, true, false, true, VK_VOCAB_SMALL}, {8, true, true, false, VK_NONE},
                    {10, false, true, false, VK_GEMV_ROWS}, {35, false, true, false, VK_GEMV_X}};
  for (const Sw& s : sws)
    if (vocab_kernel(2, s.M, V3, 1280, s.ln, false, s.v1, s.vs) != s.want) {
      ++failures;
      fprintf(stderr, "FAIL switches M %d ln %d vocab1 %d vocab_small %d\n", s.M, s.ln, s.v1, s.vs);
    }
  // k_vocab_small's row groups: every shape given to it is one group
  for (const Case& c : CASES)
    if (c.want == VK_VOCAB_SMALL && vocab_small_groups(c.elt, c.M, c.K) != 1) {
      ++failures;
      fprintf(stderr, "FAIL groups elt %d M %d K %d\n", c.elt, c.M, c.K);
    }
  if (failures) return 1;
  printf("vocab_pick_host_check: ok (%zu shapes)\n", sizeof(CASES) / sizeof(CASES[0]));
  return 0;
}
