// The decoder's 8-bit (OCP FP8 E4M3) weight copies for the single-window step: the
// quantiser and k_proj1<w8> (wh_proj8.hip).  Format: whisper_hip.h "decoder formats".
//
// Code layout.  Every k_proj1 configuration of a model width n cuts K into per-wave ranges of
// NS * 32 (NS = p1_nstep(n): wh_proj.hip launch_proj1's NS column), and lane (r, g) of the
// wave that owns a range multiplies the codes at k = 32 s + 8 g + 0..7, s < NS, of its column.
// A row of the [N][K] matrix is therefore stored range by range as [g: 4][s: NS][8]: the
// lane's NS * 8 codes are one contiguous run (40 B at n = 1280: two 16 B loads and one 8 B
// load instead of five 16 B loads of fp16), a wave's four lane groups read NS * 32 contiguous
// bytes of each of its 16 rows, and one copy serves all five projection shapes of the width.
// The activation side (LDS rows, fragment loads) and the MFMA k-order are those of k_proj1.
#pragma once
#include "wh_gemm.h"

namespace wh {

// k-steps per wave of every k_proj1 configuration of model width n; 0: no configuration
constexpr int p1_nstep(int n) {
  return n == 1280 ? 5 : n == 1024 ? 4 : n == 768 ? 3 : n == 512 ? 2 : n == 384 ? 3 : n == 128 ? 1 : 0;
}
// where the code of logical column k sits in its stored row (ns = p1_nstep of the width)
constexpr int w8_offset(int k, int ns) {
  const int range = k / (ns * 32), q = k - range * ns * 32;
  return range * ns * 32 + ((q >> 3) & 3) * ns * 8 + (q >> 5) * 8 + (q & 7);
}

// fp16 weights [rows][K] -> codes in the layout above and one fp32 scale per row
// (scale = amax / 448, code = e4m3(clamp(w / scale))); K % (ns * 32) == 0, K <= 8192
int launch_quant_dec_w8(const void* w, uint8_t* codes, float* scales, int rows, int K, int ns, hipStream_t st);

// launch_proj1<half_t> (wh_gemm.h) with a.W = the codes of the [N][K] weight and wscale its
// N scales: the same configurations, operands and epilogues; returns -1 for a shape none serves
int launch_proj1_w8(const GemmArgs& a, const float* wscale, int epi, bool ln, hipStream_t st, hipEvent_t ev0 = nullptr,
                    hipEvent_t ev1 = nullptr);

}  // namespace wh
