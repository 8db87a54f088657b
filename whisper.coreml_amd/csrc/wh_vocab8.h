// The 8-bit (OCP FP8 E4M3) copy of the token embedding for the single-window step's logits:
// the quantiser and k_vocab1_w8 (wh_vocab8.hip).  Format: whisper_hip.h "vocabulary formats".
//
// Code layout.  Only k_vocab1_w8 reads the codes, so they are stored as it loads them.  The
// kernel cuts K into KW per-wave ranges of SW k-steps (v8_kw / v8_sw of the width) and the
// vocabulary into 16-column tiles; lane (r, g) of wave w multiplies, for every tile, the codes
// k = 32 (w SW + s) + 8 g + 0..7, s < SW, of the tile's column r.  The matrix is tile-major,
//   [tile][wave w][load j][lane][16 B]      j < SW / 2: the k-steps 2j (bytes 0..7), 2j + 1 (8..15)
//   [tile][wave w][SW / 2][lane][ 8 B]      an odd SW: its last k-step
// so a tile is 16 K contiguous bytes, a wave's share of it 512 SW, and every wave-wide load
// one aligned run of 1024 (or 512) bytes: at K = 1280 two 16 B loads and one 8 B load per lane
// and tile.  Columns V .. 16 ceil(V / 16) - 1 exist, with codes 0 and scale 0.
#pragma once
#include "wh_gemm.h"

namespace wh {

constexpr int V8_TMAX = 13;  // tiles per workgroup the kernel is unrolled to

// waves per workgroup and k-steps per wave at model width n (KW * SW * 32 == n); 0: not served.
// (384 = 12 k-steps and 128 = 4 do not cut into eight ranges: 6 x 2 and 4 x 1)
constexpr int v8_kw(int n) {
  return n == 1280 || n == 1024 || n == 768 || n == 512 ? 8 : n == 384 ? 6 : n == 128 ? 4 : 0;
}
constexpr int v8_sw(int n) { return v8_kw(n) ? n / (32 * v8_kw(n)) : 0; }
// the columns the copy holds, and where the code of (column n, element k) of a [.][K] matrix sits
constexpr int v8_cols(int V) { return (V + 15) / 16 * 16; }
constexpr int64_t v8_offset(int n, int k, int K, int SW) {
  const int ks = k >> 5, g = (k >> 3) & 3, w = ks / SW, s = ks - w * SW, ln = g * 16 + (n & 15);
  const int64_t base = (int64_t)(n >> 4) * 16 * K + w * 512 * SW;
  return s < (SW & ~1) ? base + (s >> 1) * 1024 + ln * 16 + (s & 1) * 8 + (k & 7)
                       : base + (SW >> 1) * 1024 + ln * 8 + (k & 7);
}
// workgroups of the projection: 256 (one per CU), fewer for under 256 tiles, more where 256
// would leave one more than V8_TMAX tiles
constexpr int v8_grid(int V) {
  const int nt = (V + 15) / 16, a = nt < 256 ? nt : 256, b = (nt + V8_TMAX - 1) / V8_TMAX;
  return a > b ? a : b;
}

// fp16 embedding [V][K] -> codes [v8_cols(V)][K] in the layout above and v8_cols(V) fp32 scales
// (scale = amax / 448, code = e4m3(clamp(w / scale))); -1: a width v8_kw does not serve
int launch_quant_vocab_w8(const void* E, uint8_t* codes, float* scales, int V, int K, hipStream_t st);

// logits[m][n] = scale[n] * sum_k LN(a.xf32[m])[k] code[n][k] for a.M <= 8 rows: a.W the codes,
// a.xf32 / ln_g / ln_b / ln_eps the final LayerNorm's operands, a.out_f32 / ldo the logits, a.N = V,
// a.K the width.  -1: a shape it does not serve, -5: the LDS attribute was refused
int launch_vocab1_w8(const GemmArgs& a, const float* wscale, hipStream_t st);

}  // namespace wh
