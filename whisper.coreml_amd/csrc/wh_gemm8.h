// The encoder's 8-bit (OCP FP8 E4M3) GEMM path: quantisers and k_gemm8 (wh_gemm8.hip).
// Format: whisper_hip.h "encoder formats".
#pragma once
#include "wh_gemm.h"

namespace wh {

constexpr int G8_BK = 128;  // K-tile of k_gemm8: one 16x16x128 MFMA deep, 128 B per row

// fp16 rows [rows][K] -> E4M3 codes [rows][K] and one fp32 scale per row (k_quant_rows for
// activations, k_quant_weights for the [out][in] weights: the same rule).  K % 8 == 0, K <= 8192
void launch_quant_rows(const void* x, uint8_t* codes, float* scales, int rows, int K, hipStream_t st);
void launch_quant_weights(const void* w, uint8_t* codes, float* scales, int rows, int K, hipStream_t st);
// LayerNorm (k_layernorm's arithmetic, rounded to fp16) written as codes + row scale; n <= 2048
void launch_layernorm_quant(const float* x, uint8_t* codes, float* scales, const float* g, const float* b, int rows,
                            int n, float eps, hipStream_t st);

// Y = sa[m] sw[n] sum_k X8[m][k] W8[n][k] (+ bias, epilogue epi: EPI_STORE, EPI_STORE_GELU,
// EPI_RESID, EPI_QKV_ENC); a.X / a.W are the codes (plain [M][K] / [N][K], a.ldx == K).
// tile: 0 = by grid size (256 x 128 tiles from one per CU, else 128 x 64), 256 / 128 = forced.
// Returns 0, or < 0 for a shape no tile serves (N % tile, K % 128) or an unknown epilogue.
int launch_gemm8(const GemmArgs& a, const float* sa, const float* sw, int epi, int tile, hipStream_t st);
// the tile launch_gemm8 picks for tile = 0 (256 or 128), 0 when the shape is not served
int gemm8_tile(int M, int N, int K);

}  // namespace wh
