// vocab="fp8" (wh_set_vocab_format): the single-window step's logits over an 8-bit (OCP FP8
// E4M3) copy of the token embedding, one fp32 scale per vocabulary row.
//   * k_quant_vocab_w8: one wave per embedding row, the row in registers, amax by the wave
//     butterfly, codes written in k_vocab1_w8's tile-major order (wh_vocab8.h);
//   * k_vocab1_w8: k_vocab1's decomposition (wh_gemm.hip: 256 workgroups, each a contiguous
//     range_split of the 16-column tiles, its waves splitting K, the partial tiles summed in
//     LDS in wave order) over half the bytes.  The activations stay fp16, the MFMA is the
//     fp16 one, accumulation fp32; a code becomes its fp16 value exactly in registers, and the
//     column's scale multiplies the fixed-order sum once, before the store.
// A translation unit of its own: the native vocabulary kernels (wh_gemm.hip) do not change.
#include "wh_vocab8.h"

namespace wh {

// ============================================================ quantiser
// 4 fp32 values -> 4 E4M3 codes, round to nearest even (v_cvt_pk_fp8_f32; gfx950: OCP E4M3).
// x / scale is an IEEE fp32 division, clamped to +-448: never the NaN code.  scale == 0 (an
// all-zero row): codes 0.  (wh_proj8.hip w8_encode4's rule)
WH_DEV unsigned v8_encode4(float x0, float x1, float x2, float x3, float scale) {
  auto q = [&](float x) { return scale > 0.f ? fminf(fmaxf(x / scale, -448.f), 448.f) : 0.f; };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x0), q(x1), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x2), q(x3), w, true);
  return (unsigned)w;
}

constexpr int V8_QMAXC = 3;  // 8-element chunks per lane: K <= 64 * 8 * 3 = 1536

// Lane l holds the chunks l, l + 64, l + 128 of its wave's row: every load is issued before
// the reduction.  Chunk c (k = 8 c .. + 7) is 8 contiguous bytes of the layout, at
// v8_offset(row, 8 c).  The rows V .. cols - 1 of the last tile are written as zero rows.
__global__ __launch_bounds__(256) void k_quant_vocab_w8(const half_t* __restrict__ E, uint8_t* __restrict__ codes,
                                                        float* __restrict__ scales, int V, int cols, int K, int SW) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= cols) return;
  const half_t* wr = E + (int64_t)min(row, V - 1) * K;
  const int nch = row < V ? K >> 3 : 0;  // (a padding row: nothing loaded, amax 0)
  half8_t v[V8_QMAXC];
#pragma unroll
  for (int i = 0; i < V8_QMAXC; ++i) {
    v[i] = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
    if (lane + 64 * i < nch) v[i] = *reinterpret_cast<const half8_t*>(wr + 8 * (lane + 64 * i));
  }
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < V8_QMAXC; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)v[i][e]));
  const float scale = wave_max(am) / 448.f;
#pragma unroll
  for (int i = 0; i < V8_QMAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < (K >> 3)) {
      uint2 o;
      o.x = v8_encode4((float)v[i][0], (float)v[i][1], (float)v[i][2], (float)v[i][3], scale);
      o.y = v8_encode4((float)v[i][4], (float)v[i][5], (float)v[i][6], (float)v[i][7], scale);
      *reinterpret_cast<uint2*>(codes + v8_offset(row, 8 * c, K, SW)) = o;
    }
  }
  if (lane == 0) scales[row] = scale;
}

int launch_quant_vocab_w8(const void* E, uint8_t* codes, float* scales, int V, int K, hipStream_t st) {
  if (!v8_kw(K) || K > 64 * 8 * V8_QMAXC || V < 1) return -1;
  const int cols = v8_cols(V);
  k_quant_vocab_w8<<<cols / 4, 256, 0, st>>>(reinterpret_cast<const half_t*>(E), codes, scales, V, cols, K, v8_sw(K)),
      wh_launched("k_quant_vocab_w8");
  return 0;
}

// ============================================================ the projection
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

// 8 codes -> the fp16 fragment of one k-step (v_cvt_scalef32_pk_f16_fp8, scale 1: exact)
WH_DEV Frag<half_t> v8_frag(unsigned c0, unsigned c1) {
  const u32x4_t w = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c0, 1.f, false)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c0, 1.f, true)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c1, 1.f, false)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c1, 1.f, true))};
  Frag<half_t> f;
  f.v = __builtin_bit_cast(half8_t, w);
  return f;
}

// Workgroup b owns the tiles [range_split(b), range_split(b + 1)) (12 or 13 at V = 51866, at
// most V8_TMAX: v8_grid), and its KW waves cut K into ranges of SW k-steps across all of them.
//  1. the final LayerNorm's operands (row wave, wave + KW, .. of the <= 8 fp32 residual rows)
//     and the scales of the columns this thread will store go out first;
//  2. then the wave's codes: a tile is 8 SW bytes per lane (half of k_vocab1's), so the ring is
//     D tiles deep, tile t + D - 1 issued while tile t is multiplied.  With D = V8_TMAX every
//     tile of the workgroup is requested before the first wait: 13 x 512 SW bytes per wave in
//     flight (32.5 KB at K = 1280, against 6 x 5 KB of k_vocab1<6>), in 2 SW registers each.
//     A workgroup of fewer than V8_TMAX tiles re-reads its last tile and stores nothing for it;
//  3. LayerNorm as k_vocab1 / k_proj1 compute it, the rows to LDS as fp16 (rows >= M: zeros);
//  4. per tile: its codes widened to fp16 fragments once they have landed (the later tiles
//     are still in flight under the conversions), SW MFMAs in ascending k, the partial tile to
//     LDS.  Per row the k order is the wave's SW k-steps ascending, the KW ranges in order;
//  5. per stored element: the KW partials summed in wave order, times the column's scale,
//     one write-through 16-byte store (scalar stores for a last group that crosses V).
template <int KW, int SW, int D>
__global__ __launch_bounds__(64 * KW) void k_vocab1_w8(GemmArgs a, const float* __restrict__ wscale) {
  CT_MARK(CT_VOCAB, 0);
  constexpr int K = KW * SW * 32, TMAX = V8_TMAX, XROW = K * 2 + 16, NT = 64 * KW;
  constexpr int CH = K / 4, CPL = (CH + 63) / 64, RPW = (8 + KW - 1) / KW;  // float4 chunks per row, per lane; rows per wave
  constexpr int NIT = (TMAX * 64 + NT - 1) / NT;                          // stored float4s per thread
  constexpr int TILE_B = 16 * K, WAVE_B = 512 * SW, N16 = SW / 2;
  static_assert(D >= 2 && D <= TMAX, "ring depth");
  extern __shared__ __attribute__((aligned(16))) char xs8[];
  float4_t* red = reinterpret_cast<float4_t*>(xs8 + 8 * XROW);  // [TMAX tiles][KW][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int nt = (a.N + 15) / 16, b = blockIdx.x, nb = gridDim.x;
  const int t0 = range_split(b, nt, nb), t1 = range_split(b + 1, nt, nb), ntl = t1 - t0;  // 1 <= ntl <= TMAX (launcher)
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(a.W) + wave * WAVE_B;
  auto load_tile = [&](int tl, unsigned (&c)[2 * SW]) {
    const uint8_t* p = wb + (int64_t)(t0 + min(tl, ntl - 1)) * TILE_B;
#pragma unroll
    for (int j = 0; j < N16; ++j) {
#if WH_NT
      const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p + j * 1024 + lane * 16));
#else
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(p + j * 1024 + lane * 16);
#endif
      c[4 * j] = v[0], c[4 * j + 1] = v[1], c[4 * j + 2] = v[2], c[4 * j + 3] = v[3];
    }
    if constexpr (SW & 1) {
#if WH_NT
      const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p + N16 * 1024 + lane * 8));
#else
      const u32x2_t v = *reinterpret_cast<const u32x2_t*>(p + N16 * 1024 + lane * 8);
#endif
      c[2 * SW - 2] = v[0], c[2 * SW - 1] = v[1];
    }
  };
  // 1. LayerNorm operands (clamped addresses, no branch around a load), then the scales
  float4_t xv[RPW][CPL], gv[CPL], bv[CPL];
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const float* xr = a.xf32 + (int64_t)min(wave + KW * j, a.M - 1) * K;
#pragma unroll
    for (int i = 0; i < CPL; ++i) xv[j][i] = load4f(xr + 4 * min(lane + 64 * i, CH - 1));
  }
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = min(lane + 64 * i, CH - 1);
    gv[i] = load4f(a.ln_g + 4 * c);
    bv[i] = load4f(a.ln_b + 4 * c);
  }
  float4_t sc[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + NT * it;
    sc[it] = load4f(wscale + (t0 + min(i >> 6, ntl - 1)) * 16 + 4 * ((i & 63) >> 4));
  }
  __builtin_amdgcn_sched_barrier(0);  // (in this order: the LayerNorm's waits then leave the codes in flight)
  // 2. the first D - 1 tiles of codes
  unsigned wc[D][2 * SW];
#pragma unroll
  for (int t = 0; t < D - 1; ++t) load_tile(t, wc[t]);
  __builtin_amdgcn_sched_barrier(0);  // every load above is issued before any wait
  // 3. LayerNorm, one wave per row
#pragma unroll
  for (int j = 0; j < RPW; ++j) {
    const int row = wave + KW * j;
    if (row >= 8) break;
    half_t* dst = reinterpret_cast<half_t*>(xs8 + row * XROW);
    if (row >= a.M) {
      for (int c = lane; c < CH; c += 64) store4(dst + 4 * c, 0.f, 0.f, 0.f, 0.f);
      continue;
    }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      if (lane + 64 * i < CH) sm += xv[j][i][0] + xv[j][i][1] + xv[j][i][2] + xv[j][i][3];
    const float mean = wave_sum(sm) / (float)K;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      if (lane + 64 * i < CH) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xv[j][i][e] - mean;
          q += d * d;
        }
      }
    const float rstd = rsqrtf(wave_sum(q) / (float)K + a.ln_eps);
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      if (lane + 64 * i < CH) {
        const float4_t v = xv[j][i];
        store4(dst + 4 * (lane + 64 * i), (v[0] - mean) * rstd * gv[i][0] + bv[i][0],
               (v[1] - mean) * rstd * gv[i][1] + bv[i][1], (v[2] - mean) * rstd * gv[i][2] + bv[i][2],
               (v[3] - mean) * rstd * gv[i][3] + bv[i][3]);
      }
  }
  __syncthreads();
  // this wave's X fragments (rows r < 8 valid; rows 8..15 repeat row 7, never stored)
  Frag<half_t> xf[SW];
#pragma unroll
  for (int s = 0; s < SW; ++s)
    frag_load(xf[s], reinterpret_cast<const half_t*>(xs8 + min(r, 7) * XROW) + (wave * SW + s) * 32 + 8 * g);
  // 4. the tiles
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    if (t + D - 1 < TMAX) load_tile(t + D - 1, wc[(t + D - 1) % D]);
    float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SW; ++s) mfma_step(acc, v8_frag(wc[t % D][2 * s], wc[t % D][2 * s + 1]), xf[s]);
    if (t < ntl) red[(t * KW + wave) * 64 + lane] = acc;
  }
  __syncthreads();
  // 5. lane (r, g) of a tile: row r, columns 4g .. +3
  const auto rs = wt_rsrc(a.out_f32);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + NT * it;
    if (i >= ntl * 64) break;
    const int tl = i >> 6, ln = i & 63, rr = ln & 15, n = (t0 + tl) * 16 + 4 * (ln >> 4);
    float4_t v = red[(tl * KW) * 64 + ln];
#pragma unroll
    for (int w = 1; w < KW; ++w) v += red[(tl * KW + w) * 64 + ln];
    v *= sc[it];
    if (rr < a.M) {
      if (n + 3 < a.N) {
        wt_store4(rs, (rr * a.ldo + n) * 4, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < a.N) wt_store1(rs, (rr * a.ldo + n + e) * 4, v[e]);
      }
    }
  }
  CT_END(CT_VOCAB);
}

namespace {
template <int KW, int SW, int D>
int v8_go(const GemmArgs& a, const float* wscale, hipStream_t st) {
  constexpr int K = KW * SW * 32, LDS = 8 * (K * 2 + 16) + V8_TMAX * KW * 64 * 16;
  static_assert(LDS <= 160 * 1024, "k_vocab1_w8 LDS");
  static bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vocab1_w8<KW, SW, D>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, LDS) == hipSuccess;
  if (!attr) return -5;
  k_vocab1_w8<KW, SW, D><<<v8_grid(a.N), 64 * KW, LDS, st>>>(a, wscale), wh_launched("k_vocab1_w8");
  return 0;
}
}  // namespace

int launch_vocab1_w8(const GemmArgs& a, const float* wscale, hipStream_t st) {
  // the shapes served: wh_vocab_pick.h (the switch below holds one case per width it admits)
  if (vocab_kernel(2, a.M, a.N, a.K, a.xf32 != nullptr, true) != VK_VOCAB1_W8 || a.ldo < a.N || !a.W || !wscale || !a.ln_g ||
      !a.ln_b || !a.out_f32 || a.bias || a.x_rows)
    return -1;
  switch (a.K) {  //                 KW SW  D
    case 1280: return v8_go<v8_kw(1280), v8_sw(1280), V8_TMAX>(a, wscale, st);
    case 1024: return v8_go<v8_kw(1024), v8_sw(1024), V8_TMAX>(a, wscale, st);
    case 768: return v8_go<v8_kw(768), v8_sw(768), V8_TMAX>(a, wscale, st);
    case 512: return v8_go<v8_kw(512), v8_sw(512), V8_TMAX>(a, wscale, st);
    case 384: return v8_go<v8_kw(384), v8_sw(384), V8_TMAX>(a, wscale, st);
    case 128: return v8_go<v8_kw(128), v8_sw(128), V8_TMAX>(a, wscale, st);
    default: return -1;
  }
}

}  // namespace wh

#if WH_TUNING
WH_CT_READER(vocab8)
#endif
