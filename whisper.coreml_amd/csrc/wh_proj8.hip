// decoder="fp8" (wh_set_decoder_format): the single-window step's projections over 8-bit
// (OCP FP8 E4M3) copies of the decoder's linear weights, one fp32 scale per output channel.
//   * k_quant_dec_w8: one wave per weight row, the row in registers, amax by the wave
//     butterfly, codes written in k_proj1<w8>'s fragment order (wh_proj8.h);
//   * k_proj1_w8: k_proj1 (wh_proj.h) with the weight stream halved.  Activations stay fp16,
//     the MFMA is the fp16 one, accumulation fp32; a code becomes its fp16 value exactly
//     (every E4M3 value is an fp16 value) in registers, and the column's scale multiplies the
//     fp32 tile once, before anything leaves the workgroup.
// A translation unit of its own: the native k_proj1 code objects (wh_proj.hip) do not change.
// The chain-trace marks (tuning build) are k_proj1's, in this unit's own table
// (wh_tune_ct_trace_proj8).
#include <hip/hip_ext.h>

#include "wh_proj.h"
#include "wh_proj8.h"

namespace wh {

// ============================================================ quantiser
// 4 fp32 values -> 4 E4M3 codes, round to nearest even (v_cvt_pk_fp8_f32; gfx950: OCP E4M3).
// x / scale is an IEEE fp32 division, clamped to +-448: never the NaN code (a NaN input
// clamps to -448).  scale == 0 (an all-zero row): codes 0.  (wh_gemm8.hip encode4's rule)
WH_DEV unsigned w8_encode4(float x0, float x1, float x2, float x3, float scale) {
  auto q = [&](float x) { return scale > 0.f ? fminf(fmaxf(x / scale, -448.f), 448.f) : 0.f; };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x0), q(x1), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x2), q(x3), w, true);
  return (unsigned)w;
}

constexpr int W8_QMAXC = 16;  // 8-element chunks per lane: K <= 64 * 8 * 16 = 8192

// Lane l holds the chunks l, l + 64, .. of its wave's row: every load is issued before the
// reduction.  Chunk c (k = 8 c .. + 7) is (s, g) = ((c / 4) % ns, c % 4) of range c / (4 ns)
// and lands at 8-byte slot range * 4 ns + g * ns + s.
__global__ __launch_bounds__(256) void k_quant_dec_w8(const half_t* __restrict__ w, uint8_t* __restrict__ codes,
                                                      float* __restrict__ scales, int rows, int K, int ns) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const half_t* wr = w + (int64_t)row * K;
  const int nch = K >> 3;
  half8_t v[W8_QMAXC];
#pragma unroll
  for (int i = 0; i < W8_QMAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) v[i] = *reinterpret_cast<const half8_t*>(wr + 8 * c);
  }
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < W8_QMAXC; ++i)
    if (lane + 64 * i < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)v[i][e]));
    }
  const float scale = wave_max(am) / 448.f;
  uint2* cr = reinterpret_cast<uint2*>(codes + (int64_t)row * K);
#pragma unroll
  for (int i = 0; i < W8_QMAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const int range = c / (4 * ns), q = c - range * 4 * ns;
      uint2 o;
      o.x = w8_encode4((float)v[i][0], (float)v[i][1], (float)v[i][2], (float)v[i][3], scale);
      o.y = w8_encode4((float)v[i][4], (float)v[i][5], (float)v[i][6], (float)v[i][7], scale);
      cr[range * 4 * ns + (q & 3) * ns + (q >> 2)] = o;
    }
  }
  if (lane == 0) scales[row] = scale;
}

int launch_quant_dec_w8(const void* w, uint8_t* codes, float* scales, int rows, int K, int ns, hipStream_t st) {
  if (ns < 1 || K % (ns * 32) || K > 64 * 8 * W8_QMAXC) return -1;
  k_quant_dec_w8<<<(rows + 3) / 4, 256, 0, st>>>(reinterpret_cast<const half_t*>(w), codes, scales, rows, K, ns),
      wh_launched("k_quant_dec_w8");
  return 0;
}

// ============================================================ k_proj1 over the codes
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
// a lane's run starts at a multiple of 8 bytes (NSTEP * 8 per lane group), not of 16
typedef u32x4_t u32x4_a8_t __attribute__((aligned(8)));

// the lane's NSTEP * 8 codes: 16-byte loads and, for an odd NSTEP, one 8-byte load
// (the once-read stream of frag_load_stream: nontemporal when built with WH_NT=1)
template <int NSTEP>
WH_DEV void w8_load_stream(unsigned (&c)[2 * NSTEP], const uint8_t* p) {
#pragma unroll
  for (int i = 0; i + 1 < NSTEP; i += 2) {
#if WH_NT
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a8_t*>(p + 8 * i));
#else
    const u32x4_t v = *reinterpret_cast<const u32x4_a8_t*>(p + 8 * i);
#endif
    c[2 * i] = v[0], c[2 * i + 1] = v[1], c[2 * i + 2] = v[2], c[2 * i + 3] = v[3];
  }
  if constexpr (NSTEP & 1) {
#if WH_NT
    const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p + 8 * (NSTEP - 1)));
#else
    const u32x2_t v = *reinterpret_cast<const u32x2_t*>(p + 8 * (NSTEP - 1));
#endif
    c[2 * NSTEP - 2] = v[0], c[2 * NSTEP - 1] = v[1];
  }
}
// 8 codes -> the fp16 fragment of one k-step (v_cvt_scalef32_pk_f16_fp8, scale 1: exact)
WH_DEV Frag<half_t> w8_frag(unsigned c0, unsigned c1) {
  const u32x4_t w = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c0, 1.f, false)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c0, 1.f, true)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c1, 1.f, false)),
                     __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c1, 1.f, true))};
  Frag<half_t> f;
  f.v = __builtin_bit_cast(half8_t, w);
  return f;
}

// k_proj1<half_t, ..> step for step (wh_proj.h: tiling, LayerNorm prologue, pending / deferred
// residual, in-launch split-K, epilogues), except:
//  2. the wave's weights are NSTEP * 8 codes per lane (a.W: the codes, wh_proj8.h layout) and
//     the lane's 4 column scales, issued with every other operand before the first wait;
//  4. a k-step's 8 codes are converted to its fp16 fragment right before its MFMA (the
//     compiler moves the conversions of landed codes under the LayerNorm math);
//  5. the scales multiply the fp32 tile after the fixed-order sum of the KW wave tiles, so
//     the split-K slabs, the deferred slabs and every epilogue see scaled values.
template <int NSUB, int KW, int NSTEP, int ZS, int CPL, int EPI, int MODE>
__global__ __launch_bounds__(64 * NSUB * KW) void k_proj1_w8(GemmArgs a, const float* __restrict__ wscale) {
  typedef half_t T;
  using P = Proj1Shape<T, NSUB, KW, NSTEP, CPL>;
  constexpr bool LN = CPL > 0;
  constexpr bool PEND = LN && (MODE & P1_PEND), DEFER = (MODE & P1_DEFER) && ZS == 2 && EPI == EPI_RESID;
  constexpr int NWV = NSUB * KW;
  constexpr int RPW = (P1_RMAX + NWV - 1) / NWV;  // LayerNorm rows per wave
  extern __shared__ __attribute__((aligned(16))) char xs[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int sub = wave % NSUB, kw = wave / NSUB;
  const int R = a.M, K = a.K, kz = blockIdx.y;
  const int tile = blockIdx.x * NSUB + sub;  // this wave's 16-column tile
  const int n0 = tile * 16;
  const int kb = kz * P::KC;               // this workgroup's K range [kb, kb + KC)
  const int kw0 = kb + kw * NSTEP * 32;    // this wave's
  const int ct_slot = a.N == a.K ? CT_PROJ_NN : a.N == 3 * a.K ? CT_PROJ_QKV : a.N == 4 * a.K ? CT_PROJ_FC1 : CT_PROJ_FC2;
  CT_MARK(ct_slot, 0);

  // 1. activations (clamped addresses, no branch around a load)
  const int CH = K / 4;  // LN: float4 chunks per residual row
  float4_t xv[LN ? RPW : 1][LN ? CPL : 1], gv[LN ? CPL : 1], bv[LN ? CPL : 1];
  float4_t s0v[PEND ? RPW : 1][PEND ? CPL : 1], s1v[PEND ? RPW : 1][PEND ? CPL : 1], rbv[PEND ? CPL : 1];
  Frag<T> xf[LN ? 1 : NSTEP];
  if constexpr (LN) {
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const float* xr = a.xf32 + (int64_t)min(wave + NWV * j, R - 1) * K;
#pragma unroll
      for (int i = 0; i < CPL; ++i) xv[j][i] = load4f(xr + 4 * min(lane + 64 * i, CH - 1));
    }
    if constexpr (PEND) {
      // the pending residual's two K-half slabs, row-major [2][R][K] like the rows
#pragma unroll
      for (int j = 0; j < RPW; ++j) {
        const int row = min(wave + NWV * j, R - 1);
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int off = row * K + 4 * min(lane + 64 * i, CH - 1);
          s0v[j][i] = load4f(a.res_slab + off);
          s1v[j][i] = load4f(a.res_slab + R * K + off);
        }
      }
#pragma unroll
      for (int i = 0; i < CPL; ++i) rbv[i] = load4f(a.res_bias + 4 * min(lane + 64 * i, CH - 1));
    }
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = min(lane + 64 * i, CH - 1);
      gv[i] = load4f(a.ln_g + 4 * c);
      bv[i] = load4f(a.ln_b + 4 * c);
    }
  } else {
    const T* xp = reinterpret_cast<const T*>(a.X) + (int64_t)min(r, R - 1) * a.ldx + kw0 + 8 * g;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) frag_load(xf[s], xp + s * 32);
  }
  // 2. the wave's weight codes: 16 columns x NSTEP k-steps, one run per lane
  unsigned wc[2 * NSTEP];
  w8_load_stream<NSTEP>(wc, reinterpret_cast<const uint8_t*>(a.W) + (int64_t)min(n0 + r, a.N - 1) * K + kw0 + NSTEP * 8 * g);
  // the scales of the lane's accumulator columns, and the epilogue's operands, ride in the
  // same round trip
  const int n = n0 + 4 * g, re = min(r, R - 1);
  const float4_t wsc = load4f(wscale + n);
  float4_t pre_b = (float4_t){0.f, 0.f, 0.f, 0.f}, pre_x = (float4_t){0.f, 0.f, 0.f, 0.f};
  if constexpr (!DEFER) pre_b = load4f(a.bias + n);
  if constexpr (EPI == EPI_RESID && !DEFER) pre_x = load4f(a.out_f32 + (int64_t)re * a.ldo + n);
  // every load above is issued before any wait
  __builtin_amdgcn_sched_barrier(0);

  // 3. LayerNorm of the full rows (k_proj1's arithmetic); this workgroup's K range -> LDS
  if constexpr (LN) {
    if constexpr (PEND) {
      // x_new = x + ((slab0 + slab1) + bias): the order of the in-launch reduction
#pragma unroll
      for (int j = 0; j < RPW; ++j)
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          float4_t t = s0v[j][i] + s1v[j][i];
          t += rbv[i];
          xv[j][i] += t;
        }
      if (blockIdx.x == 0 && blockIdx.y == 0) {  // one workgroup publishes x_new
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
          const int row = wave + NWV * j;
          if (row < R) {
#pragma unroll
            for (int i = 0; i < CPL; ++i)
              if (lane + 64 * i < CH) {
                const float4_t v = xv[j][i];
                store4(a.x_out + (int64_t)row * K + 4 * (lane + 64 * i), v[0], v[1], v[2], v[3]);
              }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int row = wave + NWV * j;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CPL; ++i)
        if (lane + 64 * i < CH) s += xv[j][i][0] + xv[j][i][1] + xv[j][i][2] + xv[j][i][3];
      const float mean = wave_sum(s) / (float)K;
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
      if (row < R) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int k = 4 * (lane + 64 * i) - kb;
          if (k >= 0 && k < P::KC) {
            const float4_t v = xv[j][i];
            store4(reinterpret_cast<T*>(xs + row * P::XROW) + k, (v[0] - mean) * rstd * gv[i][0] + bv[i][0],
                   (v[1] - mean) * rstd * gv[i][1] + bv[i][1], (v[2] - mean) * rstd * gv[i][2] + bv[i][2],
                   (v[3] - mean) * rstd * gv[i][3] + bv[i][3]);
          }
        }
      }
    }
    __syncthreads();
  }

  // 4. codes -> fp16 fragments, MFMAs in load order
  float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
  if constexpr (LN) {
    const char* xl = xs + min(r, R - 1) * P::XROW + (kw * NSTEP * 32 + 8 * g) * (int)sizeof(T);
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      Frag<T> x1;
      frag_load(x1, reinterpret_cast<const T*>(xl + s * 32 * (int)sizeof(T)));
      mfma_step(acc, w8_frag(wc[2 * s], wc[2 * s + 1]), x1);
    }
  } else {
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) mfma_step(acc, w8_frag(wc[2 * s], wc[2 * s + 1]), xf[s]);
  }

  // 5. fixed-order sum of the KW wave tiles, then the columns' scales
  if constexpr (KW > 1) {
    if constexpr (LN) __syncthreads();  // xs is reused
    float4_t* red = reinterpret_cast<float4_t*>(xs);  // [KW-1][NSUB][64]
    if (kw > 0) red[((kw - 1) * NSUB + sub) * 64 + lane] = acc;
    __syncthreads();
    if (kw > 0) return;  // (thread 0 is kw 0)
#pragma unroll
    for (int q = 1; q < KW; ++q) acc += red[((q - 1) * NSUB + sub) * 64 + lane];
  }
  acc *= wsc;

  // 6. split-K: the column tile's ZS workgroups meet; the last to arrive sums the slabs
  // (k_proj1's write-through form: sc1 slab store drained by its wave, relaxed agent counter)
  if constexpr (ZS > 1) {
    const int ntile = gridDim.x * NSUB;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(a.p1_slab, 0, 0x7fffffff, 0x00020000);
    if constexpr (DEFER) {  // row-major [2][R][N] for the next LayerNorm prologue, which sums them
      if (r < R) store4(a.p1_slab + ((int64_t)kz * R + r) * a.N + n, acc[0], acc[1], acc[2], acc[3]);
      CT_END(ct_slot);
      return;
    }
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc), rs, ((kz * ntile + tile) * 256 + lane * 4) * 4,
                                           0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(a.p1_cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    if (ticket != ZS - 1) {
      CT_END(ct_slot);
      return;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the add
    if (lane == 0) __hip_atomic_store(a.p1_cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float4_t pv[ZS];  // every slab load issued before the first add; summed in slice order
#pragma unroll
    for (int s = 0; s < ZS; ++s)
      pv[s] = __builtin_bit_cast(float4_t,
                                 __builtin_amdgcn_raw_buffer_load_b128(rs, ((s * ntile + tile) * 256 + lane * 4) * 4, 0, 16));
    acc = pv[0];
#pragma unroll
    for (int s = 1; s < ZS; ++s) acc += pv[s];
  }

  // 7. epilogue: lane holds Y[r][n0 + 4g .. +3]
  if (r >= R) {
    CT_END(ct_slot);
    return;
  }
  acc += pre_b;
  if constexpr (EPI == EPI_RESID) {
    pre_x += acc;
    store4(a.out_f32 + (int64_t)r * a.ldo + n, pre_x[0], pre_x[1], pre_x[2], pre_x[3]);
  } else {
    epilogue_store<T, EPI>(a, r, 0, r, n, acc);
  }
  CT_END(ct_slot);
}

// ------------------------------------------------------------ launch
// The configurations are launch_proj1<half_t>'s (wh_proj.hip), width by width: the code
// layout depends on NS alone (p1_nstep), the grid and the LDS on the rest.
namespace {
template <int NSUB, int KW, int NS, int ZS, int CPL, int EPI, int MODE = 0>
int p18_go(const GemmArgs& a, const float* wscale, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  using P = Proj1Shape<half_t, NSUB, KW, NS, CPL>;
  static_assert(P::LDS <= 64 * 1024, "k_proj1_w8 LDS");
  static_assert(NSUB * KW <= 16, "k_proj1_w8 waves");
  if (a.K != ZS * P::KC || a.N % (16 * NSUB)) return -1;
  if (ZS > 1 && (!a.p1_slab || !a.p1_cnt || (int64_t)ZS * (a.N / 16) > a.p1_slabs)) return -1;
  if ((MODE & P1_PEND) && (!a.res_slab || !a.res_bias || !a.x_out || a.x_out == a.xf32)) return -1;
  const dim3 grid(a.N / (16 * NSUB), ZS), block(64 * NSUB * KW);
  void (*f)(GemmArgs, const float*) = &k_proj1_w8<NSUB, KW, NS, ZS, CPL, EPI, MODE>;
  if (ev0)
    hipExtLaunchKernelGGL(f, grid, block, P::LDS, st, ev0, ev1, 0, a, wscale), wh_launched("k_proj1<w8>");
  else {
    hipLaunchKernelGGL(f, grid, block, P::LDS, st, a, wscale);
    wh_launched("k_proj1<w8>");
  }
  return 0;
}

// one model width: the ten kernels its step uses (p1_width_launch's rows)
template <int CPL, int BKW, int NS, int F1SUB>
int p18_width_launch(const GemmArgs& a, const float* ws, int epi, bool ln, int n, hipStream_t st, hipEvent_t e0,
                     hipEvent_t e1) {
  if (ln) {
    if (a.K != n) return -1;
    if (a.res_slab) {  // a deferred residual is pending on the input rows
      if (epi == EPI_QKV_DEC && a.N == 3 * n) return p18_go<1, BKW, NS, 1, CPL, EPI_QKV_DEC, P1_PEND>(a, ws, st, e0, e1);
      // (16 columns per workgroup whatever F1SUB: at n = 1280 the 16-wave form has 128 registers
      // per lane and two more row copies to hold; the sums are the same, whole K per wave tile)
      if (epi == EPI_STORE_GELU && a.N == 4 * n) return p18_go<1, BKW, NS, 1, CPL, EPI_STORE_GELU, P1_PEND>(a, ws, st, e0, e1);
      if (epi == EPI_STORE && a.N == n) return p18_go<1, BKW, NS, 1, CPL, EPI_STORE, P1_PEND>(a, ws, st, e0, e1);
      return -1;
    }
    if (epi == EPI_QKV_DEC && a.N == 3 * n) return p18_go<1, BKW, NS, 1, CPL, EPI_QKV_DEC>(a, ws, st, e0, e1);
    if (epi == EPI_STORE_GELU && a.N == 4 * n) return p18_go<F1SUB, BKW, NS, 1, CPL, EPI_STORE_GELU>(a, ws, st, e0, e1);
    if (epi == EPI_STORE && a.N == n) return p18_go<1, BKW, NS, 1, CPL, EPI_STORE>(a, ws, st, e0, e1);
    return -1;
  }
  if (epi != EPI_RESID || a.N != n) return -1;
  if (a.p1_defer) {
    if (a.K == n) return p18_go<1, BKW / 2, NS, 2, 0, EPI_RESID, P1_DEFER>(a, ws, st, e0, e1);
    if (a.K == 4 * n) return p18_go<1, 2 * BKW, NS, 2, 0, EPI_RESID, P1_DEFER>(a, ws, st, e0, e1);
    return -1;
  }
  if (a.K == n) return p18_go<1, BKW / 2, NS, 2, 0, EPI_RESID>(a, ws, st, e0, e1);
  if (a.K == 4 * n) return p18_go<1, 2 * BKW, NS, 2, 0, EPI_RESID>(a, ws, st, e0, e1);
  return -1;
}
}  // namespace

int launch_proj1_w8(const GemmArgs& a, const float* wscale, int epi, bool ln, hipStream_t st, hipEvent_t ev0,
                    hipEvent_t ev1) {
  if (a.M < 1 || a.M > P1_RMAX || a.N % 16 || !a.bias || !a.W || !wscale) return -1;
  if (ln && (!a.xf32 || !a.ln_g || !a.ln_b)) return -1;
  const int n = ln ? a.K : a.N;
  switch (n) {  //                               CPL BKW NS F1SUB    (NS: p1_nstep(n), the code layout's)
    case 1280: return p18_width_launch<5, 8, p1_nstep(1280), 2>(a, wscale, epi, ln, n, st, ev0, ev1);
    case 1024: return p18_width_launch<4, 8, p1_nstep(1024), 1>(a, wscale, epi, ln, n, st, ev0, ev1);
    case 768: return p18_width_launch<3, 8, p1_nstep(768), 1>(a, wscale, epi, ln, n, st, ev0, ev1);
    case 512: return p18_width_launch<2, 8, p1_nstep(512), 1>(a, wscale, epi, ln, n, st, ev0, ev1);
    case 384: return p18_width_launch<2, 4, p1_nstep(384), 1>(a, wscale, epi, ln, n, st, ev0, ev1);
    case 128: return p18_width_launch<1, 4, p1_nstep(128), 1>(a, wscale, epi, ln, n, st, ev0, ev1);
    default: return -1;
  }
}

}  // namespace wh

#if WH_TUNING
WH_CT_READER(proj8)
#endif
