// The encoder's 8-bit GEMM path (encoder="fp8", wh_set_encoder_format): OCP FP8 E4M3 codes
// with one fp32 scale per activation row and per weight output channel, multiplied by the
// gfx950 16x16x128 8-bit MFMA with fp32 accumulation.
//
//   Y[m][n] = sa[m] * sw[n] * sum_k X8[m][k] W8[n][k]   (+ bias, then the fp16 path's epilogue)
//
//   * k_quant_rows / k_quant_weights / k_layernorm_quant: one wave per row, the row in
//     registers, amax by the wave butterfly, scale = amax / 448, code = e4m3(clamp(x / scale)).
//   * k_gemm8: the tile GEMM over the codes.
#include "wh_gemm8.h"

namespace wh {

// ============================================================ quantisers
// 4 fp32 values -> 4 E4M3 codes, round to nearest even (v_cvt_pk_fp8_f32; gfx950: OCP E4M3).
// q = x / scale is an IEEE fp32 division, clamped to +-448: never the NaN code (a NaN input
// clamps to -448).  scale == 0 (an all-zero row): codes 0.
WH_DEV unsigned encode4(float x0, float x1, float x2, float x3, float scale) {
  auto q = [&](float x) { return scale > 0.f ? fminf(fmaxf(x / scale, -448.f), 448.f) : 0.f; };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x0), q(x1), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(q(x2), q(x3), w, true);
  return (unsigned)w;
}

constexpr int QMAXC = 16;  // 8-element chunks per lane: K <= 64 * 8 * 16 = 8192

// one wave: fp16 row xr[K] -> codes cr[K], *sc = amax / 448.  Lane l holds the chunks
// l, l + 64, ..: every load of the row is issued before the reduction.
WH_DEV void quant_row(const half_t* __restrict__ xr, uint8_t* __restrict__ cr, float* __restrict__ sc, int K, int lane) {
  const int nch = K >> 3;
  half8_t v[QMAXC];
#pragma unroll
  for (int i = 0; i < QMAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) v[i] = *reinterpret_cast<const half8_t*>(xr + 8 * c);
  }
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < QMAXC; ++i)
    if (lane + 64 * i < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) am = fmaxf(am, fabsf((float)v[i][e]));
    }
  const float scale = wave_max(am) / 448.f;
#pragma unroll
  for (int i = 0; i < QMAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      uint2 o;
      o.x = encode4((float)v[i][0], (float)v[i][1], (float)v[i][2], (float)v[i][3], scale);
      o.y = encode4((float)v[i][4], (float)v[i][5], (float)v[i][6], (float)v[i][7], scale);
      *reinterpret_cast<uint2*>(cr + 8 * c) = o;
    }
  }
  if (lane == 0) *sc = scale;
}

// activations: the inputs of attention-out (att_e) and fc2 (hm_e), whose row amax spans every
// N tile of the GEMM that wrote them
__global__ __launch_bounds__(256) void k_quant_rows(const half_t* __restrict__ x, uint8_t* __restrict__ codes,
                                                    float* __restrict__ scales, int rows, int K) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  quant_row(x + (int64_t)row * K, codes + (int64_t)row * K, scales + row, K, threadIdx.x & 63);
}

// weights [out][in]: one scale per output channel; run once per weight (finalize / format set)
__global__ __launch_bounds__(256) void k_quant_weights(const half_t* __restrict__ w, uint8_t* __restrict__ codes,
                                                       float* __restrict__ scales, int rows, int K) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  quant_row(w + (int64_t)row * K, codes + (int64_t)row * K, scales + row, K, threadIdx.x & 63);
}

// k_layernorm (wh_kernels.hip) with the fp16 result quantised in the same pass: the inputs
// of QKV and fc1.  The normalised value is rounded to fp16 first (what the fp16 path stores
// and k_quant_rows would read), then the row's amax / scale / codes as quant_row.
__global__ __launch_bounds__(256) void k_layernorm_quant(const float* __restrict__ x, uint8_t* __restrict__ codes,
                                                         float* __restrict__ scales, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int rows, int n, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * n;
  constexpr int MAXV = 8;  // n <= 2048
  float4_t v[MAXV];
  const int nv = n >> 2;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) v[i] = load4f(xr + 4 * c);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + 64 * i < nv) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  const float mean = wave_sum(s) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + 64 * i < nv) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  const float rstd = rsqrtf(wave_sum(q) / (float)n + eps);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) {
      const float4_t gm = load4f(gamma + 4 * c), bt = load4f(beta + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[i][j] = (float)(half_t)((v[i][j] - mean) * rstd * gm[j] + bt[j]);
        am = fmaxf(am, fabsf(v[i][j]));
      }
    }
  }
  const float scale = wave_max(am) / 448.f;
  unsigned* cr = reinterpret_cast<unsigned*>(codes + (int64_t)row * n);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + 64 * i;
    if (c < nv) cr[c] = encode4(v[i][0], v[i][1], v[i][2], v[i][3], scale);
  }
  if (lane == 0) scales[row] = scale;
}

void launch_quant_rows(const void* x, uint8_t* codes, float* scales, int rows, int K, hipStream_t st) {
  if (rows <= 0) return;
  k_quant_rows<<<(rows + 3) / 4, 256, 0, st>>>(reinterpret_cast<const half_t*>(x), codes, scales, rows, K),
      wh_launched("k_quant_rows");
}
void launch_quant_weights(const void* w, uint8_t* codes, float* scales, int rows, int K, hipStream_t st) {
  if (rows <= 0) return;
  k_quant_weights<<<(rows + 3) / 4, 256, 0, st>>>(reinterpret_cast<const half_t*>(w), codes, scales, rows, K),
      wh_launched("k_quant_weights");
}
void launch_layernorm_quant(const float* x, uint8_t* codes, float* scales, const float* g, const float* b, int rows,
                            int n, float eps, hipStream_t st) {
  if (rows <= 0) return;
  k_layernorm_quant<<<(rows + 3) / 4, 256, 0, st>>>(x, codes, scales, g, b, rows, n, eps), wh_launched("k_layernorm_quant");
}

// ============================================================ k_gemm8
// Workgroup tile BM x BN = (WM MI 16) x (WN NI 16) over WM x WN waves, K-tile 128 codes (128 B
// per row: the LDS bytes per stage of the fp16 kernel's 64-deep tile).  One
// v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 block and K-tile, both operands E4M3 (cbsz =
// blgp = 0) with unit block scales (E8M0 127); as everywhere here the swapped product
// D^T = W X^T, so a lane ends with 4 consecutive columns of one row.  A lane's operand is the
// 32 bytes k = 32 g .. 32 g + 31 of its row for both operands (the contraction only needs the
// two to agree): a fragment is 8 VGPRs, twice the fp16 kernel's, so a phase holds half the
// fragments for the same bytes.
//
// LDS: two buffers of four regions, A0 | A1 | B0 | B1.  A_h holds, for every wave row, the
// h-th half (MI 8 rows) of that wave row's rows, B_h for every wave column the h-th half of
// its columns; rows are 128 B, and the 16 B chunk c of region row lr sits at chunk position
// c ^ ((lr >> 1) & 7): 16 lanes reading the same k chunk of 16 consecutive rows cover all 64
// banks once (conflict-free ds_read_b128), and the global_load_lds staging (lane-linear in
// LDS, 8 rows per wave instruction) applies the same xor to the chunk it fetches.
//
// K-tile t (buffer t & 1) is four phases, one quadrant of the wave tile each, in the order
// Q(0,0) Q(0,1) Q(1,1) Q(1,0) so a phase re-reads only one operand half:
//     phase:  read the half it lacks (A0+B0 | B1 | A1 | B0);  barrier;
//             issue that half's region of tile t+2 into THIS buffer (every wave has read it);
//             MI/2 x NI/2 MFMAs
// The last phase waits, before its barrier, with one counted s_waitcnt vmcnt until only the
// three regions of tile t+2 issued so far are outstanding: tile t+1 has landed, and every
// region has had more than a tile of MFMAs to do so.  The loads stay in flight across the
// barriers (raw s_barrier: a __syncthreads() would drain them).
namespace g8 {
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
constexpr int UNIT = 0x7f7f7f7f;  // E8M0 2^0 in whichever byte the instruction selects

WH_DEV void raw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}
WH_DEV void glds16(const char* src, char* lds) {
  __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)(src),
                                   (__attribute__((address_space(3))) void*)(lds), 16, 0, 0);
}
template <int N>
WH_DEV void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
}  // namespace g8

template <int EPI, int WM, int WN, int MI, int NI>
__global__ __launch_bounds__(64 * WM * WN, WM * WN == 8 ? 1 : 2) void k_gemm8(GemmArgs a, const float* __restrict__ sa,
                                                                              const float* __restrict__ sw) {
  using namespace g8;
  constexpr int NW = WM * WN, BM = WM * MI * 16, BN = WN * NI * 16, MH = MI / 2, NH = NI / 2;
  constexpr int AROWS = MH * 16, BROWS = NH * 16;           // rows of a wave's half
  constexpr int REG_A = BM * 64, REG_B = BN * 64;            // bytes of a region (half an operand's tile)
  constexpr int BUF = 2 * REG_A + 2 * REG_B;
  constexpr int NA = BM / 16 / NW, NB = BN / 16 / NW;        // staging instructions per wave and region
  static_assert(MI % 2 == 0 && NI % 2 == 0 && NA >= 1 && NB >= 1 && BM % (16 * NW) == 0 && BN % (16 * NW) == 0, "tile shape");
  __shared__ __attribute__((aligned(1024))) char smem[2 * BUF];  // the kernel's only LDS object

  const int ntn = a.N / BN;
  const int ntm = (a.M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, ntm * ntn);
  const int tm = bid / ntn, tn = bid % ntn;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WN, wc = wave % WN;
  const int r = lane & 15, g = lane >> 4;

  // staging: instruction j of this wave fills region rows (wave N_ + j) 8 .. + 7; lane -> row
  // lane >> 3, chunk position lane & 7, fetching the chunk the swizzle puts there.  A wave's
  // rows of a region lie in one wave row / column (static_assert), so instruction j of half h
  // is 8 j + h x (rows of a half) rows below the wave's first: one row index per operand stays
  // in registers and the byte offset (< 2^31: launcher) is formed at the load.
  static_assert(AROWS % (8 * NA) == 0 && BROWS % (8 * NB) == 0, "a wave's staging rows stay in one half");
  const char* X = reinterpret_cast<const char*>(a.X);
  const char* W = reinterpret_cast<const char*>(a.W);
  const int l3 = lane >> 3;
  const int am0 = m0 + ((wave * NA * 8) / AROWS) * (MI * 16) + (wave * NA * 8) % AROWS + l3;
  const int bn0 = n0 + ((wave * NB * 8) / BROWS) * (NI * 16) + (wave * NB * 8) % BROWS + l3;
  auto chunk = [&](int inst) { return ((lane & 7) ^ ((4 * inst + (l3 >> 1)) & 7)) << 4; };  // region row inst * 8 + l3
  auto stage_a = [&](int buf, int h, int kt) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int m = min(am0 + h * AROWS + 8 * j, a.M - 1);  // the M tail re-reads the last row (never stored)
      glds16(X + (m * a.K + chunk(wave * NA + j) + kt * G8_BK), smem + buf * BUF + h * REG_A + (wave * NA + j) * 1024);
    }
  };
  auto stage_b = [&](int buf, int h, int kt) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
      glds16(W + ((bn0 + h * BROWS + 8 * j) * a.K + chunk(wave * NB + j) + kt * G8_BK),
             smem + buf * BUF + 2 * REG_A + h * REG_B + (wave * NB + j) * 1024);
  };

  // fragment reads: lane (r, g) reads chunks 2g, 2g + 1 of its row (a fragment's region rows
  // start at a multiple of 16, so the swizzle term is (r >> 1) & 7)
  const int roff = r * G8_BK + (((2 * g) ^ ((r >> 1) & 7)) << 4);
  i32x8_t af[MH], bf[NH];
  auto frag = [&](const char* p) {
    const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(p + roff), hi = *reinterpret_cast<const i32x4_t*>(p + (roff ^ 16));
    return (i32x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  auto read_a = [&](int buf, int h) {
    const char* base = smem + buf * BUF + h * REG_A + wr * AROWS * G8_BK;
#pragma unroll
    for (int mi = 0; mi < MH; ++mi) af[mi] = frag(base + mi * 16 * G8_BK);
  };
  auto read_b = [&](int buf, int h) {
    const char* base = smem + buf * BUF + 2 * REG_A + h * REG_B + wc * BROWS * G8_BK;
#pragma unroll
    for (int ni = 0; ni < NH; ++ni) bf[ni] = frag(base + ni * 16 * G8_BK);
  };

  float4_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
  auto mfma_quadrant = [&](int mh, int nh) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < MH; ++mi)
#pragma unroll
      for (int ni = 0; ni < NH; ++ni)
        acc[mh * MH + mi][nh * NH + ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            bf[ni], af[mi], acc[mh * MH + mi][nh * NH + ni], 0, 0, 0, UNIT, 0, UNIT);
    __builtin_amdgcn_s_setprio(0);
  };

  const int nk = a.K / G8_BK;
  // (the buffer is a run-time offset, one loop body: with the two buffers as two unrolled
  // bodies behind a branch the compiler kept a second copy of the accumulators)
  auto ktile = [&](int t) {
    const int buf = t & 1;
    const bool s2 = t + 2 < nk;
    read_a(buf, 0);
    read_b(buf, 0);
    raw_barrier();
    if (s2) stage_a(buf, 0, t + 2);
    mfma_quadrant(0, 0);
    read_b(buf, 1);
    raw_barrier();
    if (s2) stage_b(buf, 1, t + 2);
    mfma_quadrant(0, 1);
    read_a(buf, 1);
    raw_barrier();
    if (s2) stage_a(buf, 1, t + 2);
    mfma_quadrant(1, 1);
    read_b(buf, 0);
    if (s2) wait_vm<2 * NA + NB>();  // tile t+1 has landed; A0 B1 A1 of tile t+2 may be in flight
    else wait_vm<0>();
    raw_barrier();
    if (s2) stage_b(buf, 0, t + 2);
    mfma_quadrant(1, 0);
  };

  // prologue: tile 0 complete, tile 1 in flight
  stage_a(0, 0, 0);
  stage_b(0, 0, 0);
  stage_b(0, 1, 0);
  stage_a(0, 1, 0);
  if (nk > 1) {
    stage_a(1, 0, 1);
    stage_b(1, 1, 1);
    stage_a(1, 1, 1);
    stage_b(1, 0, 1);
    wait_vm<2 * NA + 2 * NB>();
  } else {
    wait_vm<0>();
  }
  raw_barrier();
  for (int t = 0; t < nk; ++t) ktile(t);

  // lane holds sum_k for Y[m = m0 + wr MI 16 + mi 16 + r][n = n0 + wc NI 16 + ni 16 + 4g .. +3]:
  // the two scales go on the accumulator, then the fp16 path's epilogue (bias, ...)
  auto mrow = [&](int mi) { return m0 + (wr * MI + mi) * 16 + r; };
  auto ncol = [&](int ni) { return n0 + (wc * NI + ni) * 16 + 4 * g; };
  float4_t swv[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) swv[ni] = load4f(sw + ncol(ni));
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const float sm = sa[min(mrow(mi), a.M - 1)];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[mi][ni][e] = acc[mi][ni][e] * sm * swv[ni][e];
  }
  tile_epilogue<half_t, EPI, MI, NI, MI / 2>(a, acc, mrow, ncol);
}

int gemm8_tile(int M, int N, int K) {
  if (M <= 0 || K <= 0 || K % G8_BK) return 0;
  // below one 256 x 128 tile per CU the 128 x 64 tiles fill the chip (one window, n 1280:
  // 60 -> 240 workgroups); both accumulate a row's K-tiles in the same order
  if (N % 128 == 0 && ((M + 255) / 256) * (N / 128) >= 256) return 256;
  return N % 64 == 0 ? 128 : 0;
}

// The large tile is 256 x 128 (2 x 4 waves of 128 x 32): 64 accumulator and 40 fragment
// registers.  A 256 x 256 tile (128 + 48, its fragments spread over more registers by the
// allocator) came out of the compiler with 20 B of scratch per lane, reloaded inside the
// K loop behind a full vmcnt drain.
int launch_gemm8(const GemmArgs& a, const float* sa, const float* sw, int epi, int tile, hipStream_t st) {
  if (a.M <= 0) return 0;
  if (tile == 0) tile = gemm8_tile(a.M, a.N, a.K);
  if (a.K % G8_BK || a.ldx != a.K || !(tile == 256 ? a.N % 128 == 0 : tile == 128 && a.N % 64 == 0)) return -2;
  if ((int64_t)a.M * a.K >= ((int64_t)1 << 31) || (int64_t)a.N * a.K >= ((int64_t)1 << 31)) return -2;  // 32-bit staging offsets
  const int nwg = tile == 256 ? ((a.M + 255) / 256) * (a.N / 128) : ((a.M + 127) / 128) * (a.N / 64);
  switch (epi) {
#define CASE(E)                                                                                               \
  case E:                                                                                                     \
    if (tile == 256) k_gemm8<E, 2, 4, 8, 2><<<nwg, 512, 0, st>>>(a, sa, sw), wh_launched("k_gemm8<256x128>"); \
    else k_gemm8<E, 2, 2, 4, 2><<<nwg, 256, 0, st>>>(a, sa, sw), wh_launched("k_gemm8<128x64>");              \
    break;
    CASE(EPI_STORE) CASE(EPI_STORE_GELU) CASE(EPI_RESID) CASE(EPI_QKV_ENC)
#undef CASE
    default: return -1;
  }
  return 0;
}

}  // namespace wh
