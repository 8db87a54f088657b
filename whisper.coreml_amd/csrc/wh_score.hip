// Fused vocabulary scoring: the log-probability of a given token, the argmax and its
// log-probability for every row of LN(x) E^T, with no [rows][V] logits in memory.
//
//   z[v] = sum_k X[r][k] E[v][k]   fp32, k ascending in one accumulator per 16 x 16 block
//   m = max_v z, lse = m + log sum_v exp(z[v] - m)
//   logprob = z[target] - lse, top_id = min {v : z[v] == m}, top_logprob = m - lse
//
// Work split.  The 16-column tiles of the vocabulary are dealt to SCORE_SLICES = 256
// contiguous slices (12 or 13 tiles at V = 51 866), the rows to blocks of RB = 16 MT; the
// grid is (slice, row block), slices fastest, so the 256 workgroups of one row block run
// together, one per CU, and later row blocks stream E again (from the Infinity Cache as far
// as it holds the 133 MB).  A workgroup has 16 waves; wave w owns tile t0 + w of the slice.
//
// LDS: the block's rows over ALL of K (padded by 16 B per row: conflict-free ds_read_b128),
// so one accumulator per block sees k ascending in one pass, as the vocabulary kernels of
// wh_gemm.hip do; behind them one 16-B record per (wave, row).  RB is the largest multiple
// of 16 rows, at most 64, for which both fit 160 KB: fp16 at K = 1280 keeps 48 rows
// (48 x 2576 B + 16 x 48 x 16 B = 133 KB; 64 rows would need 177 KB), fp32 at 1280 keeps 16,
// either type at K = 128 keeps 64.  Half of K at a time would hold twice the rows, but every
// wave would have to keep its accumulators across a second staging of X; the row block only
// sets how often E is streamed, never a result.
//
// Registers: per wave MT accumulators (4 VGPRs each) and DEPTH = 3 chunks of the tile's
// weight rows in flight (48 VGPRs), streamed exactly as k_vocab_2p streams them.  What is new
// is the epilogue: lane (r, g) holds z[row 16 mt + r][columns 16 tile + 4 g .. + 3], so a
// row's 16 columns of the tile sit in the 4 registers of the 4 lanes r, r + 16, r + 32,
// r + 48.  They are reduced in registers and with two permlane swaps (lanes ^ 16, ^ 32) to
// {m, s = sum exp(z - m), z[target] or -inf, lowest column equal to m}; columns >= V take no
// part.  The 16 waves' records meet in LDS, where thread `row` folds them in ascending wave
// (= column) order and writes one record per (slice, row).  k_score_merge folds a row's 256
// records in ascending slice order in one thread.  No atomics; neither order depends on the
// number of rows, so a row's outputs are bit-identical wherever and with whatever it runs.
#include "wh_score.h"

#include <limits.h>

#include <algorithm>
#include <type_traits>

namespace wh {
namespace {

constexpr int SCORE_LDS = 160 * 1024;

WH_DEV int xor16_imin(int v) {
  int a = v, b = v;
  perm16_pair(a, b);
  return min(a, b);
}
WH_DEV int xor32_imin(int v) {
  int a = v, b = v;
  perm32_pair(a, b);
  return min(a, b);
}

// n records {m, s, zt, argmax} in ascending column order -> one: the maximum first (exact
// in any order), then the sums rescaled to it and added in the order given
template <typename F>
WH_DEV float4_t score_fold(int n, F at) {
  float M = -INFINITY;
  for (int i = 0; i < n; ++i) M = fmaxf(M, at(i)[0]);
  float S = 0.f, zt = -INFINITY;
  int am = INT_MAX;
  for (int i = 0; i < n; ++i) {
    const float4_t q = at(i);
    S += q[1] * __expf(q[0] - M);
    zt = fmaxf(zt, q[2]);
    if (q[0] == M && am == INT_MAX) am = __float_as_int(q[3]);
  }
  return (float4_t){M, S, zt, __int_as_float(am)};
}

template <typename T, int MT>
__global__ __launch_bounds__(1024) void k_score_part(ScoreArgs a) {
  constexpr int NW = SCORE_WAVES, RB = 16 * MT, DEPTH = 3, VC = 8 / (int)sizeof(T);  // k-steps per chunk: 4 fp16, 2 fp32
  extern __shared__ __attribute__((aligned(16))) char sc_lds[];
  const int K = a.K, XROW = K * (int)sizeof(T) + 16, NCH = K / 32 / VC;
  float4_t* const red = reinterpret_cast<float4_t*>(sc_lds + RB * XROW);  // [NW][RB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int slice = blockIdx.x, row0 = blockIdx.y * RB, nrows = min(RB, a.R - row0);
  const int nt = (a.V + 15) / 16;
  const int t0 = range_split(slice, nt, SCORE_SLICES), t1 = range_split(slice + 1, nt, SCORE_SLICES);
  const int tile = t0 + wave;
  const bool act = tile < t1;
  // the ragged last tile reads row V - 1 again instead of past E; its columns >= V are masked below
  const T* wrow = reinterpret_cast<const T*>(a.E) + (int64_t)min(tile * 16 + r, a.V - 1) * K + 8 * g;
  Frag<T> wbuf[DEPTH][VC];
  auto load_chunk = [&](int c, Frag<T>(&wf)[VC]) {
#pragma unroll
    for (int u = 0; u < VC; ++u) frag_load_stream(wf[u], wrow + (c * VC + u) * 32);
  };
  // the first DEPTH - 1 weight chunks ride with the staging loads
  if (act) {
#pragma unroll
    for (int c = 0; c < DEPTH - 1; ++c)
      if (c < NCH) load_chunk(c, wbuf[c]);
  }
  const int CPR = XROW / 16 - 1;  // 16-B chunks per row
  const char* const X = reinterpret_cast<const char*>(a.X);
  const int* const xrows = a.x_rows;
  for (int c = tid; c < nrows * CPR; c += 64 * NW) {
    const int row = c / CPR, col = c - row * CPR;
    const int64_t src = xrows ? xrows[row0 + row] : row0 + row;
    *reinterpret_cast<float4_t*>(sc_lds + row * XROW + col * 16) =
        *reinterpret_cast<const float4_t*>(X + src * a.ldx * (int64_t)sizeof(T) + col * 16);
  }
  __syncthreads();
  if (act) {
    float4_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
    const char* xl[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xl[mt] = sc_lds + min(mt * 16 + r, nrows - 1) * XROW + 8 * g * (int)sizeof(T);
    // chunk c lives in wbuf[c % DEPTH]; the loop steps by DEPTH so that every index is static
#pragma unroll 1
    for (int c = 0; c < NCH; c += DEPTH) {
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) {
        if (c + d < NCH) {
          if (c + d + DEPTH - 1 < NCH) load_chunk(c + d + DEPTH - 1, wbuf[(d + DEPTH - 1) % DEPTH]);
#pragma unroll
          for (int u = 0; u < VC; ++u) {
            const int ks = (c + d) * VC + u;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              if (mt * 16 < nrows) {  // wave-uniform: a short block skips its empty row tiles
                Frag<T> xf;
                frag_load(xf, reinterpret_cast<const T*>(xl[mt]) + ks * 32);
                mfma_step(acc[mt], wbuf[d][u], xf);
              }
            }
          }
        }
      }
    }
    // the tile's 16 columns of a row: 4 registers in each of the lanes r + 16 g
    const int col0 = tile * 16 + 4 * g;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (mt * 16 < nrows) {
        const int row = mt * 16 + r;
        const int tg = row < nrows ? a.target[row0 + row] : -1;
        const float4_t z = acc[mt];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col0 + j < a.V) m = fmaxf(m, z[j]);
        m = xor32_max(xor16_max(m));  // finite: a tile below nt has a column below V
        float s = 0.f, zt = -INFINITY;
        int am = INT_MAX;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col0 + j < a.V) {
            s += __expf(z[j] - m);
            if (z[j] == m) am = min(am, col0 + j);
            if (col0 + j == tg) zt = z[j];
          }
        s = xor32_sum(xor16_sum(s));
        zt = xor32_max(xor16_max(zt));
        am = xor32_imin(xor16_imin(am));
        if (g == 0 && row < nrows) red[wave * RB + row] = (float4_t){m, s, zt, __int_as_float(am)};
      }
    }
  }
  __syncthreads();
  if (tid < nrows) {
    const int nwv = t1 - t0;  // <= NW (launcher); an empty slice leaves {-inf, 0, -inf, none}
    const float4_t q = score_fold(nwv, [&](int w) { return red[w * RB + tid]; });
    a.rec[(int64_t)slice * a.R + row0 + tid] = q;
  }
}

__global__ __launch_bounds__(256) void k_score_merge(ScoreArgs a) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= a.R) return;
  const float4_t q = score_fold(SCORE_SLICES, [&](int s) { return a.rec[(int64_t)s * a.R + row]; });
  const float lse = q[0] + logf(q[1]);
  a.logprob[row] = q[2] - lse;
  a.top_id[row] = __float_as_int(q[3]);
  a.top_logprob[row] = q[0] - lse;
}

template <typename T>
__global__ __launch_bounds__(256) void k_score_cast(const float* x, T* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = from_f32<T>(x[i]);  // v_cvt_f16_f32: round to nearest even
}

template <typename T>
constexpr int score_lds_bytes(int K, int mt) {
  return 16 * mt * (K * (int)sizeof(T) + 16 + SCORE_WAVES * 16);
}

}  // namespace

template <typename T>
int score_row_block(int K) {
  int mt = 4;
  while (mt > 1 && score_lds_bytes<T>(K, mt) > SCORE_LDS) --mt;
  return 16 * mt;
}

template <typename T>
int launch_vocab_score(const ScoreArgs& a, hipStream_t st) {
  const int nt = (a.V + 15) / 16;
  if (a.R < 1 || a.V < 1 || a.K < 128 || a.K % 128 || a.K > 2048 || nt > SCORE_SLICES * SCORE_WAVES) return -1;
  const int rb = score_row_block<T>(a.K);
  if (score_lds_bytes<T>(a.K, rb / 16) > SCORE_LDS) return -1;
  const dim3 grid(SCORE_SLICES, (a.R + rb - 1) / rb);
  auto go = [&](auto mtc) {  // one attribute flag per instantiation
    constexpr int MT = decltype(mtc)::value;
    static bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score_part<T, MT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, SCORE_LDS) == hipSuccess;
    if (!attr) return -1;
    k_score_part<T, MT><<<grid, 64 * SCORE_WAVES, score_lds_bytes<T>(a.K, MT), st>>>(a), wh_launched("k_score_part");
    return 0;
  };
  int rc;
  switch (rb / 16) {
    case 1: rc = go(std::integral_constant<int, 1>()); break;
    case 2: rc = go(std::integral_constant<int, 2>()); break;
    case 3: rc = go(std::integral_constant<int, 3>()); break;
    default: rc = go(std::integral_constant<int, 4>()); break;
  }
  if (rc) return rc;
  k_score_merge<<<(a.R + 255) / 256, 256, 0, st>>>(a), wh_launched("k_score_merge");
  return 0;
}

template <typename T>
void launch_score_cast(const float* x, T* out, int64_t n, hipStream_t st) {
  k_score_cast<T><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, out, n), wh_launched("k_score_cast");
}

template int score_row_block<half_t>(int);
template int score_row_block<float>(int);
template int launch_vocab_score<half_t>(const ScoreArgs&, hipStream_t);
template int launch_vocab_score<float>(const ScoreArgs&, hipStream_t);
template void launch_score_cast<half_t>(const float*, half_t*, int64_t, hipStream_t);
template void launch_score_cast<float>(const float*, float*, int64_t, hipStream_t);

}  // namespace wh
