// The decoder step's cross-attention kernel (k_xattn_seg) with its query staging, in-kernel
// query projection and pair merge.  A header because two translation units instantiate it:
// wh_kernels.hip (K / V in the compute type) and wh_ckv8.hip (the 8-bit copy, KV8).
#pragma once
#include "wh_kernels.h"

namespace wh {

// ------------------------------------------------------------ step cross-attention
// Decoder-step cross-attention (decoder.py:74-91 for the step's query rows: <= 16 rows
// per window, the beams), batch-invariant and balanced over the chip.
//
// Numerics are fixed per (window, head) pair, whatever the batch: every 64-key tile of
// the pair gives one softmax partial (m = the tile's max score, l = sum exp(s - m),
// O = sum exp(s - m) v), and the pair's nsp = ceil(Tk / 64) partials are merged in tile
// order by the flat merge of xs_merge (M = max m, then L and O accumulated over the
// tiles in order).  How many windows share the launch changes only which workgroup
// computes a tile and where the pair is merged, never an arithmetic operation, so a
// window's output is bit-identical in any batch.
//
// Work distribution (speed only): the tiles of all pairs, in (pair, tile) order, are
// dealt in contiguous ranges to nwg <= 256 workgroups; the workgroup's 8 waves take its
// tiles round-robin, the next tile's K and V in flight while one is computed (no tile
// depends on another, the last one is peeled: no load is clamped or wasted).  A pair
// whose tiles are all in the workgroup merges from LDS.  A pair cut between workgroups
// has this workgroup's partials stored write-through (sc1) at [pair][tile] (the window's
// rows only), drained by every storing wave, and counted on the pair's arrival counter
// (relaxed agent atomic, + the tiles contributed); the workgroup that completes the
// count re-arms it and merges every partial with sc1 loads (cdna_hip_programming.md §6
// Guideline 16 R1, MI355X_MICROARCH.md "Valid forms").  RR: rows kept per partial in LDS
// (8 when the beams are <= 8, else 16).
// K: [slot][head][TKP][64]; V transposed, tile-major (xv_index: a 64-key tile's 64 x 64
// V^T is 8 KB contiguous, keys permuted within 32-key groups), so both MFMA operands load
// straight from HBM into fragments and each tile is two contiguous 8 KB streams.
constexpr float XS_LOG2E = 1.4426950408889634f;

template <int RR>
struct XsShape {
  static constexpr int SMAX = RR == 8 ? 48 : 32;  // tiles per workgroup (LDS partials)
};

// ---- KV8: the tiles come from the 8-bit copy of the cross-KV (whisper_hip.h "cross-KV
// formats", records written by k_ckv_quant: wh_ckv8.hip).  A tile is one CKV8_REC-byte
// record, so a wave's whole tile is ONE contiguous stream of 9 x 16-B loads per lane: 4 of
// K codes (key row kt * 16 + r, chunk g: channels 8g.. and 32 + 8g..), 4 of V^T codes (row
// dt * 16 + r, chunk g: the keys of both 32-key halves), 1 of scales (lanes 0..15: the K
// scales of keys 4 lane..+3, lanes 16..31: the V scales; the upper half repeats them).
// At the tile's turn lanes 0..31 put the 128 scales into the wave's own 512 B of LDS and every
// lane reads the 16 + 16 of its keys back (in-order LDS queue of one wave: no barrier).
// 36 VGPRs per tile against 64 of fp16 fragments, so a ring of 4 tile buffers (3 in flight
// under the one computed) holds the bytes in flight of the fp16 A / B pair.
// E4M3 is exact in fp16: the codes become the same 16x16x32 f16 MFMA operands as the fp16
// path's (v_cvt_scalef32_pk_f16_fp8 with scale 1, 64 per tile and lane), q and P keep fp16
// precision, and the per-key scales meet the fp32 scores (K) and probabilities (V).
struct Kv8Buf {
  u32x4_t k[4], v[4];
  float4_t s;
};
struct Kv8Frags {
  Frag<half_t> f[2];
  WH_DEV const Frag<half_t>& operator[](int i) const { return f[i]; }
};
// 16 codes -> two 8-element fp16 fragments (bytes 0..7, 8..15)
WH_DEV Kv8Frags kv8_frags(u32x4_t c) {
  unsigned w[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[2 * i] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[i], 1.f, false));
    w[2 * i + 1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[i], 1.f, true));
  }
  Kv8Frags o;
  o.f[0].v = __builtin_bit_cast(half8_t, (u32x4_t){w[0], w[1], w[2], w[3]});
  o.f[1].v = __builtin_bit_cast(half8_t, (u32x4_t){w[4], w[5], w[6], w[7]});
  return o;
}
// the pair merge shared by the LDS and the record path: `get(k, m, l, o)` fetches tile
// k's partial; every fetch is issued before the first use (one round trip on the record
// path), then M = max m, and L, O accumulate over the tiles in order
template <typename Get>
WH_DEV float4_t xs_merge(int n, Get get) {
  float mv[XS_NSP], lv[XS_NSP];
  float4_t ov[XS_NSP];
#pragma unroll
  for (int k = 0; k < XS_NSP; ++k) get(k < n ? k : n - 1, mv[k], lv[k], ov[k]);
  float M = -INFINITY;
#pragma unroll
  for (int k = 0; k < XS_NSP; ++k)
    if (k < n) M = fmaxf(M, mv[k]);
  float L = 0.f;
  float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < XS_NSP; ++k)
    if (k < n) {
      const float f = mv[k] == -INFINITY ? 0.f : hw_exp2((mv[k] - M) * XS_LOG2E);
      L = __builtin_fmaf(f, lv[k], L);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(f, ov[k][e], acc[e]);
    }
  const float inv = 1.f / L;
  return acc * inv;
}

#if WH_TUNING && !defined(WH_XS_NO_TRACE)
// tuning build: per-workgroup wall-clock marks (s_memrealtime, 100 MHz) of the last
// k_xattn_seg launch, read by wh_tune_xs_trace (profiles/xattn_trace.py); of wh_kernels.hip's
// instantiations only (the KV8 ones define WH_XS_NO_TRACE: one copy of the table)
constexpr int XS_MARKS = 10;
__device__ unsigned long long g_xs_trace[256][XS_MARKS];
#define XS_MARK(k)                                                                         \
  do {                                                                                     \
    if (threadIdx.x == 0) g_xs_trace[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();   \
  } while (0)
#else
#define XS_MARK(k) \
  do {             \
  } while (0)
#endif

// Round 6: the decoder step's cross-attention query projected inside k_xattn_seg (QK > 0)
// instead of by a split-K k_proj launch whose fp16 slabs the kernel summed: the range's
// pairs (at most XS_QF: a range holds <= 2 x nsp tiles with nsp = 24) each need
//   q[row][c] = (S0 + S1) + bias[c],  S_kh = sum over the K half kh of X[row][k] W_q[c][k]
// (MFMA accumulation in k-step order; the two halves meet in LDS in that order), the
// same arithmetic whichever workgroup, grid form or batch computes it (batch invariance).
// The 8 waves are (16-column tile c of the head's 64, K half kh); a pair's window rows
// (<= RR) are staged in LDS (rows past the window are never emitted), the wave's
// 16 x n / 2 slice of W_q (QK fragments) is loaded once per head.  X, the K-half sums and
// the biases live in the tile partials' LDS (dead until the first tile).  Reference:
// decoder.py:73-91 (cross-attention query), :42 (the 0.125 query scale, folded in W_q).
//
// Load order: X and bias (registers) and W_q first; the first two tiles' K / V are issued only
// once X is staged, so the few KB the projection waits on are not queued behind 25 MB of
// K / V; the tiles then stream while W_q lands and the projection runs (issued with X they
// staged the query at 10.5 us against 4.4 with the slabs, profiles/r06/xattn_trace_qv.txt).
constexpr int XS_QF = 3;
// KV8: ring_first() issues the wave's first tiles instead of load_kv into the A / B pair
template <typename T, int QK, int RR, bool KV8, typename PairWH, typename LoadKV, typename RingFirst>
WH_DEV void xq_project(const XQPart& xq, int pa, int plast, int cnt, const int* __restrict__ win_row0,
                       const int* __restrict__ win_nrows, PairWH pair_wh, LoadKV load_kv, Frag<T> (&kA)[4][2],
                       Frag<T> (&vA)[4][2], Frag<T> (&kB)[4][2], Frag<T> (&vB)[4][2], RingFirst ring_first, char* xst,
                       T (*qs)[16][72], int* s_wnr, int* s_wr0) {
  static_assert(sizeof(T) == 2, "fused query projection: fp16 contexts");
  constexpr int N = QK * 64;                           // model width = K
  constexpr int CPR = N * (int)sizeof(T) / 16;         // 16-B chunks per row
  constexpr int XROWB = N * (int)sizeof(T) + 16;       // LDS row (bytes)
  constexpr int XPT = (RR * CPR + 511) / 512;          // chunks per thread per pair
  // LDS (byte offsets in xst): X rows, the K-half sums [2][XS_QF][4][64] float4, the biases
  constexpr int RED_OFF = XS_QF * RR * XROWB, BIAS_OFF = RED_OFF + 2 * XS_QF * 4 * 64 * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int c = wave & 3, kh = wave >> 2;
  const int np = plast - pa + 1;
  // the pairs' heads (arithmetic only) and window rows (scalar loads, one round trip)
  int q_h[XS_QF], q_w[XS_QF], q_nr[XS_QF], q_r0[XS_QF];
#pragma unroll
  for (int j = 0; j < XS_QF; ++j) {
    const int pj = __builtin_amdgcn_readfirstlane(min(pa + j, plast));
    pair_wh(pj, q_w[j], q_h[j]);
  }
  Frag<T> wf[QK];
  auto load_w = [&](int h) {  // fragment order (launch_wq_frag): each k-step one 1 KB contiguous wave load
    const T* wp = reinterpret_cast<const T*>(xq.qwf) + ((int64_t)((h * 4 + c) * 2 + kh) * QK * 64 + lane) * 8;
#pragma unroll
    for (int s = 0; s < QK; ++s) frag_load_stream(wf[s], wp + s * 512);
  };
#pragma unroll
  for (int j = 0; j < XS_QF; ++j) {
    q_nr[j] = win_nrows[q_w[j]];
    q_r0[j] = win_row0[q_w[j]];
  }
  // 1. each pair's window rows and head biases: unconditional buffer loads, the buffer limit
  // is the window's rows (0 past it and for pairs past the range); the biases by wave 0, one
  // float per lane and pair
  float4_t xv[XS_QF][XPT];
  float bv[XS_QF];
#pragma unroll
  for (int j = 0; j < XS_QF; ++j) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(reinterpret_cast<const T*>(xq.qx)) + (int64_t)q_r0[j] * N, 0, j < np ? q_nr[j] * N * (int)sizeof(T) : 0,
        0x00020000);
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int ch = tid + 512 * i, off = (ch / CPR) * (N * (int)sizeof(T)) + (ch % CPR) * 16;
      xv[j][i] = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
    }
  }
#pragma unroll
  for (int j = 0; j < XS_QF; ++j) bv[j] = xq.bias[q_h[min(j, np - 1)] * 64 + lane];
  __builtin_amdgcn_sched_barrier(0);
  // 2. the wave's W_q fragments for the first pair's head: rows h*64 + 16c + r, K half kh
  load_w(q_h[0]);
  __builtin_amdgcn_sched_barrier(0);
  // 3. X (and the biases) -> LDS: waits for them alone (issued first; vmcnt retires in order)
#pragma unroll
  for (int j = 0; j < XS_QF; ++j)
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int ch = tid + 512 * i;
      if (ch < RR * CPR)
        *reinterpret_cast<float4_t*>(xst + (j * RR + ch / CPR) * XROWB + (ch % CPR) * 16) = xv[j][i];
    }
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < XS_QF; ++j) reinterpret_cast<float*>(xst + BIAS_OFF)[j * 64 + lane] = bv[j];
  }
  if (tid == 0) {  // the merge's window rows (LDS, behind the barriers below)
#pragma unroll
    for (int j = 0; j < XS_QF; ++j) {
      s_wnr[j] = q_nr[j];
      s_wr0[j] = q_r0[j];
    }
  }
  wh_lds_barrier();
  XS_MARK(7);  // X staged
  // 4. the first two tiles' K / V leave now, behind the few KB the projection waited on
  if constexpr (KV8) {
    ring_first();
  } else {
    load_kv(min(wave, cnt - 1), kA, vA);
    load_kv(min(wave + 8, cnt - 1), kB, vB);
  }
  // 5. pair by pair: MFMAs in k-step order (W reloaded only where the head changes); each
  // pair's K-half sum goes to LDS at once (no register per pair)
  float4_t* red2 = reinterpret_cast<float4_t*>(xst + RED_OFF);  // [kh][pair][c][lane]
#pragma unroll
  for (int j = 0; j < XS_QF; ++j) {
    if (j < np) {
      if (j > 0 && q_h[j] != q_h[j - 1]) load_w(q_h[j]);
      float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
      const int rr = min(r, RR - 1);
      const char* xl = xst + (j * RR + rr) * XROWB;
#pragma unroll
      for (int s = 0; s < QK; ++s) {
        Frag<T> xf;
        const int ch = kh * QK * 4 + 4 * s + g;  // 16-B chunk of k = kh * N / 2 + 32 s + 8 g
        frag_load(xf, reinterpret_cast<const T*>(xl + ch * 16));
        mfma_step(acc, wf[s], xf);
      }
      red2[((kh * XS_QF + j) * 4 + c) * 64 + lane] = acc;
    }
  }
  XS_MARK(8);  // this wave's (thread 0's) MFMAs done: its W_q fragments landed
  // 6. the K halves meet (half 0 + half 1, then the bias) -> qs[pair][row][64] (fp16)
  wh_lds_barrier();
  if (kh == 0) {
    const float* bl = reinterpret_cast<const float*>(xst + BIAS_OFF);
#pragma unroll
    for (int j = 0; j < XS_QF; ++j)
      if (j < np) {
        float4_t v = red2[(j * 4 + c) * 64 + lane] + red2[((XS_QF + j) * 4 + c) * 64 + lane];
        v += *reinterpret_cast<const float4_t*>(bl + j * 64 + c * 16 + 4 * g);
        store4(&qs[j][r][c * 16 + 4 * g], v[0], v[1], v[2], v[3]);
      }
  }
}

template <typename T, int QZ, int RR, typename S = float, bool FULL = false, int QK = 0, bool KV8 = false>
__global__ __launch_bounds__(512, 1) void k_xattn_seg(const T* __restrict__ q, int ldq, const T* ck, const T* cvt, int Tk,
                                                     int H, int npair, int nsp, const int* __restrict__ win_row0,
                                                     const int* __restrict__ win_nrows,
                                                     const int* __restrict__ win_slot, int64_t win_stride, XQPart xq,
                                                     T* __restrict__ out, int ldo) {
  constexpr int NW = 8, SMAX = XsShape<RR>::SMAX, PPASS = 512 / (RR * 16);  // pairs merged per pass
  constexpr bool QP = QZ > 0;
  // QK > 0 (round 6): the query projection itself runs here (xq.qx rows x W_q^T + bias,
  // QK k-steps per K half), pairs are numbered head-major (p = head * nwin + window: a
  // workgroup's pairs share one head's 64 x n slice of W_q) and workgroups are laid over
  // the XCDs in contiguous logical runs, so a head's slice crosses HBM about once per XCD
  constexpr bool QF = QK > 0;
  // KV8: ck is the layer's 8-bit records (bytes), win_stride a slot's bytes, cvt unused
  static_assert(!KV8 || sizeof(T) == 2, "8-bit cross-KV: fp16 contexts");
  __shared__ float seg_m[SMAX][RR], seg_l[SMAX][RR];
  // partial outputs row-major, 68-float rows: a lane's 4 columns are one 16-B store / load
  // (tile(): lanes r = 0..7 of a store group hit banks 4r.. +3, conflict-free; round 4 kept
  // [tile][64][RR + 1] and moved them as 16 + 4 single floats)
  __shared__ __attribute__((aligned(16))) float seg_o[SMAX][RR][68];
  __shared__ __attribute__((aligned(16))) T qs[XS_QP][16][72];
  __shared__ int s_ticket[2];
  __shared__ __attribute__((aligned(16))) float s_kv8[KV8 ? 8 : 1][KV8 ? 128 : 4];  // a wave's tile scales: K, then V
  __shared__ int s_wnr[XS_QP], s_wr0[XS_QP];  // the range's pairs' window rows / first row, for the merge
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int nseg = npair * nsp, nwg = gridDim.x, b = QF ? xcd_remap(blockIdx.x, nwg) : (int)blockIdx.x;
  const int s0 = range_split(b, nseg, nwg), s1 = range_split(b + 1, nseg, nwg), cnt = s1 - s0;
  const int pa = s0 / nsp, plast = (s1 - 1) / nsp;
  const int nwin = QF ? npair / H : 0;
  // pair p -> (window, head)
  auto pair_wh = [&](int p, int& wi, int& h) {
    if constexpr (QF) {
      h = p / nwin;
      wi = p - h * nwin;
    } else {
      wi = p / H;
      h = p - wi * H;
    }
  };
  XS_MARK(0);
  CT_MARK(CT_XATTN, 0);

  // local tile i: K and V fragments
  // (wsl >= 0: the tile's window slot, already loaded)
  auto load_kv = [&](int i, Frag<T>(&kf)[4][2], Frag<T>(&vf)[4][2], int wsl = -1) {
    // i is wave-uniform: the tile's window slot comes by a scalar load (lgkmcnt).  Round 4:
    // as a vector load it sat in vmcnt order, and the s_waitcnt vmcnt(0) before the K / V
    // addresses drained the tile in flight: one tile per wave in flight, not two
    const int gs = __builtin_amdgcn_readfirstlane(s0 + i), p = gs / nsp, k = gs - p * nsp;
    int wi, h;
    pair_wh(p, wi, h);
    const int64_t off = (int64_t)(wsl >= 0 ? wsl : win_slot[wi]) * win_stride;
    const T* kbase = ck + off + (int64_t)h * TKP * 64;
    const T* vbase = cvt + off + (int64_t)h * 64 * TKP;
    const int kt0 = k * 64;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const T* kp = kbase + (int64_t)(kt0 + kt * 16 + r) * 64 + 8 * g;
      frag_load_stream(kf[kt][0], kp);
      frag_load_stream(kf[kt][1], kp + 32);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int s = 0; s < 2; ++s) frag_load_stream(vf[dt][s], vbase + ((int64_t)k * 64 + dt * 16 + r) * 64 + 32 * s + 8 * g);
  };
  // KV8: local tile i's record -> one ring buffer (every tile < nsp <= CKV8_TILES has a
  // whole record, the padding keys' codes and scales are 0).  Buffer loads whose limit is the
  // record, or 0 for a tile past the workgroup's range (i >= cnt): the instruction stream is
  // unconditional (no branch join for the vmcnt bookkeeping to merge) and a tile that does
  // not exist moves no bytes
  auto load_kv8 = [&](int i, Kv8Buf& b) {
    const int il = __builtin_amdgcn_readfirstlane(i), gs = s0 + min(il, cnt - 1), p = gs / nsp, k = gs - p * nsp;
    int wi, h;
    pair_wh(p, wi, h);
    const char* rec = reinterpret_cast<const char*>(ck) + (int64_t)win_slot[wi] * win_stride +
                      ((int64_t)h * CKV8_TILES + k) * CKV8_REC;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rec), 0, il < cnt ? CKV8_REC : 0, 0x00020000);
    const int off = r * 64 + 16 * g;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) b.k[kt] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + kt * 1024, 0, 0);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) b.v[dt] = __builtin_amdgcn_raw_buffer_load_b128(rs, 4096 + off + dt * 1024, 0, 0);
    b.s = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, 8192 + (lane & 31) * 16, 0, 0));
  };
  // local tile i's softmax partial -> LDS slot i (kb / vb: the K / V fragments, or twice the
  // tile's Kv8Buf)
  auto tile = [&](const auto& kb, const auto& vb, int i) {
    auto kfr = [&](int kt) -> decltype(auto) {
      if constexpr (KV8) return kv8_frags(kb.k[kt]);
      else return (kb[kt]);
    };
    const int gs = s0 + i, p = gs / nsp, kt0 = (gs - p * nsp) * 64;
    if constexpr (KV8) {  // the tile's scales -> the wave's LDS, in key order (K, then V)
      __builtin_amdgcn_wave_barrier();  // behind the previous tile's reads
      if (lane < 32) *reinterpret_cast<float4_t*>(&s_kv8[wave][4 * lane]) = kb.s;
      __builtin_amdgcn_wave_barrier();
    }
    // KV8: the scales of the lane's keys kt * 16 + 4 g .. + 3 (v: the V scales)
    auto kv8_scales = [&](int kt, int v) {
      return *reinterpret_cast<const float4_t*>(&s_kv8[wave][KV8 ? v * 64 + kt * 16 + 4 * g : 0]);
    };
    Frag<T> qf[2];
    frag_load(qf[0], &qs[p - pa][r][8 * g]);
    frag_load(qf[1], &qs[p - pa][r][32 + 8 * g]);
    float4_t sc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      sc[kt] = (float4_t){0.f, 0.f, 0.f, 0.f};
      decltype(auto) kf = kfr(kt);
      mfma_step(sc[kt], kf[0], qf[0]);
      mfma_step(sc[kt], kf[1], qf[1]);
      if constexpr (KV8) sc[kt] *= kv8_scales(kt, 0);  // the keys' K scales
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kt0 + kt * 16 + 4 * g + j >= Tk) sc[kt][j] = -INFINITY;
        mx = fmaxf(mx, sc[kt][j]);
      }
    mx = xor16_max(mx);
    mx = xor32_max(mx);
    Frag<T> pf[2];
    float ps = 0.f;
    // KV8: a key's V scale multiplies its fp32 probability before the rounding to fp16,
    // relative to the tile's largest (vmax, back on the fp32 sums below): the scaled
    // probabilities span [0, 1] as the plain ones do, whatever the magnitude of V
    float4_t vsc[KV8 ? 4 : 1];
    float vmax = 0.f;
    if constexpr (KV8) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        vsc[kt] = kv8_scales(kt, 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) vmax = fmaxf(vmax, vsc[kt][j]);
      }
      vmax = xor16_max(vmax);
      vmax = xor32_max(vmax);
      const float vinv = vmax > 0.f ? 1.f / vmax : 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) vsc[kt] *= vinv;
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pv = hw_exp2((sc[kt][j] - mx) * XS_LOG2E);
        ps += pv;
        if constexpr (KV8) pf[kt >> 1].v[(kt & 1) * 4 + j] = from_f32<T>(pv * vsc[kt][j]);
        else pf[kt >> 1].v[(kt & 1) * 4 + j] = from_f32<T>(pv);
      }
    ps = xor16_sum(ps);
    ps = xor32_sum(ps);
    float4_t acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = (float4_t){0.f, 0.f, 0.f, 0.f};
    if constexpr (KV8) {  // a V^T load holds both key halves: per column tile, halves in order
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const Kv8Frags vf = kv8_frags(vb.v[dt]);
        mfma_step(acc[dt], vf[0], pf[0]);
        mfma_step(acc[dt], vf[1], pf[1]);
        acc[dt] *= vmax;
      }
    } else {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) mfma_step(acc[dt], vb[dt][s], pf[s]);
    }
    if (r < RR) {
      if (g == 0) {
        seg_m[i][r] = mx;
        seg_l[i][r] = ps;
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<float4_t*>(&seg_o[i][r][dt * 16 + 4 * g]) = acc[dt];
    }
  };

  Frag<T> kA[4][2], vA[4][2], kB[4][2], vB[4][2];
  Kv8Buf ring[4];  // KV8 only
  // KV8: the wave's first three tiles (those that exist)
  auto ring_first = [&] {
    load_kv8(wave, ring[0]);
    load_kv8(wave + NW, ring[1]);
    load_kv8(wave + 2 * NW, ring[2]);
  };
  // the query rows of the pairs this range touches -> LDS (rows past a window's beams
  // repeat its last row).  Round 4: their loads are issued BEFORE the first tile's K / V:
  // vmcnt retires loads in issue order, so the staging below waits for the query alone,
  // the barrier passes ~a round trip in, and the second tile's K / V leave while the first
  // burst is still landing (the query used to wait behind the whole first tile,
  // profiles/xattn_trace.py: query staged at 5.3 us of a 34 us launch at 20 windows)
  constexpr int NQP = XS_QP / 2;
  if constexpr (QF) {
    static_assert(XS_QF * RR * (QK * 64 * sizeof(T) + 16) + 2 * XS_QF * 4 * 64 * 16 + XS_QF * 256 <= sizeof(seg_o),
                  "X rows, K-half sums and biases in the partials' LDS");
    static_assert(XS_QF * 4 * 64 * 16 <= sizeof(seg_o), "K-half sums in the partials' LDS");
    xq_project<T, QK, RR, KV8>(xq, pa, plast, cnt, win_row0, win_nrows, pair_wh, load_kv, kA, vA, kB, vB, ring_first,
                               reinterpret_cast<char*>(&seg_o[0][0][0]), qs, s_wnr, s_wr0);
  } else {
  // FULL (the launcher: every workgroup holds >= 8 tiles, one per wave at least): the order
  // above; otherwise (few windows, <= 1 tile per wave) the first tile leaves first, as the
  // query then has no second tile to overlap
  if constexpr (!FULL) {
    if constexpr (KV8) {
      // (at most one tile per wave, the latency path: that tile alone)
      if (wave < cnt) {
        if (cnt > NW) ring_first();
        else load_kv8(wave, ring[0]);
      }
    } else {
      if (wave < cnt) load_kv(wave, kA, vA);
    }
  }
  float4_t qld[NQP][QP ? QZ + 1 : 1];  // QP: the QZ slabs, then the bias
  // wave-uniform pairs: their windows' metadata by scalar loads (lgkmcnt, not behind
  // vmcnt), all issued before the first use: one round trip, not one per load and pass
  int q_hj[NQP], q_nr[NQP], q_r0[NQP];
#pragma unroll
  for (int pass = 0; pass < NQP; ++pass) {
    const int pj = __builtin_amdgcn_readfirstlane(min(pa + 2 * pass + (tid >> 8), plast)), wj = pj / H;
    q_hj[pass] = pj - wj * H;
    q_nr[pass] = win_nrows[wj];
    q_r0[pass] = win_row0[wj];
  }
  // FULL: the first tile's window slot rides in the same round trip
  const int slot0 = FULL ? win_slot[__builtin_amdgcn_readfirstlane(s0 + wave) / nsp / H] : -1;
  __builtin_amdgcn_sched_barrier(0);  // (else the second pass's loads sink below the first's wait)
#pragma unroll
  for (int pass = 0; pass < NQP; ++pass) {
    const int t = tid & 255;
    if (t == 0) {  // kept for the merge (LDS, behind the staging barrier): no global round trip there
      s_wnr[2 * pass + (tid >> 8)] = q_nr[pass];
      s_wr0[2 * pass + (tid >> 8)] = q_r0[pass];
    }
    const int qq = min(t >> 4, q_nr[pass] - 1), c = q_hj[pass] * 64 + (t & 15) * 4, row = q_r0[pass] + qq;
    if constexpr (QP) {
      const S* src = reinterpret_cast<const S*>(xq.part) + (int64_t)row * ldq + c;
#pragma unroll
      for (int z = 0; z < QZ; ++z) qld[pass][z] = load4f(src + z * xq.stride);
      qld[pass][QZ] = load4f(xq.bias + c);
    } else {
      qld[pass][0] = load4f(q + (int64_t)row * ldq + c);
    }
  }
  if constexpr (FULL) {
    __builtin_amdgcn_sched_barrier(0);  // keep the K / V loads behind the query's
    // every wave's query loads enter the CU's memory pipeline before any wave's K / V
    // (a barrier that waits for nothing: no s_waitcnt before it)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  auto stage_q = [&] {
#pragma unroll
    for (int pass = 0; pass < NQP; ++pass) {
      const int j = 2 * pass + (tid >> 8), t = tid & 255;
      float4_t qv = qld[pass][0];
      if constexpr (QP) {
        qv = qld[pass][QZ];
#pragma unroll
        for (int z = 0; z < QZ; ++z) qv += qld[pass][z];
      }
      store4(&qs[j][t >> 4][(t & 15) * 4], qv[0], qv[1], qv[2], qv[3]);
    }
  };
  // FULL: unconditional (every wave has a tile), so no branch join: behind one the
  // compiler's vmcnt bookkeeping made the query staging wait for the K / V loads as well
  if constexpr (FULL) {
    if constexpr (KV8) ring_first();
    else load_kv(wave, kA, vA, slot0);
    __builtin_amdgcn_sched_barrier(0);
  }
  stage_q();
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // LDS only
  XS_MARK(1);

  if constexpr (KV8) {
    // ring of 4: the wave's tiles i, i + NW, .. with three in flight under the one computed;
    // each iteration refills the buffer it has just computed (load_kv8: unconditional, nothing
    // moves for a tile past the range), the last <= 3 tiles are peeled: no load there
    if (wave < cnt) {
      int i = wave;
      for (; i + 3 * NW < cnt; i += 4 * NW) {
        load_kv8(i + 3 * NW, ring[3]);
        tile(ring[0], ring[0], i);
        load_kv8(i + 4 * NW, ring[0]);
        tile(ring[1], ring[1], i + NW);
        load_kv8(i + 5 * NW, ring[1]);
        tile(ring[2], ring[2], i + 2 * NW);
        load_kv8(i + 6 * NW, ring[2]);
        tile(ring[3], ring[3], i + 3 * NW);
      }
      if (i < cnt) tile(ring[0], ring[0], i);
      if (i + NW < cnt) tile(ring[1], ring[1], i + NW);
      if (i + 2 * NW < cnt) tile(ring[2], ring[2], i + 2 * NW);
    }
  } else if (QF && wave < cnt) {
    // (xq_project) kB / vB already hold tile wave + NW (clamped): the next tile is in flight on
    // entry, so each iteration refills the buffer it has just computed
    int i = wave;
    for (; i + 2 * NW < cnt; i += 2 * NW) {
      tile(kA, vA, i);
      load_kv(i + 2 * NW, kA, vA);
      tile(kB, vB, i + NW);
      load_kv(min(i + 3 * NW, cnt - 1), kB, vB);
    }
    if (i + NW < cnt) {
      tile(kA, vA, i);
      tile(kB, vB, i + NW);
    } else {
      tile(kA, vA, i);
    }
  } else if (wave < cnt) {
    int i = wave;
    // two tiles per iteration, the next one always in flight (unconditional loads)
    for (; i + 2 * NW < cnt; i += 2 * NW) {
      load_kv(i + NW, kB, vB);
      tile(kA, vA, i);
      load_kv(i + 2 * NW, kA, vA);
      tile(kB, vB, i + NW);
    }
    if (i + NW < cnt) {
      load_kv(i + NW, kB, vB);
      tile(kA, vA, i);
      tile(kB, vB, i + NW);
    } else {
      tile(kA, vA, i);
    }
  }
  XS_MARK(2);
  __syncthreads();
  XS_MARK(3);

  // merge: RR * 16 threads per pair, (row qq, 4 columns dc)
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(xq.split_rec, 0, 0x7fffffff, 0x00020000);
  const int part = tid / (RR * 16), t = tid - part * (RR * 16), qq = t >> 4, dc = (t & 15) * 4;
  auto emit = [&](int pj, const float4_t& o) {
    int wj, hj;
    pair_wh(pj, wj, hj);
    store4(out + (int64_t)(s_wr0[pj - pa] + qq) * ldo + hj * 64 + dc, o[0], o[1], o[2], o[3]);
  };
#pragma unroll
  for (int pass = 0; pass < (XS_QP + PPASS - 1) / PPASS; ++pass) {
    const int pj = pa + pass * PPASS + part;
    if (pj <= plast && qq < s_wnr[pj - pa]) {
      const int l0 = pj * nsp - s0, l1 = l0 + nsp;  // the pair's tiles as local slots
      if (l0 >= 0 && l1 <= cnt) {                   // whole here: merge from LDS
        emit(pj, xs_merge(nsp, [&](int k, float& m, float& l, float4_t& o) {
               m = seg_m[l0 + k][qq];
               l = seg_l[l0 + k][qq];
               o = *reinterpret_cast<const float4_t*>(&seg_o[l0 + k][qq][dc]);
             }));
      } else {  // cut: this workgroup's partials of the pair -> records [pair][tile]
        for (int s = max(l0, 0); s < min(l1, cnt); ++s) {
          const int rb = (pj * nsp + (s - l0)) * XREC * 4;
          const float4_t o = *reinterpret_cast<const float4_t*>(&seg_o[s][qq][dc]);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, rb + (qq * 64 + dc) * 4, 0, 16);
          if (dc == 0) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, seg_m[s][qq]), rs, rb + (1024 + qq) * 4, 0, 16);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, seg_l[s][qq]), rs, rb + (1040 + qq) * 4, 0, 16);
          }
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its records
  __syncthreads();
  XS_MARK(4);
  // the cut pairs: the first if it began before this range, the last if it continues
  // after it (the same pair when the range lies inside one pair)
  const bool cut_a = pa * nsp < s0 || pa * nsp + nsp > s1;
  const bool cut_b = plast != pa && plast * nsp + nsp > s1;
  if (tid == 0) {
    const int ca = min(s1, pa * nsp + nsp) - s0, cb = s1 - plast * nsp;
    s_ticket[0] = cut_a && __hip_atomic_fetch_add(xq.split_cnt + pa, ca, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + ca == nsp;
    s_ticket[1] = cut_b && __hip_atomic_fetch_add(xq.split_cnt + plast, cb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + cb == nsp;
  }
  __syncthreads();
  XS_MARK(5);
  CT_MARK(CT_XATTN, 3);
  if (part > 1 || !s_ticket[part]) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the add
  const int pj = part ? plast : pa;
  if (t == 0) __hip_atomic_store(xq.split_cnt + pj, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (qq >= s_wnr[pj - pa]) return;  // only the window's rows were recorded
  emit(pj, xs_merge(nsp, [&](int k, float& m, float& l, float4_t& o) {
         const int rb = (pj * nsp + k) * XREC * 4;
         m = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, rb + (1024 + qq) * 4, 0, 16));
         l = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, rb + (1040 + qq) * 4, 0, 16));
         o = __builtin_bit_cast(float4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, rb + (qq * 64 + dc) * 4, 0, 16));
       }));
  XS_MARK(6);
}

}  // namespace wh
