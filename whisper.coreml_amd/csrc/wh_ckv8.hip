// The 8-bit (OCP FP8 E4M3) copy of the cross-KV for the decoder step's cross-attention:
// the quantiser (k_ckv_quant) and the KV8 instantiations of k_xattn_seg (wh_xattn.h).
// Format and record layout: whisper_hip.h "cross-KV formats", wh_kernels.h CKV8_REC.
#define WH_XS_NO_TRACE 1
#include "wh_xattn.h"

namespace wh {

// 16 fp32 values -> 16 E4M3 codes (round to nearest even; inv = 448 / amax, so |x inv| <= 448
// up to rounding: clamped, never the NaN code; a NaN input clamps to -448)
WH_DEV u32x4_t ckv8_encode(const float (&x)[16], float inv) {
  u32x4_t o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = fminf(fmaxf(x[4 * i + j] * inv, -448.f), 448.f);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
    o[i] = (unsigned)w;
  }
  return o;
}

// One workgroup per (64-key tile, head, layer x slot): reads the tile's 8 KB of fp16 K
// ([64 keys][64]) and 8 KB of fp16 V^T ([64 d][64 positions], xv_index) and writes its
// 8.5 KB record.  Thread (row = t >> 2, g = t & 3) holds the row's chunk g of both: elements
// 8 g .. + 7 and 32 + 8 g .. + 7, the 16 bytes lane group g of the step kernel loads.
//  * K: the row is a key, its amax a 4-lane reduction (xor 1, 2);
//  * V^T: the row is a channel and a key is a column: the 64 rows' |x| meet per column in
//    LDS (atomic max on the bits of a non-negative float), then every thread scales its 16.
// Padding keys (>= 1500) get scale 0 and code 0 whatever the fp16 rows hold.
__global__ __launch_bounds__(256) void k_ckv_quant(const half_t* __restrict__ ckv, char* __restrict__ ckv8, int nslots_cap,
                                                   int slot0, int nslots, int H) {
  __shared__ unsigned s_amax[64];
  const int t = threadIdx.x, row = t >> 2, g = t & 3;
  const int tile = blockIdx.x, h = blockIdx.y, layer = blockIdx.z / nslots, slot = slot0 + blockIdx.z % nslots;
  const int64_t per = (int64_t)H * TKP * 64;  // a slot's K (or V^T) elements
  const half_t* kp = ckv + ((int64_t)(2 * layer) * nslots_cap + slot) * per + ((int64_t)h * TKP + tile * 64 + row) * 64;
  const half_t* vp = kp + (int64_t)nslots_cap * per;  // V^T rows of a tile: [tile][64 d][64]
  char* rec = ckv8 + ((((int64_t)layer * nslots_cap + slot) * H + h) * CKV8_TILES + tile) * CKV8_REC;
  if (t < 64) s_amax[t] = 0u;
  const half8_t k0 = *reinterpret_cast<const half8_t*>(kp + 8 * g), k1 = *reinterpret_cast<const half8_t*>(kp + 32 + 8 * g);
  const half8_t v0 = *reinterpret_cast<const half8_t*>(vp + 8 * g), v1 = *reinterpret_cast<const half8_t*>(vp + 32 + 8 * g);
  float kx[16], vx[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    kx[e] = (float)k0[e], kx[8 + e] = (float)k1[e];
    vx[e] = (float)v0[e], vx[8 + e] = (float)v1[e];
  }
  __syncthreads();
  // position 32 s + 8 g + e of a V^T row is key 32 s + 16 (e >> 2) + 4 g + (e & 3) of the tile
  auto vkey = [&](int i) { return tile * 64 + 32 * (i >> 3) + 16 * ((i & 7) >> 2) + 4 * g + (i & 3); };
  float ka = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ka = fmaxf(ka, fabsf(kx[i]));
    atomicMax(&s_amax[32 * (i >> 3) + 8 * g + (i & 7)], __builtin_bit_cast(unsigned, fabsf(vx[i])));
  }
  ka = fmaxf(ka, __shfl_xor(ka, 1));
  ka = fmaxf(ka, __shfl_xor(ka, 2));
  if (tile * 64 + row >= 1500) ka = 0.f;
  *reinterpret_cast<u32x4_t*>(rec + row * 64 + 16 * g) = ckv8_encode(kx, ka > 0.f ? 448.f / ka : 0.f);
  if (g == 0) reinterpret_cast<float*>(rec + 8192)[row] = ka / 448.f;
  __syncthreads();
  // V^T: every element has its own key's scale
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float va = vkey(i) < 1500 ? __builtin_bit_cast(float, s_amax[32 * (i >> 3) + 8 * g + (i & 7)]) : 0.f;
    vx[i] *= va > 0.f ? 448.f / va : 0.f;
  }
  *reinterpret_cast<u32x4_t*>(rec + 4096 + row * 64 + 16 * g) = ckv8_encode(vx, 1.f);
  if (t < 64) {  // position t of the rows -> its key's V scale
    const int key = 32 * (t >> 5) + 16 * ((t & 7) >> 2) + 4 * ((t >> 3) & 3) + (t & 3);
    reinterpret_cast<float*>(rec + 8448)[key] = tile * 64 + key < 1500 ? __builtin_bit_cast(float, s_amax[t]) / 448.f : 0.f;
  }
}

void launch_ckv_quant(const void* ckv, void* ckv8, int layers, int nslots_cap, int slot0, int nslots, int H,
                      hipStream_t st) {
  k_ckv_quant<<<dim3(CKV8_TILES, H, layers * nslots), 256, 0, st>>>(reinterpret_cast<const half_t*>(ckv),
                                                                   reinterpret_cast<char*>(ckv8), nslots_cap, slot0,
                                                                   nslots, H),
      wh_launched("k_ckv_quant");
}

// the step cross-attention over the records: every query form, row count and grid form of
// launch_cross_attn's fp16 dispatch (wh_kernels.hip)
void launch_xattn_seg8(const void* q_, int ldq, const void* kv8, int Tk, int H, int npair, int nsp, int nwg, bool full,
                       const int* win_row0, const int* win_nrows, const int* win_slot, const XQPart& xq, void* out_,
                       int ldo, hipStream_t st) {
  typedef half_t T;
  const T* q = reinterpret_cast<const T*>(q_);
  const T* rec = reinterpret_cast<const T*>(kv8);
  T* out = reinterpret_cast<T*>(out_);
  const int64_t slot_bytes = (int64_t)ckv8_slot_bytes(H);
#define XS8(QZ_, RR_, S_, FULL_, QK_, NAME_)                                                                      \
  k_xattn_seg<T, QZ_, RR_, S_, FULL_, QK_, true><<<nwg, 512, 0, st>>>(q, ldq, rec, nullptr, Tk, H, npair, nsp,    \
                                                                      win_row0, win_nrows, win_slot, slot_bytes, \
                                                                      xq, out, ldo),                            \
      wh_launched(NAME_)
  if (xq.qx) {
    if (full) XS8(0, 8, float, true, 20, "k_xattn_seg<kv8,qproj>");
    else XS8(0, 8, float, false, 20, "k_xattn_seg<kv8,qproj>");
    return;
  }
#define XS8F(QZ_, RR_, S_)                                    \
  if (full) XS8(QZ_, RR_, S_, true, 0, "k_xattn_seg<kv8>");   \
  else XS8(QZ_, RR_, S_, false, 0, "k_xattn_seg<kv8>")
#define XS8S(QZ_, RR_)          \
  if constexpr (QZ_ > 0) {      \
    if (xq.part_half) {         \
      XS8F(QZ_, RR_, half_t);   \
      return;                   \
    }                           \
  }                             \
  XS8F(QZ_, RR_, float)
#define XS8R(QZ_)               \
  if (xq.max_rows <= 8) {       \
    XS8S(QZ_, 8);               \
  } else {                      \
    XS8S(QZ_, 16);              \
  }
  switch (xq.part ? xq.z : 0) {
    case 4: XS8R(4) break;
    case 8: XS8R(8) break;
    case 10: XS8R(10) break;
    default: XS8R(0) break;
  }
#undef XS8R
#undef XS8S
#undef XS8F
#undef XS8
}

}  // namespace wh
