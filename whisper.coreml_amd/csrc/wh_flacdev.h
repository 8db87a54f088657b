// FLAC frame code shared by the host and the device (wh_flac_decode_indexed, wh_flacdev.hip).
// One frame is decoded in three steps that need nothing from any other frame:
//   fd_parse_frame  the subframe headers and the Rice residuals of a frame-header candidate:
//                   warm-up samples and residuals go to the candidate's staging slot
//                   ([channel][block size] int32), the predictor to a Sub record per channel;
//   fd_restore      the prediction of one channel, in place;
//   fd_gather       one inter-channel sample: the stereo decorrelation undone.
// Each mirrors wh_flac.cpp's subframe / residual / wh_flac_decode operation for operation, so a
// frame both accept gives the same samples.  A candidate may be a false one (a header-shaped
// byte run inside a frame body), so this code meets garbage in ordinary operation: every read is
// bounded by a byte limit (the stream's end or the frame's byte budget, whichever is nearer),
// every count by the candidate's block size, every store lies in the candidate's own slot, and
// whatever the host decoder would treat differently from a plain valid frame (a sample that
// leaves int32, a partition count that does not divide the block, more than 24 bits) marks the
// candidate bad, which sends the whole stream to the host decoder.  Like the host decoder, this
// code verifies neither the frame CRC-16 nor the STREAMINFO MD5.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define WH_FD __host__ __device__ inline
#else
#define WH_FD inline
#endif

namespace whflac {

struct Info {  // STREAMINFO
  int rate = 0, channels = 0, bps = 0;
  int max_block = 0, max_frame = 0;  // 0: unknown
  int64_t total = 0;
  int64_t frames_at = 0;  // byte offset of the first frame
};

struct Cand {      // a frame-header candidate
  int64_t off;     // byte offset of the sync code
  int64_t slot;    // first int32 of its staging slot: channels * bs of them
  int32_t hdr_len, bs, chc, bps;
};

enum { SUB_CONSTANT = 0, SUB_VERBATIM = 1, SUB_FIXED = 2, SUB_LPC = 3 };
struct Sub {  // one channel's predictor
  int32_t type, order, shift, wasted;
  int16_t coef[32];  // LPC precision is at most 15 bits
};

constexpr int MAX_BITS = 24;      // bits per sample the indexed path takes (a side channel has one more)
constexpr int STAGE_MULTIPLE = 4; // staging ints allowed per PCM int: more false candidates than that go to the host

WH_FD int channels_of(int chc) { return chc < 8 ? chc + 1 : 2; }

// bytes a frame may take before its candidate is given up
WH_FD int64_t frame_budget(const Cand& c, int max_frame) {
  if (max_frame > 0) return max_frame;
  const int64_t verbatim = ((int64_t)c.bs * channels_of(c.chc) * (c.bps + 1) + 7) / 8 + 8 * 2;
  return 2 * verbatim + c.hdr_len + 2;
}

WH_FD uint8_t crc8_step(uint8_t crc, uint8_t byte) {
  crc ^= byte;
  for (int k = 0; k < 8; ++k) crc = (uint8_t)((crc & 0x80) ? (crc << 1) ^ 0x07 : crc << 1);
  return crc;
}

// A frame header at d[i] (n = stream length)?  Sync code with the reserved bit clear, no
// reserved block-size / sample-rate / sample-size code, a channel code <= 10 of `channels`
// channels, a well-formed UTF-8-style number, reserved bit clear, CRC-8 correct.
WH_FD bool fd_header(const uint8_t* d, int64_t n, int64_t i, int channels, int stream_bps, Cand* c) {
  if (i + 5 > n || d[i] != 0xFF || (d[i + 1] & 0xFE) != 0xF8) return false;
  const int bsc = d[i + 2] >> 4, src = d[i + 2] & 15, chc = d[i + 3] >> 4, ssc = (d[i + 3] >> 1) & 7;
  if (bsc == 0 || src == 15 || ssc == 3 || (d[i + 3] & 1)) return false;
  if (chc > 10 || channels_of(chc) != channels) return false;
  const uint8_t f0 = d[i + 4];
  int ones = 0;
  for (int m = 0x80; m && (f0 & m); m >>= 1) ++ones;
  if (ones == 1 || ones == 8) return false;
  const int nbytes = ones ? ones : 1;
  int64_t p = i + 4 + nbytes;
  if (p > n) return false;
  for (int k = 1; k < nbytes; ++k)
    if ((d[i + 4 + k] & 0xC0) != 0x80) return false;
  int bs;
  if (bsc == 1) bs = 192;
  else if (bsc <= 5) bs = 576 << (bsc - 2);
  else if (bsc == 6) {
    if (p + 1 > n) return false;
    bs = d[p] + 1;
    p += 1;
  } else if (bsc == 7) {
    if (p + 2 > n) return false;
    bs = ((d[p] << 8) | d[p + 1]) + 1;
    p += 2;
  } else bs = 256 << (bsc - 8);
  p += src == 12 ? 1 : (src == 13 || src == 14) ? 2 : 0;
  if (p + 1 > n) return false;
  uint8_t crc = 0;
  for (int64_t k = i; k < p; ++k) crc = crc8_step(crc, d[k]);
  if (crc != d[p]) return false;
  const int ssz[8] = {0, 8, 12, 0, 16, 20, 24, 32};
  c->off = i;
  c->slot = 0;
  c->hdr_len = (int32_t)(p + 1 - i);
  c->bs = bs;
  c->chc = chc;
  c->bps = ssc == 0 ? stream_bps : ssz[ssc];
  return true;
}

struct Bits {  // MSB-first reader over p[0, lim)
  const uint8_t* p;
  int64_t lim;  // bytes that may be read
  int64_t pos;  // in bits
  bool bad;
  WH_FD Bits(const uint8_t* d, int64_t limit, int64_t byte0) : p(d), lim(limit), pos(byte0 * 8), bad(false) {}
  // the 64 bits from the byte that holds pos; bytes from lim on read as zeros
  WH_FD uint64_t window() const {
    const int64_t b = pos >> 3;
    uint64_t w = 0;
    if (b + 8 <= lim) {
      for (int i = 0; i < 8; ++i) w = (w << 8) | p[b + i];
    } else {
      for (int i = 0; i < 8; ++i) w = (w << 8) | (b + i < lim ? p[b + i] : 0);
    }
    return w;
  }
  WH_FD uint64_t u(int k) {  // k <= 56
    if (k <= 0) return 0;
    if (bad || pos + k > lim * 8) {
      bad = true;
      return 0;
    }
    const uint64_t v = (window() << (pos & 7)) >> (64 - k);
    pos += k;
    return v;
  }
  WH_FD int64_t s(int k) {  // two's complement, k bits
    if (k <= 0) return 0;
    const uint64_t v = u(k);
    return (int64_t)(v << (64 - k)) >> (64 - k);
  }
  WH_FD uint32_t unary() {  // zeros before the next 1; each turn consumes a bit or ends
    uint32_t q = 0;
    while (!bad) {
      const int64_t left = lim * 8 - pos;
      if (left <= 0) {
        bad = true;
        break;
      }
      const int avail = left < 57 ? (int)left : 57;
      const uint64_t w = window() << (pos & 7);
      const int z = w ? __builtin_clzll(w) : 64;
      if (z < avail) {
        q += (uint32_t)z;
        pos += z + 1;
        break;
      }
      q += (uint32_t)avail;
      pos += avail;
    }
    return q;
  }
  WH_FD void align() { pos = (pos + 7) & ~int64_t(7); }
};

// residual of a FIXED / LPC subframe (partitioned Rice, 4- or 5-bit parameters) into out[order, bs)
WH_FD bool fd_residual(Bits& b, int bs, int order, int32_t* out) {
  const int method = (int)b.u(2);
  if (method > 1) return false;
  const int pbits = method == 0 ? 4 : 5, esc = method == 0 ? 15 : 31;
  const int po = (int)b.u(4);
  const int parts = 1 << po;
  if ((bs >> po) < order) return false;
  if (bs & (parts - 1)) return false;  // the host decoder leaves the tail to its last frame: not ours to mirror
  int k = order;
  for (int pi = 0; pi < parts; ++pi) {
    const int cnt = (bs >> po) - (pi == 0 ? order : 0);
    const int rp = (int)b.u(pbits);
    if (rp == esc) {
      const int nb = (int)b.u(5);
      for (int j = 0; j < cnt && !b.bad; ++j) out[k++] = (int32_t)b.s(nb);
    } else {
      for (int j = 0; j < cnt && !b.bad; ++j) {
        const uint64_t q = b.unary();
        const uint64_t v = (q << rp) | (rp ? b.u(rp) : 0);
        out[k++] = (int32_t)((int64_t)(v >> 1) ^ -(int64_t)(v & 1));
      }
    }
    if (b.bad) return false;
  }
  return true;
}

// one subframe: warm-up / verbatim / constant samples and residuals into s[0, bs), the rest into *sub
WH_FD bool fd_subframe(Bits& b, int bs, int bps, int32_t* s, Sub* sub) {
  if (b.u(1) != 0) return false;
  const int type = (int)b.u(6);
  int wasted = 0;
  if (b.u(1)) wasted = (int)b.unary() + 1;
  if (b.bad) return false;
  bps -= wasted;
  if (bps <= 0) return false;
  sub->wasted = wasted;
  sub->order = 0;
  sub->shift = 0;
  if (type == 0) {
    sub->type = SUB_CONSTANT;
    s[0] = (int32_t)b.s(bps);
  } else if (type == 1) {
    sub->type = SUB_VERBATIM;
    for (int i = 0; i < bs && !b.bad; ++i) s[i] = (int32_t)b.s(bps);
  } else if (type >= 8 && type <= 12) {
    const int order = type - 8;
    if (order > bs) return false;
    sub->type = SUB_FIXED;
    sub->order = order;
    for (int i = 0; i < order; ++i) s[i] = (int32_t)b.s(bps);
    if (!fd_residual(b, bs, order, s)) return false;
  } else if (type >= 32) {
    const int order = type - 31;
    if (order > bs) return false;
    sub->type = SUB_LPC;
    sub->order = order;
    for (int i = 0; i < order; ++i) s[i] = (int32_t)b.s(bps);
    const int prec = (int)b.u(4) + 1;
    if (prec == 16) return false;
    const int shift = (int)b.s(5);
    if (shift < 0) return false;
    sub->shift = shift;
    for (int j = 0; j < order; ++j) sub->coef[j] = (int16_t)b.s(prec);
    if (!fd_residual(b, bs, order, s)) return false;
  } else {
    return false;
  }
  return !b.bad;
}

// The frame of candidate c: its subframes into slot ([channel][bs]) and subs ([channel]).
// Returns the byte offset where the frame ends (after alignment and the CRC-16), or -1.
WH_FD int64_t fd_parse_frame(const uint8_t* d, int64_t n, const Cand& c, int max_frame, int32_t* slot, Sub* subs) {
  if (c.bps < 4 || c.bps > MAX_BITS || c.bs < 1) return -1;
  int64_t lim = c.off + frame_budget(c, max_frame);
  if (lim > n) lim = n;
  Bits b(d, lim, c.off + c.hdr_len);
  const int nch = channels_of(c.chc);
  for (int ch = 0; ch < nch; ++ch) {
    const bool side = (c.chc == 8 && ch == 1) || (c.chc == 9 && ch == 0) || (c.chc == 10 && ch == 1);
    if (!fd_subframe(b, c.bs, c.bps + (side ? 1 : 0), slot + (int64_t)ch * c.bs, subs + ch)) return -1;
  }
  b.align();
  b.u(16);  // CRC-16 of the frame
  if (b.bad) return -1;
  return b.pos >> 3;
}

// The prediction of one channel restored in place.  False: a sample left int32, where the host
// decoder's int64 history and ours would part.
WH_FD bool fd_restore(int32_t* s, int bs, const Sub& sub) {
  bool ok = true;
  const int order = sub.order;
  if (sub.type == SUB_CONSTANT) {
    const int32_t v = s[0];
    for (int i = 1; i < bs; ++i) s[i] = v;
  } else if (sub.type == SUB_FIXED) {
    for (int i = order; i < bs; ++i) {
      int64_t p = 0;
      switch (order) {
        case 1: p = s[i - 1]; break;
        case 2: p = 2 * (int64_t)s[i - 1] - s[i - 2]; break;
        case 3: p = 3 * (int64_t)s[i - 1] - 3 * (int64_t)s[i - 2] + s[i - 3]; break;
        case 4: p = 4 * (int64_t)s[i - 1] - 6 * (int64_t)s[i - 2] + 4 * (int64_t)s[i - 3] - s[i - 4]; break;
        default: break;
      }
      const int64_t v = p + s[i];
      ok = ok && v == (int32_t)v;
      s[i] = (int32_t)v;
    }
  } else if (sub.type == SUB_LPC) {
    for (int i = order; i < bs; ++i) {
      int64_t acc = 0;
      for (int j = 0; j < order; ++j) acc += (int64_t)sub.coef[j] * s[i - 1 - j];
      const int64_t v = s[i] + (acc >> sub.shift);
      ok = ok && v == (int32_t)v;
      s[i] = (int32_t)v;
    }
  }
  if (sub.wasted)
    for (int i = 0; i < bs; ++i) {
      const int64_t v = (int64_t)((uint64_t)(int64_t)s[i] << sub.wasted);
      ok = ok && v == (int32_t)v;
      s[i] = (int32_t)v;
    }
  return ok;
}

// sample i of a restored frame: v[0, channels) with left/side, side/right and mid/side undone
WH_FD void fd_gather(const int32_t* slot, int bs, int chc, int i, int64_t* v) {
  const int nch = channels_of(chc);
  for (int c = 0; c < nch; ++c) v[c] = slot[(int64_t)c * bs + i];
  if (chc == 8) v[1] = v[0] - v[1];
  else if (chc == 9) v[0] = v[0] + v[1];
  else if (chc == 10) {
    const int64_t mid = (v[0] * 2) | (v[1] & 1), sd = v[1];
    v[0] = (mid + sd) >> 1;
    v[1] = (mid - sd) >> 1;
  }
}

// ---- host side (wh_flac.cpp)
struct Plan {
  Info si;
  std::vector<Cand> cands;  // sorted by offset, slots assigned
  int64_t stage = 0;        // staging ints in all
};
// STREAMINFO and the candidate index.  0: the indexed path may run; 1: the stream is outside it
// (32 bits, unknown total, too much staging, no frame at the first frame's offset); < 0: not FLAC
// (the host decoder's code and message, wh_flac_last_error)
int flac_plan(const uint8_t* data, int64_t n, Plan* plan);
// Follow "frame end = next candidate's offset" from the first frame to the end of the stream.
// ends[i]: where candidate i's frame ends, or -1.  True: the chain holds and its block sizes sum
// to the total; frames = the chain's candidates, starts = their first samples (and the total).
bool flac_chain(const Plan& plan, int64_t n, const int64_t* ends, std::vector<int32_t>* frames,
                std::vector<int64_t>* starts);

}  // namespace whflac

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace wh {
// wh_flacdev.hip.  All pointers are device pointers; cands [n_cands] with their slots inside
// stage, subs [n_cands][channels], ends [n_cands]; chain [n_frames] indexes cands, starts
// [n_frames + 1] are the chain frames' first samples; *bad must be 0 before the restore.
void launch_flac_parse(const uint8_t* data, int64_t n, const whflac::Cand* cands, int n_cands, int channels,
                       int max_frame, int32_t* stage, whflac::Sub* subs, int64_t* ends, hipStream_t st);
void launch_flac_restore(const whflac::Cand* cands, const int32_t* chain, int n_frames, int channels, int32_t* stage,
                         const whflac::Sub* subs, int* bad, hipStream_t st);
// out: interleaved PCM [total][channels], int32 (s32) or int16
void launch_flac_gather(const whflac::Cand* cands, const int32_t* chain, const int64_t* starts, int n_frames,
                        int channels, const int32_t* stage, void* out, int s32, int64_t total, hipStream_t st);
}  // namespace wh
#endif
