// FLAC decoded on the device (wh_flac_ingest, wh_flac_decode_device): the frame code of
// wh_flacdev.h, one lane per frame-header candidate, then one lane per channel of every frame
// on the chain, then one thread per inter-channel sample.  A translation unit of its own, like
// wh_ingest.hip: the code object of wh_kernels.hip, whose kernels run in every decoder step,
// stays as it is.  Like the host decoder, nothing here verifies the frame CRC-16 or the
// STREAMINFO MD5.
//
// Staging is int32 [candidate slot][channel][block size]: a slot is channels * bs ints at the
// exclusive prefix sum of the candidates before it, tight, so a false candidate costs only its
// own block.  The parse lanes of a wave write wherever their frames are (nothing to coalesce
// there: each lane is a serial bit reader); channel-major slots make the gather's reads
// contiguous per channel across a wave, and its writes are the interleaved PCM in order.
#include "wh_flacdev.h"
#include "wh_kernels.h"

namespace wh {

using namespace whflac;

// Candidates per workgroup of k_flac_parse.  Its lanes are unrelated serial bit readers, so a
// wave runs as long as the union of its lanes' paths; a quarter-filled wave measured faster
// than a full one (FLAC on the device) and the device has SIMDs to spare here.
constexpr int PARSE_LANES = 16;

// one lane per candidate; ends[i] = where its frame ends, or -1
__global__ __launch_bounds__(64) void k_flac_parse(const uint8_t* __restrict__ data, int64_t n,
                                                   const Cand* __restrict__ cands, int n_cands, int channels,
                                                   int max_frame, int32_t* __restrict__ stage, Sub* __restrict__ subs,
                                                   int64_t* __restrict__ ends) {
  const int i = blockIdx.x * PARSE_LANES + threadIdx.x;
  if (i >= n_cands) return;
  const Cand c = cands[i];
  // the index made candidates of `channels` channels only, and slots of channels * bs ints
  ends[i] = channels_of(c.chc) == channels ? fd_parse_frame(data, n, c, max_frame, stage + c.slot, subs + (int64_t)i * channels)
                                          : -1;
}

// one lane per (chain frame, channel): the prediction restored in place
__global__ __launch_bounds__(64) void k_flac_restore(const Cand* __restrict__ cands, const int32_t* __restrict__ chain,
                                                     int n_frames, int channels, int32_t* __restrict__ stage,
                                                     const Sub* __restrict__ subs, int* __restrict__ bad) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= n_frames * channels) return;
  const int f = id / channels, ch = id - f * channels;
  const int ci = chain[f];
  const Cand c = cands[ci];
  if (!fd_restore(stage + c.slot + (int64_t)ch * c.bs, c.bs, subs[(int64_t)ci * channels + ch])) *bad = 1;
}

// one thread per inter-channel sample t: its frame by bisection of the chain's first samples
template <typename O>
__global__ __launch_bounds__(256) void k_flac_gather(const Cand* __restrict__ cands, const int32_t* __restrict__ chain,
                                                     const int64_t* __restrict__ starts, int n_frames, int channels,
                                                     const int32_t* __restrict__ stage, O* __restrict__ out,
                                                     int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int lo = 0, hi = n_frames - 1;  // starts[lo] <= t < starts[hi + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const Cand c = cands[chain[lo]];
  const int64_t i = t - starts[lo];
  if (i >= c.bs) return;  // cannot happen: the chain's block sizes tile [0, total)
  int64_t v[8];
  fd_gather(stage + c.slot, c.bs, c.chc, (int)i, v);
  for (int ch = 0; ch < channels; ++ch) out[t * channels + ch] = (O)v[ch];
}

void launch_flac_parse(const uint8_t* data, int64_t n, const Cand* cands, int n_cands, int channels, int max_frame,
                       int32_t* stage, Sub* subs, int64_t* ends, hipStream_t st) {
  if (n_cands < 1) return;
  k_flac_parse<<<(n_cands + PARSE_LANES - 1) / PARSE_LANES, PARSE_LANES, 0, st>>>(data, n, cands, n_cands, channels,
                                                                                  max_frame, stage, subs, ends),
      wh_launched("k_flac_parse");
}

void launch_flac_restore(const Cand* cands, const int32_t* chain, int n_frames, int channels, int32_t* stage,
                         const Sub* subs, int* bad, hipStream_t st) {
  if (n_frames < 1) return;
  k_flac_restore<<<(n_frames * channels + 63) / 64, 64, 0, st>>>(cands, chain, n_frames, channels, stage, subs, bad),
      wh_launched("k_flac_restore");
}

void launch_flac_gather(const Cand* cands, const int32_t* chain, const int64_t* starts, int n_frames, int channels,
                        const int32_t* stage, void* out, int s32, int64_t total, hipStream_t st) {
  if (n_frames < 1 || total < 1) return;
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (s32)
    k_flac_gather<int32_t><<<grid, 256, 0, st>>>(cands, chain, starts, n_frames, channels, stage, (int32_t*)out, total),
        wh_launched("k_flac_gather");
  else
    k_flac_gather<int16_t><<<grid, 256, 0, st>>>(cands, chain, starts, n_frames, channels, stage, (int16_t*)out, total),
        wh_launched("k_flac_gather");
}

}  // namespace wh
