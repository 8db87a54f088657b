// PCM ingest kernels of libwhisper_hip (wh_audio_ingest, wh_flac_ingest, wh_wav_ingest and their
// _split forms, which keep the channels apart).  A
// translation unit of its own: the code object of wh_kernels.hip, whose kernels run in every
// decoder step, stays as it is.
#include "wh_kernels.h"
#include "whisper_hip.h"

namespace wh {

// ---------------------------------------------------------------- PCM ingest
// Interleaved PCM [frames][channels] in one of the WH_WAV_* encodings -> mono float32 at
// 16 kHz, the arithmetic of whisper/audio.py pcm_to_waveform in fp64 (include/whisper_hip.h,
// wh_audio_ingest):
//   x[m] = (sum of the frame's channels) * 2^-(bits-1) / channels   (exact up to the division)
//   y[k] = sum_m x[m] * taps[k*down - m*up + half],  out[k] = clip(rint(32768 y[k])) / 32768
// A workgroup owns `block` consecutive outputs.  Their inputs are one contiguous span of
// frames, mixed down once into LDS (frames before 0 and from n on are zeros, never read);
// thread k then walks the taps of its phase, taps[phase + j*up], against frames going
// backwards from mt = (k*down + half) / up.  Every index that grows with the file is 64-bit.
struct ResampleArgs {
  const void* pcm;
  int64_t n, n_out;
  int channels, up, down, half, block, span_cap;
  double scale;        // 2^-(bits-1)
  const double* taps;  // [2*half + 1]; null: no filter (up == down), out[k] is x[k] quantised
  float* out;
};

// Sample readers: how sample j of the uploaded bytes is read, one per encoding.  Integer
// readers return the sample's integer (the frame's channels are summed in int64), float
// readers return fp64.
// The bytes start at sample 0 of the data (wh_wav_ingest uploads the data chunk alone), so
// sample j lies at byte j * container, naturally aligned for 2-, 4- and 8-byte containers.
struct ReadS16 {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) { return ((const int16_t*)b)[j]; }
};
struct ReadS32 {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) { return ((const int32_t*)b)[j]; }
};
struct ReadU8 {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) { return (int)b[j] - 128; }
};
// 24-bit packed: a sample straddles dwords at three of its four byte phases.  Two aligned
// dword loads and a byte align (the buffer is reserved 8 bytes past the data, so the second
// dword is inside the allocation; what it holds past the data is shifted out).  Three byte
// loads per sample were measured 2 % slower on 600 s of 44.1 kHz stereo.
struct ReadS24 {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) {
    const int64_t at = 3 * j;
    const uint32_t* w = (const uint32_t*)b + (at >> 2);
    const uint32_t v = __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(at & 3));
    return (int32_t)(v << 8) >> 8;
  }
};
// G.711 by shifts (include/whisper_hip.h), no table in memory
struct ReadUlaw {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) {
    const int u = ~b[j] & 0xFF, e = (u >> 4) & 7, m = u & 15;
    const int mag = (((m << 3) + 0x84) << e) - 0x84;
    return u & 0x80 ? -mag : mag;
  }
};
struct ReadAlaw {
  typedef int64_t Acc;
  static __device__ inline int64_t at(const uint8_t* __restrict__ b, int64_t j) {
    const int a = b[j] ^ 0x55, e = (a >> 4) & 7, m = a & 15;
    const int mag = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8;
    return a & 0x80 ? mag : -mag;
  }
};
// float samples: a non-finite value is 0, finite ones are clamped so that no sum overflows
__device__ inline double float_sample(double v) {
  if (!(fabs(v) <= 1.7976931348623157e308)) return 0.0;  // NaN, +-Inf
  return fmin(fmax(v, -256.0), 256.0);
}
struct ReadF32 {
  typedef double Acc;
  static __device__ inline double at(const uint8_t* __restrict__ b, int64_t j) { return float_sample((double)((const float*)b)[j]); }
};
struct ReadF64 {
  typedef double Acc;
  static __device__ inline double at(const uint8_t* __restrict__ b, int64_t j) { return float_sample(((const double*)b)[j]); }
};

// x[m]: the frame's channels added in channel order (int64 for the integer encodings, fp64 for
// the float ones, whose scale is 1), scaled and divided by the channel count
template <typename R>
__device__ inline double pcm_frame(const uint8_t* __restrict__ pcm, int64_t m, int64_t n, int channels, double scale) {
  if (m < 0 || m >= n) return 0.0;
  const int64_t j = m * channels;
  typename R::Acc s = R::at(pcm, j);
  for (int c = 1; c < channels; ++c) s += R::at(pcm, j + c);
  return (double)s * scale / (double)channels;
}

// MODE 1, 2: the span goes through LDS (span_cap doubles of dynamic LDS), and in mode 2 the
// taps lie behind it (short filters: up = 1 gives every thread the same tap, and a vector
// load of one shared global address costs as much as a gather).  MODE 0: every tap reads its
// frame from global memory (ratios whose span does not fit, and the no-filter case).
template <typename R, int MODE>
__global__ __launch_bounds__(256) void k_pcm_resample(ResampleArgs a) {
  extern __shared__ __align__(16) double pcm_span[];
  const uint8_t* __restrict__ pcm = (const uint8_t*)a.pcm;
  const int64_t k0 = (int64_t)blockIdx.x * a.block;
  const int64_t k1 = k0 + a.block < a.n_out ? k0 + a.block : a.n_out;
  if (k0 >= k1) return;
  const int last_tap = 2 * a.half;
  int64_t m_lo = 0;
  constexpr bool STAGED = MODE != 0;
  const double* taps_lds = pcm_span + a.span_cap;
  if (STAGED) {
    const int64_t m_hi = ((k1 - 1) * a.down + a.half) / a.up;
    m_lo = (k0 * a.down + a.half) / a.up - last_tap / a.up;
    const int64_t len = m_hi - m_lo + 1;
    if (len > a.span_cap) return;  // cannot happen for the block the launcher chose
    for (int i = threadIdx.x; i < (int)len; i += 256) pcm_span[i] = pcm_frame<R>(pcm, m_lo + i, a.n, a.channels, a.scale);
    if (MODE == 2)
      for (int i = threadIdx.x; i <= last_tap; i += 256) pcm_span[a.span_cap + i] = a.taps[i];
    __syncthreads();
  }
  for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
    double y;
    if (!a.taps) {
      y = pcm_frame<R>(pcm, k, a.n, a.channels, a.scale);
    } else {
      const int64_t c = k * a.down + a.half;
      int64_t m = c / a.up;                // the newest frame that reaches output k
      int t = (int)(c - m * a.up);         // and its tap: the thread's phase
      y = 0.0;
      int i = (int)(m - m_lo);  // the frame's place in the span
      for (; t <= last_tap; t += a.up, --m, --i) {
        const double x = STAGED ? pcm_span[i] : pcm_frame<R>(pcm, m, a.n, a.channels, a.scale);
        y = fma(x, MODE == 2 ? taps_lds[t] : a.taps[t], y);
      }
    }
    double r = rint(y * 32768.0);  // round half to even, as np.round
    r = fmin(fmax(r, -32768.0), 32767.0);
    a.out[k] = (float)r * (1.0f / 32768.0f);
  }
}

void launch_pcm_resample(const void* pcm, int encoding, int64_t n_frames, int channels, int bits, int up, int down,
                         const double* taps, float* out, int64_t n_out, hipStream_t st) {
  if (n_out < 1) return;
  ResampleArgs a;
  a.pcm = pcm; a.n = n_frames; a.n_out = n_out; a.channels = channels; a.up = up; a.down = down;
  a.half = taps ? 10 * (up > down ? up : down) : 0;
  a.scale = ldexp(1.0, -(bits - 1));
  a.taps = taps; a.out = out;
  // the largest block whose span of frames fits 64 KiB of LDS
  a.block = 0;
  a.span_cap = 0;
  if (taps)
    for (int b = 1024; b >= 256 && !a.block; b /= 2) {
      const int64_t span = (int64_t)(b - 1) * down / up + 2 * a.half / up + 2;
      if (span * 8 <= 65536) a.block = b, a.span_cap = (int)span;
    }
  const bool staged = a.block != 0;
  if (!staged) a.block = 1024;
  const bool taps_in_lds = staged && ((size_t)a.span_cap + 2 * a.half + 1) * 8 <= 65536;
  const unsigned grid = (unsigned)((n_out + a.block - 1) / a.block);
  const size_t lds = ((size_t)a.span_cap + (taps_in_lds ? 2 * a.half + 1 : 0)) * 8;
#define LAUNCH_RESAMPLE_AS(R_, MODE_) \
  k_pcm_resample<R_, MODE_><<<grid, 256, lds, st>>>(a), wh_launched("k_pcm_resample")
#define LAUNCH_RESAMPLE(MODE_)                                       \
  do {                                                               \
    switch (encoding) {                                              \
      case WH_WAV_U8: LAUNCH_RESAMPLE_AS(ReadU8, MODE_); break;     \
      case WH_WAV_S16: LAUNCH_RESAMPLE_AS(ReadS16, MODE_); break;   \
      case WH_WAV_S24: LAUNCH_RESAMPLE_AS(ReadS24, MODE_); break;   \
      case WH_WAV_S32: LAUNCH_RESAMPLE_AS(ReadS32, MODE_); break;   \
      case WH_WAV_F32: LAUNCH_RESAMPLE_AS(ReadF32, MODE_); break;   \
      case WH_WAV_F64: LAUNCH_RESAMPLE_AS(ReadF64, MODE_); break;   \
      case WH_WAV_ALAW: LAUNCH_RESAMPLE_AS(ReadAlaw, MODE_); break; \
      case WH_WAV_ULAW: LAUNCH_RESAMPLE_AS(ReadUlaw, MODE_); break; \
      default: break; /* the callers pass one of the eight */       \
    }                                                                \
  } while (0)
  if (taps_in_lds) LAUNCH_RESAMPLE(2);
  else if (staged) LAUNCH_RESAMPLE(1);
  else LAUNCH_RESAMPLE(0);
#undef LAUNCH_RESAMPLE
#undef LAUNCH_RESAMPLE_AS
}

// ---------------------------------------------------------------- PCM ingest, a chunk of a stream
// k_pcm_resample for a recording that arrives in chunks (wh_stream_append, wh_stream_finish).
// All indices are those of the whole recording: the chunk holds frames [n0, n0 + nc), the launch
// writes outputs [k0, k0 + n_emit), k0 = E(n0), whose newest frame (k*down + half) / up lies in
// the chunk.  Output k walks the same taps in the same order with the same fma as the one-shot
// kernel, so it is that kernel's output k; the only difference is where x[m] comes from:
//   m >= n0 + nc   0.0 (only wh_stream_finish asks: the frames behind the recording)
//   m >= n0        pcm_frame of the chunk's frame m - n0
//   m >= n0 - H    hist_old[m - (n0 - H)], the fp64 x[m] the launch that owned frame m stored
// and nothing older is reached: the walk of output k >= E(n0) ends at or after frame
// n0 - 2*half/up, and H = 2*half/up.  Frames before the recording are stored as the 0.0 they
// are (the history starts zeroed).  The block behind the output blocks writes the next
// history, x[n0 + nc - H .. n0 + nc), into the other half of the double buffer: a chunk
// shorter than H takes the frames it lacks from the old history, and a launch that emits
// nothing still moves the history on.  No filter (taps null): out[k] is x[k] quantised, H = 0.
struct StreamArgs {
  const void* pcm;  // the chunk
  int64_t n0, nc, k0, n_emit;
  int channels, up, down, half, hist;
  double scale;
  const double* taps;
  const double* hist_old;
  double* hist_new;
  float* out;  // output k0
};

template <typename R>
__device__ inline double stream_frame(const StreamArgs& a, int64_t m) {
  if (m >= a.n0) return pcm_frame<R>((const uint8_t*)a.pcm, m - a.n0, a.nc, a.channels, a.scale);
  const int64_t j = m - (a.n0 - a.hist);
  return j >= 0 ? a.hist_old[j] : 0.0;
}

// what workgroup `block` of a stream's launch does: blocks [0, ceil(n_emit / 256)) own 256
// outputs each, the block behind them writes the next history.  k_pcm_resample_stream and
// k_pcm_resample_pool both run this body, so a pool slot's samples are the single stream's.
template <typename R>
__device__ inline void stream_block(const StreamArgs& a, int64_t block) {
  const int64_t out_blocks = (a.n_emit + 255) / 256;
  if (block >= out_blocks) {
    for (int j = threadIdx.x; j < a.hist; j += 256) a.hist_new[j] = stream_frame<R>(a, a.n0 + a.nc - a.hist + j);
    return;
  }
  const int64_t i = block * 256 + threadIdx.x;
  if (i >= a.n_emit) return;
  const int64_t k = a.k0 + i;
  double y;
  if (!a.taps) {
    y = stream_frame<R>(a, k);
  } else {
    const int last_tap = 2 * a.half;
    const int64_t c = k * a.down + a.half;
    int64_t m = c / a.up;         // the newest frame that reaches output k
    int t = (int)(c - m * a.up);  // and its tap
    y = 0.0;
    for (; t <= last_tap; t += a.up, --m) y = fma(stream_frame<R>(a, m), a.taps[t], y);
  }
  double r = rint(y * 32768.0);  // round half to even, as np.round
  r = fmin(fmax(r, -32768.0), 32767.0);
  a.out[i] = (float)r * (1.0f / 32768.0f);
}

template <typename R>
__global__ __launch_bounds__(256) void k_pcm_resample_stream(StreamArgs a) {
  stream_block<R>(a, (int64_t)blockIdx.x);
}

// the arguments of one stream's chunk, for its own launch or as its descriptor in a pool launch
static StreamArgs stream_args(const void* pcm, int64_t n0, int64_t nc, int channels, int bits, int up, int down,
                              const double* taps, const double* hist_old, double* hist_new, int hist, float* out,
                              int64_t k0, int64_t n_emit) {
  StreamArgs a;
  a.pcm = pcm; a.n0 = n0; a.nc = nc; a.k0 = k0; a.n_emit = n_emit; a.channels = channels; a.up = up; a.down = down;
  a.half = taps ? 10 * (up > down ? up : down) : 0;
  a.hist = hist;
  a.scale = ldexp(1.0, -(bits - 1));
  a.taps = taps; a.hist_old = hist_old; a.hist_new = hist_new; a.out = out;
  return a;
}

void launch_pcm_resample_stream(const void* pcm, int encoding, int64_t n0, int64_t nc, int channels, int bits, int up,
                                int down, const double* taps, const double* hist_old, double* hist_new, int hist,
                                float* out, int64_t k0, int64_t n_emit, hipStream_t st) {
  if (n_emit < 1 && hist < 1) return;
  const StreamArgs a = stream_args(pcm, n0, nc, channels, bits, up, down, taps, hist_old, hist_new, hist, out, k0, n_emit);
  const unsigned grid = (unsigned)((n_emit + 255) / 256) + (hist > 0 ? 1 : 0);
#define LAUNCH_STREAM_AS(R_) k_pcm_resample_stream<R_><<<grid, 256, 0, st>>>(a), wh_launched("k_pcm_resample_stream")
  switch (encoding) {
    case WH_WAV_U8: LAUNCH_STREAM_AS(ReadU8); break;
    case WH_WAV_S16: LAUNCH_STREAM_AS(ReadS16); break;
    case WH_WAV_S24: LAUNCH_STREAM_AS(ReadS24); break;
    case WH_WAV_S32: LAUNCH_STREAM_AS(ReadS32); break;
    case WH_WAV_F32: LAUNCH_STREAM_AS(ReadF32); break;
    case WH_WAV_F64: LAUNCH_STREAM_AS(ReadF64); break;
    case WH_WAV_ALAW: LAUNCH_STREAM_AS(ReadAlaw); break;
    case WH_WAV_ULAW: LAUNCH_STREAM_AS(ReadUlaw); break;
    default: break; /* the callers pass one of the eight */
  }
#undef LAUNCH_STREAM_AS
}

// ---------------------------------------------------------------- PCM ingest, many streams per launch
// k_pcm_resample_stream for the stream pool (wh_pool_append, wh_pool_finish): one grid covers a
// chunk of each of n streams.  Stream s of the call has a descriptor: the StreamArgs its own
// launch would get, its encoding and the index of its first workgroup; it owns the workgroups
// [block0[s], block0[s + 1]), ceil(n_emit / 256) + (hist > 0) of them, never none (the host leaves
// out a stream that has no work).  A workgroup finds its stream by a binary search of the
// first-workgroup indices (log2(n) block-uniform loads of a table that stays in the scalar
// cache; a per-block map would cost a host write and a copied word per workgroup, and a tick of
// 20 ms packets has one or two workgroups per stream anyway), copies the descriptor and runs
// stream_block through a block-uniform switch on the encoding.
struct PoolStream {
  StreamArgs a;
  int encoding;  // WH_WAV_*
  int block0;
};

__global__ __launch_bounds__(256) void k_pcm_resample_pool(const PoolStream* __restrict__ d, int n) {
  const int b = (int)blockIdx.x;
  int lo = 0, hi = n - 1;  // the last stream whose first workgroup is at or before b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].block0 <= b) lo = mid;
    else hi = mid - 1;
  }
  const StreamArgs a = d[lo].a;
  const int64_t block = b - d[lo].block0;
  switch (d[lo].encoding) {
    case WH_WAV_U8: stream_block<ReadU8>(a, block); break;
    case WH_WAV_S16: stream_block<ReadS16>(a, block); break;
    case WH_WAV_S24: stream_block<ReadS24>(a, block); break;
    case WH_WAV_S32: stream_block<ReadS32>(a, block); break;
    case WH_WAV_F32: stream_block<ReadF32>(a, block); break;
    case WH_WAV_F64: stream_block<ReadF64>(a, block); break;
    case WH_WAV_ALAW: stream_block<ReadAlaw>(a, block); break;
    case WH_WAV_ULAW: stream_block<ReadUlaw>(a, block); break;
    default: break; /* the host passes one of the eight */
  }
}

size_t pool_stream_bytes() { return sizeof(PoolStream); }

int64_t pool_stream_fill(void* desc, int i, int64_t block0, const void* pcm, int encoding, int64_t n0, int64_t nc,
                         int channels, int bits, int up, int down, const double* taps, const double* hist_old,
                         double* hist_new, int hist, float* out, int64_t k0, int64_t n_emit) {
  PoolStream& p = ((PoolStream*)desc)[i];
  p.a = stream_args(pcm, n0, nc, channels, bits, up, down, taps, hist_old, hist_new, hist, out, k0, n_emit);
  p.encoding = encoding;
  p.block0 = (int)block0;
  return (n_emit + 255) / 256 + (hist > 0 ? 1 : 0);
}

void launch_pcm_resample_pool(const void* desc, int n, int64_t n_blocks, hipStream_t st) {
  if (n < 1 || n_blocks < 1) return;
  k_pcm_resample_pool<<<(unsigned)n_blocks, 256, 0, st>>>((const PoolStream*)desc, n), wh_launched("k_pcm_resample_pool");
}

// wh_pool_trim: move i copies n floats from src to dst, which never overlap (a slot's two
// buffers).  blockIdx.y is the move, the workgroups of a row stride over its floats.
__global__ __launch_bounds__(256) void k_pool_move(const PoolMove* __restrict__ mv) {
  const PoolMove m = mv[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m.n; i += (int64_t)gridDim.x * 256) m.dst[i] = m.src[i];
}

void launch_pool_move(const PoolMove* moves, int n, int64_t longest, hipStream_t st) {
  if (n < 1 || longest < 1) return;
  const int64_t want = (longest + 1023) / 1024;  // four floats per thread, at most 64 workgroups per move
  k_pool_move<<<dim3((unsigned)(want < 64 ? want : 64), (unsigned)n), 256, 0, st>>>(moves), wh_launched("k_pool_move");
}

// ---------------------------------------------------------------- PCM ingest, channels apart
// The sibling of k_pcm_resample for wh_*_ingest_split: no mix, selected channel s (the file's
// channel select[s]) becomes a waveform of its own at out + s * n_out.  Its input is that
// channel alone,
//   x_c[m] = sample(m, c) * 2^-(bits-1)      (integers: exact;  floats: float_sample, scale 1)
// zero outside [0, n), and from x_c[m] on the arithmetic is k_pcm_resample's: the same tap
// walk with fma in the same order, rint, clip, /32768.  pcm_frame of a one-channel file is
// sample * scale / 1.0, so by construction channel c here equals what k_pcm_resample computes
// for a mono file that holds only that channel (tests/test_gpu_channel_split.py pins it).
//
// A workgroup (blockIdx.x, blockIdx.y) owns `block` consecutive outputs of a group of up to
// `group` selected channels, select[blockIdx.y * group ...].  It stages the span of frames
// once: element i of the walk is (frame i / G, selected channel i % G), so with all channels
// selected neighbouring threads read neighbouring samples of the interleaved bytes, and a
// sparse selection reads only its own samples; every byte is read once per workgroup, not once
// per channel.  Each channel has a plane of span_cap doubles in LDS (plane g at g * span_cap),
// which keeps a thread's tap walk stride-1 as in k_pcm_resample; the taps lie behind the last
// plane in MODE 2.  Then the block x G outputs: a thread walks the taps of its phase once for
// up to 4 channels, one accumulator each (two launches with one channel each were measured
// faster than one launch that walked the taps per channel: DESIGN.md).  MODE 0 stages nothing:
// ratios whose span does not fit, and the no-filter case, which is a de-interleave and
// quantise.
struct SplitArgs {
  const void* pcm;
  int64_t n, n_out;
  int channels, up, down, half, block, span_cap, n_select, group;
  double scale;
  const double* taps;
  float* out;
  uint8_t select[256];  // channel ids (channels <= 256)
};

template <typename R>
__device__ inline double pcm_channel(const uint8_t* __restrict__ pcm, int64_t m, int64_t n, int channels, int c,
                                     double scale) {
  if (m < 0 || m >= n) return 0.0;
  return (double)R::at(pcm, m * channels + c) * scale;
}

// what the output phase of a workgroup needs for NG of its channels: their planes start at
// `planes` (span_cap doubles apart), their outputs at `out` (n_out apart)
struct SplitWalk {
  const uint8_t* __restrict__ pcm;
  int64_t n, n_out;
  int channels, up, down, half;
  double scale;
  const double* taps;      // global
  const double* taps_lds;  // MODE 2
  const double* planes;
  int span_cap;
  int64_t m_lo, k0, k1;
  int ch[4];  // the channels' ids
  float* out;
};

// outputs [k0, k1) of NG channels.  Per channel this is k_pcm_resample's walk: the same taps in
// the same order into an accumulator of its own
template <typename R, int MODE, int NG>
__device__ inline void split_outputs(const SplitWalk& w) {
  constexpr bool STAGED = MODE != 0;
  const int last_tap = 2 * w.half;
  for (int64_t k = w.k0 + threadIdx.x; k < w.k1; k += 256) {
    double y[NG];
    if (!w.taps) {
#pragma unroll
      for (int j = 0; j < NG; ++j) y[j] = pcm_channel<R>(w.pcm, k, w.n, w.channels, w.ch[j], w.scale);
    } else {
      const int64_t c = k * w.down + w.half;
      int64_t m = c / w.up;         // the newest frame that reaches output k
      int t = (int)(c - m * w.up);  // and its tap: the thread's phase
#pragma unroll
      for (int j = 0; j < NG; ++j) y[j] = 0.0;
      int i = (int)(m - w.m_lo);  // the frame's place in the planes
      for (; t <= last_tap; t += w.up, --m, --i) {
        const double tap = MODE == 2 ? w.taps_lds[t] : w.taps[t];
#pragma unroll
        for (int j = 0; j < NG; ++j) {
          const double x = STAGED ? w.planes[j * w.span_cap + i]
                                  : pcm_channel<R>(w.pcm, m, w.n, w.channels, w.ch[j], w.scale);
          y[j] = fma(x, tap, y[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      double r = rint(y[j] * 32768.0);  // round half to even, as np.round
      r = fmin(fmax(r, -32768.0), 32767.0);
      w.out[(int64_t)j * w.n_out + k] = (float)r * (1.0f / 32768.0f);
    }
  }
}

template <typename R, int MODE>
__global__ __launch_bounds__(256) void k_pcm_resample_split(SplitArgs a) {
  extern __shared__ __align__(16) double pcm_planes[];
  const uint8_t* __restrict__ pcm = (const uint8_t*)a.pcm;
  const int64_t k0 = (int64_t)blockIdx.x * a.block;
  const int64_t k1 = k0 + a.block < a.n_out ? k0 + a.block : a.n_out;
  const int s0 = blockIdx.y * a.group;
  const int G = a.n_select - s0 < a.group ? a.n_select - s0 : a.group;
  if (k0 >= k1 || G < 1) return;
  const int last_tap = 2 * a.half;
  int64_t m_lo = 0;
  constexpr bool STAGED = MODE != 0;
  const double* taps_lds = pcm_planes + (size_t)a.group * a.span_cap;
  if (STAGED) {
    const int64_t m_hi = ((k1 - 1) * a.down + a.half) / a.up;
    m_lo = (k0 * a.down + a.half) / a.up - last_tap / a.up;
    const int64_t len = m_hi - m_lo + 1;
    if (len > a.span_cap) return;  // cannot happen for the block the launcher chose
    const int total = (int)len * G;  // group * span_cap doubles fit the LDS budget
    for (int i = threadIdx.x; i < total; i += 256) {
      const int f = i / G, g = i - f * G;
      pcm_planes[g * a.span_cap + f] = pcm_channel<R>(pcm, m_lo + f, a.n, a.channels, a.select[s0 + g], a.scale);
    }
    if (MODE == 2)
      for (int i = threadIdx.x; i <= last_tap; i += 256) pcm_planes[(size_t)a.group * a.span_cap + i] = a.taps[i];
    __syncthreads();
  }
  // up to 4 channels share one tap walk: a tap is loaded once for all of them and their fma
  // chains are independent
  for (int g = 0; g < G; g += 4) {
    const int ng = G - g < 4 ? G - g : 4;
    SplitWalk w{pcm, a.n, a.n_out, a.channels, a.up, a.down, a.half, a.scale, a.taps, taps_lds,
                pcm_planes + g * a.span_cap, a.span_cap, m_lo, k0, k1, {0, 0, 0, 0},
                a.out + (int64_t)(s0 + g) * a.n_out};
#pragma unroll
    for (int j = 0; j < 4; ++j) w.ch[j] = j < ng ? a.select[s0 + g + j] : 0;
    if (ng == 1) split_outputs<R, MODE, 1>(w);
    else if (ng == 2) split_outputs<R, MODE, 2>(w);
    else if (ng == 3) split_outputs<R, MODE, 3>(w);
    else split_outputs<R, MODE, 4>(w);
  }
}

// block and group: the largest block (1024, 512, 256) at which the planes of all selected
// channels fit 20 KiB, one group then; failing that the largest at which they fit the 64 KiB of
// k_pcm_resample's launcher; if not even 256 does, block 256 and the fewest groups whose planes
// fit 64 KiB, of equal size (gridDim.y of them).  20 KiB first: a CU's 160 KiB then hold the 8
// workgroups its wave slots allow, and the tap walk is bound by latency: on 600 s of 44.1 kHz
// stereo, blocks of 256 (12 KiB of planes) ran in 0.62 ms, 512 (23 KiB) in 0.68 and 1024
// (46 KiB) in 0.85.  Where the planes are small anyway (8 kHz) the largest block
// stays the fastest.  The taps go behind the planes when they still fit 64 KiB.  No block at
// which one plane fits, or no filter: unstaged, block 1024 and up to 4 channels (one tap walk)
// per group.
void launch_pcm_resample_split(const void* pcm, int encoding, int64_t n_frames, int channels, int bits, int up,
                               int down, const double* taps, const int* select, int n_select, float* out,
                               int64_t n_out, hipStream_t st) {
  if (n_out < 1 || n_select < 1 || n_select > 256) return;
  SplitArgs a;
  a.pcm = pcm; a.n = n_frames; a.n_out = n_out; a.channels = channels; a.up = up; a.down = down;
  a.half = taps ? 10 * (up > down ? up : down) : 0;
  a.scale = ldexp(1.0, -(bits - 1));
  a.taps = taps; a.out = out; a.n_select = n_select;
  for (int s = 0; s < 256; ++s) a.select[s] = s < n_select ? (uint8_t)select[s] : 0;
  const int64_t budget = 65536 / 8;  // doubles
  a.block = 0;
  a.span_cap = 0;
  a.group = n_select < 4 ? n_select : 4;  // unstaged: the channels of one tap walk
  if (taps) {
    auto span_of = [&](int b) { return (int64_t)(b - 1) * down / up + 2 * a.half / up + 2; };
    for (const int64_t room : {(int64_t)20480 / 8, budget})
      for (int b = 1024; b >= 256 && !a.block; b /= 2)
        if (span_of(b) * n_select <= room) a.block = b, a.span_cap = (int)span_of(b), a.group = n_select;
    if (!a.block && span_of(256) <= budget) {
      const int fit = (int)(budget / span_of(256));
      const int groups = (n_select + fit - 1) / fit;
      a.block = 256, a.span_cap = (int)span_of(256), a.group = (n_select + groups - 1) / groups;
    }
  }
  const bool staged = a.block != 0;
  if (!staged) a.block = 1024;
  const size_t planes = (size_t)a.span_cap * a.group;
  const bool taps_in_lds = staged && (int64_t)(planes + 2 * a.half + 1) <= budget;
  const dim3 grid((unsigned)((n_out + a.block - 1) / a.block), (unsigned)((n_select + a.group - 1) / a.group));
  const size_t lds = (planes + (taps_in_lds ? 2 * a.half + 1 : 0)) * 8;
#define LAUNCH_SPLIT_AS(R_, MODE_) \
  k_pcm_resample_split<R_, MODE_><<<grid, 256, lds, st>>>(a), wh_launched("k_pcm_resample_split")
#define LAUNCH_SPLIT(MODE_)                                       \
  do {                                                            \
    switch (encoding) {                                           \
      case WH_WAV_U8: LAUNCH_SPLIT_AS(ReadU8, MODE_); break;     \
      case WH_WAV_S16: LAUNCH_SPLIT_AS(ReadS16, MODE_); break;   \
      case WH_WAV_S24: LAUNCH_SPLIT_AS(ReadS24, MODE_); break;   \
      case WH_WAV_S32: LAUNCH_SPLIT_AS(ReadS32, MODE_); break;   \
      case WH_WAV_F32: LAUNCH_SPLIT_AS(ReadF32, MODE_); break;   \
      case WH_WAV_F64: LAUNCH_SPLIT_AS(ReadF64, MODE_); break;   \
      case WH_WAV_ALAW: LAUNCH_SPLIT_AS(ReadAlaw, MODE_); break; \
      case WH_WAV_ULAW: LAUNCH_SPLIT_AS(ReadUlaw, MODE_); break; \
      default: break; /* the callers pass one of the eight */    \
    }                                                             \
  } while (0)
  if (taps_in_lds) LAUNCH_SPLIT(2);
  else if (staged) LAUNCH_SPLIT(1);
  else LAUNCH_SPLIT(0);
#undef LAUNCH_SPLIT
#undef LAUNCH_SPLIT_AS
}

}  // namespace wh
