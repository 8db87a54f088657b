// Speech-span kernels of libwhisper_hip (wh_speech_spans).  A translation unit of its own: the
// code object of wh_kernels.hip, whose kernels run in every decoder step, stays as it is.
// The definition (quantise, frame energy, quarter-octave histogram, threshold, run-length
// rules) is in include/whisper_hip.h; whisper/vad.py restates it in numpy.  Everything is
// integer arithmetic behind the quantisation, so the order of the sums does not matter.
#include "wh_vad.h"

namespace wh {

// ---------------------------------------------------------------- frame energy
// vad_sq, vad_bin and vad_edge (steps 1 and 3 of the definition) live in wh_vad.h: the streaming
// detector (wh_svad.hip) computes the same.

// A workgroup owns VAD_FB consecutive frames of one file: one contiguous span of samples.
// The span starts wherever the file's offset puts it, so it is read as 16-byte vectors from
// the aligned address below it; a vector that is not wholly inside the file's samples (the
// head, the end of the file) is read one guarded float at a time, and samples past n are
// zeros that are never read.  The squares go to LDS, a row of VAD_HOP per frame padded to
// VAD_ROW words so that the eight lanes that sum a frame and the eight frames of a wave hit
// 64 different banks; the sums are uint64.  The histogram is kept per workgroup in LDS and
// added to the file's counters with one integer atomic per non-empty bin: integer adds
// commute, the result does not depend on the order of the workgroups.
constexpr int VAD_ROW = VAD_HOP + 8;

__global__ __launch_bounds__(256) void k_frame_energy(const float* __restrict__ audio,
                                                      const VadFile* __restrict__ files, int n_files,
                                                      unsigned long long* __restrict__ energy,
                                                      unsigned* __restrict__ hist) {
  __shared__ unsigned sq[VAD_FB * VAD_ROW];
  __shared__ unsigned bins[VAD_BINS];
  const int64_t b = blockIdx.x;
  int lo = 0, hi = n_files - 1;  // the last file whose first workgroup is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (files[mid].block_base <= b) lo = mid;
    else hi = mid - 1;
  }
  const VadFile f = files[lo];
  const int64_t f0 = (b - f.block_base) * VAD_FB;
  if (f0 >= f.frames) return;
  const int nf = f.frames - f0 < VAD_FB ? (int)(f.frames - f0) : VAD_FB;
  const int64_t s0 = f0 * VAD_HOP;  // the span's first sample in the file
  const int span = nf * VAD_HOP;
  const int valid = f.n - s0 < span ? (int)(f.n - s0) : span;  // samples of the span the file has
  const float* __restrict__ src = audio + f.off + s0;
  const int head = (int)(((uintptr_t)src >> 2) & 3);  // floats between the 16-byte boundary and src
  const float4* __restrict__ v4 = (const float4*)(src - head);
  const int nvec = (head + span + 3) >> 2;
  for (int i = threadIdx.x; i < VAD_BINS; i += 256) bins[i] = 0;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const int p0 = 4 * v - head;  // the vector's first float, relative to the span
    float x[4];
    if (p0 >= 0 && p0 + 4 <= valid) {
      const float4 t = v4[v];
      x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = (p0 + j >= 0 && p0 + j < valid) ? src[p0 + j] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j;
      if (p >= 0 && p < span) sq[p + 8 * (p / VAD_HOP)] = vad_sq(x[j]);
    }
  }
  __syncthreads();
  // eight lanes per frame, lane `part` sums the squares part, part + 8, ...
  const int fr = threadIdx.x >> 3, part = threadIdx.x & 7;
  unsigned long long s = 0;
  if (fr < nf) {
    const unsigned* row = sq + fr * VAD_ROW + part;
#pragma unroll
    for (int i = 0; i < VAD_HOP / 8; ++i) s += row[8 * i];
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 4);
  if (fr < nf && part == 0) {
    energy[f.e_base + f0 + fr] = s;
    atomicAdd(&bins[vad_bin(s)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VAD_BINS; i += 256)
    if (bins[i]) atomicAdd(&hist[(int64_t)lo * VAD_BINS + i], bins[i]);
}

void launch_frame_energy(const float* audio, const VadFile* files, int n_files, int64_t n_blocks,
                         unsigned long long* energy, unsigned* hist, hipStream_t st) {
  if (n_blocks < 1) return;
  k_frame_energy<<<(unsigned)n_blocks, 256, 0, st>>>(audio, files, n_files, energy, hist), wh_launched("k_frame_energy");
}

// ---------------------------------------------------------------- threshold and spans
// One workgroup of VAD_T threads per file.  Both run-length stages are the same scan over a
// list of items in ascending order, some of them live, each live item an interval [lo, hi):
//   stage 1: items = frames, live = E[f] > T, interval [f, f + 1); a live frame starts a new
//            run when it lies at least max(1, min_silence) behind the end of the live frame
//            before it, otherwise the gap between them is closed;
//   stage 2: items = the runs of stage 1, live = at least min_speech long, interval = the run
//            with its pad, clamped to [0, F); a live run starts a new span when it lies at
//            least 1 behind the padded end of the live run before it (overlapping or
//            touching runs merge).
// A thread owns a contiguous chunk of the items.  One walk gives the chunk's summary: the lo
// of its first live item, the hi of its last, the starts inside it (which need only the
// chunk's own items).  The workgroup scans the summaries: a prefix maximum of hi, "the end
// of the last live item before my chunk", decides whether the chunk's first live item is a
// start, and a prefix sum of the starts gives every start its place in the output.  A second
// walk writes them: a start writes its own lo and, as the end of the run before it, the hi
// of the live item before it; the last run ends at the hi of the file's last live item.
// Looking back from the next live item finds what a suffix "next live item" scan would, so
// only prefixes are scanned.
constexpr int VAD_T = 1024;

// inclusive scan of s[VAD_T] in place, sum (MAX = false) or maximum
template <bool MAX>
__device__ inline void vad_scan(int* s) {
  const int t = threadIdx.x;
  for (int d = 1; d < VAD_T; d <<= 1) {
    const int v = t >= d ? s[t - d] : (MAX ? -1 : 0);
    __syncthreads();
    s[t] = MAX ? max(s[t], v) : s[t] + v;
    __syncthreads();
  }
}

struct VadFrames {  // stage 1
  const unsigned long long* e;
  unsigned long long thr;
  __device__ bool live(int64_t i, int& lo, int& hi) const {
    if (!(e[i] > thr)) return false;
    lo = (int)i;
    hi = (int)i + 1;
    return true;
  }
};
struct VadRuns {  // stage 2
  const int* runs;
  int min_speech, pad, frames;
  __device__ bool live(int64_t i, int& lo, int& hi) const {
    const int s = runs[2 * i], e = runs[2 * i + 1];
    if (e - s < min_speech) return false;
    lo = s - pad > 0 ? s - pad : 0;
    hi = e + pad < frames ? e + pad : frames;  // frames, pad < 2^30: no overflow
    return true;
  }
};

// the runs of `items` (n of them) with a new run wherever lo - (hi before) >= gap; out takes
// the pairs when there are at most cap of them.  Returns the count (the same in every thread).
template <typename Items>
__device__ int vad_runs(const Items& items, int64_t n, int gap, int* out, int64_t cap, int* s_hi, int* s_cnt) {
  const int t = threadIdx.x;
  const int64_t chunk = (n + VAD_T - 1) / VAD_T;
  const int64_t c0 = t * chunk < n ? t * chunk : n;
  const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
  int first_lo = -1, last_hi = -1, inner = 0, lo = 0, hi = 0;
  for (int64_t i = c0; i < c1; ++i)
    if (items.live(i, lo, hi)) {
      if (last_hi < 0) first_lo = lo;
      else if (lo - last_hi >= gap) ++inner;
      last_hi = hi;
    }
  __syncthreads();  // the arrays may still be read by the call before this one
  s_hi[t] = last_hi;
  __syncthreads();
  vad_scan<true>(s_hi);
  const int before = t ? s_hi[t - 1] : -1;  // the end of the last live item before the chunk
  const int mine = inner + ((first_lo >= 0 && (before < 0 || first_lo - before >= gap)) ? 1 : 0);
  s_cnt[t] = mine;
  __syncthreads();
  vad_scan<false>(s_cnt);
  const int total = s_cnt[VAD_T - 1];
  if (total > cap) return total;
  int k = s_cnt[t] - mine;
  int last = before;
  for (int64_t i = c0; i < c1; ++i)
    if (items.live(i, lo, hi)) {
      if (last < 0 || lo - last >= gap) {
        out[2 * (int64_t)k] = lo;
        if (k > 0) out[2 * (int64_t)k - 1] = last;
        ++k;
      }
      last = hi;
    }
  if (t == 0 && total > 0) out[2 * (int64_t)total - 1] = s_hi[VAD_T - 1];
  return total;
}

__global__ __launch_bounds__(VAD_T) void k_speech_spans(const unsigned long long* __restrict__ energy,
                                                        const unsigned* __restrict__ hist,
                                                        const VadFile* __restrict__ files, VadOpts o, int* runs,
                                                        int cap, unsigned long long* __restrict__ thr,
                                                        int* __restrict__ counts, int* spans) {
  __shared__ int s_hi[VAD_T], s_cnt[VAD_T];
  __shared__ unsigned long long s_thr;
  const int file = blockIdx.x;
  const VadFile f = files[file];
  if (threadIdx.x == 0) {
    // the noise level: the lower edge of the first bin whose cumulative count reaches the rank
    int64_t rank = (f.frames * o.percentile + 99) / 100;
    if (rank < 1) rank = 1;
    const unsigned* h = hist + (int64_t)file * VAD_BINS;
    int64_t cum = 0;
    int bin = 0;
    for (; bin < VAD_BINS - 1; ++bin) {
      cum += h[bin];
      if (cum >= rank) break;
    }
    unsigned long long t = (vad_edge(bin) * o.ratio_q8) >> 8;
    t = t < o.t_lo ? o.t_lo : t;
    t = t > o.t_hi ? o.t_hi : t;
    s_thr = t;
    thr[file] = t;
  }
  __syncthreads();
  int* my_runs = runs + 2 * f.run_base;
  const VadFrames frames{energy + f.e_base, s_thr};
  const int n_runs = vad_runs(frames, f.frames, o.min_silence > 1 ? o.min_silence : 1, my_runs, vad_run_pairs(f.frames),
                              s_hi, s_cnt);
  // the runs went through global memory: the workgroup's other threads read them next
  __threadfence_block();
  __syncthreads();
  const VadRuns closed{my_runs, o.min_speech, o.pad, (int)f.frames};
  const int n_spans = vad_runs(closed, n_runs, 1, spans + 2 * (int64_t)file * cap, cap, s_hi, s_cnt);
  if (threadIdx.x == 0) counts[file] = n_spans;
}

void launch_speech_spans(const unsigned long long* energy, const unsigned* hist, const VadFile* files, int n_files,
                         const VadOpts& o, int* runs, int cap, unsigned long long* thr, int* counts, int* spans,
                         hipStream_t st) {
  if (n_files < 1) return;
  k_speech_spans<<<n_files, VAD_T, 0, st>>>(energy, hist, files, o, runs, cap, thr, counts, spans),
      wh_launched("k_speech_spans");
}

}  // namespace wh
