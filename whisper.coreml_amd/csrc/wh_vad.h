// Speech-span detector of libwhisper_hip (wh_speech_spans): launch declarations of the two
// kernels in csrc/wh_vad.hip.  The definition they compute is in include/whisper_hip.h.
#pragma once
#include <cstdint>

#include "wh_common.h"

namespace wh {

constexpr int VAD_HOP = 160;   // samples per frame: the mel hop
constexpr int VAD_BINS = 160;  // histogram bins per file
constexpr int VAD_FB = 32;     // frames one workgroup of k_frame_energy owns

// one file of a call: its samples start at `off` of the resident audio, its energies at
// e_base, its workgroups of k_frame_energy at block_base, its run scratch (pairs of int) at
// run_base
struct VadFile {
  int64_t off, n, frames, e_base, block_base, run_base;
};
struct VadOpts {
  unsigned long long ratio_q8, t_lo, t_hi;
  int percentile, min_silence, min_speech, pad;
};
WH_DEV_HOST int64_t vad_blocks(int64_t frames) { return (frames + VAD_FB - 1) / VAD_FB; }
// pairs of run scratch a file needs: active runs before any rule, at most every other frame
WH_DEV_HOST int64_t vad_run_pairs(int64_t frames) { return frames / 2 + 1; }

// q^2 of one sample: q = clamp(rint(32768 x)), rint to even in fp32 (the product is exact);
// NaN counts as 0
__device__ inline unsigned vad_sq(float x) {
  if (x != x) return 0;  // before the clamp: fmaxf(NaN, a) is a
  float r = rintf(32768.0f * x);
  r = fminf(fmaxf(r, -32768.0f), 32767.0f);
  const int q = (int)r;
  return (unsigned)(q * q);  // at most 2^30
}
__device__ inline int vad_bin(unsigned long long e) {
  if (e == 0) return 0;
  const int m = 63 - __clzll((long long)e);
  const int sub = (int)((m >= 2 ? e >> (m - 2) : e << (2 - m)) & 3);
  return 1 + 4 * m + sub;
}
__device__ inline unsigned long long vad_edge(int bin) {
  if (bin < 1) return 0;
  const int m = (bin - 1) >> 2, sub = (bin - 1) & 3;
  return m >= 2 ? (unsigned long long)(4 + sub) << (m - 2) : (unsigned long long)(4 + sub) >> (2 - m);
}

// E[f] of every file (energy[e_base + f]) and the files' histograms (hist[file][VAD_BINS],
// zero before the launch).  One launch for all files.
void launch_frame_energy(const float* audio, const VadFile* files, int n_files, int64_t n_blocks,
                         unsigned long long* energy, unsigned* hist, hipStream_t st);
// threshold and spans of every file, one workgroup per file: thr[file] = T, counts[file] = the
// spans found, spans[file][cap][2] written only where counts[file] <= cap
void launch_speech_spans(const unsigned long long* energy, const unsigned* hist, const VadFile* files, int n_files,
                         const VadOpts& o, int* runs, int cap, unsigned long long* thr, int* counts, int* spans,
                         hipStream_t st);

}  // namespace wh
