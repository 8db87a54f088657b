// The causal speech detector of a live stream (wh_pool_vad_* / wh_stream_vad_*): descriptors and
// launch declarations of the kernel in csrc/wh_svad.hip.  The definition it computes is in
// include/whisper_hip.h ("Voice activity of a live stream"); whisper/vad.py (StreamVad) restates
// it in numpy.
#pragma once
#include <cstddef>
#include <cstdint>

#include "wh_vad.h"
#include "whisper_hip.h"

namespace wh {

constexpr int SVAD_MAX_WINDOW = 6000;
constexpr int SVAD_MAX_RUN = 1 << 20;

// A detector's state block in device memory: the scalars, the options it was enabled with,
// hist[VAD_BINS] and, behind the struct, ring[window] bytes.
struct SvadBlock {
  wh_svad_state s;
  wh_svad_opts o;
  unsigned hist[VAD_BINS];
};
inline size_t svad_block_bytes(int window) { return sizeof(SvadBlock) + (((size_t)window + 15) & ~(size_t)15); }

// One detecting slot of a call.  src: the n_new samples the call's ingest appended to the slot's
// resident buffer (any 4-byte alignment).  energy: scratch for svad_frames(fill, n_new) values,
// fill = the samples of the incomplete frame the detector already holds (state.samples % 160).
// finish: close an incomplete last frame with zeros.  The state after the call also goes to
// out[out_index] of the launch.
struct SvadDesc {
  const float* src;
  int64_t n_new;
  unsigned long long* energy;
  SvadBlock* block;
  int finish, out_index;
};
// frames of the call's frame grid that the new samples touch: the scratch the call needs
WH_DEV_HOST int64_t svad_frames(int fill, int64_t n_new) { return (fill + n_new + VAD_HOP - 1) / VAD_HOP; }

// One workgroup per descriptor: the energies in parallel, the recurrence on one wave.
void launch_stream_vad_pool(const SvadDesc* descs, int n, wh_svad_state* out, hipStream_t st);
// the same for one descriptor passed by value (the single stream has no descriptor copy)
void launch_stream_vad_one(const SvadDesc& desc, wh_svad_state* out, hipStream_t st);

}  // namespace wh
