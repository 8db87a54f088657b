// The audio front end of a context: resident waveforms (upload, PCM ingest, FLAC decoded on
// the device) and the log-mel spectrogram the encoder reads.  None of it depends on the
// model's element type, so it is a plain struct compiled once (csrc/wh_audio.hip); the
// context lends it its stream and its stage counters and reads the mel through mel().
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "wh_flacdev.h"
#include "wh_host.h"
#include "wh_kernels.h"
#include "wh_svad.h"
#include "wh_vad.h"
#include "whisper_hip.h"

// the stored log-mel as the encoder reads it: rows of `frames` floats, one per mel bin
struct MelView {
  const float* p;
  int64_t frames, f0;  // f0: the absolute index of the first stored frame
  int n_mels;
};

struct AudioFront {
  int init(hipStream_t stream, double* counters);
  // every buffer, map entry and event, each release checked
  void release(Releases& rel);
  MelView mel() const { return MelView{d_mel.p, mel_frames, mel_f0, mel_nm}; }

  int set_mel_filters(int n_mels, const float* filters);
  int audio_upload(const float* audio, int64_t n);
  int audio_ingest(const void* pcm, int format, int64_t n, int channels, int bits, int up, int down,
                   const double* taps, int n_taps, int64_t dst, int64_t reserve, int64_t* n_out);
  int audio_read(float* out, int64_t offset, int64_t n);
  int flac_decode_device(const uint8_t* data, int64_t n, int32_t* out, int64_t cap, int64_t* n_frames, int* path);
  int flac_ingest(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps, int64_t dst,
                  int64_t reserve, int64_t* n_out, int* path);
  int wav_ingest(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps, int64_t dst,
                 int64_t reserve, int64_t* n_out);
  // the same three with the channels kept apart: n_select segments, one per select[s]
  int audio_ingest_split(const void* pcm, int format, int64_t n, int channels, int bits, int up, int down,
                         const double* taps, int n_taps, const int* select, int n_select, int64_t dst,
                         int64_t reserve, int64_t* n_out);
  int flac_ingest_split(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                        const int* select, int n_select, int64_t dst, int64_t reserve, int64_t* n_out, int* path);
  int wav_ingest_split(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                       const int* select, int n_select, int64_t dst, int64_t reserve, int64_t* n_out);
  // a recording that arrives in chunks: one growing resident segment (include/whisper_hip.h)
  int stream_begin(int encoding, int channels, int up, int down, const double* taps, int n_taps, int64_t reserve);
  int stream_append(const void* data, int64_t n_frames, int64_t* n_out);
  int stream_finish(int64_t* n_out);
  int stream_trim(int64_t n_drop);
  int stream_info(int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished);
  // the causal speech detector of a live stream (include/whisper_hip.h), updated by the appends
  int stream_vad_enable(const wh_svad_opts* o);
  int stream_vad_state(wh_svad_state* out);
  int pool_vad_enable(int slot, const wh_svad_opts* o);
  int pool_vad_state(int n, const int* slots, wh_svad_state* out);
  int pool_vad_read(int slot, uint8_t* ring, int cap, uint32_t* hist);
  // many live streams at once: slots with buffers of their own (include/whisper_hip.h)
  int pool_create(int n_slots, int64_t slot_samples);
  int pool_destroy();
  int pool_open(int slot, int encoding, int channels, int up, int down, const double* taps, int n_taps);
  int pool_close(int slot);
  int pool_append(int n, const int* slots, const void* const* data, const int64_t* n_frames, int64_t* n_out);
  int pool_finish(int n, const int* slots, int64_t* n_out);
  int pool_trim(int n, const int* slots, const int64_t* n_drop);
  int pool_info(int slot, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished);
  int pool_read(int slot, float* out, int64_t offset, int64_t n);
  int pool_log_mel(int n, const int* slots, int64_t pad, int n_mels, int64_t* frame_base);
  // audio == nullptr: use the resident buffer of wh_audio_upload (n must match)
  int log_mel(const float* audio, int64_t n, int64_t pad, int n_mels, int normalize, int64_t* nf) {
    return log_mel_frames(audio, n, pad, n_mels, 0, -1, normalize, nf);
  }
  int log_mel_frames(const float* audio, int64_t n, int64_t pad, int n_mels, int64_t frame0, int64_t count,
                     int normalize, int64_t* total_frames);
  int log_mel_batch(const float* audio, int n_files, const int64_t* n_samples, int64_t pad, int n_mels,
                    int64_t* frame_base);
  int mel_max(float* g);
  int mel_max_batch(float* g, int n_files);
  int mel_normalize(float g);
  int mel_read(float* out, int64_t f0, int64_t nf);
  int mel_write(const float* mel, int64_t nf, int n_mels);
  // speech spans of the first n_files resident segments (include/whisper_hip.h)
  int speech_spans(const wh_vad_opts* o, int n_files, int32_t* spans, int cap, int32_t* n_spans,
                   uint64_t* thresholds);
  int frame_energy_read(int file, uint64_t* energy_out, int64_t cap, uint32_t* hist_out);

 private:
  hipStream_t st = nullptr;  // the context's
  double* stats = nullptr;   // the context's stage counters (WH_STAT_*)
  Timer tm;

  DevBuf<float> d_audio;
  int64_t audio_n = 0;
  // resident audio: segments (offset, length) lying back to back in d_audio from sample 0
  // (wh_audio_ingest appends; an upload leaves one; a host wh_log_mel_batch leaves none)
  std::vector<std::pair<int64_t, int64_t>> audio_segs;
  DevBuf<char> d_pcm;  // wh_audio_ingest / wh_wav_ingest: the file's PCM as uploaded
  std::map<std::pair<int, int>, double*> d_taps;  // resampling filters by (up, down)
  // wh_flac_ingest / wh_flac_decode_device: the stream, its candidates, their subframe records,
  // frame ends and staging slots, the chain and its first samples (the restore's flag behind them)
  DevBuf<uint8_t> fl_bytes;
  DevBuf<whflac::Cand> fl_cands;
  DevBuf<whflac::Sub> fl_subs;
  DevBuf<int64_t> fl_ends;
  DevBuf<int32_t> fl_stage;
  DevBuf<int32_t> fl_chain;
  DevBuf<int64_t> fl_starts;

  // wh_stream_*: the open stream.  The resident segment is (0, samples_out - dropped); the
  // history of the last `hist` mixed-down frames lies in half `cur` of d_hist ([2][hist]
  // doubles), the next append writes the other half.  ended_by: the call that closed it
  // A stream's speech detector: the options it was enabled with, the host copy of its state as
  // of the last append or finish, and its state block on the device (kept across begin / open)
  struct Svad {
    bool on = false;
    wh_svad_opts o{};
    wh_svad_state host{};
    DevBuf<char> block;
  };
  struct Stream {
    bool open = false, finished = false;
    int encoding = 0, channels = 0, bits = 0, frame_bytes = 0, up = 1, down = 1, hist = 0, cur = 0;
    const double* taps = nullptr;  // the device filter of (up, down), null when up == down
    int64_t frames_in = 0, samples_out = 0, dropped = 0;
    std::string ended_by;
    Svad vad;
  } stream;
  DevBuf<double> d_hist;
  DevBuf<float> d_bounce;  // wh_stream_trim, when the move overlaps itself

  // wh_pool_*: n_slots streams, none of whose state is shared with the single stream or the
  // resident segments.  Slot s owns floats [s][2][slot_samples] of pool_audio: its resident
  // samples are the first samples_out - dropped of buffer `buf`, a trim copies the remainder
  // into the other buffer and flips `buf`.  Its history is a double buffer of its own, as the
  // single stream's.  A batched call gathers its packets in pool_stage (pinned; every packet
  // 16-byte aligned with 8 readable bytes behind it) and its descriptors in pool_hdesc (pinned):
  // one copy each to pool_pcm and pool_desc, one launch, one synchronisation.
  struct PoolSlot : Stream {
    int buf = 0;
    DevBuf<double> hist_buf;  // [2][hist], kept across close / open
  };
  std::vector<PoolSlot> pool;
  int64_t pool_samples = 0;  // slot_samples
  DevBuf<float> pool_audio;
  DevBuf<char> pool_pcm, pool_desc;
  char* pool_stage = nullptr;
  char* pool_hdesc = nullptr;
  size_t pool_stage_cap = 0, pool_hdesc_cap = 0;
  // what the detectors of one call share: the frame energies between the kernel's two phases,
  // the states the launch leaves (device) and their pinned host copy
  DevBuf<unsigned long long> svad_energy;
  DevBuf<wh_svad_state> svad_out;
  char* svad_hout = nullptr;
  size_t svad_hout_cap = 0;
  int svad_enable(const std::string& who, Svad& v, const wh_svad_opts* o);
  int svad_room(int n, int64_t frames);
  float* pool_base(int slot, int buf) { return pool_audio.p + ((size_t)slot * 2 + buf) * pool_samples; }
  void pool_release(Releases& rel);
  int pool_slots(const std::string& who, int n, const int* slots, bool for_input);
  int pool_pinned(char** p, size_t* cap, size_t bytes);
  int pool_run(int n, const int* slots, const void* const* data, const int64_t* n_frames, const int64_t* totals,
               int64_t* n_out, const char* where);

  DevBuf<float> d_mel;
  int64_t mel_frames = 0;
  int64_t mel_f0 = 0;  // absolute index of the first stored frame
  int mel_nm = 0;
  DevBuf<unsigned> gmax;  // the mel's ordered-uint maximum; mel_normalize's override at [4]
  // wh_log_mel_batch: per-file descriptors and per-file ordered-uint maxima
  DevBuf<wh::MelFile> mel_files;
  DevBuf<unsigned> gmax_files;
  int mel_batch_files = 0;  // files of the last wh_log_mel_batch (0: the mel is not from one)
  std::map<int, float*> d_filters;
  std::map<int, std::vector<float>> h_filters;

  // wh_speech_spans: the files' descriptors, frame energies and histograms, the run scratch
  // between the two rules, and what goes back to the host (thresholds, counts, spans)
  DevBuf<wh::VadFile> vad_files;
  DevBuf<unsigned long long> vad_energy;
  DevBuf<unsigned> vad_hist;
  DevBuf<int> vad_runs;
  DevBuf<char> vad_out;

  void one_segment(int64_t n);
  void stream_ends(const char* by);
  int stream_open(const std::string& who, bool for_input);
  int stream_run(const void* data, int64_t nc, int64_t total, int64_t* n_out, bool finish);
  int filter_taps(const std::string& who, int up, int down, const double* taps, int n_taps, double** dt);
  int vad_plan(const char* who, int n_files, std::vector<wh::VadFile>* files, int64_t* blocks);
  int vad_energy_launch(const std::vector<wh::VadFile>& files, int64_t blocks);
  int audio_room(size_t samples);
  void mel_is(int64_t frames, int64_t f0, int n_mels, int batch_files);
  int ingest_check(const std::string& who, int format, int64_t n, int channels, int bits, int up, int down,
                   const double* taps, int n_taps, int64_t dst, int64_t reserve, int64_t* n_out);
  int ingest_run(const std::string& who, const void* pcm, int format, int64_t n, int channels, int bits, int up,
                 int down, const double* taps, int n_taps, int64_t dst, int64_t reserve, int64_t* n_out,
                 int wav_encoding = -1, int frame_bytes = 0, const int* select = nullptr, int n_select = 0);
  int select_check(const std::string& who, int format, int channels, const int* select, int n_select);
  int flac_device(const uint8_t* data, int64_t n, const whflac::Plan& plan, bool s32, bool* ran);
  int flac_plan_timed(const uint8_t* data, int64_t n, whflac::Plan* plan);
};
