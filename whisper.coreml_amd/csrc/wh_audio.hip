// The audio front end of a context (csrc/wh_audio.h): host code only, every kernel it
// launches lives in wh_kernels.hip, wh_ingest.hip, wh_flacdev.hip or wh_vad.hip.
#include "wh_audio.h"

#include <algorithm>
#include <chrono>
#include <cstring>

#include "wh_select.h"
#include "whisper_hip.h"

using namespace wh;

// host wall ms since t0, added to a stage counter
static void charge_host(double& counter, std::chrono::steady_clock::time_point t0) {
  counter += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int AudioFront::init(hipStream_t stream, double* counters) {
  st = stream;
  stats = counters;
  TRY(tm.create());
  return gmax.reserve(64);
}

void AudioFront::release(Releases& rel) {
  d_audio.release(rel, "hipFree(audio)");
  d_pcm.release(rel, "hipFree(pcm)");
  d_hist.release(rel, "hipFree(stream history)");
  d_bounce.release(rel, "hipFree(stream bounce)");
  stream.vad.block.release(rel, "hipFree(stream detector)");
  stream.vad.on = false;
  pool_release(rel);
  svad_energy.release(rel, "hipFree(detector energies)");
  svad_out.release(rel, "hipFree(detector states)");
  if (svad_hout) rel(hipHostFree(std::exchange(svad_hout, nullptr)), "hipHostFree(detector states)");
  svad_hout_cap = 0;
  auto flac = [&](auto&... b) { (b.release(rel, "hipFree(flac)"), ...); };
  flac(fl_bytes, fl_cands, fl_subs, fl_ends, fl_stage, fl_chain, fl_starts);
  for (auto& kv : d_taps) rel(hipFree(kv.second), "hipFree(resampling taps)");
  d_mel.release(rel, "hipFree(mel)");
  for (auto& kv : d_filters) rel(hipFree(kv.second), "hipFree(mel filters)");
  gmax.release(rel, "hipFree(mel max)");
  mel_files.release(rel, "hipFree(mel files)");
  gmax_files.release(rel, "hipFree(mel file max)");
  vad_files.release(rel, "hipFree(vad files)");
  vad_energy.release(rel, "hipFree(vad energy)");
  vad_hist.release(rel, "hipFree(vad histograms)");
  vad_runs.release(rel, "hipFree(vad runs)");
  vad_out.release(rel, "hipFree(vad spans)");
  tm.release(rel);
}

int AudioFront::set_mel_filters(int n_mels, const float* filters) {
  std::vector<float> f(filters, filters + (size_t)n_mels * 201);
  float* d = nullptr;
  if (d_filters.count(n_mels)) d = d_filters[n_mels];
  else {
    HIPCHK(hipMalloc(&d, f.size() * 4));
    d_filters[n_mels] = d;
  }
  HIPCHK(hipMemcpy(d, f.data(), f.size() * 4, hipMemcpyHostToDevice));
  h_filters[n_mels] = f;
  return 0;
}

// ------------------------------------------------------------ resident audio
int AudioFront::audio_room(size_t samples) { return d_audio.reserve(std::max<size_t>(samples, 16000) * 4); }

int AudioFront::audio_upload(const float* audio, int64_t n) {
  stream_ends("audio_upload");
  TRY(audio_room((size_t)n));
  HIPCHK(hipMemcpyAsync(d_audio.p, audio, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  one_segment(n);
  return 0;
}
void AudioFront::one_segment(int64_t n) {
  audio_segs.assign(1, std::make_pair((int64_t)0, n));
  audio_n = n;
}
// PCM of one file -> mono float32 at 16 kHz, appended to the resident segments at dst
// (include/whisper_hip.h).  Everything is checked before the first HIP call.
int AudioFront::audio_ingest(const void* pcm, int format, int64_t n, int channels, int bits, int up, int down,
                             const double* taps, int n_taps, int64_t dst, int64_t reserve, int64_t* n_out) {
  const std::string who = "audio_ingest: ";
  if (!pcm) return fail(-1, who + "null pcm");
  TRY(ingest_check(who, format, n, channels, bits, up, down, taps, n_taps, dst, reserve, n_out));
  return ingest_run(who, pcm, format, n, channels, bits, up, down, taps, n_taps, dst, reserve, n_out);
}
// what wh_audio_ingest refuses, before any HIP call
int AudioFront::ingest_check(const std::string& who, int format, int64_t n, int channels, int bits, int up, int down,
                             const double* taps, int n_taps, int64_t dst, int64_t reserve, int64_t* n_out) {
  if (!n_out) return fail(-1, who + "null n_out");
  if (format != WH_PCM_S16 && format != WH_PCM_S32 && format != WH_PCM_F32)
    return fail(-7, who + "unknown format " + std::to_string(format));
  if (n < 1 || n > ((int64_t)1 << 40)) return fail(-7, who + "n_frames = " + std::to_string(n) + " out of range");
  if (channels < 1 || channels > 256) return fail(-7, who + "channels = " + std::to_string(channels) + " out of range");
  if (up < 1 || down < 1 || up > (1 << 20) || down > (1 << 20))
    return fail(-7, who + "up = " + std::to_string(up) + ", down = " + std::to_string(down) + " out of range");
  const bool f32 = format == WH_PCM_F32;
  const bool filt = !f32 && up != down;
  if (f32) {
    if (channels != 1 || up != 1 || down != 1)
      return fail(-7, who + "format WH_PCM_F32 is a mono waveform at 16 kHz: channels, up and down must be 1");
  } else {
    if (bits < 1 || bits > 32 || (format == WH_PCM_S16 && bits > 16))
      return fail(-7, who + "bits = " + std::to_string(bits) + " out of range for the format");
    const int64_t want = 2 * 10 * (int64_t)std::max(up, down) + 1;
    if (filt && (!taps || n_taps != want))
      return fail(-7, who + "n_taps = " + std::to_string(taps ? n_taps : 0) + ", the filter of up = " +
                          std::to_string(up) + ", down = " + std::to_string(down) + " has " + std::to_string(want));
  }
  const int64_t end = audio_segs.empty() ? 0 : audio_segs.back().first + audio_segs.back().second;
  if (dst != 0 && dst != end)
    return fail(-7, who + "dst_offset = " + std::to_string(dst) + " is neither 0 nor the end of the resident segments (" +
                        std::to_string(end) + ")");
  if (reserve < 0) return fail(-7, who + "negative reserve");
  return 0;
}
// pcm: the host PCM to upload, or null when the device PCM buffer (d_pcm) already holds it
// (wh_flac_ingest's device path; its resampling time goes to WH_STAT_FLAC_RESAMPLE_MS).
// wav_encoding >= 0 (wh_wav_ingest): pcm is a WAV data chunk in that WH_WAV_* encoding,
// frame_bytes per frame; otherwise the encoding is the format's, int16 or int32.
// select (the _split forms, never WH_PCM_F32): the n_select channels go to segments of their
// own, back to back from dst, by one launch of the split kernel instead of the mixing one
int AudioFront::ingest_run(const std::string& who, const void* pcm, int format, int64_t n, int channels, int bits,
                           int up, int down, const double* taps, int n_taps, int64_t dst, int64_t reserve,
                           int64_t* n_out, int wav_encoding, int frame_bytes, const int* select, int n_select) {
  const bool f32 = format == WH_PCM_F32;
  const int n_seg = select ? n_select : 1;  // the split forms: one segment per selected channel
  const int encoding = wav_encoding >= 0 ? wav_encoding : format == WH_PCM_S32 ? WH_WAV_S32 : WH_WAV_S16;
  if (wav_encoding < 0) frame_bytes = channels * (format == WH_PCM_S32 ? 4 : 2);
  const bool filt = !f32 && up != down;
  const int64_t no = filt ? (n * up + down - 1) / down : n;
  double* dt = nullptr;
  if (filt) TRY(filter_taps(who, up, down, taps, n_taps, &dt));
  stream_ends(who.c_str());
  // room for the new end (or the caller's reserve); the segments before dst survive a move
  TRY(d_audio.reserve(std::max<size_t>(std::max(dst + n_seg * no, reserve), 16000) * 4, (size_t)dst * 4, st));
  if (f32) {
    TRY(tm.mark(0, st));
    HIPCHK(hipMemcpyAsync(d_audio.p + dst, pcm, (size_t)n * 4, hipMemcpyHostToDevice, st));
    TRY(tm.finish(st, stats[WH_STAT_INGEST_COPY_MS]));
  } else {
    const size_t bytes = (size_t)n * frame_bytes;
    if (pcm) TRY(d_pcm.reserve(bytes + 8));  // 24-bit samples are read as aligned dwords
    TRY(tm.mark(0, st));
    if (pcm) HIPCHK(hipMemcpyAsync(d_pcm.p, pcm, bytes, hipMemcpyHostToDevice, st));
    TRY(tm.mark(1, st));
    if (select) launch_pcm_resample_split(d_pcm.p, encoding, n, channels, bits, up, down, dt, select, n_select, d_audio.p + dst, no, st);
    else launch_pcm_resample(d_pcm.p, encoding, n, channels, bits, up, down, dt, d_audio.p + dst, no, st);
    TRY(tm.mark(2, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status("audio_ingest"));
    TRY(tm.charge(0, stats[WH_STAT_INGEST_COPY_MS]));
    TRY(tm.charge(1, stats[pcm ? WH_STAT_INGEST_KERNEL_MS : WH_STAT_FLAC_RESAMPLE_MS]));
  }
  if (dst == 0) audio_segs.clear();
  for (int s = 0; s < n_seg; ++s) audio_segs.emplace_back(dst + s * no, no);
  audio_n = audio_segs.size() == 1 ? no : -1;
  *n_out = no;
  return 0;
}

// the device copy of the filter of (up, down), uploaded the first time it is seen
int AudioFront::filter_taps(const std::string& who, int up, int down, const double* taps, int n_taps, double** dt) {
  const auto key = std::make_pair(up, down);
  auto it = d_taps.find(key);
  if (it != d_taps.end()) {
    *dt = it->second;
    return 0;
  }
  double* d = nullptr;
  HIPCHK(hipMalloc(&d, (size_t)n_taps * 8));
  if (hipMemcpy(d, taps, (size_t)n_taps * 8, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return fail(-100, who + "copying the filter taps failed");
  }
  d_taps[key] = d;
  *dt = d;
  return 0;
}

// ------------------------------------------------------------ a resident stream
// (include/whisper_hip.h).  Everything is checked before the first HIP call.
// E(n): the outputs that are final after n frames; the total when the recording has ended
static int64_t stream_emitted(int64_t n, int up, int down, bool final) {
  if (up == down) return n;
  if (final) return (n * up + down - 1) / down;
  const int64_t room = n * up - 10 * (int64_t)std::max(up, down);
  return room <= 0 ? 0 : (room + down - 1) / down;
}
extern "C" long long wh_stream_emitted(int64_t n_frames, int up, int down, int final) {
  if (n_frames < 0 || n_frames > ((int64_t)1 << 40) || up < 1 || down < 1 || up > (1 << 20) || down > (1 << 20)) return -1;
  return stream_emitted(n_frames, up, down, final != 0);
}
// another call took the resident buffer: the stream is over, and append says who ended it
void AudioFront::stream_ends(const char* by) {
  if (!stream.open) return;
  stream.open = false;
  stream.vad.on = false;
  stream.ended_by = by;
  while (!stream.ended_by.empty() && (stream.ended_by.back() == ' ' || stream.ended_by.back() == ':')) stream.ended_by.pop_back();
}
int AudioFront::stream_open(const std::string& who, bool for_input) {
  if (!stream.open)
    return fail(-7, who + "stream: no open stream" +
                        (stream.ended_by.empty() ? std::string() : " (ended by " + stream.ended_by + ")"));
  if (for_input && stream.finished) return fail(-7, who + "stream: already finished, no more input is taken");
  return 0;
}
// what wh_stream_begin and wh_pool_open refuse in a stream's format; `who` ends in "stream: " or "pool: "
static int stream_format_check(const std::string& who, int encoding, int channels, int up, int down,
                               const double* taps, int n_taps) {
  if (encoding < WH_WAV_U8 || encoding > WH_WAV_ULAW) return fail(-7, who + "unknown encoding " + std::to_string(encoding));
  if (channels < 1 || channels > 256) return fail(-7, who + "channels = " + std::to_string(channels) + " out of range");
  if (up < 1 || down < 1 || up > (1 << 20) || down > (1 << 20))
    return fail(-7, who + "up = " + std::to_string(up) + ", down = " + std::to_string(down) + " out of range");
  const int64_t want = 2 * 10 * (int64_t)std::max(up, down) + 1;
  if (up != down && (!taps || n_taps != want))
    return fail(-7, who + "n_taps = " + std::to_string(taps ? n_taps : 0) + ", the filter of up = " +
                        std::to_string(up) + ", down = " + std::to_string(down) + " has " + std::to_string(want));
  return 0;
}
//                                     U8 S16 S24 S32 F32 F64 ALAW ULAW
static const int stream_container[8] = {1, 2, 3, 4, 4, 8, 1, 1};
static const int stream_bits[8] = {8, 16, 24, 32, 1, 1, 16, 16};  // as in wav_ingest
int AudioFront::stream_begin(int encoding, int channels, int up, int down, const double* taps, int n_taps,
                             int64_t reserve) {
  const std::string who = "stream_begin: ";
  TRY(stream_format_check(who + "stream: ", encoding, channels, up, down, taps, n_taps));
  const int64_t half = 10 * (int64_t)std::max(up, down);
  if (reserve < 0) return fail(-7, who + "stream: negative reserve");
  double* dt = nullptr;
  if (up != down) TRY(filter_taps(who, up, down, taps, n_taps, &dt));
  const int hist = up != down ? (int)(2 * half / up) : 0;
  TRY(d_hist.reserve((size_t)std::max(hist, 1) * 16));
  TRY(d_audio.reserve(std::max<size_t>((size_t)reserve, 16000) * 4));
  // the frames before the recording are zeros
  HIPCHK(hipMemsetAsync(d_hist.p, 0, (size_t)std::max(hist, 1) * 16, st));
  HIPCHK(hipStreamSynchronize(st));
  const DevBuf<char> keep = stream.vad.block;
  stream = Stream();  // the detector goes with the stream it belonged to
  stream.vad.block = keep;
  stream.open = true;
  stream.encoding = encoding; stream.channels = channels; stream.bits = stream_bits[encoding];
  stream.frame_bytes = stream_container[encoding] * channels;
  stream.up = up; stream.down = down; stream.hist = hist; stream.taps = dt;
  one_segment(0);
  return 0;
}
// frames [frames_in, frames_in + nc) arrive (data), or the recording ends (nc = 0, total = all
// there will be): the outputs that become final are appended to the resident segment
int AudioFront::stream_run(const void* data, int64_t nc, int64_t total, int64_t* n_out, bool finish) {
  Stream& s = stream;
  const int64_t len = s.samples_out - s.dropped, emit = total - s.samples_out;
  // the detector takes the samples this call emits; a finish also closes its incomplete frame
  const int fill = s.vad.on ? (int)(s.vad.host.samples % VAD_HOP) : 0;
  const bool detect = s.vad.on && (emit > 0 || (finish && fill));
  if (detect) TRY(svad_room(1, svad_frames(fill, emit)));
  if (len + emit > (int64_t)(d_audio.cap / 4))  // grows by doubling: an append a second does not reallocate each time
    TRY(d_audio.reserve((size_t)std::max(len + emit, 2 * len) * 4, (size_t)len * 4, st));
  const size_t bytes = (size_t)nc * s.frame_bytes;
  TRY(d_pcm.reserve(bytes + 8));  // 24-bit samples are read as aligned dwords
  double* old_half = d_hist.p + (size_t)s.cur * s.hist;
  double* new_half = d_hist.p + (size_t)(1 - s.cur) * s.hist;
  TRY(tm.mark(0, st));
  if (nc) HIPCHK(hipMemcpyAsync(d_pcm.p, data, bytes, hipMemcpyHostToDevice, st));
  TRY(tm.mark(1, st));
  const bool ingest = nc > 0 || emit > 0;  // not so only for a finish that merely closes the detector's frame
  if (ingest)
    launch_pcm_resample_stream(d_pcm.p, s.encoding, s.frames_in, nc, s.channels, s.bits, s.up, s.down, s.taps, old_half,
                               new_half, s.hist, d_audio.p + len, s.samples_out, emit, st);
  if (detect)
    launch_stream_vad_one(SvadDesc{d_audio.p + len, emit, svad_energy.p, (SvadBlock*)s.vad.block.p, finish ? 1 : 0, 0},
                          svad_out.p, st);
  TRY(tm.mark(2, st));
  if (detect) HIPCHK(hipMemcpyAsync(svad_hout, svad_out.p, sizeof(wh_svad_state), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status("stream_append"));
  TRY(tm.charge(0, stats[WH_STAT_INGEST_COPY_MS]));
  TRY(tm.charge(1, stats[WH_STAT_INGEST_KERNEL_MS]));
  if (detect) memcpy(&s.vad.host, svad_hout, sizeof(wh_svad_state));
  if (s.hist && ingest) s.cur = 1 - s.cur;
  s.frames_in += nc;
  s.samples_out = total;
  one_segment(len + emit);
  if (n_out) *n_out = emit;
  return 0;
}
int AudioFront::stream_append(const void* data, int64_t n_frames, int64_t* n_out) {
  const std::string who = "stream_append: ";
  TRY(stream_open(who, true));
  if (n_frames < 0 || n_frames > ((int64_t)1 << 40) - stream.frames_in)
    return fail(-7, who + "stream: n_frames = " + std::to_string(n_frames) + " out of range");
  if (n_frames == 0) {
    if (n_out) *n_out = 0;
    return 0;
  }
  if (!data) return fail(-1, who + "stream: null data with n_frames > 0");
  return stream_run(data, n_frames, stream_emitted(stream.frames_in + n_frames, stream.up, stream.down, false), n_out,
                    false);
}
int AudioFront::stream_finish(int64_t* n_out) {
  const std::string who = "stream_finish: ";
  TRY(stream_open(who, false));
  if (!stream.finished) {
    const int64_t total = stream_emitted(stream.frames_in, stream.up, stream.down, true);
    const bool open_frame = stream.vad.on && stream.vad.host.samples % VAD_HOP != 0;
    if (total > stream.samples_out || open_frame) TRY(stream_run(nullptr, 0, total, n_out, true));
    else if (n_out) *n_out = 0;
    stream.finished = true;
    return 0;
  }
  if (n_out) *n_out = 0;
  return 0;
}
int AudioFront::stream_trim(int64_t n_drop) {
  const std::string who = "stream_trim: ";
  TRY(stream_open(who, false));
  const int64_t len = stream.samples_out - stream.dropped;
  if (n_drop < 0 || n_drop > len)
    return fail(-7, who + "stream: n_drop = " + std::to_string(n_drop) + " outside [0, " + std::to_string(len) + "]");
  const int64_t rest = len - n_drop;
  if (n_drop && rest) {
    const bool overlap = rest > n_drop;  // [n_drop, len) reaches into [0, rest)
    if (overlap) TRY(d_bounce.reserve((size_t)rest * 4));
    TRY(tm.mark(0, st));
    if (overlap) {
      HIPCHK(hipMemcpyAsync(d_bounce.p, d_audio.p + n_drop, (size_t)rest * 4, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(d_audio.p, d_bounce.p, (size_t)rest * 4, hipMemcpyDeviceToDevice, st));
    } else {
      HIPCHK(hipMemcpyAsync(d_audio.p, d_audio.p + n_drop, (size_t)rest * 4, hipMemcpyDeviceToDevice, st));
    }
    TRY(tm.finish(st, stats[WH_STAT_INGEST_COPY_MS]));
  }
  stream.dropped += n_drop;
  one_segment(rest);
  return 0;
}
int AudioFront::stream_info(int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished) {
  TRY(stream_open("stream_info: ", false));
  if (frames_in) *frames_in = stream.frames_in;
  if (samples_out) *samples_out = stream.samples_out;
  if (samples_dropped) *samples_dropped = stream.dropped;
  if (finished) *finished = stream.finished ? 1 : 0;
  return 0;
}

// ------------------------------------------------------------ the detector of a live stream
// (include/whisper_hip.h, "Voice activity of a live stream"): what the single stream and a pool
// slot share.  svad_check is host arithmetic only.
static int svad_check(const std::string& who, const wh_svad_opts* o) {
  if (!o) return fail(-1, who + "null opts");
  if (o->percentile < 1 || o->percentile > 99)
    return fail(-7, who + "percentile = " + std::to_string(o->percentile) + " outside 1..99");
  if (o->ratio_q8 < 256 || o->ratio_q8 > 2560000)
    return fail(-7, who + "ratio_q8 = " + std::to_string(o->ratio_q8) + " outside [256, 2560000]");
  if (o->t_lo > o->t_hi)
    return fail(-7, who + "t_lo = " + std::to_string(o->t_lo) + " above t_hi = " + std::to_string(o->t_hi));
  if (o->window < 1 || o->window > SVAD_MAX_WINDOW)
    return fail(-7, who + "window = " + std::to_string(o->window) + " outside 1.." + std::to_string(SVAD_MAX_WINDOW));
  if (o->min_silence < 1 || o->min_silence > SVAD_MAX_RUN)
    return fail(-7, who + "min_silence = " + std::to_string(o->min_silence) + " outside 1..2^20");
  if (o->min_speech < 0 || o->min_speech > SVAD_MAX_RUN)
    return fail(-7, who + "min_speech = " + std::to_string(o->min_speech) + " outside 0..2^20");
  return 0;
}
// the caller has checked everything: the state block, all zero behind the options
int AudioFront::svad_enable(const std::string& who, Svad& v, const wh_svad_opts* o) {
  const size_t bytes = svad_block_bytes(o->window);
  TRY(v.block.reserve(bytes));
  SvadBlock head{};
  head.o = *o;
  HIPCHK(hipMemsetAsync(v.block.p, 0, bytes, st));
  HIPCHK(hipMemcpyAsync(v.block.p, &head, offsetof(SvadBlock, hist), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  v.o = *o;
  v.host = wh_svad_state{};
  v.on = true;
  return 0;
}
// room for a call with n detecting slots and `frames` frame energies between them
int AudioFront::svad_room(int n, int64_t frames) {
  TRY(svad_energy.reserve((size_t)std::max<int64_t>(frames, 64) * 8));
  TRY(svad_out.reserve((size_t)std::max(n, 16) * sizeof(wh_svad_state)));
  const size_t bytes = (size_t)n * sizeof(wh_svad_state);
  return pool_pinned(&svad_hout, &svad_hout_cap, bytes > svad_hout_cap ? std::max(bytes, 2 * svad_hout_cap) : bytes);
}
int AudioFront::stream_vad_enable(const wh_svad_opts* o) {
  const std::string who = "stream_vad_enable: stream: ";
  TRY(svad_check(who, o));
  TRY(stream_open("stream_vad_enable: ", false));
  if (stream.frames_in || stream.finished) return fail(-7, who + "has already taken frames: enable the detector right after wh_stream_begin");
  if (stream.vad.on) return fail(-7, who + "is already detecting");
  return svad_enable(who, stream.vad, o);
}
int AudioFront::stream_vad_state(wh_svad_state* out) {
  const std::string who = "stream_vad_state: stream: ";
  if (!out) return fail(-1, who + "null out");
  TRY(stream_open("stream_vad_state: ", false));
  if (!stream.vad.on) return fail(-7, who + "has no detector (wh_stream_vad_enable)");
  *out = stream.vad.host;
  return 0;
}

// ------------------------------------------------------------ a pool of streams
// (include/whisper_hip.h).  A batched call is all or nothing: everything is checked before the
// first HIP call, and a refused call leaves every slot and every n_out[] entry as it was.
static std::string field_at(const char* field, int i) { return std::string(field) + "[" + std::to_string(i) + "]"; }

int AudioFront::pool_create(int n_slots, int64_t slot_samples) {
  const std::string who = "pool_create: pool: ";
  if (!pool.empty()) return fail(-7, who + "already created (" + std::to_string(pool.size()) + " slots)");
  if (n_slots < 1 || n_slots > 4096) return fail(-7, who + "n_slots = " + std::to_string(n_slots) + " outside 1..4096");
  if (slot_samples < 1 || slot_samples > 0x7fffffff)
    return fail(-7, who + "slot_samples = " + std::to_string(slot_samples) + " out of range");
  TRY(pool_audio.reserve((size_t)n_slots * 2 * (size_t)slot_samples * 4));
  pool.assign(n_slots, PoolSlot());
  pool_samples = slot_samples;
  return 0;
}
void AudioFront::pool_release(Releases& rel) {
  for (auto& s : pool) {
    s.hist_buf.release(rel, "hipFree(pool history)");
    s.vad.block.release(rel, "hipFree(pool detector)");
  }
  pool.clear();
  pool_samples = 0;
  pool_audio.release(rel, "hipFree(pool audio)");
  pool_pcm.release(rel, "hipFree(pool pcm)");
  pool_desc.release(rel, "hipFree(pool descriptors)");
  if (pool_stage) rel(hipHostFree(std::exchange(pool_stage, nullptr)), "hipHostFree(pool staging)");
  if (pool_hdesc) rel(hipHostFree(std::exchange(pool_hdesc, nullptr)), "hipHostFree(pool descriptors)");
  pool_stage_cap = pool_hdesc_cap = 0;
}
int AudioFront::pool_destroy() {
  if (pool.empty()) return fail(-7, "pool_destroy: pool: no pool");
  Releases rel;
  pool_release(rel);
  return rel.first.empty() ? 0 : fail(-100, "pool_destroy: " + rel.first);
}
int AudioFront::pool_open(int slot, int encoding, int channels, int up, int down, const double* taps, int n_taps) {
  const std::string who = "pool_open: pool: ";
  if (pool.empty()) return fail(-7, who + "no pool");
  if (slot < 0 || slot >= (int)pool.size())
    return fail(-7, who + "slot = " + std::to_string(slot) + " outside [0, " + std::to_string(pool.size()) + ")");
  if (pool[slot].open) return fail(-7, who + "slot " + std::to_string(slot) + " is already open");
  TRY(stream_format_check(who, encoding, channels, up, down, taps, n_taps));
  const int64_t half = 10 * (int64_t)std::max(up, down);
  double* dt = nullptr;
  if (up != down) TRY(filter_taps(who, up, down, taps, n_taps, &dt));
  const int hist = up != down ? (int)(2 * half / up) : 0;
  PoolSlot& s = pool[slot];
  TRY(s.hist_buf.reserve((size_t)std::max(hist, 1) * 16));
  // the frames before the recording are zeros
  HIPCHK(hipMemsetAsync(s.hist_buf.p, 0, (size_t)std::max(hist, 1) * 16, st));
  HIPCHK(hipStreamSynchronize(st));
  const DevBuf<double> keep = s.hist_buf;
  const DevBuf<char> keep_vad = s.vad.block;
  s = PoolSlot();
  s.hist_buf = keep;
  s.vad.block = keep_vad;
  s.open = true;
  s.encoding = encoding; s.channels = channels; s.bits = stream_bits[encoding];
  s.frame_bytes = stream_container[encoding] * channels;
  s.up = up; s.down = down; s.hist = hist; s.taps = dt;
  return 0;
}
int AudioFront::pool_close(int slot) {
  const int one[1] = {slot};
  TRY(pool_slots("pool_close: pool: ", 1, one, false));
  pool[slot].open = false;
  pool[slot].vad.on = false;
  return 0;
}
// the slots of a batched call: a pool, n >= 1, every slot in range, open (and still taking
// input) and named once
int AudioFront::pool_slots(const std::string& who, int n, const int* slots, bool for_input) {
  if (pool.empty()) return fail(-7, who + "no pool");
  if (n < 1) return fail(-7, who + "n = " + std::to_string(n) + ", need at least one slot");
  if (!slots) return fail(-1, who + "null slots");
  std::vector<char> seen(pool.size(), 0);
  for (int i = 0; i < n; ++i) {
    const int s = slots[i];
    if (s < 0 || s >= (int)pool.size())
      return fail(-7, who + field_at("slots", i) + " = " + std::to_string(s) + " outside [0, " + std::to_string(pool.size()) + ")");
    if (!pool[s].open) return fail(-7, who + field_at("slots", i) + " = " + std::to_string(s) + " is not open");
    if (seen[s]) return fail(-7, who + field_at("slots", i) + " = " + std::to_string(s) + " is twice in the call");
    seen[s] = 1;
    if (for_input && pool[s].finished)
      return fail(-7, who + field_at("slots", i) + " = " + std::to_string(s) + " is already finished, no more input is taken");
  }
  return 0;
}
// pinned host memory that grows by doubling
int AudioFront::pool_pinned(char** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  if (*p) HIPCHK(hipHostFree(std::exchange(*p, nullptr)));
  *cap = 0;
  const size_t want = std::max<size_t>(bytes, 4096);
  void* q = nullptr;
  HIPCHK(hipHostMalloc(&q, want, hipHostMallocDefault));
  *p = (char*)q;
  *cap = want;
  return 0;
}
// entry i: frames [frames_in, frames_in + n_frames[i]) of slot slots[i] arrive (data[i]), or its
// recording ends (data null, totals[i] = all there will be).  The caller has checked everything.
int AudioFront::pool_run(int n, const int* slots, const void* const* data, const int64_t* n_frames,
                         const int64_t* totals, int64_t* n_out, const char* where) {
  std::vector<size_t> offs(n, 0);
  size_t bytes = 0;
  int work = 0, vwork = 0;  // slots with samples to ingest; detecting slots with frames to take
  int64_t vframes = 0;
  // a detecting slot takes the samples the call emits for it; a finish also closes its incomplete frame
  auto detects = [&](const PoolSlot& s, int64_t emit) {
    return s.vad.on && (emit > 0 || (!data && !s.finished && s.vad.host.samples % VAD_HOP != 0));
  };
  for (int i = 0; i < n; ++i) {
    const PoolSlot& s = pool[slots[i]];
    const int64_t nc = data ? n_frames[i] : 0;
    if (detects(s, totals[i] - s.samples_out)) {
      ++vwork;
      vframes += svad_frames((int)(s.vad.host.samples % VAD_HOP), totals[i] - s.samples_out);
    }
    if (!nc && totals[i] == s.samples_out) continue;  // nothing arrives, nothing becomes final
    ++work;
    offs[i] = bytes;
    bytes += ((size_t)nc * s.frame_bytes + 8 + 15) & ~(size_t)15;  // 24-bit samples are read as aligned dwords
  }
  if (work || vwork) {
    // the detectors' descriptors lie behind the streams' in the one descriptor copy
    const size_t voff = ((size_t)work * pool_stream_bytes() + 15) & ~(size_t)15;
    const size_t dbytes = vwork ? voff + (size_t)vwork * sizeof(SvadDesc) : (size_t)work * pool_stream_bytes();
    TRY(pool_pinned(&pool_stage, &pool_stage_cap, bytes > pool_stage_cap ? std::max(bytes, 2 * pool_stage_cap) : bytes));
    TRY(pool_pinned(&pool_hdesc, &pool_hdesc_cap, dbytes));
    TRY(pool_pcm.reserve(std::max<size_t>(pool_stage_cap, 16)));
    TRY(pool_desc.reserve(pool_hdesc_cap));
    if (vwork) TRY(svad_room(vwork, vframes));
    SvadDesc* vd = (SvadDesc*)(pool_hdesc + voff);
    int64_t blocks = 0, e_base = 0;
    int j = 0, jv = 0;
    for (int i = 0; i < n; ++i) {
      const PoolSlot& s = pool[slots[i]];
      const int64_t nc = data ? n_frames[i] : 0;
      const int64_t len = s.samples_out - s.dropped, emit = totals[i] - s.samples_out;
      if (detects(s, emit)) {
        vd[jv] = SvadDesc{pool_base(slots[i], s.buf) + len, emit, svad_energy.p + e_base, (SvadBlock*)s.vad.block.p,
                          data ? 0 : 1, jv};
        e_base += svad_frames((int)(s.vad.host.samples % VAD_HOP), emit);
        ++jv;
      }
      if (!nc && totals[i] == s.samples_out) continue;
      if (nc) memcpy(pool_stage + offs[i], data[i], (size_t)nc * s.frame_bytes);
      blocks += pool_stream_fill(pool_hdesc, j++, blocks, pool_pcm.p + offs[i], s.encoding, s.frames_in, nc, s.channels,
                                 s.bits, s.up, s.down, s.taps, s.hist_buf.p + (size_t)s.cur * s.hist,
                                 s.hist_buf.p + (size_t)(1 - s.cur) * s.hist, s.hist,
                                 pool_base(slots[i], s.buf) + len, s.samples_out, emit);
    }
    TRY(tm.mark(0, st));
    if (data && work) HIPCHK(hipMemcpyAsync(pool_pcm.p, pool_stage, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(pool_desc.p, pool_hdesc, dbytes, hipMemcpyHostToDevice, st));
    TRY(tm.mark(1, st));
    if (work) launch_pcm_resample_pool(pool_desc.p, work, blocks, st);
    if (vwork) launch_stream_vad_pool((const SvadDesc*)(pool_desc.p + voff), vwork, svad_out.p, st);
    TRY(tm.mark(2, st));
    if (vwork)
      HIPCHK(hipMemcpyAsync(svad_hout, svad_out.p, (size_t)vwork * sizeof(wh_svad_state), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(where));
    TRY(tm.charge(0, stats[WH_STAT_INGEST_COPY_MS]));
    TRY(tm.charge(1, stats[WH_STAT_INGEST_KERNEL_MS]));
  }
  for (int i = 0, jv = 0; i < n; ++i) {
    PoolSlot& s = pool[slots[i]];
    const int64_t nc = data ? n_frames[i] : 0;
    if (n_out) n_out[i] = totals[i] - s.samples_out;
    if (detects(s, totals[i] - s.samples_out)) memcpy(&s.vad.host, svad_hout + (size_t)jv++ * sizeof(wh_svad_state), sizeof(wh_svad_state));
    if (!nc && totals[i] == s.samples_out) continue;
    if (s.hist) s.cur = 1 - s.cur;
    s.frames_in += nc;
    s.samples_out = totals[i];
  }
  return 0;
}
int AudioFront::pool_append(int n, const int* slots, const void* const* data, const int64_t* n_frames, int64_t* n_out) {
  const std::string who = "pool_append: pool: ";
  TRY(pool_slots(who, n, slots, true));
  if (!data) return fail(-1, who + "null data");
  if (!n_frames) return fail(-1, who + "null n_frames");
  std::vector<int64_t> totals(n);
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    const PoolSlot& s = pool[slots[i]];
    const int64_t nc = n_frames[i];
    if (nc < 0 || nc > ((int64_t)1 << 40) - s.frames_in)
      return fail(-7, who + field_at("n_frames", i) + " = " + std::to_string(nc) + " out of range");
    if (nc > 0 && !data[i]) return fail(-1, who + "null " + field_at("data", i) + " with n_frames > 0");
    totals[i] = stream_emitted(s.frames_in + nc, s.up, s.down, false);
    const int64_t after = totals[i] - s.dropped;
    if (after > pool_samples)
      return fail(-7, who + field_at("n_frames", i) + " = " + std::to_string(nc) + " takes slot " + std::to_string(slots[i]) +
                          " to " + std::to_string(after) + " resident samples, past its capacity of " +
                          std::to_string(pool_samples) + ": the caller must trim first");
    blocks += (totals[i] - s.samples_out + 255) / 256 + 1;
  }
  if (blocks > 0x7fffffff) return fail(-7, who + "too many samples for one call");
  return pool_run(n, slots, data, n_frames, totals.data(), n_out, "pool_append");
}
int AudioFront::pool_finish(int n, const int* slots, int64_t* n_out) {
  const std::string who = "pool_finish: pool: ";
  TRY(pool_slots(who, n, slots, false));
  std::vector<int64_t> totals(n);
  for (int i = 0; i < n; ++i) {
    const PoolSlot& s = pool[slots[i]];
    totals[i] = s.finished ? s.samples_out : stream_emitted(s.frames_in, s.up, s.down, true);
    if (totals[i] - s.dropped > pool_samples)
      return fail(-7, who + field_at("slots", i) + " = " + std::to_string(slots[i]) + " would hold " +
                          std::to_string(totals[i] - s.dropped) + " resident samples, past its capacity of " +
                          std::to_string(pool_samples) + ": the caller must trim first");
  }
  TRY(pool_run(n, slots, nullptr, nullptr, totals.data(), n_out, "pool_finish"));
  for (int i = 0; i < n; ++i) pool[slots[i]].finished = true;
  return 0;
}
int AudioFront::pool_trim(int n, const int* slots, const int64_t* n_drop) {
  const std::string who = "pool_trim: pool: ";
  TRY(pool_slots(who, n, slots, false));
  if (!n_drop) return fail(-1, who + "null n_drop");
  int moves = 0;
  int64_t longest = 0;
  for (int i = 0; i < n; ++i) {
    const PoolSlot& s = pool[slots[i]];
    const int64_t len = s.samples_out - s.dropped;
    if (n_drop[i] < 0 || n_drop[i] > len)
      return fail(-7, who + field_at("n_drop", i) + " = " + std::to_string(n_drop[i]) + " outside [0, " + std::to_string(len) + "]");
    if (n_drop[i] && len - n_drop[i]) ++moves, longest = std::max(longest, len - n_drop[i]);
  }
  if (moves) {
    const size_t dbytes = (size_t)moves * sizeof(PoolMove);
    TRY(pool_pinned(&pool_hdesc, &pool_hdesc_cap, dbytes));
    TRY(pool_desc.reserve(pool_hdesc_cap));
    PoolMove* mv = (PoolMove*)pool_hdesc;
    for (int i = 0, j = 0; i < n; ++i) {
      const PoolSlot& s = pool[slots[i]];
      const int64_t rest = s.samples_out - s.dropped - n_drop[i];
      if (n_drop[i] && rest) mv[j++] = PoolMove{pool_base(slots[i], s.buf) + n_drop[i], pool_base(slots[i], 1 - s.buf), rest};
    }
    TRY(tm.mark(0, st));
    HIPCHK(hipMemcpyAsync(pool_desc.p, pool_hdesc, dbytes, hipMemcpyHostToDevice, st));
    TRY(tm.mark(1, st));
    launch_pool_move((const PoolMove*)pool_desc.p, moves, longest, st);
    TRY(tm.mark(2, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status("pool_trim"));
    TRY(tm.charge(0, stats[WH_STAT_INGEST_COPY_MS]));
    TRY(tm.charge(1, stats[WH_STAT_INGEST_KERNEL_MS]));
  }
  for (int i = 0; i < n; ++i) {
    PoolSlot& s = pool[slots[i]];
    if (n_drop[i] && s.samples_out - s.dropped - n_drop[i]) s.buf = 1 - s.buf;
    s.dropped += n_drop[i];
  }
  return 0;
}
int AudioFront::pool_info(int slot, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished) {
  const int one[1] = {slot};
  TRY(pool_slots("pool_info: pool: ", 1, one, false));
  const PoolSlot& s = pool[slot];
  if (frames_in) *frames_in = s.frames_in;
  if (samples_out) *samples_out = s.samples_out;
  if (samples_dropped) *samples_dropped = s.dropped;
  if (finished) *finished = s.finished ? 1 : 0;
  return 0;
}
int AudioFront::pool_vad_enable(int slot, const wh_svad_opts* o) {
  const std::string who = "pool_vad_enable: pool: ";
  TRY(svad_check(who, o));
  const int one[1] = {slot};
  TRY(pool_slots(who, 1, one, false));
  PoolSlot& s = pool[slot];
  if (s.frames_in || s.finished)
    return fail(-7, who + "slot " + std::to_string(slot) + " has already taken frames: enable the detector right after wh_pool_open");
  if (s.vad.on) return fail(-7, who + "slot " + std::to_string(slot) + " is already detecting");
  return svad_enable(who, s.vad, o);
}
int AudioFront::pool_vad_state(int n, const int* slots, wh_svad_state* out) {
  const std::string who = "pool_vad_state: pool: ";
  TRY(pool_slots(who, n, slots, false));
  if (!out) return fail(-1, who + "null out");
  for (int i = 0; i < n; ++i)
    if (!pool[slots[i]].vad.on)
      return fail(-7, who + field_at("slots", i) + " = " + std::to_string(slots[i]) + " has no detector (wh_pool_vad_enable)");
  for (int i = 0; i < n; ++i) out[i] = pool[slots[i]].vad.host;
  return 0;
}
int AudioFront::pool_vad_read(int slot, uint8_t* ring, int cap, uint32_t* hist) {
  const std::string who = "pool_vad_read: pool: ";
  const int one[1] = {slot};
  TRY(pool_slots(who, 1, one, false));
  if (!ring) return fail(-1, who + "null ring");
  const PoolSlot& s = pool[slot];
  if (!s.vad.on) return fail(-7, who + "slot " + std::to_string(slot) + " has no detector (wh_pool_vad_enable)");
  if (cap < s.vad.o.window)
    return fail(-7, who + "cap = " + std::to_string(cap) + " is less than the window of " + std::to_string(s.vad.o.window) + " frames");
  HIPCHK(hipMemcpy(ring, s.vad.block.p + sizeof(SvadBlock), (size_t)s.vad.o.window, hipMemcpyDeviceToHost));
  if (hist) HIPCHK(hipMemcpy(hist, s.vad.block.p + offsetof(SvadBlock, hist), VAD_BINS * 4, hipMemcpyDeviceToHost));
  return 0;
}
int AudioFront::pool_read(int slot, float* out, int64_t offset, int64_t n) {
  const std::string who = "pool_read: pool: ";
  const int one[1] = {slot};
  TRY(pool_slots(who, 1, one, false));
  if (!out) return fail(-1, who + "null out");
  const PoolSlot& s = pool[slot];
  const int64_t len = s.samples_out - s.dropped;
  if (offset < 0 || n < 0 || offset > len || n > len - offset)
    return fail(-7, who + "[" + std::to_string(offset) + ", " + std::to_string(offset) + " + " + std::to_string(n) +
                        ") is outside the " + std::to_string(len) + " resident samples of slot " + std::to_string(slot));
  if (n) HIPCHK(hipMemcpy(out, pool_base(slot, s.buf) + offset, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}
// wh_log_mel_batch with the files taken from the slots' buffers: the same descriptors, the same
// launch_mel_seg, only audio_off points into pool_audio.  Writes the context mel alone.
int AudioFront::pool_log_mel(int n, const int* slots, int64_t pad, int n_mels, int64_t* frame_base) {
  const std::string who = "pool_log_mel: pool: ";
  TRY(pool_slots(who, n, slots, false));
  if (!frame_base) return fail(-1, who + "null frame_base");
  if (pad < 0) return fail(-7, who + "negative padding");
  if (!h_filters.count(n_mels)) return fail(-7, who + "mel filters for n_mels=" + std::to_string(n_mels) + " not set");
  std::vector<MelFile> files(n);
  int64_t frames = 0, blocks = 0;
  for (int i = 0; i < n; ++i) {
    const PoolSlot& s = pool[slots[i]];
    const int64_t len = s.samples_out - s.dropped;
    if (len < 1) return fail(-7, who + field_at("slots", i) + " = " + std::to_string(slots[i]) + " has no samples");
    if (len + pad <= 200) return fail(-7, who + field_at("slots", i) + " = " + std::to_string(slots[i]) + " too short for reflect padding");
    MelFile& f = files[i];
    f.audio_off = (int64_t)(pool_base(slots[i], s.buf) - pool_audio.p);
    f.n_real = len;
    f.n_padded = len + pad;
    f.nframes = (len + pad) / 160;
    f.frame_base = frames;
    f.block_base = blocks;
    frames += f.nframes;
    blocks += mel_blocks(f.nframes);
  }
  if (blocks > 0x7fffffff) return fail(-7, who + "too many frames for one call");
  TRY(d_mel.reserve((size_t)n_mels * frames * 4));
  const size_t room = std::max<size_t>(n, 64);
  TRY(mel_files.reserve(room * sizeof(MelFile)));
  TRY(gmax_files.reserve(room * 4));
  mel_batch_files = 0;
  TRY(tm.mark(0, st));
  HIPCHK(hipMemcpyAsync(mel_files.p, files.data(), n * sizeof(MelFile), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(gmax_files.p, 0, (size_t)n * 4, st));
  launch_mel_seg(pool_audio.p, mel_files.p, n, blocks, d_filters[n_mels], n_mels, d_mel.p, frames, gmax_files.p, st);
  TRY(tm.finish(st, stats[WH_STAT_MEL_MS]));
  mel_is(frames, 0, n_mels, n);
  for (int i = 0; i < n; ++i) frame_base[i] = files[i].frame_base;
  frame_base[n] = frames;
  return 0;
}

// ------------------------------------------------------------ FLAC on the device
// (include/whisper_hip.h, csrc/wh_flacdev.h).  Device buffers grow to the largest stream seen.
// The stream of `plan` decoded into d_pcm as interleaved int32 (s32) or int16.  *ran = false:
// the chain did not hold or a sample left int32, the device path does not run (d_pcm is
// scratch; nothing else of the front end was touched).
int AudioFront::flac_device(const uint8_t* data, int64_t n, const whflac::Plan& plan, bool s32, bool* ran) {
  using namespace whflac;
  *ran = false;
  const int C = plan.si.channels;
  const size_t nc = plan.cands.size();
  if (nc > (size_t)(1 << 24)) return 0;  // lanes are counted in int
  TRY(fl_bytes.reserve((size_t)n));
  TRY(fl_cands.reserve(nc * sizeof(Cand)));
  TRY(fl_subs.reserve(nc * C * sizeof(Sub)));
  TRY(fl_ends.reserve(nc * 8));
  TRY(fl_stage.reserve((size_t)plan.stage * 4));
  TRY(fl_chain.reserve(nc * 4));
  TRY(fl_starts.reserve((nc + 1) * 8 + 8));  // the flag lies behind the starts
  TRY(d_pcm.reserve((size_t)plan.si.total * C * (s32 ? 4 : 2)));
  TRY(tm.mark(0, st));
  HIPCHK(hipMemcpyAsync(fl_bytes.p, data, (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(fl_cands.p, plan.cands.data(), nc * sizeof(Cand), hipMemcpyHostToDevice, st));
  TRY(tm.mark(1, st));
  launch_flac_parse(fl_bytes.p, n, fl_cands.p, (int)nc, C, plan.si.max_frame, fl_stage.p, fl_subs.p, fl_ends.p, st);
  TRY(tm.mark(2, st));
  std::vector<int64_t> ends(nc);
  HIPCHK(hipMemcpyAsync(ends.data(), fl_ends.p, nc * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status("flac_decode"));
  TRY(tm.charge(0, stats[WH_STAT_FLAC_UPLOAD_MS]));
  TRY(tm.charge(1, stats[WH_STAT_FLAC_PARSE_MS]));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> frames;
  std::vector<int64_t> starts;
  const bool chained = flac_chain(plan, n, ends.data(), &frames, &starts);
  charge_host(stats[WH_STAT_FLAC_INDEX_MS], t0);
  if (!chained) return 0;
  const int nf = (int)frames.size();
  int* d_bad = (int*)(fl_starts.p + nf + 1);
  starts.push_back(0);  // the flag, cleared with the same copy
  HIPCHK(hipMemcpyAsync(fl_chain.p, frames.data(), (size_t)nf * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(fl_starts.p, starts.data(), (size_t)(nf + 2) * 8, hipMemcpyHostToDevice, st));
  TRY(tm.mark(0, st));
  launch_flac_restore(fl_cands.p, fl_chain.p, nf, C, fl_stage.p, fl_subs.p, d_bad, st);
  TRY(tm.mark(1, st));
  launch_flac_gather(fl_cands.p, fl_chain.p, fl_starts.p, nf, C, fl_stage.p, d_pcm.p, s32 ? 1 : 0, plan.si.total, st);
  TRY(tm.mark(2, st));
  int bad = 1;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status("flac_decode"));
  TRY(tm.charge(0, stats[WH_STAT_FLAC_RESTORE_MS]));
  TRY(tm.charge(1, stats[WH_STAT_FLAC_GATHER_MS]));
  *ran = bad == 0;
  return 0;
}
// STREAMINFO and the index, timed into WH_STAT_FLAC_INDEX_MS.  < 0: not a FLAC stream (the
// host decoder's error)
int AudioFront::flac_plan_timed(const uint8_t* data, int64_t n, whflac::Plan* plan) {
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = whflac::flac_plan(data, n, plan);
  charge_host(stats[WH_STAT_FLAC_INDEX_MS], t0);
  if (rc < 0) return fail(rc, wh_flac_last_error());
  return rc;
}
int AudioFront::flac_decode_device(const uint8_t* data, int64_t n, int32_t* out, int64_t cap, int64_t* n_frames,
                                   int* path) {
  if (!data || !out || !n_frames || !path) return fail(-1, "flac_decode_device: null argument");
  whflac::Plan plan;
  const int rc = flac_plan_timed(data, n, &plan);
  if (rc < 0) return rc;
  if (rc == 0 && plan.si.total <= cap) {
    bool ran = false;
    TRY(flac_device(data, n, plan, true, &ran));
    if (ran) {
      HIPCHK(hipMemcpy(out, d_pcm.p, (size_t)plan.si.total * plan.si.channels * 4, hipMemcpyDeviceToHost));
      *n_frames = plan.si.total;
      *path = 0;
      return 0;
    }
  }
  *path = 1;
  const int hrc = wh_flac_decode(data, n, out, cap, n_frames);
  return hrc ? fail(hrc, wh_flac_last_error()) : 0;
}
int AudioFront::flac_ingest(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                            int64_t dst, int64_t reserve, int64_t* n_out, int* path) {
  const std::string who = "flac_ingest: ";
  if (!data) return fail(-1, who + "null data");
  if (!path) return fail(-1, who + "null path_out");
  whflac::Plan plan;
  const int rc = flac_plan_timed(data, n, &plan);
  if (rc < 0) return rc;
  const whflac::Info& si = plan.si;
  const int format = si.bps <= 16 ? WH_PCM_S16 : WH_PCM_S32;
  if (rc == 0) {
    TRY(ingest_check(who, format, si.total, si.channels, si.bps, up, down, taps, n_taps, dst, reserve, n_out));
    bool ran = false;
    TRY(flac_device(data, n, plan, format == WH_PCM_S32, &ran));
    if (ran) {
      *path = 0;
      return ingest_run(who, nullptr, format, si.total, si.channels, si.bps, up, down, taps, n_taps, dst, reserve,
                        n_out);
    }
  }
  // the host decoder and the PCM ingest, as a caller without this entry point would run them
  *path = 1;
  const int64_t cap = si.total > 0 ? si.total : n * 8;
  std::vector<int32_t> pcm((size_t)cap * si.channels);
  int64_t got = 0;
  const int hrc = wh_flac_decode(data, n, pcm.data(), cap, &got);
  if (hrc) return fail(hrc, wh_flac_last_error());
  if (format == WH_PCM_S32) return audio_ingest(pcm.data(), format, got, si.channels, si.bps, up, down, taps, n_taps, dst, reserve, n_out);
  std::vector<int16_t> pcm16(pcm.begin(), pcm.begin() + (size_t)got * si.channels);
  return audio_ingest(pcm16.data(), format, got, si.channels, si.bps, up, down, taps, n_taps, dst, reserve, n_out);
}
// ------------------------------------------------------------ WAV
// (include/whisper_hip.h).  The header is parsed on the host (csrc/wh_wav.cpp); the data chunk
// goes up as it is and the resampling kernel reads its encoding.
int AudioFront::wav_ingest(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                           int64_t dst, int64_t reserve, int64_t* n_out) {
  const std::string who = "wav_ingest: ";
  if (!data) return fail(-1, who + "null data");
  wh_wav_fmt f;
  if (wh_wav_info(data, n, &f) != 0) return fail(-7, who + wh_wav_last_error());
  //                         U8 S16 S24 S32 F32 F64 ALAW ULAW
  static const int container[8] = {1, 2, 3, 4, 4, 8, 1, 1};
  static const int bits[8] = {8, 16, 24, 32, 1, 1, 16, 16};  // the scale is 2^-(bits-1): 1 for floats
  // the ingest's own refusals; the sample format is the file's, so a valid one stands in
  TRY(ingest_check(who, WH_PCM_S32, f.n_frames, f.channels, 32, up, down, taps, n_taps, dst, reserve, n_out));
  return ingest_run(who, data + f.data_offset, WH_PCM_S32, f.n_frames, f.channels, bits[f.encoding], up, down, taps,
                    n_taps, dst, reserve, n_out, f.encoding, container[f.encoding] * f.channels);
}
// ------------------------------------------------------------ channels apart
// (include/whisper_hip.h).  The non-split call's checks, then the selection's, all before the
// first HIP call; then the same upload and one launch of the split kernel.
int AudioFront::select_check(const std::string& who, int format, int channels, const int* select, int n_select) {
  if (format == WH_PCM_F32)
    return fail(-7, who + "format WH_PCM_F32 is a mono waveform: there are no channels to split");
  const std::string why = select_error(channels, select, n_select);
  return why.empty() ? 0 : fail(why == "null select" ? -1 : -7, who + why);
}
int AudioFront::audio_ingest_split(const void* pcm, int format, int64_t n, int channels, int bits, int up, int down,
                                   const double* taps, int n_taps, const int* select, int n_select, int64_t dst,
                                   int64_t reserve, int64_t* n_out) {
  const std::string who = "audio_ingest_split: ";
  if (!pcm) return fail(-1, who + "null pcm");
  TRY(ingest_check(who, format, n, channels, bits, up, down, taps, n_taps, dst, reserve, n_out));
  TRY(select_check(who, format, channels, select, n_select));
  return ingest_run(who, pcm, format, n, channels, bits, up, down, taps, n_taps, dst, reserve, n_out, -1, 0, select,
                    n_select);
}
int AudioFront::flac_ingest_split(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                                  const int* select, int n_select, int64_t dst, int64_t reserve, int64_t* n_out,
                                  int* path) {
  const std::string who = "flac_ingest_split: ";
  if (!data) return fail(-1, who + "null data");
  if (!path) return fail(-1, who + "null path_out");
  whflac::Plan plan;
  const int rc = flac_plan_timed(data, n, &plan);
  if (rc < 0) return rc;
  const whflac::Info& si = plan.si;
  const int format = si.bps <= 16 ? WH_PCM_S16 : WH_PCM_S32;
  // the selection is checked here on both paths: the host decoder below is not run for a call
  // that will be refused
  TRY(select_check(who, format, si.channels, select, n_select));
  if (rc == 0) {
    TRY(ingest_check(who, format, si.total, si.channels, si.bps, up, down, taps, n_taps, dst, reserve, n_out));
    bool ran = false;
    TRY(flac_device(data, n, plan, format == WH_PCM_S32, &ran));
    if (ran) {
      *path = 0;
      return ingest_run(who, nullptr, format, si.total, si.channels, si.bps, up, down, taps, n_taps, dst, reserve,
                        n_out, -1, 0, select, n_select);
    }
  }
  *path = 1;
  const int64_t cap = si.total > 0 ? si.total : n * 8;
  std::vector<int32_t> pcm((size_t)cap * si.channels);
  int64_t got = 0;
  const int hrc = wh_flac_decode(data, n, pcm.data(), cap, &got);
  if (hrc) return fail(hrc, wh_flac_last_error());
  if (format == WH_PCM_S32)
    return audio_ingest_split(pcm.data(), format, got, si.channels, si.bps, up, down, taps, n_taps, select, n_select,
                              dst, reserve, n_out);
  std::vector<int16_t> pcm16(pcm.begin(), pcm.begin() + (size_t)got * si.channels);
  return audio_ingest_split(pcm16.data(), format, got, si.channels, si.bps, up, down, taps, n_taps, select, n_select,
                            dst, reserve, n_out);
}
int AudioFront::wav_ingest_split(const uint8_t* data, int64_t n, int up, int down, const double* taps, int n_taps,
                                 const int* select, int n_select, int64_t dst, int64_t reserve, int64_t* n_out) {
  const std::string who = "wav_ingest_split: ";
  if (!data) return fail(-1, who + "null data");
  wh_wav_fmt f;
  if (wh_wav_info(data, n, &f) != 0) return fail(-7, who + wh_wav_last_error());
  //                         U8 S16 S24 S32 F32 F64 ALAW ULAW
  static const int container[8] = {1, 2, 3, 4, 4, 8, 1, 1};
  static const int bits[8] = {8, 16, 24, 32, 1, 1, 16, 16};  // as in wav_ingest
  TRY(ingest_check(who, WH_PCM_S32, f.n_frames, f.channels, 32, up, down, taps, n_taps, dst, reserve, n_out));
  TRY(select_check(who, WH_PCM_S32, f.channels, select, n_select));
  return ingest_run(who, data + f.data_offset, WH_PCM_S32, f.n_frames, f.channels, bits[f.encoding], up, down, taps,
                    n_taps, dst, reserve, n_out, f.encoding, container[f.encoding] * f.channels, select, n_select);
}
int AudioFront::audio_read(float* out, int64_t offset, int64_t n) {
  if (!out) return fail(-1, "audio_read: null out");
  const int64_t end = audio_segs.empty() ? 0 : audio_segs.back().first + audio_segs.back().second;
  if (offset < 0 || n < 0 || offset + n > end)
    return fail(-8, "audio_read: [" + std::to_string(offset) + ", " + std::to_string(offset + n) +
                        ") is outside the " + std::to_string(end) + " resident samples");
  if (n) HIPCHK(hipMemcpy(out, d_audio.p + offset, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------ speech spans
// (include/whisper_hip.h, csrc/wh_vad.hip).  The files are the first n_files resident
// segments; nothing here touches the segments or the mel.
int AudioFront::vad_plan(const char* who, int n_files, std::vector<VadFile>* files, int64_t* blocks) {
  const std::string w = std::string(who) + ": ";
  if (n_files < 1) return fail(-7, w + "n_files = " + std::to_string(n_files) + ", need at least one file");
  if ((size_t)n_files > audio_segs.size())
    return fail(-7, w + std::to_string(n_files) + " files asked for, " + std::to_string(audio_segs.size()) +
                        " segments are resident");
  files->resize(n_files);
  int64_t frames = 0, nb = 0, pairs = 0;
  for (int i = 0; i < n_files; ++i) {
    VadFile& f = (*files)[i];
    f.off = audio_segs[i].first;
    f.n = audio_segs[i].second;
    f.frames = (f.n + VAD_HOP - 1) / VAD_HOP;
    if (f.n < 1 || f.frames >= ((int64_t)1 << 30))
      return fail(-7, w + "resident file " + std::to_string(i) + " has " + std::to_string(f.n) + " samples: out of range");
    f.e_base = frames;
    f.block_base = nb;
    f.run_base = pairs;
    frames += f.frames;
    nb += vad_blocks(f.frames);
    pairs += vad_run_pairs(f.frames);
  }
  if (nb > 0x7fffffff) return fail(-7, w + "too many frames for one call");
  *blocks = nb;
  return 0;
}
// descriptors up, histograms cleared, k_frame_energy launched (between the caller's marks)
int AudioFront::vad_energy_launch(const std::vector<VadFile>& files, int64_t blocks) {
  const int n_files = (int)files.size();
  HIPCHK(hipMemcpyAsync(vad_files.p, files.data(), files.size() * sizeof(VadFile), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(vad_hist.p, 0, (size_t)n_files * VAD_BINS * 4, st));
  launch_frame_energy(d_audio.p, vad_files.p, n_files, blocks, vad_energy.p, vad_hist.p, st);
  return 0;
}
int AudioFront::speech_spans(const wh_vad_opts* o, int n_files, int32_t* spans, int cap, int32_t* n_spans,
                             uint64_t* thresholds) {
  const char* who = "speech_spans";
  const std::string w = "speech_spans: ";
  if (!o || !n_spans || !thresholds) return fail(-1, w + "null argument");
  if (cap < 0 || cap > (1 << 29)) return fail(-7, w + "cap = " + std::to_string(cap) + " out of range");
  if (cap > 0 && !spans) return fail(-1, w + "null spans with cap > 0");
  if (o->percentile < 1 || o->percentile > 99)
    return fail(-7, w + "percentile = " + std::to_string(o->percentile) + " outside 1..99");
  if (o->ratio_q8 < 256 || o->ratio_q8 > 2560000)
    return fail(-7, w + "ratio_q8 = " + std::to_string(o->ratio_q8) + " outside [256, 2560000] (0 to 40 dB)");
  if (o->t_lo > o->t_hi) return fail(-7, w + "t_lo above t_hi");
  const int lim = 1 << 30;
  if (o->min_silence < 0 || o->min_speech < 0 || o->pad < 0 || o->min_silence > lim || o->min_speech > lim || o->pad > lim)
    return fail(-7, w + "min_silence, min_speech and pad are frame counts from 0 to 2^30");
  std::vector<VadFile> files;
  int64_t blocks = 0;
  TRY(vad_plan(who, n_files, &files, &blocks));
  const VadFile& last = files.back();
  // a file has at most frames / 2 + 1 spans: more room than the largest file can fill is not
  // allocated or copied (the caller's rows keep their stride of cap)
  int64_t most = 0;
  for (const VadFile& f : files) most = std::max(most, vad_run_pairs(f.frames));
  const int dcap = (int)std::min<int64_t>(cap, most);
  const size_t room = std::max<size_t>(n_files, 64);
  TRY(vad_files.reserve(room * sizeof(VadFile)));
  TRY(vad_hist.reserve(room * VAD_BINS * 4));
  TRY(vad_energy.reserve((size_t)(last.e_base + last.frames) * 8));
  TRY(vad_runs.reserve((size_t)(last.run_base + vad_run_pairs(last.frames)) * 8));
  // what goes back: thresholds [n_files] uint64, counts [n_files] int, spans [n_files][cap][2] int
  const size_t off_cnt = (size_t)n_files * 8, off_spans = off_cnt + (size_t)n_files * 4;
  const size_t bytes = off_spans + (size_t)n_files * dcap * 8;
  TRY(vad_out.reserve(std::max<size_t>(bytes, 4096)));
  std::vector<char> host(bytes);
  VadOpts vo;
  vo.ratio_q8 = o->ratio_q8; vo.t_lo = o->t_lo; vo.t_hi = o->t_hi;
  vo.percentile = o->percentile; vo.min_silence = o->min_silence; vo.min_speech = o->min_speech; vo.pad = o->pad;
  TRY(tm.mark(0, st));
  TRY(vad_energy_launch(files, blocks));
  TRY(tm.mark(1, st));
  launch_speech_spans(vad_energy.p, vad_hist.p, vad_files.p, n_files, vo, vad_runs.p, dcap,
                      (unsigned long long*)vad_out.p, (int*)(vad_out.p + off_cnt), (int*)(vad_out.p + off_spans), st);
  TRY(tm.mark(2, st));
  HIPCHK(hipMemcpyAsync(host.data(), vad_out.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(who));
  TRY(tm.charge(0, stats[WH_STAT_VAD_ENERGY_MS]));
  TRY(tm.charge(1, stats[WH_STAT_VAD_SPANS_MS]));
  memcpy(thresholds, host.data(), (size_t)n_files * 8);
  memcpy(n_spans, host.data() + off_cnt, (size_t)n_files * 4);
  // a file that needs more room has none written: its part of the buffer is not data
  for (int i = 0; i < n_files; ++i)
    if (n_spans[i] <= dcap && n_spans[i] > 0)
      memcpy(spans + (size_t)i * cap * 2, host.data() + off_spans + (size_t)i * dcap * 8, (size_t)n_spans[i] * 8);
  return 0;
}
int AudioFront::frame_energy_read(int file, uint64_t* energy_out, int64_t cap, uint32_t* hist_out) {
  const char* who = "frame_energy_read";
  if (file < 0 || (size_t)file >= audio_segs.size())
    return fail(-7, "frame_energy_read: file = " + std::to_string(file) + ", " + std::to_string(audio_segs.size()) +
                        " segments are resident");
  std::vector<VadFile> files;
  int64_t blocks = 0;
  TRY(vad_plan(who, file + 1, &files, &blocks));
  const VadFile& f = files[file];
  if (!energy_out) return (int)f.frames;  // the size query: nothing is computed
  if (cap < f.frames)
    return fail(-7, "frame_energy_read: cap = " + std::to_string(cap) + ", the file has " + std::to_string(f.frames) +
                        " frames");
  const size_t room = std::max<size_t>(files.size(), 64);
  TRY(vad_files.reserve(room * sizeof(VadFile)));
  TRY(vad_hist.reserve(room * VAD_BINS * 4));
  TRY(vad_energy.reserve((size_t)(f.e_base + f.frames) * 8));
  TRY(tm.mark(0, st));
  TRY(vad_energy_launch(files, blocks));
  TRY(tm.mark(1, st));
  HIPCHK(hipMemcpyAsync(energy_out, vad_energy.p + f.e_base, (size_t)f.frames * 8, hipMemcpyDeviceToHost, st));
  if (hist_out)
    HIPCHK(hipMemcpyAsync(hist_out, vad_hist.p + (size_t)file * VAD_BINS, VAD_BINS * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(who));
  return tm.charge(0, stats[WH_STAT_VAD_ENERGY_MS]);
}

// ------------------------------------------------------------ mel
// what d_mel now holds
void AudioFront::mel_is(int64_t frames, int64_t f0, int n_mels, int batch_files) {
  mel_frames = frames; mel_f0 = f0; mel_nm = n_mels; mel_batch_files = batch_files;
}
// frames [frame0, frame0 + count) of the padded signal's log-mel (count < 0: to the
// end); the front end keeps them with their absolute frame offset (mel_f0), so window
// seeks stay absolute.  A rank of a sharded file computes only its own frames.
int AudioFront::log_mel_frames(const float* audio, int64_t n, int64_t pad, int n_mels, int64_t frame0, int64_t count,
                               int normalize, int64_t* total_frames) {
  if (!h_filters.count(n_mels)) return fail(-7, "mel filters for n_mels=" + std::to_string(n_mels) + " not set");
  if (n + pad <= 200 || n < 1) return fail(-7, "audio too short for reflect padding");
  if (!audio && n != audio_n) return fail(-7, "no resident audio of that length");
  const int64_t total = (n + pad) / 160;
  if (count < 0) count = total - frame0;
  if (frame0 < 0 || count < 1 || frame0 + count > total) return fail(-7, "mel frame range out of bounds");
  if (audio) {
    stream_ends("log_mel with a host array");
    TRY(audio_room((size_t)n));
  }
  TRY(d_mel.reserve((size_t)n_mels * count * 4));
  TRY(tm.mark(0, st));
  if (audio) {
    HIPCHK(hipMemcpyAsync(d_audio.p, audio, n * 4, hipMemcpyHostToDevice, st));
    one_segment(n);
  }
  HIPCHK(hipMemsetAsync(gmax.p, 0, 16, st));
  launch_mel(d_audio.p, n, n + pad, frame0, count, d_filters[n_mels], n_mels, d_mel.p, count, gmax.p, st);
  if (normalize) launch_mel_norm(d_mel.p, count, count, n_mels, gmax.p, nullptr, st);
  TRY(tm.finish(st, stats[WH_STAT_MEL_MS]));
  mel_is(count, frame0, n_mels, 0);
  *total_frames = total;
  return 0;
}
// log-mel of n_files waveforms (concatenated in `audio`) in one pass: one upload, one
// descriptor copy, the segmented frames + normalisation launches, one synchronisation.
// The files' frames lie back to back in d_mel (row stride = all frames of the call).
int AudioFront::log_mel_batch(const float* audio, int n_files, const int64_t* n_samples, int64_t pad, int n_mels,
                              int64_t* frame_base) {
  if (n_files < 1) return fail(-7, "log_mel_batch: n_files = " + std::to_string(n_files) + ", need at least one file");
  if (!n_samples || !frame_base) return fail(-1, "null argument");
  if (pad < 0) return fail(-7, "log_mel_batch: negative padding");
  if (!h_filters.count(n_mels)) return fail(-7, "mel filters for n_mels=" + std::to_string(n_mels) + " not set");
  std::vector<MelFile> files(n_files);
  int64_t samples = 0, frames = 0, blocks = 0;
  for (int i = 0; i < n_files; ++i) {
    const int64_t n = n_samples[i];
    if (n < 1) return fail(-7, "log_mel_batch: file " + std::to_string(i) + " has no samples");
    if (n + pad <= 200) return fail(-7, "log_mel_batch: file " + std::to_string(i) + " too short for reflect padding");
    MelFile& f = files[i];
    f.audio_off = samples;
    f.n_real = n;
    f.n_padded = n + pad;
    f.nframes = (n + pad) / 160;
    f.frame_base = frames;
    f.block_base = blocks;
    samples += n;
    frames += f.nframes;
    blocks += mel_blocks(f.nframes);
  }
  if (blocks > 0x7fffffff) return fail(-7, "log_mel_batch: too many frames for one call");
  if (!audio) {
    // the files are the resident segments (wh_audio_ingest), which stay resident
    bool same = (int)audio_segs.size() == n_files;
    for (int i = 0; same && i < n_files; ++i)
      same = audio_segs[i].first == files[i].audio_off && audio_segs[i].second == files[i].n_real;
    if (!same)
      return fail(-7, "log_mel_batch: the " + std::to_string(audio_segs.size()) +
                          " resident segments are not these " + std::to_string(n_files) + " files");
  } else {
    stream_ends("log_mel_batch with a host array");
    TRY(audio_room((size_t)samples));
    audio_n = -1;  // the buffer now holds several files: no resident audio of any length
    audio_segs.clear();
  }
  TRY(d_mel.reserve((size_t)n_mels * frames * 4));
  const size_t room = std::max<size_t>(n_files, 64);
  TRY(mel_files.reserve(room * sizeof(MelFile)));
  TRY(gmax_files.reserve(room * 4));
  mel_batch_files = 0;
  TRY(tm.mark(0, st));
  if (audio) HIPCHK(hipMemcpyAsync(d_audio.p, audio, (size_t)samples * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(mel_files.p, files.data(), n_files * sizeof(MelFile), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(gmax_files.p, 0, (size_t)n_files * 4, st));
  launch_mel_seg(d_audio.p, mel_files.p, n_files, blocks, d_filters[n_mels], n_mels, d_mel.p, frames, gmax_files.p, st);
  TRY(tm.finish(st, stats[WH_STAT_MEL_MS]));
  mel_is(frames, 0, n_mels, n_files);
  for (int i = 0; i < n_files; ++i) frame_base[i] = files[i].frame_base;
  frame_base[n_files] = frames;
  return 0;
}
// an ordered-uint maximum (as the kernels' atomicMax keeps it) back to its float
static void ordered_to_float(unsigned u, float* g) {
  const unsigned v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  memcpy(g, &v, 4);
}
int AudioFront::mel_max_batch(float* g, int n_files) {
  if (!g) return fail(-1, "null argument");
  if (n_files < 1 || n_files != mel_batch_files)
    return fail(-7, "mel_max_batch: the context mel is of " + std::to_string(mel_batch_files) + " batch files, not " +
                        std::to_string(n_files));
  std::vector<unsigned> u(n_files);
  HIPCHK(hipMemcpy(u.data(), gmax_files.p, (size_t)n_files * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n_files; ++i) ordered_to_float(u[i], g + i);
  return 0;
}
int AudioFront::mel_max(float* g) {
  unsigned u = 0;
  HIPCHK(hipMemcpy(&u, gmax.p, 4, hipMemcpyDeviceToHost));
  ordered_to_float(u, g);
  return 0;
}
int AudioFront::mel_normalize(float g) {
  if (mel_batch_files) return fail(-7, "mel_normalize: the context mel is of a wh_log_mel_batch call, each file already normalised");
  float* ovr = (float*)(gmax.p + 4);
  HIPCHK(hipMemcpyAsync(ovr, &g, 4, hipMemcpyHostToDevice, st));
  launch_mel_norm(d_mel.p, mel_frames, mel_frames, mel_nm, gmax.p, ovr, st);
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
int AudioFront::mel_read(float* out, int64_t f0, int64_t nf) {
  f0 -= mel_f0;  // absolute frame -> stored frame
  if (f0 < 0 || nf < 0 || f0 + nf > mel_frames) return fail(-8, "mel_read out of range");
  HIPCHK(hipMemcpy2D(out, nf * 4, d_mel.p + f0, mel_frames * 4, nf * 4, mel_nm, hipMemcpyDeviceToHost));
  return 0;
}
// a host mel of the model's n_mels bins, nf frames from frame 0
int AudioFront::mel_write(const float* mel, int64_t nf, int n_mels) {
  const size_t need = (size_t)n_mels * nf;
  TRY(d_mel.reserve(need * 4));
  HIPCHK(hipMemcpy(d_mel.p, mel, need * 4, hipMemcpyHostToDevice));
  mel_is(nf, 0, n_mels, 0);
  return 0;
}
