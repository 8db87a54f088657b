// RIFF/WAVE header parser of libwhisper_hip (wh_wav_info; include/whisper_hip.h states the
// rules).  Host only: no context, no GPU.  It finds the sample encoding and where the data
// chunk lies; the samples themselves are never touched here, the data chunk is uploaded as it
// is and read by the resampling kernel (csrc/wh_ingest.hip).  Every read goes through the
// bounds-checked helpers below: nothing at or past data + n is read, whatever the bytes say.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "whisper_hip.h"

namespace {

thread_local std::string g_wav_err;

int refuse(const std::string& msg) {
  g_wav_err = "wav: " + msg;
  return -2;
}

struct Bytes {
  const uint8_t* p;
  int64_t n;
  bool has(int64_t at, int64_t len) const { return at >= 0 && len >= 0 && at <= n && len <= n - at; }
  // callers check has() first
  uint32_t u16(int64_t at) const { return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8; }
  uint32_t u32(int64_t at) const { return u16(at) | u16(at + 2) << 16; }
  bool is(int64_t at, const char* id) const { return memcmp(p + at, id, 4) == 0; }
};

std::string hex(uint32_t v) {
  char b[16];
  snprintf(b, sizeof b, "0x%X", v);
  return b;
}

// bytes 2..15 of KSDATAFORMAT_SUBTYPE_*: the GUID whose first two bytes are the format tag
const uint8_t kSubFormatTail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};

// the `fmt ` chunk body at [at, at + size) -> encoding, channels, rate, valid bits, block align
int parse_fmt(const Bytes& b, int64_t at, int64_t size, wh_wav_fmt* out, int* block_align) {
  if (size < 16) return refuse("fmt chunk of " + std::to_string(size) + " bytes is too short (16 at least)");
  uint32_t tag = b.u16(at);
  const int channels = (int)b.u16(at + 2);
  const uint32_t rate = b.u32(at + 4);
  const int align = (int)b.u16(at + 12);
  const int bits = (int)b.u16(at + 14);
  int valid = bits;
  if (tag == 0xFFFE) {
    if (size < 18 || b.u16(at + 16) < 22 || size < 40)
      return refuse("extensible fmt chunk too short (cbSize >= 22 and 40 bytes needed)");
    if (memcmp(b.p + at + 26, kSubFormatTail, 14) != 0)
      return refuse("extensible SubFormat is not a KSDATAFORMAT_SUBTYPE wave format GUID");
    if (b.u16(at + 18)) valid = (int)b.u16(at + 18);
    tag = b.u16(at + 24);
  }
  if (tag != 1 && tag != 3 && tag != 6 && tag != 7)
    return refuse("unsupported format tag " + hex(tag) + " (supported: 1 PCM, 3 IEEE float, 6 A-law, 7 mu-law)");
  if (channels < 1 || channels > 256) return refuse("channels = " + std::to_string(channels) + " out of range (1..256)");
  if (rate < 1 || rate > 0x7FFFFFFFu) return refuse("sample rate = " + std::to_string(rate) + " out of range");
  if (align < 1 || align % channels != 0)
    return refuse("block_align = " + std::to_string(align) + " is not a multiple of channels = " +
                  std::to_string(channels));
  const int container = align / channels;
  if ((bits + 7) / 8 != container)
    return refuse("bits per sample = " + std::to_string(bits) + " does not fill a container of " +
                  std::to_string(container) + " bytes");
  int enc = -1;
  if (tag == 1) {
    const int by_container[5] = {-1, WH_WAV_U8, WH_WAV_S16, WH_WAV_S24, WH_WAV_S32};
    if (container > 4) return refuse("PCM container of " + std::to_string(container) + " bytes (supported: 1, 2, 3, 4)");
    enc = by_container[container];
  } else if (tag == 3) {
    if (container != 4 && container != 8)
      return refuse("IEEE float container of " + std::to_string(container) + " bytes (supported: 4, 8)");
    enc = container == 4 ? WH_WAV_F32 : WH_WAV_F64;
  } else {
    if (container != 1)
      return refuse(std::string(tag == 6 ? "A-law" : "mu-law") + " container of " + std::to_string(container) +
                    " bytes (supported: 1)");
    enc = tag == 6 ? WH_WAV_ALAW : WH_WAV_ULAW;
  }
  if (valid < 1 || valid > container * 8) valid = container * 8;
  out->encoding = enc;
  out->channels = channels;
  out->sample_rate = (int)rate;
  out->valid_bits = valid;
  *block_align = align;
  return 0;
}

}  // namespace

extern "C" {

const char* wh_wav_last_error(void) { return g_wav_err.c_str(); }

int wh_wav_info(const uint8_t* data, int64_t n, wh_wav_fmt* out) {
  if (!data || !out) {
    g_wav_err = "wav: null argument";
    return -1;
  }
  const Bytes b{data, n};
  if (b.has(0, 4) && (b.is(0, "RF64") || b.is(0, "BW64")))
    return refuse(std::string(b.is(0, "RF64") ? "RF64" : "BW64") + " (64-bit RIFF) is not supported");
  if (!b.has(0, 12) || !b.is(0, "RIFF") || !b.is(8, "WAVE")) return refuse("not a RIFF/WAVE file");
  wh_wav_fmt f;
  memset(&f, 0, sizeof f);
  int align = 0;
  bool have_fmt = false;
  int64_t pos = 12;
  while (b.has(pos, 8)) {
    const int64_t size = (int64_t)b.u32(pos + 4);
    const int64_t body = pos + 8;
    if (b.is(pos, "data")) {
      if (!have_fmt) return refuse("data chunk before the fmt chunk");
      const int64_t present = n - body;
      const bool to_end = size == 0 || size == 0xFFFFFFFFll;  // what an encoder writing to a pipe leaves
      const int64_t avail = to_end || size > present ? present : size;
      f.data_offset = body;
      f.n_frames = avail / align;  // a trailing partial frame is dropped
      if (f.n_frames < 1) return refuse("no whole frame in the data chunk");
      *out = f;
      return 0;
    }
    if (!b.has(body, size))
      return refuse("chunk '" + std::string((const char*)data + pos, 4) + "' of " + std::to_string(size) +
                    " bytes runs past the end of the file");
    if (b.is(pos, "fmt ") && !have_fmt) {
      const int rc = parse_fmt(b, body, size, &f, &align);
      if (rc) return rc;
      have_fmt = true;
    }
    pos = body + size + (size & 1);  // chunks are padded to even sizes
  }
  return refuse(have_fmt ? "no data chunk" : "no fmt chunk");
}

}  // extern "C"
