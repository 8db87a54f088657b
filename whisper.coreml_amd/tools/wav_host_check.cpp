// wh_wav_info on untrusted bytes, meant to be built with -fsanitize=address,undefined
// (make tools/wav_host_check): the RIFF/WAVE parser of csrc/wh_wav.cpp meets truncated and
// altered headers here, on the CPU, in a program of its own.
//   wav_host_check FILE.wav...
// Every file is parsed whole, at every prefix length up to the data chunk plus a spread of
// lengths beyond it, and with every header byte altered to several values.  Each buffer is a
// heap copy of exactly the length given, so a read at or past data + n is an AddressSanitizer
// report.  Whenever the parser accepts, data_offset + n_frames * block_align <= n and the
// field ranges of include/whisper_hip.h must hold.  Exit status 1 on a violation.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "whisper_hip.h"

namespace {

struct Tally {
  long runs = 0, accepted = 0, violations = 0;
};

const int kContainer[8] = {1, 2, 3, 4, 4, 8, 1, 1};  // WH_WAV_U8 ... WH_WAV_ULAW

// 0 fine (accepted within bounds, or refused with a message), 1 violation
int check(const uint8_t* p, int64_t n, Tally* t, const char* what, long where) {
  // exactly n bytes on the heap: the sanitizer's red zone starts at data + n
  std::vector<uint8_t> d(p, p + n);
  wh_wav_fmt f;
  memset(&f, 0x5a, sizeof f);
  ++t->runs;
  const int rc = wh_wav_info(d.empty() ? (const uint8_t*)"" : d.data(), n, &f);
  if (rc != 0) {
    const char* msg = wh_wav_last_error();
    if (rc > 0 || !msg || !msg[0]) {
      printf("VIOLATION %s %ld: rc %d without a message\n", what, where, rc);
      ++t->violations;
      return 1;
    }
    return 0;
  }
  ++t->accepted;
  const bool fields = f.encoding >= 0 && f.encoding < 8 && f.channels >= 1 && f.channels <= 256 &&
                      f.sample_rate >= 1 && f.n_frames >= 1 && f.data_offset >= 20 && f.valid_bits >= 1 &&
                      f.valid_bits <= 8 * kContainer[f.encoding];
  const bool inside = fields && f.data_offset + f.n_frames * kContainer[f.encoding] * f.channels <= n;
  if (!fields || !inside) {
    printf("VIOLATION %s %ld: encoding %d channels %d rate %d valid_bits %d data_offset %lld n_frames %lld of %lld bytes\n",
           what, where, f.encoding, f.channels, f.sample_rate, f.valid_bits, (long long)f.data_offset,
           (long long)f.n_frames, (long long)n);
    ++t->violations;
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) {
    FILE* fp = fopen(argv[i], "rb");
    if (!fp) {
      printf("cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(fp);
    const long n = (long)d.size();
    Tally whole, cut, alt;
    check(d.data(), n, &whole, "whole", 0);
    wh_wav_fmt f;
    // the header: everything up to the data chunk's first sample (the whole file when refused)
    const long head = wh_wav_info(d.data(), n, &f) == 0 ? (long)f.data_offset : (n < 4096 ? n : 4096);
    for (long c = 0; c <= head && c <= n; ++c) check(d.data(), c, &cut, "truncated at", c);
    for (int k = 1; k <= 64; ++k) {  // a spread beyond the header, and the last bytes
      const long c = head + (n - head) * k / 64 - (k % 7);
      if (c > head && c < n) check(d.data(), c, &cut, "truncated at", c);
    }
    std::vector<uint8_t> m = d;
    const uint8_t values[6] = {0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF};
    for (long at = 0; at < head && at < n; ++at) {
      const uint8_t keep = m[at];
      for (uint8_t v : values) {
        m[at] = v;
        check(m.data(), n, &alt, "byte altered at", at);
      }
      m[at] = (uint8_t)(keep ^ 0x01), check(m.data(), n, &alt, "byte altered at", at);
      m[at] = (uint8_t)(keep + 1), check(m.data(), n, &alt, "byte altered at", at);
      m[at] = keep;
    }
    const long v = whole.violations + cut.violations + alt.violations;
    printf("%s: %ld bytes, header %ld; whole %s; truncated %ld runs (%ld accepted); altered %ld runs (%ld accepted); "
           "%ld violations\n",
           argv[i], n, head, whole.accepted ? "accepted" : "refused", cut.runs, cut.accepted, alt.runs, alt.accepted, v);
    bad += v != 0;
  }
  return bad ? 1 : 0;
}
