// wh_flac_decode_indexed against wh_flac_decode on the host, meant to be built with
// -fsanitize=address,undefined (make tools/flac_host_check): the frame code of wh_flacdev.h
// meets false candidates and damaged streams here, on the CPU, before it runs on a GPU.
//   flac_host_check [--stride N] FILE.flac...
// Every file is decoded whole, truncated at a spread of byte counts, and with single bytes
// altered (every N-th byte; N = 1 for files under 64 KiB unless given).  Both decoders must
// agree each time: the same samples, or both an error.  Exit status 1 on a disagreement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "whisper_hip.h"

namespace {

struct Tally {
  long runs = 0, indexed = 0, errors = 0, mismatches = 0;
};

// 0 agree, 1 disagree
int compare(const std::vector<uint8_t>& d, Tally* t, const char* what, long where) {
  int rate = 0, ch = 0, bps = 0;
  int64_t total = 0;
  const uint8_t* p = d.empty() ? (const uint8_t*)"" : d.data();
  const int64_t n = (int64_t)d.size();
  ++t->runs;
  if (wh_flac_info(p, n, &rate, &ch, &bps, &total) != 0) {
    std::vector<int32_t> one(8);
    int64_t got = 0;
    if (wh_flac_decode_indexed(p, n, one.data(), 1, &got) == 0) {
      printf("MISMATCH %s %ld: the indexed decoder took a stream without STREAMINFO\n", what, where);
      ++t->mismatches;
      return 1;
    }
    ++t->errors;
    return 0;
  }
  int64_t cap = total > 0 ? total : n * 8;
  if (cap > (int64_t)1 << 24) cap = (int64_t)1 << 24;  // an altered total: both decoders then hit the same capacity
  std::vector<int32_t> a((size_t)cap * ch + 8, 0x5a5a5a5a), b((size_t)cap * ch + 8, 0x5a5a5a5a);
  int64_t na = -1, nb = -1;
  const int ra = wh_flac_decode(p, n, a.data(), cap, &na);
  const std::string ea = ra ? wh_flac_last_error() : "";
  const int rb = wh_flac_decode_indexed(p, n, b.data(), cap, &nb);
  const std::string eb = rb ? wh_flac_last_error() : "";
  if (rb == 0 && wh_flac_last_path() == 0) ++t->indexed;
  if (ra != rb || ea != eb) {
    printf("MISMATCH %s %ld: host rc %d (%s), indexed rc %d (%s)\n", what, where, ra, ea.c_str(), rb, eb.c_str());
    ++t->mismatches;
    return 1;
  }
  if (ra != 0) {
    ++t->errors;
    return 0;
  }
  if (na != nb || memcmp(a.data(), b.data(), (size_t)na * ch * 4) != 0) {
    printf("MISMATCH %s %ld: %lld and %lld frames, or other samples\n", what, where, (long long)na, (long long)nb);
    ++t->mismatches;
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  long stride = 0;
  int bad = 0;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--stride") && i + 1 < argc) {
      stride = atol(argv[++i]);
      continue;
    }
    FILE* f = fopen(argv[i], "rb");
    if (!f) {
      printf("cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    Tally whole, cut, alt;
    compare(d, &whole, "whole", 0);
    if (whole.indexed != 1) printf("NOTE %s: the whole stream went through the host decoder\n", argv[i]);
    const long n = (long)d.size();
    // truncations: around the head, a spread through the body, the last bytes
    std::vector<long> cuts = {0, 3, 4, 8, 41, 42, 43, 50, n - 1, n - 2, n - 3, n - 17};
    for (int k = 1; k < 24; ++k) cuts.push_back(n * k / 24 + k);
    for (long c : cuts)
      if (c >= 0 && c < n) compare(std::vector<uint8_t>(d.begin(), d.begin() + c), &cut, "truncated at", c);
    const long step = stride > 0 ? stride : (n < 65536 ? 1 : n / 1500 + 1);
    std::vector<uint8_t> m = d;
    for (long at = 0; at < n; at += step) {
      const uint8_t keep = m[at];
      const uint8_t flips[3] = {(uint8_t)(keep ^ 0x01), (uint8_t)(keep ^ 0x80), (uint8_t)(keep ^ 0xFF)};
      m[at] = flips[(at / step) % 3];
      compare(m, &alt, "byte altered at", at);
      m[at] = keep;
    }
    printf("%s: %ld bytes; truncated %ld runs (%ld both error, %ld indexed); altered %ld runs (%ld both error, %ld indexed); "
           "%ld mismatches\n",
           argv[i], n, cut.runs, cut.errors, cut.indexed, alt.runs, alt.errors, alt.indexed,
           whole.mismatches + cut.mismatches + alt.mismatches);
    bad += (whole.mismatches + cut.mismatches + alt.mismatches) != 0;
  }
  return bad ? 1 : 0;
}
