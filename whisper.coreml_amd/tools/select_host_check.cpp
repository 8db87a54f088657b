// The channel-selection check of the wh_*_ingest_split calls (csrc/wh_select.h) under the host
// sanitizers, without a context, a GPU or Python:
//   make -C whisper.coreml_amd tools/select_host_check && ./whisper.coreml_amd/tools/select_host_check
#include <cstdio>
#include <string>
#include <vector>

#include "wh_select.h"

static int failures = 0;

static void expect(const char* what, int channels, const std::vector<int>* select, int n_select, const char* needle) {
  const std::string why = wh::select_error(channels, select ? select->data() : nullptr, n_select);
  const bool ok = needle ? why.find(needle) != std::string::npos : why.empty();
  if (!ok) {
    ++failures;
    fprintf(stderr, "FAIL %s: got \"%s\", want %s%s\n", what, why.c_str(), needle ? "a message with " : "no error",
            needle ? needle : "");
  }
}

int main() {
  std::vector<int> all256(256), rev{2, 1, 0}, dup{1, 2, 1}, high{0, 3}, low{-1}, one{4}, huge{1 << 30};
  for (int i = 0; i < 256; ++i) all256[i] = 255 - i;
  expect("all of 256, reversed", 256, &all256, 256, nullptr);
  expect("three reversed", 3, &rev, 3, nullptr);
  expect("one of five", 5, &one, 1, nullptr);
  expect("null select", 3, nullptr, 2, "null select");
  expect("n_select 0", 3, &rev, 0, "n_select");
  expect("n_select negative", 3, &rev, -5, "n_select");
  expect("n_select above channels", 2, &rev, 3, "n_select");
  expect("id == channels", 3, &high, 2, "select[1]");
  expect("negative id", 3, &low, 1, "select[0]");
  expect("huge id", 256, &huge, 1, "select[0]");
  expect("repeat", 3, &dup, 3, "select[2] = 1 repeats");
  expect("channels 0", 0, &rev, 1, "channels");
  expect("channels 257", 257, &rev, 3, "channels");
  if (failures) return 1;
  puts("select_host_check: ok");
  return 0;
}
