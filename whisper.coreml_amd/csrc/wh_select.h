// The channel selection of wh_audio_ingest_split / wh_flac_ingest_split / wh_wav_ingest_split,
// checked on the host before anything is launched (include/whisper_hip.h).  Plain C++ with no
// HIP in it, so tools/select_host_check.cpp runs it under the host sanitizers.
#pragma once
#include <string>

namespace wh {

// "" when select[0 .. n_select) are distinct channel ids of a file with `channels` channels;
// otherwise what is wrong, naming the field
inline std::string select_error(int channels, const int* select, int n_select) {
  if (channels < 1 || channels > 256) return "channels = " + std::to_string(channels) + " out of range";
  if (!select) return "null select";
  if (n_select < 1 || n_select > channels)
    return "n_select = " + std::to_string(n_select) + " outside 1.." + std::to_string(channels) + " (channels)";
  bool seen[256] = {false};  // channels <= 256 (ingest_check)
  for (int s = 0; s < n_select; ++s) {
    const int c = select[s];
    if (c < 0 || c >= channels)
      return "select[" + std::to_string(s) + "] = " + std::to_string(c) + " is not a channel of a file with " +
             std::to_string(channels);
    if (seen[c]) return "select[" + std::to_string(s) + "] = " + std::to_string(c) + " repeats a channel";
    seen[c] = true;
  }
  return "";
}

}  // namespace wh
