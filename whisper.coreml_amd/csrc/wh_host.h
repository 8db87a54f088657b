// Host plumbing shared by the runtime's translation units (wh_runtime.hip, wh_audio.hip):
// the thread's error text and the status macros, the checked releases of a context's
// destructor, stage timing between HIP events and the grow-only device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "wh_common.h"

// what wh_last_error returns: one string per thread for the whole library
inline std::string& wh_error() {
  static thread_local std::string err;
  return err;
}
inline int fail(int code, const std::string& msg) { wh_error() = msg; return code; }

#define HIPCHK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return fail(-100, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

#define TRY(expr) do { int rc_ = (expr); if (rc_ != 0) return rc_; } while (0)

// A launch error (or any HIP error left pending) surfaces at the next hipGetLastError():
// report it with the launch that raised it (tuning build: wh_launched checked every launch)
// or, in the shipped build, the last launch before the check (wh_common.h)
inline int launch_status(const char* where) {
  const hipError_t e = hipGetLastError();
  std::string& first = wh_first_launch_error();
  if (e == hipSuccess && first.empty()) return 0;
  std::string msg = std::string(where) + ": ";
  if (!first.empty()) msg += first;
  else msg += std::string(hipGetErrorString(e)) + " (raised at or before the launch of " + wh_last_launch() + ")";
  first.clear();
  return fail(-100, msg);
}

// A context's destructor checks every release: the first failure is kept and reported by
// wh_destroy instead of staying pending for the next context's first call
struct Releases {
  std::string first;
  void operator()(hipError_t e, const char* what) {
    if (e != hipSuccess && first.empty()) first = std::string(what) + ": " + hipGetErrorString(e);
  }
};

// Stage timing on one stream: marks 0, 1 (and 2, for two stages back to back) around the
// work, then, once the stream has been waited for, charge(i, counter) adds the ms between
// marks i and i + 1 to a stage counter.
struct Timer {
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int create() { for (auto& e : ev) HIPCHK(hipEventCreate(&e)); return 0; }
  int mark(int i, hipStream_t st) { HIPCHK(hipEventRecord(ev[i], st)); return 0; }
  int charge(int i, double& counter) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
    counter += ms;
    return 0;
  }
  // the usual whole after mark(0): the end mark, the wait for it, the launch check of
  // `where` (if given) and the interval charged
  int finish(hipStream_t st, double& counter, const char* where = nullptr) {
    TRY(mark(1, st));
    HIPCHK(hipStreamSynchronize(st));
    if (where) TRY(launch_status(where));
    return charge(0, counter);
  }
  void release(Releases& rel) {
    for (auto& e : ev)
      if (e) rel(hipEventDestroy(e), "hipEventDestroy(timer)");
  }
};

// Grow-only device buffer: reserve() leaves at least `bytes` behind p.  The capacity is
// published only after the allocation succeeded; when one fails the buffer is empty.
template <typename P>
struct DevBuf {
  P* p = nullptr;
  size_t cap = 0;  // bytes
  // the contents are not kept: the old block is freed first, so the peak is the new size
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    P* old = std::exchange(p, nullptr);
    cap = 0;
    if (old) HIPCHK(hipFree(old));
    P* q = nullptr;
    HIPCHK(hipMalloc(&q, bytes));
    p = q;
    cap = bytes;
    return 0;
  }
  // the first `keep` bytes survive the move to a larger block (which must exist before
  // the old one goes: a failed allocation leaves the buffer as it was)
  int reserve(size_t bytes, size_t keep, hipStream_t st) {
    if (bytes <= cap) return 0;
    P* q = nullptr;
    HIPCHK(hipMalloc(&q, bytes));
    if (keep && p) {
      HIPCHK(hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    std::swap(p, q);
    cap = bytes;
    if (q) HIPCHK(hipFree(q));
    return 0;
  }
  void release(Releases& rel, const char* what) {
    if (p) rel(hipFree(p), what);
    p = nullptr;
    cap = 0;
  }
};
