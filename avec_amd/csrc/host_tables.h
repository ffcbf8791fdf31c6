// Host-side bookkeeping behind api.hip, free of HIP so that it can be compiled and raced on its own (tests/host_tables_main.cpp):
// the reduction-workspace registry and the table of dynamic-LDS opt-ins.  Streams and kernels are opaque addresses, devices are ints.
// Entry points may be called from any thread (the autograd thread makes the first backward call): every read and write takes the mutex.
// Both classes stay out of the shared library's exported symbols.
#pragma once
#include <stddef.h>
#include <mutex>
#include <vector>

// Reduction workspaces (vec.h, two-pass column reductions): one default per device plus a few bound to specific streams.
class __attribute__((visibility("hidden"))) WsRegistry {
 public:
  static constexpr int MAX_DEV = 64, MAX_STREAMS = 4;
  // (nullptr, 0) unregisters; false: no such device
  bool set_default(int dev, void* base, size_t bytes) {
    if (dev < 0 || dev >= MAX_DEV) return false;
    std::lock_guard<std::mutex> g(mu_);
    def_[dev] = Buf{base, bytes};
    return true;
  }
  // replaces the entry of (dev, stream) in place; false: MAX_STREAMS other entries exist
  bool set_stream(int dev, const void* stream, void* base, size_t bytes) {
    std::lock_guard<std::mutex> g(mu_);
    for (int i = 0; i < nbound_; ++i) if (bound_[i].stream == stream && bound_[i].dev == dev) { bound_[i].buf = Buf{base, bytes}; return true; }
    if (nbound_ == MAX_STREAMS) return false;
    bound_[nbound_++] = Bound{stream, dev, Buf{base, bytes}};
    return true;
  }
  // the workspace a launch on (dev, stream) may use for `bytes`: a stream-bound entry wins, and one that is too small yields none
  // (the default may be in use by the stream it serves); else the device default when large enough; else nullptr
  void* find(int dev, const void* stream, size_t bytes) const {
    if (dev < 0 || dev >= MAX_DEV) return nullptr;
    std::lock_guard<std::mutex> g(mu_);
    for (int i = 0; i < nbound_; ++i) if (bound_[i].stream == stream && bound_[i].dev == dev) return bytes <= bound_[i].buf.bytes ? bound_[i].buf.base : nullptr;
    return bytes <= def_[dev].bytes ? def_[dev].base : nullptr;
  }

 private:
  struct Buf { void* base = nullptr; size_t bytes = 0; };
  struct Bound { const void* stream; int dev; Buf buf; };
  mutable std::mutex mu_;
  Buf def_[MAX_DEV];
  Bound bound_[MAX_STREAMS];
  int nbound_ = 0;
};

// Dynamic LDS above 48 KB must be granted per kernel AND device before a launch.  The table remembers the largest size granted to every
// (device, kernel), so `set` (the HIP call) runs only when a request grows, and the last refusal, so a refused size costs no second call.
class __attribute__((visibility("hidden"))) LdsOptin {
 public:
  static constexpr size_t FREE_BYTES = 48 * 1024, MAX_BYTES = 160 * 1024;
  static constexpr int TOO_LARGE = -1;
  // 0: a launch with `bytes` of dynamic LDS may go ahead; TOO_LARGE: more than the CU has; else the code `set(kernel, bytes)` returned
  // when it refused this size (or a smaller one).  `set` returns 0 on success and runs under the mutex.
  template <typename Set> int request(int dev, const void* kernel, size_t bytes, Set&& set) {
    if (bytes > MAX_BYTES) return TOO_LARGE;
    if (bytes <= FREE_BYTES) return 0;
    std::lock_guard<std::mutex> g(mu_);
    Entry* e = nullptr;
    for (Entry& x : tab_) if (x.kernel == kernel && x.dev == dev) { e = &x; break; }
    if (!e) { tab_.push_back(Entry{kernel, dev, 0, 0, 0}); e = &tab_.back(); }
    if (bytes <= e->granted) return 0;
    if (e->refused_err && bytes >= e->refused_bytes) return e->refused_err;
    const int err = set(kernel, bytes);
    if (err) { e->refused_bytes = bytes; e->refused_err = err; } else e->granted = bytes;
    return err;
  }

 private:
  struct Entry { const void* kernel; int dev; size_t granted, refused_bytes; int refused_err; };
  std::mutex mu_;
  std::vector<Entry> tab_;
};
