// lds_grants.hpp -- the dynamic-LDS limits the library has asked for, process wide (host types only: no kernel, no HIP).
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel on a device, not to a handle: a handle that remembered
// only its own requests would LOWER the limit under another handle whose likelihood needs more (two handles in one
// process: a larger sample after a smaller one on the other worker), and two threads could set and launch in between each
// other.  So every request goes through one table that only ever raises a limit: a launch whose LDS was granted once stays
// within the limit whatever other handles ask for later.  tests/cpp/lds_grants_test.cpp runs it under ThreadSanitizer.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <utility>

namespace msw {

struct LdsGrants {
  std::mutex mu;
  std::map<std::pair<int, const void *>, size_t> granted;  // (device, kernel) -> bytes
  // The limit of `kernel` on `device` becomes at least `bytes`: set(bytes) is called, under the lock, only when it grows;
  // a set that throws leaves the table as it was.
  template <class Set>
  void raise(int device, const void *kernel, size_t bytes, Set &&set) {
    std::lock_guard<std::mutex> g(mu);
    auto it = granted.find({device, kernel});
    if (it != granted.end() && bytes <= it->second) return;
    set(bytes);
    granted[{device, kernel}] = bytes;
  }
};

}  // namespace msw
