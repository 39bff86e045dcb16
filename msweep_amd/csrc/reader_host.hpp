// reader_host.hpp -- what the device reader keeps on the handle between calls (host types only: no kernel), so that
// handle.hpp can hold them without the kernels of reader_kernels.hpp.
#pragma once
#include "common.hpp"

#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>

namespace msw {

// ---- host: pinned staging of the text on its way to the device (host_reader.inc) ------------------------------------------
// Every reader thread streams its own interleaved share of the file -- blocks k, k + T, k + 2 T, ... -- through two
// pinned sub-buffers of its own: pread, hipMemcpyAsync, the next block into the other sub-buffer while this one
// travels.  No meeting point between the threads (a gang that filled ONE staging chunk together and was started per
// chunk paid ~0.3 ms of thread start-up per 32 MB).  Owned by the handle: pinning costs ~0.4 ms per MB, once.
struct TextStager {
  size_t block = 0, threads = 0;   // bytes per sub-buffer (MSWEEP_READER_BLOCK_MB, developer switch), threads it is laid out for
  void *pinned = nullptr;          // 2 * threads * block bytes
  std::vector<hipEvent_t> ev;      // [2 * threads]: the copy that last read a sub-buffer
  hipStream_t copy = nullptr;      // the text travels on a stream of its own: the next strand's under this strand's kernels
  size_t block_bytes() {
    if (!block) {
      const char *e = getenv("MSWEEP_READER_BLOCK_MB");
      const long mb = e ? atol(e) : 0;
      block = (size_t)(mb >= 1 && mb <= 256 ? mb : 4) << 20;  // (1-2 MB: the fixed cost per copy shows; 4-8 MB alike)
    }
    return block;
  }
  void ready(size_t T) {
    (void)block_bytes();
    if (T > threads) {
      release();
      MSW_HIP(hipHostMalloc(&pinned, 2 * T * block, hipHostMallocDefault));
      ev.assign(2 * T, nullptr);
      for (auto &e : ev) MSW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      threads = T;
    }
    if (!copy) MSW_HIP(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
  }
  char *sub(size_t thread, int slot) const { return static_cast<char *>(pinned) + (2 * thread + slot) * block; }
  void release() {
    if (pinned) (void)hipHostFree(pinned);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
    pinned = nullptr;
    ev.clear();
    threads = 0;
  }
  ~TextStager() {
    release();
    if (copy) (void)hipStreamDestroy(copy);
  }
};

// Device memory of the reader, kept on the handle between calls.  Two facts of the runtime shape it: hipFree waits for
// EVERY stream of the device (also the copy stream that carries the next strand's text), and memory given back is
// scrubbed by the driver before it is handed out again -- ~10 GB of temporaries at cfg3 stalled the allocations of
// the likelihood build that follows by 0.2 s (tools/reader_probe.py: 0.230 s, 0.021 s after a pause).  So nothing is
// freed while the handle lives: blocks handed back during a call become reusable from the NEXT call on (no ordering
// question between the streams of one call), a second read of the same size allocates nothing, and msw_core_trim /
// msw_core_destroy give the memory back.
struct ReaderPool {
  std::mutex mu;
  std::multimap<size_t, void *> idle;        // reusable blocks by size
  std::unordered_map<void *, size_t> live;   // blocks handed out (and those handed back during this call)
  std::vector<void *> returned;
  size_t bytes = 0;
  void *take(size_t need) {
    {
      std::lock_guard<std::mutex> g(mu);
      auto it = idle.lower_bound(need);
      if (it != idle.end() && it->first <= need + need / 2 + (1u << 20)) {
        void *p = it->second;
        live[p] = it->first;
        idle.erase(it);
        return p;
      }
    }
    void *p = nullptr;
    MSW_HIP(hipMalloc(&p, need));
    std::lock_guard<std::mutex> g(mu);
    live[p] = need;
    bytes += need;
    return p;
  }
  void give(void *p) {
    std::lock_guard<std::mutex> g(mu);
    returned.push_back(p);
  }
  void recycle() {  // between calls: what was handed back may be handed out again
    std::lock_guard<std::mutex> g(mu);
    for (void *p : returned) {
      auto it = live.find(p);
      if (it == live.end()) continue;
      idle.emplace(it->second, p);
      live.erase(it);
    }
    returned.clear();
  }
  size_t idle_bytes() {
    std::lock_guard<std::mutex> g(mu);
    size_t b = 0;
    for (auto &kv : idle) b += kv.first;
    return b;
  }
  void trim() {  // every idle block back to the device
    recycle();
    std::lock_guard<std::mutex> g(mu);
    for (auto &kv : idle) {
      (void)hipFree(kv.second);
      bytes -= kv.first;
    }
    idle.clear();
  }
  ~ReaderPool() {
    trim();
    for (auto &kv : live) (void)hipFree(kv.first);
  }
};

}  // namespace msw
