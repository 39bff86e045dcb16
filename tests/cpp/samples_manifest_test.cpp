// samples_manifest_test.cpp -- msweep_amd/cpp/samples_manifest.hpp and msweep_amd/csrc/lds_grants.hpp stand alone: no
// device, no library.  `parse FILE bin_reads(0|1)` prints the manifest as the parser read it, or its refusal, for
// tests/test_samples_flags_cpu.py to hold against msweep_amd/samples.py; without arguments the queue and the LDS table
// run on several threads (built with -fsanitize=thread, or address,undefined, by the same test).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "lds_grants.hpp"
#include "samples_manifest.hpp"

#define REQUIRE(c)                                              \
  do {                                                          \
    if (!(c)) {                                                 \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                 \
    }                                                           \
  } while (0)

static int parse(const char *path, bool bin_reads) {
  try {
    const auto samples = msw_samples::read_manifest(path);
    msw_samples::check_samples(path, samples, bin_reads);
    for (const auto &s : samples) {
      printf("%zu\t%s\t", s.line, s.prefix.c_str());
      for (size_t i = 0; i < s.files.size(); ++i) printf("%s%s", i ? "," : "", s.files[i].c_str());
      if (s.have_fastqs) {
        printf("\t");
        for (size_t i = 0; i < s.fastqs.size(); ++i) printf("%s%s", i ? "," : "", s.fastqs[i].c_str());
      }
      printf("\n");
    }
  } catch (const msw_samples::ManifestError &ex) {
    printf("refused: %s\n", ex.what());
  }
  return 0;
}

// 8 workers over 1000 samples; sample 400 fails: every sample up to it ran exactly once, none twice, and what ran behind
// it -- the samples in flight when it failed -- continues the manifest without a gap
static int queue_threads() {
  constexpr size_t kN = 1000, kBad = 400, kT = 8;
  msw_samples::Queue q(kN);
  std::vector<std::atomic<int>> ran(kN);
  for (auto &r : ran) r = 0;
  std::vector<std::thread> pool;
  for (size_t t = 0; t < kT; ++t)
    pool.emplace_back([&] {
      size_t i = 0;
      while (q.next(i)) {
        ++ran[i];
        q.done(i != kBad);
      }
    });
  for (auto &th : pool) th.join();
  size_t started = 0;
  for (size_t i = 0; i < kN; ++i) {
    REQUIRE(ran[i] <= 1);
    if (i <= kBad) REQUIRE(ran[i] == 1);
    if (i > 0 && ran[i]) REQUIRE(ran[i - 1] == 1);  // handed out in manifest order: what ran is a prefix of the manifest
    started += (size_t)ran[i];
  }
  REQUIRE(q.failed() == 1 && q.finished() + q.failed() == started && q.not_started() == kN - started);
  msw_samples::Queue all(5);
  size_t i = 0, n = 0;
  while (all.next(i)) {
    REQUIRE(i == n++);
    all.done(true);
  }
  REQUIRE(n == 5 && all.finished() == 5 && all.failed() == 0 && all.not_started() == 0);
  printf("queue: ok\n");
  return 0;
}

// 8 threads ask for limits of 4 kernels on 2 devices in every order: a limit is only ever raised, set() runs under the
// lock, a set that throws leaves the table as it was
static int grants_threads() {
  msw::LdsGrants g;
  static int kernels[4];
  size_t limit[2][4] = {};  // what the "runtime" holds: written by set() only
  std::atomic<int> lowered{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < 8; ++t)
    pool.emplace_back([&, t] {
      for (int r = 0; r < 2000; ++r) {
        const int d = (r + t) & 1, k = (r * 7 + t) & 3;
        const size_t want = (size_t)(((r * 2654435761u) >> 8) % 160) * 1024 + 1;
        g.raise(d, &kernels[k], want, [&](size_t b) {
          if (b <= limit[d][k]) ++lowered;
          limit[d][k] = b;
        });
        // (what a launch relies on: the limit is at least what this thread was granted)
        std::lock_guard<std::mutex> lk(g.mu);
        if (limit[d][k] < want) ++lowered;
      }
    });
  for (auto &th : pool) th.join();
  REQUIRE(lowered == 0);
  bool thrown = false;
  try {
    g.raise(0, &kernels[0], (size_t)1 << 30, [&](size_t) { throw std::runtime_error("refused"); });
  } catch (const std::runtime_error &) {
    thrown = true;
  }
  const size_t kept = g.granted[std::make_pair(0, (const void *)&kernels[0])];
  REQUIRE(thrown && kept == limit[0][0]);
  printf("lds grants: ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "parse") return parse(argv[2], atoi(argv[3]) != 0);
  if (queue_threads() || grants_threads()) return 1;
  REQUIRE(msw_samples::normal_path("./a//b/../c/") == "a/c" && msw_samples::normal_path("/../x") == "/x" &&
          msw_samples::normal_path("../x") == "../x" && msw_samples::bin_dir("p") == "" && msw_samples::bin_dir("./p") == "" &&
          msw_samples::bin_dir("a/p") == "a" && msw_samples::bin_dir("/p") == "/");
  printf("samples manifest: ok\n");
  return 0;
}
