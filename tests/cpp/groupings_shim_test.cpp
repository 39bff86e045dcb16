// msw::DeviceLikelihood::read_files + build_from_alignment: the C++ face of the reference's grouping loop
// (src/mSWEEP.cpp:282) -- ONE read in front of the loop, one build per column of the -i file -- against
// build_from_files per column on objects of their own.
//   groupings_shim_test <min_hits> path...      stdin: T K; then per column: G; target_group[T]; group_sizes[G]
// Prints per column `loop <k> <theta as hex floats>` (the one object, columns in order, then column 0 once more as
// `again 0 ...`) and `files <k> <theta as hex floats>` (a fresh object per column through build_from_files).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../msweep_amd/cpp/rcgpar_hip.hpp"

namespace {
struct Column {
  std::vector<uint32_t> tg;
  std::vector<uint64_t> sizes;
};

void print_theta(const char *what, size_t k, msw::DeviceLikelihood &lik) {
  std::vector<double> alpha(lik.n_groups(), 1.0);
  const msw::Estimate est = msw::solve(lik, {}, alpha, 1e-6, 5000, MSW_ALGO_RCG, MSW_PREC_DOUBLE, nullptr);
  std::printf("%s %zu", what, k);
  for (double t : est.theta) std::printf(" %a", t);
  std::printf("\n");
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const size_t min_hits = (size_t)std::atoll(argv[1]);
  const std::vector<std::string> paths(argv + 2, argv + argc);
  size_t T = 0, K = 0;
  if (!(std::cin >> T >> K)) return 2;
  std::vector<Column> cols(K);
  for (Column &c : cols) {
    size_t G = 0;
    if (!(std::cin >> G)) return 2;
    c.tg.resize(T);
    c.sizes.resize(G);
    for (auto &x : c.tg) std::cin >> x;
    for (auto &x : c.sizes) std::cin >> x;
  }
  try {
    {
      msw::DeviceLikelihood lik(0);
      lik.read_files(paths, false, T);
      std::printf("n_ecs %zu\nn_reads %zu\nn_aligned %zu\n", lik.ec_counts().size(), lik.n_reads(), lik.n_aligned());
      for (size_t k = 0; k < K; ++k) {
        lik.build_from_alignment(cols[k].tg, cols[k].sizes, 0.65, 0.01, min_hits, 0.01);
        print_theta("loop", k, lik);
      }
      lik.build_from_alignment(cols[0].tg, cols[0].sizes, 0.65, 0.01, min_hits, 0.01);
      print_theta("again", 0, lik);
      lik.release_alignment();
      bool refused = false;
      try {
        lik.build_from_alignment(cols[0].tg, cols[0].sizes, 0.65, 0.01, min_hits, 0.01);
      } catch (const std::exception &) {
        refused = true;
      }
      std::printf("released %d\n", refused ? 1 : 0);
    }
    for (size_t k = 0; k < K; ++k) {
      msw::DeviceLikelihood lik(0);
      lik.build_from_files(paths, false, cols[k].tg, cols[k].sizes, 0.65, 0.01, min_hits, 0.01);
      print_theta("files", k, lik);
    }
  } catch (const std::exception &ex) {
    std::printf("exception %s\n", ex.what());
    return 1;
  }
  return 0;
}
