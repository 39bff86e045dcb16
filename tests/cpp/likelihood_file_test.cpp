// msw::DeviceLikelihood::from_file (msweep_amd/cpp/rcgpar_hip.hpp), the mirror of LL_WOR21::from_file
// (include/Likelihood.hpp:224-253): `likelihood_file_test <file> <n_groups>` reads the file twice -- parsed on the device,
// and, under MSWEEP_HOST_LIKELIHOOD_FILE=1, cell by cell on the host and uploaded as a matrix -- and prints both estimates
// (tests/test_gpu_likelihood_file.py).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../msweep_amd/cpp/rcgpar_hip.hpp"

static void report(const char *tag, msw::DeviceLikelihood &lik) {
  std::vector<double> alpha(lik.n_groups(), 1.0);
  msw::Estimate est = msw::solve(lik, lik.log_counts(), alpha, 1e-6, 5000, MSW_ALGO_RCG, MSW_PREC_DOUBLE, nullptr);
  std::printf("iters_%s %zu\ntheta_%s", tag, est.iters, tag);
  for (double t : est.theta) std::printf(" %.17g", t);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const std::string path = argv[1];
  const size_t G = (size_t)std::atoll(argv[2]);
  try {
    msw::DeviceLikelihood a(0), b(0);
    unsetenv("MSWEEP_HOST_LIKELIHOOD_FILE");
    a.from_file(path, G);
    std::printf("served %d\nn_ecs %zu\nn_reads %zu\n", a.parsed_on_device() ? 1 : 0, a.n_ecs(), a.n_reads());
    report("file", a);
    setenv("MSWEEP_HOST_LIKELIHOOD_FILE", "1", 1);
    b.from_file(path, G);
    std::printf("served_matrix %d\n", b.parsed_on_device() ? 1 : 0);
    report("matrix", b);
  } catch (const std::exception &ex) {
    std::printf("exception %s\n", ex.what());
    return 1;
  }
  return 0;
}
