// g6_format_test.cpp -- the host build of msweep_amd/csrc/g6_format.hpp against glibc's snprintf("%g")
// (tests/test_g6_format_cpu.py).  `--table` prints the power-of-ten table, one "k P q" per line.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "g6_format.hpp"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
double next_unit() { return (double)(next_u64() >> 11) * 0x1p-53; }

uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

struct Tally {
  size_t n = 0, wrong = 0, undecided = 0;
};

// the routine's own decision against snprintf; an undecided value counts as such and is then checked through
// format_host, the path the library takes for it
void check(double x, Tally &t) {
  const uint64_t bits = bits_of(x);
  char want[32], got[32];
  const int wl = snprintf(want, sizeof want, "%g", x);
  msw::g6::Text tx;
  const msw::g6::Class c = msw::g6::format(bits, tx);
  ++t.n;
  if (c == msw::g6::kUndecided) ++t.undecided;
  bool by_snprintf = false;
  const int gl = msw::g6::format_host(bits, got, &by_snprintf);
  if (by_snprintf != (c == msw::g6::kUndecided) || gl != wl || std::memcmp(want, got, (size_t)wl) != 0) {
    if (t.wrong < 20) printf("MISMATCH bits=%016llx want=%s got=%.*s\n", (unsigned long long)bits, want, gl, got);
    ++t.wrong;
  }
}

void report(const char *name, const Tally &t, bool pass) {
  printf("%s: values=%zu wrong=%zu undecided=%zu%s\n", name, t.n, t.wrong, t.undecided, pass ? " ok" : " FAILED");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "--table") {
    for (int k = msw::g6::kKmin; k <= msw::g6::kKmax; ++k)
      printf("%d %llu %d\n", k, (unsigned long long)msw::g6::kPow10[k - msw::g6::kKmin].P, (int)msw::g6::kPow10[k - msw::g6::kKmin].q);
    return 0;
  }
  bool all = true;

  // ---- the adversarial list
  Tally adv;
  {
    const double inf = INFINITY;
    std::vector<double> v = {0.0, -0.0, 0.5, 1.0, 100000.0, 1e6, 123456.7, 0.0001, 1e-5, 0.9999995, 0.99999951, 999999.5,
                             999999.4999999999, 9.9999995e-5, 0.000099999949, 5e-324, DBL_MIN, DBL_MAX, inf, -inf,
                             std::nan(""), -std::nan("")};
    for (int k = -323; k <= 308; ++k) {
      const double p = std::strtod(("1e" + std::to_string(k)).c_str(), nullptr);
      v.push_back(p);
      v.push_back(std::nextafter(p, 0.0));
      v.push_back(std::nextafter(p, inf));
      v.push_back(-p);
    }
    for (double x : v) check(x, adv);
    const bool pass = adv.wrong == 0;
    all &= pass;
    report("adversarial", adv, pass);
  }

  // ---- 18 000 exact ties inside the range the routine resolves itself: odd m, value = m 2^-(6 - X) in [10^X, 10^(X+1))
  Tally ties;
  for (int X = -3; X <= 5; ++X) {
    const double unit = std::ldexp(1.0, -(6 - X)), lo = std::pow(10.0, X), hi = std::pow(10.0, X + 1);
    const uint64_t m0 = (uint64_t)std::ceil(lo / unit) | 1, m1 = (uint64_t)std::floor(hi / unit);
    for (int i = 0; i < 2000; ++i) {
      const uint64_t m = (m0 + 2 * (next_u64() % ((m1 - m0) / 2))) | 1;
      const double x = (double)m * unit;  // exact: m < 2^24
      if (!(x >= lo && x < hi)) {
        printf("MISMATCH bad tie construction\n");
        all = false;
      }
      check(i & 1 ? -x : x, ties);
    }
  }
  {
    const bool pass = ties.wrong == 0 && ties.undecided == 0 && ties.n == 18000;
    all &= pass;
    report("ties", ties, pass);
  }

  // ---- ties above 1e6, where the power of ten is not exact: (2 N + 1) 5 10^j, all must be left to snprintf or be right
  Tally big;
  for (int j = 0; j <= 8; ++j)
    for (int i = 0; i < 200; ++i) {
      const uint64_t N = 100000 + next_u64() % 900000;
      check((double)((2 * N + 1) * 5) * std::pow(10.0, j), big);  // < 2^53: exact
    }
  {
    const bool pass = big.wrong == 0;
    all &= pass;
    report("ties_above_1e6", big, pass);
  }

  // ---- 2 M random values from four generators; at most 1 in 10 000 may be left undecided
  const size_t per = 500000;
  Tally rnd[4];
  const char *names[4] = {"random_bits", "uniform", "exp(-745U)", "-50U"};
  for (size_t i = 0; i < per; ++i) {
    uint64_t b;
    do b = next_u64();
    while (((b >> 52) & 0x7ff) == 0x7ff);  // finite
    double x;
    std::memcpy(&x, &b, sizeof x);
    check(x, rnd[0]);
    check(next_unit(), rnd[1]);
    check(std::exp(-745.0 * next_unit()), rnd[2]);
    check(-50.0 * next_unit(), rnd[3]);
  }
  for (int g = 0; g < 4; ++g) {
    const bool pass = rnd[g].wrong == 0 && rnd[g].undecided * 10000 <= rnd[g].n;
    all &= pass;
    report(names[g], rnd[g], pass);
  }
  return all ? 0 : 1;
}
