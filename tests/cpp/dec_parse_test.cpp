// dec_parse_test.cpp -- the host build of msweep_amd/csrc/dec_parse.hpp against glibc's strtod
// (tests/test_dec_parse_cpu.py): every token the parser DECIDES has strtod's bits; what lies outside Clinger's exact
// case is never decided; inside it, always; malformed tokens are bad.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dec_parse.hpp"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64 (the generators of g6_format_test.cpp)
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
  size_t n = 0, wrong = 0, undecided = 0, decided = 0, bad = 0;
};

// Clinger's case, restated on the token's characters (no arithmetic shared with the header): mantissa digits without
// the point and without leading zeros, at most 16 of them and as a decimal string <= "9007199254740992"; the exponent
// minus the number of fraction digits within [-22, 22].  Only called for well-formed numeric tokens.
bool in_fast_domain(const std::string &tok) {
  size_t p = tok[0] == '-' ? 1 : 0;
  std::string digits;
  long frac = 0;
  bool point = false;
  for (; p < tok.size() && tok[p] != 'e'; ++p) {
    if (tok[p] == '.') {
      point = true;
      continue;
    }
    digits += tok[p];
    frac += point;
  }
  long ex = 0;
  if (p < tok.size()) ex = strtol(tok.c_str() + p + 1, nullptr, 10);
  const size_t nz = digits.find_first_not_of('0');
  digits = nz == std::string::npos ? "" : digits.substr(nz);
  const std::string lim = "9007199254740992";
  const bool small = digits.size() < lim.size() || (digits.size() == lim.size() && digits <= lim);
  const long k = ex - frac;
  return small && k >= -22 && k <= 22;
}

// numeric: the token is a well-formed number (not one of the words)
void check(const std::string &tok, bool numeric, Tally &t) {
  double got = 0.0;
  const int r = msw::dec::parse_cell(msw::dec::Bytes{reinterpret_cast<const unsigned char *>(tok.data())}, (int)tok.size(), &got);
  ++t.n;
  if (r == msw::dec::kBad) {
    ++t.bad;
    printf("MISMATCH well-formed token called bad: %s\n", tok.c_str());
    ++t.wrong;
    return;
  }
  char *end = nullptr;
  const double want = strtod(tok.c_str(), &end);
  if (end != tok.c_str() + tok.size()) {
    printf("MISMATCH strtod stops inside %s\n", tok.c_str());
    ++t.wrong;
    return;
  }
  if (r == msw::dec::kUndecided) {
    ++t.undecided;
    if (numeric && in_fast_domain(tok)) {
      if (t.wrong < 20) printf("MISMATCH undecided inside the fast domain: %s\n", tok.c_str());
      ++t.wrong;
    }
    return;
  }
  ++t.decided;
  if (numeric && !in_fast_domain(tok)) {
    if (t.wrong < 20) printf("MISMATCH decided outside the fast domain: %s\n", tok.c_str());
    ++t.wrong;
  }
  if (bits_of(got) != bits_of(want)) {
    if (t.wrong < 20)
      printf("MISMATCH %s want=%016llx got=%016llx\n", tok.c_str(), (unsigned long long)bits_of(want), (unsigned long long)bits_of(got));
    ++t.wrong;
  }
  // the kernels' form of the same bytes: three little-endian words
  msw::dec::Words24 w = {0, 0, 0};
  unsigned char buf[24] = {0};
  std::memcpy(buf, tok.data(), tok.size());
  std::memcpy(&w.w0, buf, 8), std::memcpy(&w.w1, buf + 8, 8), std::memcpy(&w.w2, buf + 16, 8);
  double got2 = 0.0;
  if (msw::dec::parse_cell(w, (int)tok.size(), &got2) != r || bits_of(got2) != bits_of(got)) {
    printf("MISMATCH the word getter differs on %s\n", tok.c_str());
    ++t.wrong;
  }
}

bool report(const char *name, const Tally &t, bool pass) {
  printf("%s: tokens=%zu wrong=%zu decided=%zu undecided=%zu %s\n", name, t.n, t.wrong, t.decided, t.undecided, pass ? "ok" : "FAILED");
  return pass;
}

}  // namespace

int main() {
  bool ok = true;
  // ---- adversarial: (token, expectation) with 'd' decided, 'u' undecided ----
  {
    struct Case {
      const char *tok;
      char want;
      bool numeric;
    };
    const Case cases[] = {
        {"0", 'd', true}, {"-0", 'd', true}, {"1e22", 'd', true}, {"1e-22", 'd', true}, {"9007199254740992", 'd', true},
        {"9007199254740993", 'u', true}, {"1e23", 'u', true}, {"1e-23", 'u', true}, {"4.9e-324", 'u', true},
        {"1.79769e+308", 'u', true}, {"1e400", 'u', true}, {"inf", 'd', false}, {"-inf", 'd', false}, {"nan", 'd', false},
        {"-nan", 'd', false}, {"-4.60517", 'd', true}, {"1e-05", 'd', true}, {"1e+06", 'd', true}, {"123456789012345", 'd', true},
        {"0.000000000000000000001", 'd', true}, {"000000000000000000000001", 'd', true}, {"9007199254740992e22", 'd', true},
        {"9007199254740992e-22", 'd', true}, {"90071992547409920", 'u', true}, {"0e400", 'u', true}, {"-2.5e-320", 'u', true},
        {"12345678901234567890", 'u', true}, {"0.30000000000000004", 'u', true}, {"1.0e+00", 'd', true},
    };
    Tally t;
    for (const Case &c : cases) {
      const size_t d0 = t.decided, u0 = t.undecided;
      check(c.tok, c.numeric, t);
      const char was = t.decided > d0 ? 'd' : (t.undecided > u0 ? 'u' : 'b');
      if (was != c.want) {
        printf("MISMATCH %s: expected %c, was %c\n", c.tok, c.want, was);
        ++t.wrong;
      }
    }
    ok &= report("adversarial", t, t.wrong == 0);
  }
  // ---- malformed: every one bad ----
  {
    const char *bad[] = {"", "-", "+1", "+inf", ".", ".5", "5.", "1.e5", "1e", "1e+", "1e-", "e5", "1E5", "Inf", "INF", "NaN", "nan(1)",
                         "infinity", "-infinity", "0x10", "1_0", " 1", "1 ", "1..2", "1.2.3", "1e5e5", "1e+-5", "--1", "-+1", "1-", "1+",
                         "in", "na", "nanx", "1e5.0", "\t1", "1\n", "1,5", "1d5", "-.5", "1234567890123456789012345"};
    Tally t;
    for (const char *b : bad) {
      double v;
      ++t.n;
      const std::string tok = b;
      if (msw::dec::parse_cell(msw::dec::Bytes{reinterpret_cast<const unsigned char *>(tok.data())}, (int)tok.size(), &v) != msw::dec::kBad) {
        printf("MISMATCH malformed token accepted: '%s'\n", b);
        ++t.wrong;
      }
    }
    // the count column: 1 to 18 digits
    uint64_t c = 0;
    auto count = [&](const char *s) { return msw::dec::parse_count(msw::dec::Bytes{reinterpret_cast<const unsigned char *>(s)}, (int)strlen(s), &c); };
    t.n += 6;
    if (count("0") != msw::dec::kDecided || c != 0) ++t.wrong;
    if (count("007") != msw::dec::kDecided || c != 7) ++t.wrong;
    if (count("999999999999999999") != msw::dec::kDecided || c != 999999999999999999ull) ++t.wrong;
    if (count("1000000000000000000") != msw::dec::kBad) ++t.wrong;
    if (count("+5") != msw::dec::kBad || count("-5") != msw::dec::kBad || count("") != msw::dec::kBad) ++t.wrong;
    if (count("1.0") != msw::dec::kBad || count("1e3") != msw::dec::kBad) ++t.wrong;
    ok &= report("malformed", t, t.wrong == 0);
  }
  // ---- "%g" of 2 M random doubles from the four generators of g6_format_test.cpp ----
  {
    const size_t per = 500000;
    Tally rnd[4];
    const char *names[4] = {"random_bits", "uniform", "exp(-745U)", "-50U"};
    char buf[64];
    for (size_t i = 0; i < per; ++i) {
      uint64_t b;
      do b = next_u64();
      while (((b >> 52) & 0x7ff) == 0x7ff);
      double x;
      std::memcpy(&x, &b, sizeof x);
      const double xs[4] = {x, next_unit(), std::exp(-745.0 * next_unit()), -50.0 * next_unit()};
      for (int g = 0; g < 4; ++g) {
        snprintf(buf, sizeof buf, "%g", xs[g]);
        check(buf, true, rnd[g]);
      }
    }
    for (int g = 0; g < 4; ++g) ok &= report(names[g], rnd[g], rnd[g].wrong == 0);
    // log-likelihoods as the files hold them: every one decided here
    if (rnd[3].undecided * 1000 > rnd[3].n) ok = false, printf("FAILED -50U: too many undecided\n");
  }
  // ---- 1 M tokens inside the fast domain: 1-15 digits, a point anywhere, an exponent that keeps |k| <= 22: zero undecided ----
  {
    Tally t;
    char buf[64];
    for (size_t i = 0; i < 1000000; ++i) {
      const int nd = 1 + (int)(next_u64() % 15);
      std::string digits;
      for (int d = 0; d < nd; ++d) digits += (char)('0' + next_u64() % 10);
      const int frac = (int)(next_u64() % (uint64_t)nd);   // digits behind the point (0: no point)
      const int k = (int)(next_u64() % 45) - 22;           // the decimal exponent of the integer the digits form
      const int ex = k + frac;
      std::string tok = next_u64() & 1 ? "-" : "";
      tok += digits.substr(0, (size_t)(nd - frac));
      if (frac) tok += "." + digits.substr((size_t)(nd - frac));
      const unsigned form = (unsigned)(next_u64() % 3);
      if (ex != 0 || form == 0) {
        snprintf(buf, sizeof buf, form == 1 ? "e%d" : "e%+03d", ex);
        tok += buf;
      }
      if (tok.size() > 24) continue;
      check(tok, true, t);
    }
    ok &= report("fast_domain", t, t.wrong == 0 && t.undecided == 0 && t.n > 900000);
  }
  if (!ok) printf("FAILED\n");
  return ok ? 0 : 1;
}
