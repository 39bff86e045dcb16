// dec_parse.hpp -- a decimal token to the double strtod() returns for it, where one IEEE operation gives that double.
// One function for both sides, the way g6_format.hpp is: __host__ __device__ under hipcc (the likelihood-file kernels,
// likelihood_text_kernels.hpp), plain C++ under g++ (tests/cpp/dec_parse_test.cpp).
//
// A CELL of a likelihood file (include/Likelihood.hpp:224-253 reads what :255-273 wrote) is one of
//   inf  -inf  nan  -nan
//   -? digits (. digits)? (e [+-]? digits)?          at most kDecMaxToken bytes
// and nothing else: no blanks, no '+' in front of the mantissa, no upper case, no hexadecimal.  For exactly these
// tokens Python's float(), std::stod and strtod agree on the value.
//
// DECIDED here is Clinger's exact case (W. D. Clinger, "How to read floating point numbers accurately", PLDI 1990):
// the digits of the mantissa, leading zeros dropped and the point folded into the decimal exponent k, form an integer
// w <= 2^53, and |k| <= 22.  Then w and 10^|k| are both doubles, and w * 10^k (k >= 0) or w / 10^-k (k < 0) is ONE
// correctly rounded operation on two exact operands: the nearest double to the decimal value, which is what strtod
// returns.  The quotient is the plain `/` of a translation unit compiled without fast-math.  Every other well-formed
// token -- more digits, a larger exponent, whatever might round into the subnormals or overflow -- is UNDECIDED: the caller
// has strtod convert its bytes.  "%g" text of values with 1e-4 <= |x| < 1e6 has at most six digits and |k| <= 9.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MSW_DEC_HD __host__ __device__
#else
#define MSW_DEC_HD
#endif

namespace msw {
namespace dec {

constexpr int kDecided = 0, kUndecided = 1, kBad = 2;
constexpr int kDecMaxToken = 24;   // bytes of a cell
constexpr int kDecMaxCount = 18;   // digits of a line's first column

// byte d of a token held in three little-endian 64-bit words (the kernels' form: no indexed array of registers)
struct Words24 {
  uint64_t w0, w1, w2;
  MSW_DEC_HD unsigned operator()(int d) const { return (unsigned)(((d < 8 ? w0 : (d < 16 ? w1 : w2)) >> (8 * (d & 7))) & 0xffu); }
};
struct Bytes {
  const unsigned char *p;
  MSW_DEC_HD unsigned operator()(int d) const { return p[d]; }
};

// 10^k, 0 <= k <= 22: exact in a double
static constexpr double kPow10Exact[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                           1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
MSW_DEC_HD inline double pow10_exact(int k) { return kPow10Exact[k]; }
MSW_DEC_HD inline double from_bits(uint64_t b) {
  double d;
  __builtin_memcpy(&d, &b, sizeof d);
  return d;
}

// The first column: 1 to kDecMaxCount digits.  kDecided (*out = the count) or kBad.
template <class Get>
MSW_DEC_HD inline int parse_count(const Get &get, int len, uint64_t *out) {
  if (len < 1 || len > kDecMaxCount) return kBad;
  uint64_t v = 0;
  for (int d = 0; d < len; ++d) {
    const unsigned c = get(d) - '0';
    if (c > 9u) return kBad;
    v = v * 10 + c;
  }
  *out = v;
  return kDecided;
}

// A cell of len bytes.  kDecided: *out = strtod's double; kUndecided: well formed, outside Clinger's case; kBad.
template <class Get>
MSW_DEC_HD inline int parse_cell(const Get &get, int len, double *out) {
  if (len < 1 || len > kDecMaxToken) return kBad;
  int pos = 0;
  const bool neg = get(0) == '-';
  if (neg) pos = 1;
  const uint64_t sign = neg ? 0x8000000000000000ull : 0ull;
  if (len - pos == 3) {
    const unsigned a = get(pos), b = get(pos + 1), c = get(pos + 2);
    if (a == 'i' && b == 'n' && c == 'f') {
      *out = from_bits(sign | 0x7ff0000000000000ull);
      return kDecided;
    }
    if (a == 'n' && b == 'a' && c == 'n') {
      *out = from_bits(sign | 0x7ff8000000000000ull);
      return kDecided;
    }
  }
  // states: 0 mantissa, first digit due; 1 in the integer digits; 2 behind the point, digit due; 3 in the fraction;
  //         4 behind 'e', sign or digit due; 5 behind the sign, digit due; 6 in the exponent
  int st = 0, nd = 0, frac = 0, ex = 0;
  bool ex_neg = false;
  uint64_t w = 0;
  for (; pos < len; ++pos) {
    const unsigned ch = get(pos), dg = ch - '0';
    if (dg <= 9u) {
      if (st <= 3) {
        st = st == 0 ? 1 : (st == 2 ? 3 : st);
        if (nd || dg) {           // (leading zeros carry no weight)
          if (nd < 19) w = w * 10 + dg;
          ++nd;
        }
        frac += st == 3;
      } else {
        st = 6;
        if (ex < 100000) ex = ex * 10 + (int)dg;
      }
    } else if (ch == '.' && st == 1) {
      st = 2;
    } else if (ch == 'e' && (st == 1 || st == 3)) {
      st = 4;
    } else if ((ch == '+' || ch == '-') && st == 4) {
      st = 5;
      ex_neg = ch == '-';
    } else {
      return kBad;
    }
  }
  if (st != 1 && st != 3 && st != 6) return kBad;
  const int k = (ex_neg ? -ex : ex) - frac;
  if (nd > 16 || w > (1ull << 53) || k > 22 || k < -22) return kUndecided;
  const double m = (double)w;  // exact
  const double v = k >= 0 ? m * pow10_exact(k) : m / pow10_exact(-k);
  *out = neg ? -v : v;
  return kDecided;
}

}  // namespace dec
}  // namespace msw
