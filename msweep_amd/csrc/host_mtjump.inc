// host_mtjump.inc -- jump-ahead of the MT19937-64 stream (included by solve.hip).
// The reference draws all bootstrap replicates from ONE sequential std::mt19937_64
// (src/BootstrapSample.cpp:60-73), so rank r of a multi-GPU bootstrap starts r * (B / P) * draws
// words into the stream; stepping there costs 2 ns per word (17 s for the last of 8 ranks at 1000
// replicates of 10^7 draws).  The generator is linear over GF(2): with A the one-word transition and
// phi its characteristic polynomial (degree 19937), A^J s = g(A) s for g = t^J mod phi, evaluated by
// Horner's rule in 19937 transitions (Haramoto, Matsumoto, Nishimura, Panneton, L'Ecuyer 2008).
// phi comes from Berlekamp-Massey on one output bit (any bit sequence of a generator with primitive
// characteristic polynomial has it as minimal polynomial); t^J mod phi from 64 modular squarings.
// Cost: ~0.3 s of host time whatever J.
namespace mtjump {

constexpr int kN = 312, kM = 156, kDeg = 19937;
constexpr int kWords = kN + 1;  // polynomial / bit-register words (>= kDeg + 2 bits)
using Poly = std::array<uint64_t, kWords>;

inline uint64_t twist(uint64_t hi, uint64_t lo, uint64_t far) {
  const uint64_t x = (hi & 0xFFFFFFFF80000000ULL) | (lo & 0x7FFFFFFFULL);
  return far ^ (x >> 1) ^ ((x & 1ULL) ? 0xB5026F5AA96619E9ULL : 0ULL);
}

// window of the last 312 state words as a ring; step() appends the next word
struct Window {
  std::array<uint64_t, kN> w{};
  int head = 0;  // ring position of the oldest word
  uint64_t step() {
    const uint64_t v = twist(w[head], w[(head + 1) % kN], w[(head + kM) % kN]);
    w[head] = v;
    head = (head + 1) % kN;
    return v;
  }
  uint64_t at(int j) const { return w[(head + j) % kN]; }  // j-th oldest
};

inline bool bit(const Poly &p, int i) { return (p[i >> 6] >> (i & 63)) & 1ULL; }
inline void shl1(Poly &p) {
  for (int i = kWords - 1; i > 0; --i) p[i] = (p[i] << 1) | (p[i - 1] >> 63);
  p[0] <<= 1;
}

// characteristic polynomial of the transition: Berlekamp-Massey on bit 0 of the state words
inline const Poly &phi() {
  static const Poly value = [] {
    Window s;
    uint64_t x = 5489ULL;
    s.w[0] = x;
    for (int i = 1; i < kN; ++i) {
      x = 6364136223846793005ULL * (x ^ (x >> 62)) + (uint64_t)i;
      s.w[i] = x;
    }
    Poly C{}, B{}, rev{}, T{};
    C[0] = B[0] = 1;
    int L = 0, m = 1;
    for (int n = 0; n < 2 * kDeg + 64; ++n) {
      shl1(rev);
      rev[0] |= s.step() & 1ULL;  // rev bit i = sequence element n - i
      uint64_t acc = 0;
      for (int i = 0; i <= (L >> 6); ++i) acc ^= C[i] & rev[i];
      if (!(__builtin_popcountll(acc) & 1)) {
        ++m;
        continue;
      }
      T = C;
      // C ^= B << m
      const int ws = m >> 6, bs = m & 63;
      for (int i = kWords - 1; i >= ws; --i) {
        uint64_t v = B[i - ws] << bs;
        if (bs && i - ws - 1 >= 0) v |= B[i - ws - 1] >> (64 - bs);
        C[i] ^= v;
      }
      if (2 * L <= n) {
        L = n + 1 - L;
        B = T;
        m = 1;
      } else {
        ++m;
      }
    }
    if (L != kDeg) throw std::runtime_error("internal: MT19937-64 characteristic polynomial has the wrong degree");
    Poly p{};  // phi(t) = t^L * C(1/t)
    for (int i = 0; i <= L; ++i)
      if (bit(C, i)) p[(L - i) >> 6] |= 1ULL << ((L - i) & 63);
    return p;
  }();
  return value;
}

// r = a * a mod phi
inline Poly sqrmod(const Poly &a) {
  const Poly &f = phi();
  Poly r{};
  for (int i = kDeg - 1; i >= 0; --i) {  // Horner over the bits of the second factor
    shl1(r);
    if (bit(r, kDeg))
      for (int k = 0; k < kWords; ++k) r[k] ^= f[k];
    if (bit(a, i))
      for (int k = 0; k < kWords; ++k) r[k] ^= a[k];
  }
  return r;
}

// the window J words further down the stream
inline void jump(std::array<uint64_t, kN> &state /* oldest first */, uint64_t J) {
  const Poly &f = phi();
  Poly g{};
  g[0] = 1;  // t^0
  for (int b = 63; b >= 0; --b) {
    g = sqrmod(g);
    if ((J >> b) & 1ULL) {
      shl1(g);
      if (bit(g, kDeg))
        for (int k = 0; k < kWords; ++k) g[k] ^= f[k];
    }
  }
  Window r;  // Horner: r = A r + g_i s
  for (int i = kDeg - 1; i >= 0; --i) {
    r.step();
    if (bit(g, i))
      for (int j = 0; j < kN; ++j) r.w[(r.head + j) % kN] ^= state[j];
  }
  for (int j = 0; j < kN; ++j) state[j] = r.at(j);
}

}  // namespace mtjump
