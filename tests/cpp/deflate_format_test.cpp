// deflate_format_test.cpp -- host build of msweep_amd/csrc/deflate_format.hpp (tests/test_deflate_format_cpu.py).
//   (no argument)                 the code tables against RFC 1951 3.2.5, the code-length builder, canonical codes, CRC pieces
//   --encode IN OUT CHUNK STORED  the raw DEFLATE stream of file IN by the reference encoder, chunks of CHUNK bytes
//   --crc IN PIECE                crc32 of file IN from pieces of PIECE bytes combined with x^(8 n) multipliers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "deflate_format.hpp"

using namespace msw::defl;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      printf("FAILED %s: ", #cond);     \
      printf(__VA_ARGS__);              \
      printf("\n");                     \
      ++g_failed;                       \
    }                                   \
  } while (0)

// RFC 1951 3.2.5, typed in from the document (not from the header under test)
const int kRfcLen[29][3] = {{257, 0, 3},   {258, 0, 4},   {259, 0, 5},   {260, 0, 6},   {261, 0, 7},   {262, 0, 8},
                            {263, 0, 9},   {264, 0, 10},  {265, 1, 11},  {266, 1, 13},  {267, 1, 15},  {268, 1, 17},
                            {269, 2, 19},  {270, 2, 23},  {271, 2, 27},  {272, 2, 31},  {273, 3, 35},  {274, 3, 43},
                            {275, 3, 51},  {276, 3, 59},  {277, 4, 67},  {278, 4, 83},  {279, 4, 99},  {280, 4, 115},
                            {281, 5, 131}, {282, 5, 163}, {283, 5, 195}, {284, 5, 227}, {285, 0, 258}};
const int kRfcDist[30][3] = {{0, 0, 1},      {1, 0, 2},      {2, 0, 3},      {3, 0, 4},       {4, 1, 5},       {5, 1, 7},
                             {6, 2, 9},      {7, 2, 13},     {8, 3, 17},     {9, 3, 25},      {10, 4, 33},     {11, 4, 49},
                             {12, 5, 65},    {13, 5, 97},    {14, 6, 129},   {15, 6, 193},    {16, 7, 257},    {17, 7, 385},
                             {18, 8, 513},   {19, 8, 769},   {20, 9, 1025},  {21, 9, 1537},   {22, 10, 2049},  {23, 10, 3073},
                             {24, 11, 4097}, {25, 11, 6145}, {26, 12, 8193}, {27, 12, 12289}, {28, 13, 16385}, {29, 13, 24577}};

void check_tables() {
  int n = 0;
  for (int len = 3; len <= 258; ++len, ++n) {
    int row = 28;  // 258 is code 285 alone, although 284's range reaches it
    if (len < 258)
      for (row = 0; !(len >= kRfcLen[row][2] && len < kRfcLen[row + 1][2]); ++row) {}
    const Sym s = length_sym((uint32_t)len);
    CHECK((int)s.sym == kRfcLen[row][0] && (int)s.nbits == kRfcLen[row][1] && (int)s.extra == len - kRfcLen[row][2], "length %d", len);
    CHECK(s.extra < (1u << s.nbits) && lit_extra_bits(s.sym) == s.nbits, "length %d", len);
    CHECK(kLenBase[s.sym - 257] + s.extra == (uint32_t)len && kLenExtra[s.sym - 257] == s.nbits, "length table %d", len);
    CHECK(token_len(token_match((uint32_t)len, 1)) == (uint32_t)len, "token length %d", len);
  }
  printf("lengths: values=%d ok\n", n);
  n = 0;
  for (int d = 1; d <= 32768; ++d, ++n) {
    int row = 29;
    while (d < kRfcDist[row][2]) --row;
    const Sym s = dist_sym((uint32_t)d);
    CHECK((int)s.sym == kRfcDist[row][0] && (int)s.nbits == kRfcDist[row][1] && (int)s.extra == d - kRfcDist[row][2], "distance %d", d);
    CHECK(s.extra < (1u << s.nbits) && dist_extra_bits(s.sym) == s.nbits, "distance %d", d);
    CHECK(kDistBase[s.sym] + s.extra == (uint32_t)d && kDistExtra[s.sym] == s.nbits, "distance table %d", d);
    CHECK(token_dist(token_match(3, (uint32_t)d)) == (uint32_t)d && token_is_match(token_match(3, (uint32_t)d)), "token distance %d", d);
  }
  printf("distances: values=%d ok\n", n);
}

// lengths of a histogram: at most `limit`, Kraft sum <= 1 and exactly 1 from two symbols on; canonical codes prefix-free
int check_histogram(const char *name, const std::vector<uint32_t> &freq, int limit) {
  const int n = (int)freq.size();
  std::vector<uint8_t> lens(n, 99);
  std::vector<uint32_t> ws(build_lengths_ws(n)), table(n);
  build_lengths(freq.data(), n, limit, lens.data(), ws.data());
  int used = 0, maxlen = 0;
  uint64_t kraft = 0;  // in units of 2^-limit
  for (int s = 0; s < n; ++s) {
    CHECK((freq[s] != 0) == (lens[s] != 0), "%s: symbol %d", name, s);
    if (!lens[s]) continue;
    ++used;
    if (lens[s] > maxlen) maxlen = lens[s];
    if (lens[s] <= limit) kraft += 1ull << (limit - lens[s]);
  }
  CHECK(maxlen <= limit, "%s: length %d", name, maxlen);
  CHECK(kraft <= 1ull << limit, "%s: Kraft sum above 1", name);
  if (used >= 2) CHECK(kraft == 1ull << limit, "%s: incomplete code", name);
  if (used == 1) CHECK(maxlen == 1, "%s: a lone symbol gets length 1", name);
  // a rarer symbol never has the shorter code
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      if (freq[a] && freq[b] && freq[a] < freq[b]) CHECK(lens[a] >= lens[b], "%s: order of %d and %d", name, a, b);
  assign_codes(lens.data(), n, table.data(), ws.data());
  for (int a = 0; a < n && n <= 64; ++a)
    for (int b = 0; b < n; ++b) {
      if (a == b || !lens[a] || !lens[b] || lens[a] > lens[b]) continue;
      const uint32_t ca = reverse_bits(table[a] & 0xffff, lens[a]), cb = reverse_bits(table[b] & 0xffff, lens[b]);
      CHECK((cb >> (lens[b] - lens[a])) != ca, "%s: code of %d is a prefix of %d's", name, a, b);
    }
  for (int s = 0; s < n; ++s) CHECK((table[s] >> 16) == lens[s], "%s: table length %d", name, s);
  return maxlen;
}

void check_builder() {
  int hists = 0, limited = 0;
  for (int n = 2; n <= 40; ++n) {  // Fibonacci weights: the unlimited code is n - 1 deep
    std::vector<uint32_t> f(n);
    uint32_t a = 1, b = 1;
    for (int i = 0; i < n; ++i) {
      f[i] = a;
      const uint32_t c = a + b;
      a = b;
      b = c < (1u << 22) ? c : b;
    }
    for (int limit : {7, 15}) {
      const int got = check_histogram("fibonacci", f, limit);
      if (n - 1 > limit && n <= 32) {
        CHECK(got == limit, "fibonacci %d: the limit %d is reached", n, limit);
        ++limited;
      }
      ++hists;
    }
    std::vector<uint32_t> r(f.rbegin(), f.rend());
    check_histogram("fibonacci reversed", r, 15);
    ++hists;
  }
  for (int n : {1, 2, 3, 16, 19, 30, 255, 256, 286}) {
    check_histogram("flat", std::vector<uint32_t>(n, 7), 15);
    ++hists;
  }
  {
    std::vector<uint32_t> f(286, 0);
    check_histogram("empty", f, 15);
    f[256] = 1;
    check_histogram("single", f, 15);
    f[0] = 32768;
    check_histogram("two", f, 15);
    f[285] = 1;
    check_histogram("three", f, 15);
    hists += 4;
  }
  uint64_t x = 88172645463325252ull;  // xorshift: skewed random histograms
  for (int t = 0; t < 300; ++t) {
    std::vector<uint32_t> f(t % 2 ? 286 : 30);
    for (auto &v : f) {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      const int sh = (int)(x >> 59);
      v = sh > 22 ? 0 : (uint32_t)((x >> 8) & 0xffffff) >> sh;
      if (v >= (1u << 23)) v = 0;
    }
    check_histogram("random", f, t % 3 ? 15 : 9);
    ++hists;
  }
  printf("builder: histograms=%d limited=%d ok\n", hists, limited);
}

void check_header() {
  CHECK(kHeaderBits == 1338, "header bits");
  CHECK(kHeaderPrefix == (2u << 1 | (286u - 257u) << 3 | (30u - 1u) << 8 | (19u - 4u) << 13), "header prefix");
  // the flat code-length code is complete: sixteen codes of 4 bits
  int kraft = 0;
  for (int i = 0; i < 19; ++i)
    if (header_cl_len(i)) kraft += 1 << (7 - header_cl_len(i));
  CHECK(kraft == 128, "code-length code");
  CHECK(dynamic_bytes(1338 + 7) == (1338 + 7 + 3 + 7) / 8 + 4 && stored_bytes(32768) == 32778 && stored_bytes(70000) == 70015, "sizes");
  printf("header: ok\n");
}

uint32_t crc_bytes(const uint8_t *p, size_t n, uint32_t r) {
  for (size_t i = 0; i < n; ++i) r = crc_word(r, p[i], 1);
  return r;
}

uint32_t crc_pieces(const std::vector<uint8_t> &d, size_t piece) {
  uint32_t pow8[40];
  crc_pow_table(pow8);
  uint32_t sum = 0;
  for (size_t o = 0; o < d.size(); o += piece) {
    const size_t n = d.size() - o < piece ? d.size() - o : piece;
    sum ^= crc_shift(crc_bytes(d.data() + o, n, 0), d.size() - o - n, pow8);
  }
  return ~(crc_shift(0xffffffffu, d.size(), pow8) ^ sum);
}

void check_crc() {
  const char *s = "123456789";
  std::vector<uint8_t> d(s, s + 9);
  CHECK(~crc_bytes(d.data(), 9, 0xffffffffu) == 0xcbf43926u, "crc32 check value");
  for (size_t piece : {1, 2, 4, 9, 100}) CHECK(crc_pieces(d, piece) == 0xcbf43926u, "crc32 from pieces of %zu", piece);
  uint32_t w;
  memcpy(&w, s, 4);
  CHECK(crc_word(0xffffffffu, w, 4) == crc_bytes(d.data(), 4, 0xffffffffu), "crc of a word");
  CHECK(gf2_mul(0x80000000u, 0x12345678u) == 0x12345678u, "x^0 is the unit");
  printf("crc: ok\n");
}

std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> d;
  FILE *f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
  fclose(f);
  return d;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "--encode")) {
    const std::vector<uint8_t> d = read_file(argv[2]);
    const std::vector<uint8_t> out = encode(d.data(), d.size(), (uint32_t)atoi(argv[4]), atoi(argv[5]) != 0);
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) return 2;
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "--crc")) {
    printf("%u\n", crc_pieces(read_file(argv[2]), (size_t)atol(argv[3])));
    return 0;
  }
  check_tables();
  check_builder();
  check_header();
  check_crc();
  if (g_failed) printf("FAILED checks: %d\n", g_failed);
  return g_failed ? 1 : 0;
}
