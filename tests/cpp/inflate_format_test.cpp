// Host build of msweep_amd/csrc/inflate_format.hpp (tests/test_inflate_format_cpu.py):
//   (no arguments)                  the arithmetic tables against deflate_format.hpp's, the order of the code-length
//                                   code, the member header parser
//   --inflate in.gz out chunk       the plain reference (probe per chunk, pass (a), window chain, pass (b), trailer) at
//                                   that chunk size (0: one chunk); writes the text; prints why / chunks / starts and
//                                   how the probe did against the block starts of a sequential walk
//   --fuzz in.gz copies seed chunk  mutated copies (byte flips, truncations, bit insertions) through the reference and
//                                   through zlib: every copy ends in a fallback reason or in zlib's bytes
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "inflate_format.hpp"

using namespace msw;
using namespace msw::infl;

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> d;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
  fclose(f);
  return d;
}

// zlib on one gzip member: true and the text when the stream is whole and nothing follows it
static bool zlib_member(const std::vector<uint8_t> &gz, std::vector<uint8_t> &text) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
  text.clear();
  std::vector<uint8_t> buf(1 << 18);
  zs.next_in = const_cast<Bytef *>(gz.data());
  zs.avail_in = (uInt)gz.size();
  int rc = Z_OK;
  while (rc == Z_OK) {
    zs.next_out = buf.data();
    zs.avail_out = (uInt)buf.size();
    rc = inflate(&zs, Z_NO_FLUSH);
    text.insert(text.end(), buf.data(), buf.data() + (buf.size() - zs.avail_out));
    if (rc == Z_OK && zs.avail_in == 0 && zs.avail_out != 0) break;  // the input ended inside the stream
  }
  const bool whole = rc == Z_STREAM_END && zs.avail_in == 0;
  inflateEnd(&zs);
  return whole;
}

struct CountSink {
  uint64_t count = 0;
  uint32_t why = kOk;
  bool lit(uint32_t) { return ++count, true; }
  bool copy(uint32_t len, uint32_t) { return count += len, true; }
};

// the bit positions at which the stream's non-final dynamic blocks start, by a sequential walk
static bool walk_blocks(const std::vector<uint8_t> &gz, std::set<uint64_t> &dyn_starts, uint64_t &n_blocks) {
  const Member m = parse_member(gz.data(), gz.size());
  if (!m.ok) return false;
  std::vector<uint32_t> words((gz.size() + 3) / 4 + 4, 0);
  memcpy(words.data(), gz.data(), gz.size());
  const Stream s = {words.data(), words.size(), 8 * (uint64_t)(gz.size() - 8)};
  std::vector<uint16_t> ws(kWsSize);
  const Tables t = tables_in(ws.data());
  BitIn b;
  bits_open(b, s, 8 * m.payload);
  CountSink sink;
  for (n_blocks = 0;; ++n_blocks) {
    const uint64_t at = bits_pos(b);
    const BlockHead bh = read_block_head(s, b, t);
    if (bh.status != kOk) return false;
    if (!bh.final && bh.type == 2) dyn_starts.insert(at);
    const uint32_t st = bh.type == 0 ? inflate_stored(s, b, bh.stored_len, sink) : inflate_symbols(s, b, t, sink);
    if (st != kOk) return false;
    if (bh.final) return true;
  }
}

static int run_inflate(const char *in, const char *out, size_t chunk) {
  const std::vector<uint8_t> gz = read_file(in);
  if (chunk == 0) chunk = gz.size() + 1;
  const Reference R = inflate_reference(gz.data(), gz.size(), chunk);
  uint64_t n_blocks = 0, want = 0, missed = 0, false_starts = 0;
  std::set<uint64_t> dyn;
  const Member m = parse_member(gz.data(), gz.size());
  if (m.ok && walk_blocks(gz, dyn, n_blocks)) {
    if (chunk < kMinChunk) chunk = kMinChunk;
    for (uint32_t c = 1; c < R.n_chunks; ++c) {
      const uint64_t lo = 8 * m.payload + 8 * (uint64_t)c * chunk, hi = lo + 8 * (uint64_t)chunk;
      const auto it = dyn.lower_bound(lo);
      const bool has = it != dyn.end() && *it < hi;
      want += has;
      if (has && (R.starts[c] == kNoStart || R.starts[c] > *it)) ++missed;
      if (R.starts[c] != kNoStart && !dyn.count(R.starts[c])) ++false_starts;
    }
  }
  printf("why=%d status=%u chunks=%u starts=%u blocks=%llu first_in_chunk=%llu missed=%llu false=%llu bytes=%zu\n", R.why, R.bad_status,
         R.n_chunks, R.n_starts, (unsigned long long)n_blocks, (unsigned long long)want, (unsigned long long)missed,
         (unsigned long long)false_starts, R.text.size());
  FILE *f = fopen(out, "wb");
  if (!f) return 2;
  if (!R.text.empty()) fwrite(R.text.data(), 1, R.text.size(), f);
  fclose(f);
  return 0;
}

static int run_fuzz(const char *in, int copies, unsigned seed, size_t chunk) {
  const std::vector<uint8_t> gz = read_file(in);
  std::mt19937_64 rng(seed);
  int n_error = 0, n_same = 0, n_fallback_ok = 0, bad = 0;
  std::vector<uint8_t> zt;
  for (int k = 0; k < copies; ++k) {
    std::vector<uint8_t> m = gz;
    const int kind = (int)(rng() % 3);
    if (kind == 0) {  // byte flips
      const int flips = 1 + (int)(rng() % 3);
      for (int i = 0; i < flips; ++i) m[rng() % m.size()] ^= (uint8_t)(1 + rng() % 255);
    } else if (kind == 1) {  // truncation
      m.resize((size_t)(rng() % m.size()));
    } else {  // a bit inserted: everything behind it moves up by one
      const uint64_t at = rng() % (8 * m.size());
      uint32_t carry = (uint32_t)(rng() & 1);
      for (size_t i = at / 8; i < m.size(); ++i) {
        const uint32_t sh = i == at / 8 ? (uint32_t)(at & 7) : 0;
        const uint32_t low = m[i] & ((1u << sh) - 1), high = m[i] >> sh;
        const uint32_t v = low | ((high << 1 | carry) << sh);
        carry = (v >> 8) & 1;
        m[i] = (uint8_t)v;
      }
    }
    const Reference R = inflate_reference(m.data(), m.size(), chunk);
    const bool zok = zlib_member(m, zt);
    if (R.why == kWhyNone) {
      if (zok && zt == R.text) ++n_same;
      else {
        ++bad;
        printf("FAILED copy %d kind %d: the reference vouches for bytes zlib does not give\n", k, kind);
      }
    } else {
      ++n_error;
      if (zok) ++n_fallback_ok;  // (zlib takes it: the host path would serve it -- a fallback, not an error)
    }
  }
  printf("fuzz: copies=%d error=%d same=%d zlib_took_a_fallback=%d bad=%d\n", copies, n_error, n_same, n_fallback_ok, bad);
  return bad ? 1 : 0;
}

static void self_tests() {
  for (uint32_t i = 0; i < 29; ++i) CHECK(length_base(i) == defl::kLenBase[i] && defl::lit_extra_bits(257 + i) == defl::kLenExtra[i]);
  for (uint32_t d = 0; d < 30; ++d) CHECK(dist_base(d) == defl::kDistBase[d] && defl::dist_extra_bits(d) == defl::kDistExtra[d]);
  printf("tables: ok\n");
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (uint32_t i = 0; i < 19; ++i) CHECK(cl_order(i) == order[i]);
  printf("order: ok\n");
  // member headers: plain; every optional field; cut short; wrong method; reserved flag
  std::vector<uint8_t> plain = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  Member m = parse_member(plain.data(), plain.size());
  CHECK(m.ok && m.payload == 10 && m.crc == 0 && m.isize == 0);
  std::vector<uint8_t> full = {0x1f, 0x8b, 8, 4 | 8 | 16 | 2, 0, 0, 0, 0, 0, 3, 3, 0, 'a', 'b', 'c', 'n', 0, 'c', 'o', 0, 0x12, 0x34,
                               3, 0, 1, 2, 3, 4, 5, 6, 7, 8};
  m = parse_member(full.data(), full.size());
  CHECK(m.ok && m.payload == 22 && m.crc == 0x04030201u && m.isize == 0x08070605u);
  for (size_t cut = 0; cut < full.size() - 1; ++cut) {
    const Member c = parse_member(full.data(), cut);
    CHECK(!c.ok || c.payload + 8 <= cut);
  }
  plain[2] = 7;
  CHECK(!parse_member(plain.data(), plain.size()).ok);
  plain[2] = 8;
  plain[3] = 0x20;
  CHECK(!parse_member(plain.data(), plain.size()).ok);
  printf("member: ok\n");
}

int main(int argc, char **argv) {
  if (argc >= 5 && !strcmp(argv[1], "--inflate")) return run_inflate(argv[2], argv[3], (size_t)atoll(argv[4]));
  if (argc >= 6 && !strcmp(argv[1], "--fuzz")) return run_fuzz(argv[2], atoi(argv[3]), (unsigned)atoi(argv[4]), (size_t)atoll(argv[5]));
  self_tests();
  if (failures) printf("FAILED: %d checks\n", failures);
  return failures ? 1 : 0;
}
