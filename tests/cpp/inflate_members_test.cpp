// Host build of the member layer of msweep_amd/csrc/inflate_format.hpp (tests/test_inflate_members_cpu.py): files of
// gzip members that declare their lengths (BGZF), walked into a member table and decoded member by member.
//   --inflate in.gz out       the plain reference (walk, one decode per member, the per-member trailer check); writes the
//                             text; prints why / members / the first bad member and its status
//   --fuzz in.gz copies seed  mutated copies (byte flips, truncations, insertions, biased into headers and trailers)
//                             through the reference and through zlib reading every member as gzread does: every copy
//                             ends in a fallback reason or in zlib's bytes
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "inflate_format.hpp"

using namespace msw;
using namespace msw::infl;

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

// zlib over every member, gzread's rule: another member follows where the gzip magic does, anything else behind a member
// is ignored.  true and the text when every member read is whole.
static bool zlib_members(const std::vector<uint8_t> &gz, std::vector<uint8_t> &text) {
  text.clear();
  if (gz.empty()) return false;
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
  std::vector<uint8_t> buf(1 << 18);
  zs.next_in = const_cast<Bytef *>(gz.data());
  zs.avail_in = (uInt)gz.size();
  bool ok = false;
  for (;;) {
    zs.next_out = buf.data();
    zs.avail_out = (uInt)buf.size();
    const int rc = inflate(&zs, Z_NO_FLUSH);
    text.insert(text.end(), buf.data(), buf.data() + (buf.size() - zs.avail_out));
    if (rc == Z_STREAM_END) {
      const uint8_t *at = zs.next_in;
      if (zs.avail_in >= 2 && at[0] == 0x1f && at[1] == 0x8b) {
        if (inflateReset(&zs) != Z_OK) break;
        continue;
      }
      ok = true;
      break;
    }
    if (rc != Z_OK && rc != Z_BUF_ERROR) break;                  // zlib's error
    if (zs.avail_in == 0 && zs.avail_out != 0) break;            // the input ended inside a member
  }
  inflateEnd(&zs);
  return ok;
}

static int run_inflate(const char *in, const char *out) {
  const std::vector<uint8_t> gz = read_file(in);
  const MembersReference R = members_reference(gz.data(), gz.size());
  printf("why=%d members=%u bad_member=%u status=%u payload=%llu bytes=%zu\n", R.why, R.n_members, R.bad_member, R.bad_status,
         (unsigned long long)R.payload_bytes, R.text.size());
  FILE *f = fopen(out, "wb");
  if (!f) return 2;
  if (!R.text.empty()) fwrite(R.text.data(), 1, R.text.size(), f);
  fclose(f);
  return 0;
}

static int run_fuzz(const char *in, int copies, unsigned seed) {
  const std::vector<uint8_t> gz = read_file(in);
  MemberTable T;
  if (!walk_members(BufferFetch{gz.data(), gz.size()}, gz.size(), T)) {
    printf("FAILED: the input is not a file of members\n");
    return 1;
  }
  // where headers and trailers lie: a member's 18 header bytes end at its first payload bit, its trailer begins at end_bit
  std::mt19937_64 rng(seed);
  auto place = [&](size_t size) -> size_t {
    if (rng() % 2) return (size_t)(rng() % size);
    const MemberEntry &m = T.members[rng() % T.members.size()];
    const uint64_t at = rng() % 2 ? m.first_bit / 8 - 1 - rng() % 18 : m.end_bit / 8 + rng() % 8;
    return (size_t)(at < size ? at : size - 1);
  };
  int n_error = 0, n_same = 0, n_fallback_ok = 0, bad = 0;
  std::vector<uint8_t> zt;
  for (int k = 0; k < copies; ++k) {
    std::vector<uint8_t> m = gz;
    const int kind = (int)(rng() % 3);
    if (kind == 0) {  // byte flips
      const int flips = 1 + (int)(rng() % 3);
      for (int i = 0; i < flips; ++i) m[place(m.size())] ^= (uint8_t)(1 + rng() % 255);
    } else if (kind == 1) {  // truncation
      m.resize(place(m.size()));
    } else {  // bytes inserted: everything behind them moves up
      const size_t at = place(m.size());
      const int count = 1 + (int)(rng() % 4);
      for (int i = 0; i < count; ++i) m.insert(m.begin() + (ptrdiff_t)at, (uint8_t)rng());
    }
    const MembersReference R = members_reference(m.data(), m.size());
    const bool zok = zlib_members(m, zt);
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

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "--inflate")) return run_inflate(argv[2], argv[3]);
  if (argc >= 5 && !strcmp(argv[1], "--fuzz")) return run_fuzz(argv[2], atoi(argv[3]), (unsigned)atoi(argv[4]));
  fprintf(stderr, "usage: --inflate in.gz out | --fuzz in.gz copies seed\n");
  return 2;
}
