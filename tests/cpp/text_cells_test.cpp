// text_cells_test.cpp -- host build of msweep_amd/csrc/text_cells.hpp (tests/test_text_cells_cpu.py): the undecided
// cells of a text block printed and placed (text_fill_cells), checked against a host gap-closer over a synthetic block
// -- print each cell into its 13 blanks and move what follows up against it -- and applied the way k_text_close does.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "text_cells.hpp"

using namespace msw;

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

constexpr uint64_t kBlank = (uint64_t)g6::kMaxLen;

uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

// the oracle: the block's text with its 13-blank holes, closed in place
std::string close_on_host(std::string text, const std::vector<TextHostCell> &cells) {
  const size_t total = text.size();
  size_t rp = 0, wp = 0;
  char b[32];
  for (const TextHostCell &c : cells) {
    std::memmove(&text[0] + wp, &text[0] + rp, c.off - rp);
    wp += c.off - rp;
    double x;
    std::memcpy(&x, &c.bits, sizeof x);
    const int n = snprintf(b, sizeof b, "%g", x);
    std::memcpy(&text[0] + wp, b, (size_t)n);
    wp += (size_t)n;
    rp = c.off + kBlank;
  }
  std::memmove(&text[0] + wp, &text[0] + rp, total - rp);
  text.resize(wp + total - rp);
  return text;
}

// what k_text_close does with the filled cells, byte by byte
std::string close_as_kernel(const std::string &src, const std::vector<TextFilledCell> &cells, uint64_t final_len) {
  std::string dst(final_len, '?');
  for (uint64_t i = 0; i < src.size(); ++i) {
    size_t lo = 0;
    while (lo < cells.size() && cells[lo].off <= i) ++lo;
    uint64_t slack = 0;
    if (lo) {
      const TextFilledCell &c = cells[lo - 1];
      const uint64_t j = i - c.off;
      if (j < kBlank) {
        if (j < c.len) dst.at(c.off - c.slack + j) = c.s[j];
        continue;
      }
      slack = (uint64_t)c.slack + (uint32_t)(kBlank - c.len);
    }
    dst.at(i - slack) = src[i];
  }
  return dst;
}

// a block of `total` bytes: letters, and 13 blanks at every cell
std::string block_of(uint64_t total, const std::vector<TextHostCell> &cells) {
  std::string s(total, ' ');
  for (uint64_t i = 0; i < total; ++i) s[i] = (char)('a' + i % 26);
  for (const TextHostCell &c : cells) s.replace(c.off, kBlank, kBlank, ' ');
  return s;
}

void check_case(const char *name, uint64_t total, const std::vector<TextHostCell> &cells) {
  std::vector<TextFilledCell> filled(3);  // (stale entries: the call sizes it)
  uint64_t len = 0;
  try {
    len = text_fill_cells(cells, total, filled);
  } catch (const std::exception &ex) {
    CHECK(false, "%s: %s", name, ex.what());
    return;
  }
  const std::string src = block_of(total, cells), want = close_on_host(src, cells);
  CHECK(filled.size() == cells.size(), "%s", name);
  CHECK(len == want.size(), "%s: length %llu, the oracle's %zu", name, (unsigned long long)len, want.size());
  uint64_t slack = 0;
  for (size_t i = 0; i < filled.size() && i < cells.size(); ++i) {
    const TextFilledCell &f = filled[i];
    double x;
    std::memcpy(&x, &cells[i].bits, sizeof x);
    char b[32];
    const int n = snprintf(b, sizeof b, "%g", x);
    CHECK(f.off == cells[i].off && f.slack == slack && (int)f.len == n && std::memcmp(f.s, b, (size_t)n) == 0, "%s: cell %zu", name, i);
    slack += kBlank - f.len;
  }
  if (len == want.size() && filled.size() == cells.size()) {
    const std::string got = close_as_kernel(src, filled, len);
    CHECK(got == want, "%s: '%s' against '%s'", name, got.c_str(), want.c_str());
  }
  printf("%s: cells=%zu %llu -> %llu bytes\n", name, cells.size(), (unsigned long long)total, (unsigned long long)len);
}

void check_throws(const char *name, uint64_t total, const std::vector<TextHostCell> &cells, const char *words) {
  std::vector<TextFilledCell> filled;
  bool threw = false;
  try {
    (void)text_fill_cells(cells, total, filled);
  } catch (const std::runtime_error &ex) {
    threw = std::strstr(ex.what(), words) != nullptr;
  }
  CHECK(threw, "%s", name);
  printf("%s: refused\n", name);
}

}  // namespace

int main() {
  const uint64_t one = bits_of(5.0), wide = bits_of(-1.03125e-300), tie = bits_of(2469135.0);
  {
    char b[32];
    CHECK(snprintf(b, sizeof b, "%g", 5.0) == 1 && snprintf(b, sizeof b, "%g", -1.03125e-300) == 13, "the widths of the test's values");
  }
  check_case("no cells", 40, {});
  check_case("no cells, empty block", 0, {});
  check_case("a cell at offset 0", 40, {{0, tie}});
  check_case("a cell that ends at total", 40, {{40 - kBlank, tie}});
  check_case("a cell that is the block", kBlank, {{0, one}});
  check_case("two cells back to back", 60, {{7, tie}, {7 + kBlank, one}});
  check_case("a text of length 1", 40, {{11, one}});
  check_case("a text of length 13", 40, {{11, wide}});
  check_case("lengths 1 and 13, first and last", 3 * kBlank, {{0, one}, {kBlank, tie}, {2 * kBlank, wide}});
  {
    // many cells, every gap from 0 to 4 bytes, all the widths of 1 ... 13
    const double widths[13] = {1.0, -1.0, 0.5, -0.5, 1e-5, -1e-5, 1.5e-5, 1.25e-5, 1.125e-5, 1.0625e-5, 1.03125e-5, -1.03125e-5, -1.03125e-300};
    std::vector<TextHostCell> cells;
    uint64_t at = 3;
    for (int i = 0; i < 200; ++i) {
      cells.push_back({at, bits_of(widths[(i * 7) % 13])});
      at += kBlank + (uint64_t)(i % 5);
    }
    check_case("two hundred cells", at + 9, cells);
  }
  check_throws("a cell past the end", 40, {{40 - kBlank + 1, tie}}, "outside its block");
  check_throws("a cell beyond the block", 40, {{41, tie}}, "outside its block");
  check_throws("an offset that wraps", 40, {{~(uint64_t)0 - 5, tie}}, "outside its block");
  check_throws("overlapping cells", 60, {{7, tie}, {7 + kBlank - 1, one}}, "outside its block");
  check_throws("cells out of order", 60, {{30, tie}, {7, one}}, "outside its block");
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("text cells: ok\n");
  return 0;
}
