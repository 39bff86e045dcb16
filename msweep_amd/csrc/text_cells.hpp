// text_cells.hpp -- the undecided cells of a text block (text_kernels.hpp) on the host: the device leaves 13 blanks and
// (byte offset, bits) for a value its formatter cannot decide; here every such cell is printed with snprintf and told
// where it lands once the gaps are closed (k_text_close).  No HIP: tests/cpp/text_cells_test.cpp builds it with g++.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "g6_format.hpp"

namespace msw {

struct TextHostCell {  // a cell left to the host: where its 13 blanks start, and the bits of the value
  uint64_t off, bits;
};

struct TextFilledCell {  // ... as the host printed it: its text, and the blanks dropped in front of it (the slack)
  uint64_t off;
  uint32_t slack, len;
  char s[16];
};

// cells: the undecided cells of a block of `total` bytes, sorted by offset.  filled[i]: cell i printed; returns the
// length of the block with every cell's 13 blanks cut to its text.
inline uint64_t text_fill_cells(const std::vector<TextHostCell> &cells, uint64_t total, std::vector<TextFilledCell> &filled) {
  filled.resize(cells.size());
  uint64_t rp = 0, slack = 0;
  for (size_t i = 0; i < cells.size(); ++i) {
    const TextHostCell &c = cells[i];
    if (c.off < rp || c.off > total || total - c.off < (uint64_t)g6::kMaxLen)
      throw std::runtime_error("msw_core_text_block: an undecided cell lies outside its block");
    double x;
    std::memcpy(&x, &c.bits, sizeof x);
    TextFilledCell &f = filled[i];
    f.off = c.off;
    f.slack = (uint32_t)slack;
    const int n = snprintf(f.s, sizeof f.s, "%g", x);
    if (n < 1 || n > g6::kMaxLen) throw std::runtime_error("msw_core_text_block: a cell's text does not fit its blanks");
    f.len = (uint32_t)n;
    slack += (uint64_t)(g6::kMaxLen - n);
    rp = c.off + g6::kMaxLen;
  }
  return total - slack;
}

}  // namespace msw
