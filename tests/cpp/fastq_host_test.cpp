// fastq_host_test.cpp -- stand-alone check of the host loops behind MSWEEP_HOST_EXTRACT=1 (msweep_amd/csrc/fastq_host.hpp:
// index with validation, selection, gather, the end of a piece) against a restatement that splits the text into lines and
// groups them by four.  No device: g++ -std=c++17 -I msweep_amd/csrc tests/cpp/fastq_host_test.cpp, with or without
// -fsanitize=address,undefined.  Prints "ok" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "fastq_host.hpp"

using namespace msw;

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// the restatement: the lines with their line ends, in fours
std::vector<std::string> records_of(const std::string &text) {
  std::vector<std::string> lines, recs;
  for (size_t p = 0; p < text.size();) {
    const size_t e = text.find('\n', p);
    const size_t end = e == std::string::npos ? text.size() : e + 1;
    lines.push_back(text.substr(p, end - p));
    p = end;
  }
  for (size_t i = 0; i + 4 <= lines.size(); i += 4) recs.push_back(lines[i] + lines[i + 1] + lines[i + 2] + lines[i + 3]);
  return recs;
}

std::string make_text(std::mt19937 &rng, size_t n_records, bool final_newline, bool crlf) {
  static const size_t lens[] = {0, 1, 35, 151, 4095, 4096, 4097, 10000};
  std::string t;
  const std::string eol = crlf ? "\r\n" : "\n";
  for (size_t r = 0; r < n_records; ++r) {
    const size_t L = lens[rng() % 8];
    std::string seq(L, 'A'), qual(L, 'I');
    for (auto &c : seq) c = "ACGT"[rng() % 4];
    if (L && rng() % 10 == 0) qual[0] = '@';
    else if (L && rng() % 10 == 0) qual[0] = '+';
    const std::string name = "r" + std::to_string(r);
    t += "@" + name + eol + seq + eol + "+" + (rng() % 10 == 0 ? name : std::string()) + eol + qual + eol;
  }
  if (!final_newline && !t.empty()) t.resize(t.size() - eol.size() + (crlf ? 1 : 0));  // (CRLF: the '\r' stays, the '\n' goes)
  return t;
}

void check_select(const std::string &text, const std::vector<uint64_t> &rec_off, const std::vector<uint32_t> &ids) {
  const std::vector<std::string> recs = records_of(text);
  std::vector<uint32_t> sel;
  std::vector<uint64_t> out_off;
  uint64_t bad = 0;
  CHECK(fq::host_select(ids.data(), ids.size(), rec_off, sel, out_off, &bad));
  std::string want;
  for (uint32_t id : std::set<uint32_t>(ids.begin(), ids.end())) want += recs[id];
  CHECK(out_off.size() == sel.size() + 1 && out_off.back() == want.size());
  std::string got(want.size(), '\0');
  fq::host_gather(text.data(), rec_off, sel, out_off, 0, sel.size(), got.data());
  CHECK(got == want);
  // in pieces: each ends at a record end, none is longer than the limit, together they are the whole
  const uint64_t limit = 24000;  // (above the longest record: 2 x 10 000 bases and the names)
  std::string joined;
  for (uint64_t r0 = 0; r0 < sel.size();) {
    const uint64_t r1 = fq::piece_end([&](uint64_t r) { return out_off[r]; }, r0, sel.size(), limit);
    if (r1 == r0) {
      CHECK(out_off[r0 + 1] - out_off[r0] > limit);
      break;
    }
    CHECK(out_off[r1] - out_off[r0] <= limit);
    std::string piece(out_off[r1] - out_off[r0], '\0');
    fq::host_gather(text.data(), rec_off, sel, out_off, r0, r1, piece.data());
    joined += piece;
    r0 = r1;
  }
  CHECK(joined == want);
}

void check_bad(const std::string &text, int reason, uint64_t record) {
  std::vector<uint64_t> rec_off;
  uint64_t n_lines = 0, bad = 0;
  const int got = fq::host_index(text.data(), text.size(), rec_off, &n_lines, &bad);
  CHECK(got == reason);
  CHECK(bad == record);
  CHECK(fq::grammar_message("f.fq", got, bad, n_lines).find("record " + std::to_string(record + 1)) != std::string::npos);
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  for (int variant = 0; variant < 3; ++variant) {
    const std::string text = make_text(rng, 120, variant != 1, variant == 2);
    std::vector<uint64_t> rec_off;
    uint64_t n_lines = 0, bad = 0;
    CHECK(fq::host_index(text.data(), text.size(), rec_off, &n_lines, &bad) == fq::kOk);
    CHECK(n_lines == 480 && rec_off.size() == 121 && rec_off.back() == text.size());
    std::vector<uint32_t> all(120), odd, some;
    for (uint32_t i = 0; i < 120; ++i) all[i] = i;
    for (uint32_t i = 1; i < 120; i += 2) odd.push_back(i);
    for (int i = 0; i < 50; ++i) some.push_back(rng() % 120);
    for (const auto &ids : {all, odd, some, std::vector<uint32_t>{}, std::vector<uint32_t>{0}, std::vector<uint32_t>{119}})
      check_select(text, rec_off, ids);
    std::vector<uint32_t> sel;
    std::vector<uint64_t> out_off;
    const uint32_t over[2] = {3, 120};
    CHECK(!fq::host_select(over, 2, rec_off, sel, out_off, &bad) && bad == 120);
  }
  {  // records of 6 bytes, and the empty file
    const std::string text = "@a\nAC\n+\nII\n@\n\n+\n\n@\n\n+\n\n@b\nA\n+\nI\n";
    std::vector<uint64_t> rec_off;
    uint64_t n_lines = 0, bad = 0;
    CHECK(fq::host_index(text.data(), text.size(), rec_off, &n_lines, &bad) == fq::kOk);
    CHECK((rec_off == std::vector<uint64_t>{0, 11, 17, 23, 32}));
    check_select(text, rec_off, {1, 2});
    std::vector<uint64_t> none;
    CHECK(fq::host_index("", 0, none, &n_lines, &bad) == fq::kOk && n_lines == 0 && none.size() == 1);
  }
  check_bad("@a\nA\n+\nI\n@b\nA\n", fq::kLines, 1);
  check_bad("@a\nA\n+\nI\nb\nA\n+\nI\n", fq::kNoAt, 1);
  check_bad("@a\nA\n-\nI\n", fq::kNoPlus, 0);
  check_bad("@a\nAC\n+\nI\n@b\nA\n+\nI\n", fq::kLength, 0);
  check_bad("@a\nA\n+\nI\n@b\nA\n+\nI\n@c\nAC\n+\nI", fq::kLength, 2);
  if (failures) return 1;
  puts("ok");
  return 0;
}
