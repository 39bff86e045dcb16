// fastq_host.hpp -- the FASTQ record grammar of --extract-reads in plain host code: what both sides of
// host_fastq.inc share (reason codes, the failure messages) and the host loops behind MSWEEP_HOST_EXTRACT=1 -- index
// and validation, selection, gather.  Nothing here needs a device: tests/cpp/fastq_host_test.cpp runs it on the CPU.
//
// The grammar is the strict four-line one: a record is four lines, line 0 begins with '@', line 2 with '+', lines 1 and 3
// have the same length (a '\r' in front of the '\n' belongs to the line, on both), and the file's line count is a multiple
// of 4; a last line without '\n' counts as a line.  Lines are counted modulo 4 and '@' is never searched for: a quality
// line may begin with '@' or '+'.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace msw {
namespace fq {

// msw_fastq_info::reason
constexpr int kOk = 0, kLines = 1, kNoAt = 2, kNoPlus = 3, kLength = 4;

// What validation reports through one atomicMin: the smallest (record << 2 | reason - kNoAt) of the offending records.
constexpr uint64_t kNoBad = ~0ull;
inline uint64_t bad_code(uint64_t record, int reason) { return record << 2 | (uint64_t)(reason - kNoAt); }

// the failure of msw_fastq_open for a file outside the grammar; record: 0-based
inline std::string grammar_message(const std::string &path, int reason, uint64_t record, uint64_t n_lines) {
  const std::string head = "read file " + path + ": record " + std::to_string(record + 1);
  switch (reason) {
    case kLines:
      return head + " is incomplete: the file has " + std::to_string(n_lines) + " lines, which is no multiple of 4";
    case kNoAt: return head + ": its first line does not begin with '@'";
    case kNoPlus: return head + ": its third line does not begin with '+'";
    default: return head + ": its sequence line and its quality line differ in length";
  }
}
inline std::string id_message(uint64_t id, uint64_t n_records) {
  return "msw_fastq_select: read id " + std::to_string(id) + " is out of range (the read file has " + std::to_string(n_records) +
         " records)";
}

// rec_off[r] = the byte offset of record r's first line, rec_off[n_records] = n.  Returns kOk, or the reason and, in
// *bad, the 0-based number of the smallest offending record (kLines: the incomplete last one); *n_lines is the line
// count either way.
inline int host_index(const char *txt, size_t n, std::vector<uint64_t> &rec_off, uint64_t *n_lines, uint64_t *bad) {
  rec_off.clear();
  size_t pos = 0;
  uint64_t rec = 0;
  int reason = kOk;
  *bad = 0;
  while (pos < n) {
    size_t s[4], len[4];
    int k = 0;
    for (; k < 4 && pos < n; ++k) {
      s[k] = pos;
      const char *e = static_cast<const char *>(memchr(txt + pos, '\n', n - pos));
      const size_t end = e ? (size_t)(e - txt) : n;
      len[k] = end - pos;
      pos = e ? end + 1 : n;
    }
    if (k < 4) {  // (only the last record can be short: an earlier offender has been found by now)
      *n_lines = 4 * rec + (uint64_t)k;
      if (reason == kOk) reason = kLines, *bad = rec;
      return reason;
    }
    if (reason == kOk) {
      if (!(len[0] > 0 && txt[s[0]] == '@')) reason = kNoAt;
      else if (!(len[2] > 0 && txt[s[2]] == '+')) reason = kNoPlus;
      else if (len[1] != len[3]) reason = kLength;
      if (reason != kOk) *bad = rec;
    }
    rec_off.push_back((uint64_t)s[0]);
    ++rec;
  }
  rec_off.push_back((uint64_t)n);
  *n_lines = 4 * rec;
  return reason;
}

// the selection of `ids`: ascending, every id once; out_off[i] = the bytes of the records in front of sel[i],
// out_off[sel.size()] = the bytes of all.  Returns false with the largest id in *bad_id when that is >= n_records
// (sel and out_off untouched).
inline bool host_select(const uint32_t *ids, size_t n, const std::vector<uint64_t> &rec_off, std::vector<uint32_t> &sel,
                        std::vector<uint64_t> &out_off, uint64_t *bad_id) {
  const uint64_t n_records = rec_off.empty() ? 0 : rec_off.size() - 1;
  std::vector<uint32_t> s(ids, ids + n);
  std::sort(s.begin(), s.end());
  if (!s.empty() && s.back() >= n_records) {
    *bad_id = s.back();
    return false;
  }
  s.erase(std::unique(s.begin(), s.end()), s.end());
  std::vector<uint64_t> off(s.size() + 1, 0);
  for (size_t i = 0; i < s.size(); ++i) off[i + 1] = off[i] + (rec_off[(size_t)s[i] + 1] - rec_off[s[i]]);
  sel.swap(s);
  out_off.swap(off);
  return true;
}

// the records sel[r0 .. r1) one behind the other at dst (out_off[r1] - out_off[r0] bytes)
inline void host_gather(const char *txt, const std::vector<uint64_t> &rec_off, const std::vector<uint32_t> &sel,
                        const std::vector<uint64_t> &out_off, size_t r0, size_t r1, char *dst) {
  for (size_t r = r0; r < r1; ++r)
    std::memcpy(dst + (out_off[r] - out_off[r0]), txt + rec_off[sel[r]], (size_t)(out_off[r + 1] - out_off[r]));
}

// the end of the piece that starts at record r0: the largest r1 <= m with out_off(r1) - out_off(r0) <= max_bytes
// (r1 == r0: the record at r0 alone is longer).  off(r) reads out_off[r], wherever that lies.
template <class Off>
inline uint64_t piece_end(Off &&off, uint64_t r0, uint64_t m, uint64_t max_bytes) {
  const uint64_t b0 = off(r0);
  uint64_t lo = r0, hi = m;  // off(lo) - b0 <= max_bytes throughout
  if (off(m) - b0 <= max_bytes) return m;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off(mid) - b0 <= max_bytes) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace fq
}  // namespace msw
