// inflate_format.hpp -- reading a DEFLATE stream (RFC 1951) inside a gzip member (RFC 1952) in pieces that can be decoded
// side by side, for both sides: __host__ __device__ under hipcc (the inflate kernels, inflate_kernels.hpp), plain C++
// under g++ (tests/cpp/inflate_format_test.cpp).  The scheme is pugz's / rapidgzip's two passes:
//   the payload is cut into chunks of C bytes; a PROBE looks in every chunk for the first bit position at which a
//   non-final dynamic block plausibly starts (chunk 0 starts at the payload's first bit); a chunk with a start OWNS the
//   stream from there to the next owner's start;
//   pass (a): every owner decodes its blocks against an UNKNOWN window of 32 KiB in front of it: it counts its bytes
//   and keeps the last 32 Ki of them as 16-bit entries -- a byte, or a marker "byte i of the window in front of me";
//   the windows are resolved in owner order (window k read through resolved window k - 1);
//   pass (b): every owner decodes again, writing bytes at its offset; a back-reference in front of the owner reads the
//   resolved window it is handed.
// A probe that accepted a position where no block starts shows in pass (a): the owner in front does not end on it.
// Nothing here vouches for the output: the caller compares CRC-32 and ISIZE with the member's trailer.
//
// The stream is read as 32-bit little-endian words of a zero-padded buffer (bit positions count from the buffer's first
// byte, gzip header included); every loop is bounded by the payload's bit length (a symbol takes at least one bit) and
// by the sink's capacity.  Nothing indexes a local array with a run-time index: the decode tables and the code lengths
// live in a work area that is passed in (LDS on the device), the probe keeps the code-length code in registers.
#pragma once
#include "deflate_format.hpp"

#if !defined(__HIPCC__)
#include <algorithm>
#include <cstring>
#include <vector>
#endif
// (the walk over a file of members is host code under either compiler)
#include <cstring>
#include <vector>

namespace msw {
namespace infl {

constexpr uint32_t kWindow = 32768, kWinMask = kWindow - 1;
constexpr uint16_t kMarker = 0x8000;        // entry of a pass (a) window: kMarker | i = byte i of the window in front
constexpr uint32_t kDefaultChunk = 65536;   // bytes of payload per chunk
constexpr uint32_t kMinChunk = 1024;
constexpr uint64_t kNoStart = ~(uint64_t)0;

// status of an owner's decode
enum : uint32_t { kOk = 0, kErrHeader = 1, kErrSymbol = 2, kErrOverrun = 3, kErrCapacity = 4, kErrDistance = 5, kErrDiffers = 6 };
// why the host path served a file (msw_inflate_info.fallback_reason)
enum : int32_t { kWhyNone = 0, kWhyForced = 1, kWhyHeader = 2, kWhyProbe = 3, kWhyStatus = 4, kWhyCrc = 5, kWhyTrailing = 6, kWhyMemory = 7, kWhyLongSpan = 8 };

// ---- gzip member header and trailer ------------------------------------------------------------------------------------
struct Member {
  bool ok;
  uint64_t payload;      // offset of the DEFLATE stream
  uint32_t crc, isize;   // the trailer: the member's last 8 bytes
};
MSW_DF_HD inline uint32_t le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// p: the member's first `avail` bytes (a header that does not end inside them is not taken); n: the member's length;
// trailer: its last 8 bytes
MSW_DF_HD inline Member parse_member(const uint8_t *p, uint64_t avail, uint64_t n, const uint8_t *trailer) {
  Member m = {false, 0, 0, 0};
  if (n < 18 || avail < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return m;
  const uint32_t flg = p[3];
  if (flg & 0xe0) return m;  // reserved bits
  uint64_t off = 10;
  const uint64_t lim = avail < n - 8 ? avail : n - 8;
  if (flg & 4) {  // FEXTRA
    if (off + 2 > lim) return m;
    off += 2 + (p[off] | (uint64_t)p[off + 1] << 8);
    if (off > lim) return m;
  }
  for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (off < lim && p[off]) ++off;
    if (off >= lim) return m;
    ++off;
  }
  if (flg & 2) off += 2;  // FHCRC
  if (off > lim) return m;
  m.ok = true;
  m.payload = off;
  m.crc = le32(trailer);
  m.isize = le32(trailer + 4);
  return m;
}
MSW_DF_HD inline Member parse_member(const uint8_t *p, uint64_t n) {
  Member m = {false, 0, 0, 0};
  return n < 18 ? m : parse_member(p, n, n, p + n - 8);
}

// ---- the lengths and distances of 3.2.5 from their symbols (deflate_format.hpp's tables as arithmetic) -----------------
MSW_DF_HD inline uint32_t length_base(uint32_t i) {  // i = symbol - 257, 0 ... 28
  if (i < 8) return 3 + i;
  if (i == 28) return 258;
  return 3 + ((4 + (i & 3)) << ((i >> 2) - 1));
}
MSW_DF_HD inline uint32_t dist_base(uint32_t d) {  // 0 ... 29
  if (d < 4) return 1 + d;
  return 1 + ((2 + (d & 1)) << ((d >> 1) - 1));
}
// the order in which the header sends the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
MSW_DF_HD inline uint32_t cl_order(uint32_t i) {
  if (i < 3) return 16 + i;
  if (i == 3) return 0;
  const uint32_t k = (i - 4) >> 1;
  return (i & 1) ? 7 - k : 8 + k;
}

// ---- the bit stream ----------------------------------------------------------------------------------------------------
struct Stream {
  const uint32_t *w;   // the file's bytes as little-endian words, readable (and zero) up to n_words
  uint64_t n_words;
  uint64_t end_bit;    // first bit behind the DEFLATE payload's last byte (the trailer's first bit)
};
MSW_DF_HD inline uint32_t stream_word(const Stream &s, uint64_t i) { return i < s.n_words ? s.w[i] : 0u; }
// at least 33 bits from bit position pos
MSW_DF_HD inline uint64_t stream_peek(const Stream &s, uint64_t pos) {
  const uint64_t i = pos >> 5;
  const uint64_t v = (uint64_t)stream_word(s, i + 1) << 32 | stream_word(s, i);
  return v >> (pos & 31);
}

// a reader that keeps 33 ... 64 bits in a register and the next word on its way
struct BitIn {
  uint64_t buf, next;
  uint32_t cnt, ahead;
};
MSW_DF_HD inline void bits_fill(BitIn &b, const Stream &s) {
  if (b.cnt <= 32) {
    b.buf |= (uint64_t)b.ahead << b.cnt;
    b.cnt += 32;
    b.ahead = stream_word(s, b.next++);
  }
}
MSW_DF_HD inline void bits_open(BitIn &b, const Stream &s, uint64_t pos) {
  const uint64_t i = pos >> 5;
  const uint32_t sh = (uint32_t)(pos & 31);
  b.buf = stream_word(s, i) >> sh;
  b.cnt = 32 - sh;
  b.ahead = stream_word(s, i + 1);
  b.next = i + 2;
  bits_fill(b, s);
}
MSW_DF_HD inline uint64_t bits_pos(const BitIn &b) { return 32 * (b.next - 1) - b.cnt; }
MSW_DF_HD inline uint32_t bits_take(BitIn &b, uint32_t n) {  // n <= 32, and no more than 32 bits between two fills
  const uint32_t v = (uint32_t)(b.buf & (((uint64_t)1 << n) - 1));
  b.buf >>= n;
  b.cnt -= n;
  return v;
}

// ---- canonical decode tables in a work area ---------------------------------------------------------------------------
// fast[bits] = symbol << 4 | length for codes of at most `fastbits` bits (0: longer, or no code); longer codes are walked
// length by length through count[] and the symbols sorted by (length, symbol).
struct Huff {
  uint16_t *fast, *count, *offs, *sym;
  uint32_t fastbits;
};
constexpr uint32_t kLitFast = 10, kDistFast = 8;
constexpr uint32_t kLitSyms = 288, kDistSyms = 32;
// the work area in 16-bit units: the literal/length table, the distance table (the code-length code's while a header is
// read), the code lengths (one per byte)
constexpr uint32_t kWsLit = 0, kWsLitSize = (1u << kLitFast) + 32 + kLitSyms;
constexpr uint32_t kWsDist = kWsLit + kWsLitSize, kWsDistSize = (1u << kDistFast) + 32 + kDistSyms;
constexpr uint32_t kWsLens = kWsDist + kWsDistSize, kWsLensSize = (kLitSyms + kDistSyms + 1) / 2;
constexpr uint32_t kWsSize = kWsLens + kWsLensSize;  // 1824 entries, 3648 bytes
struct Tables {
  Huff lit, dist;
  uint8_t *lens;
};
MSW_DF_HD inline Tables tables_in(uint16_t *ws) {
  Tables t;
  t.lit = Huff{ws + kWsLit, ws + kWsLit + (1u << kLitFast), ws + kWsLit + (1u << kLitFast) + 16, ws + kWsLit + (1u << kLitFast) + 32, kLitFast};
  t.dist = Huff{ws + kWsDist, ws + kWsDist + (1u << kDistFast), ws + kWsDist + (1u << kDistFast) + 16, ws + kWsDist + (1u << kDistFast) + 32, kDistFast};
  t.lens = reinterpret_cast<uint8_t *>(ws + kWsLens);
  return t;
}
// what is left of the code space in units of 2^-15 (0: complete; > 0: incomplete; < 0: over-subscribed, no table);
// *n_used = symbols with a code
MSW_DF_HD inline int huff_build(const uint8_t *lens, uint32_t n, const Huff &h, uint32_t *n_used) {
  for (uint32_t l = 0; l < 16; ++l) h.count[l] = 0;
  for (uint32_t s = 0; s < n; ++s) ++h.count[lens[s] & 15];
  *n_used = n - h.count[0];
  int left = 1;
  for (uint32_t l = 1; l < 16; ++l) {
    left = 2 * left - (int)h.count[l];
    if (left < 0) return -1;
  }
  h.offs[1] = 0;
  for (uint32_t l = 1; l < 15; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t l = lens[s] & 15;
    if (l) h.sym[h.offs[l]++] = (uint16_t)s;
  }
  const uint32_t size = 1u << h.fastbits;
  for (uint32_t i = 0; i < size; ++i) h.fast[i] = 0;
  uint32_t code = 0, idx = 0;
  for (uint32_t l = 1; l <= h.fastbits; ++l) {
    const uint32_t c = h.count[l];
    for (uint32_t k = 0; k < c; ++k, ++code) {
      const uint16_t e = (uint16_t)(h.sym[idx++] << 4 | l);
      for (uint32_t j = defl::reverse_bits(code, l); j < size; j += 1u << l) h.fast[j] = e;
    }
    code <<= 1;
  }
  return left;
}
// the next symbol, or -1 where the bits are no code; at least 15 bits are in the register
MSW_DF_HD inline int huff_decode(const Huff &h, BitIn &b) {
  const uint32_t e = h.fast[(uint32_t)b.buf & ((1u << h.fastbits) - 1)];
  if (e & 15) {
    bits_take(b, e & 15);
    return (int)(e >> 4);
  }
  uint32_t bits = (uint32_t)b.buf;
  int code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (int)(bits & 1);
    bits >>= 1;
    const int c = h.count[l];
    if (code - c < first) {
      bits_take(b, l);
      return h.sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return -1;
}

// ---- a block header (3.2.3 - 3.2.7): tables for the block's symbols, or the length of a stored block ----------------
struct BlockHead {
  uint32_t status, final, type, stored_len;
};
// zlib's rule for a code set: complete, or nothing at all (distances only), or one code of one bit
MSW_DF_HD inline bool code_set_ok(int left, uint32_t n_used, const Huff &h, bool may_be_empty) {
  if (left < 0) return false;
  if (left == 0) return true;
  if (n_used == 0) return may_be_empty;
  return n_used == 1 && h.count[1] == 1;
}
MSW_DF_HD inline BlockHead read_block_head(const Stream &s, BitIn &b, const Tables &t) {
  BlockHead bh = {kOk, 0, 0, 0};
  bits_fill(b, s);
  if (bits_pos(b) + 3 > s.end_bit) {
    bh.status = kErrOverrun;
    return bh;
  }
  bh.final = bits_take(b, 1);
  bh.type = bits_take(b, 2);
  uint32_t n_used = 0;
  if (bh.type == 0) {
    bits_take(b, (uint32_t)((0 - bits_pos(b)) & 7));
    bits_fill(b, s);
    const uint32_t len = bits_take(b, 16), nlen = bits_take(b, 16);
    if ((len ^ 0xffffu) != nlen || bits_pos(b) + 8ull * len > s.end_bit) bh.status = kErrHeader;
    bh.stored_len = len;
    return bh;
  }
  if (bh.type == 1) {
    for (uint32_t i = 0; i < kLitSyms; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (uint32_t i = 0; i < 30; ++i) t.lens[kLitSyms + i] = 5;
    (void)huff_build(t.lens, kLitSyms, t.lit, &n_used);
    (void)huff_build(t.lens + kLitSyms, 30, t.dist, &n_used);  // (30 and 31 have no code here: they decode to an error)
    return bh;
  }
  if (bh.type == 3) {
    bh.status = kErrHeader;
    return bh;
  }
  const uint32_t hlit = bits_take(b, 5) + 257, hdist = bits_take(b, 5) + 1, hclen = bits_take(b, 4) + 4;
  if (hlit > 286 || hdist > 30) {
    bh.status = kErrHeader;
    return bh;
  }
  for (uint32_t i = 0; i < 19; ++i) {
    if ((i & 7) == 0) bits_fill(b, s);
    t.lens[cl_order(i)] = (uint8_t)(i < hclen ? bits_take(b, 3) : 0);
  }
  // (the code-length code sits in the distance table's area until the lengths are read)
  Huff cl = t.dist;
  cl.fastbits = 7;
  if (huff_build(t.lens, 19, cl, &n_used) != 0) {
    bh.status = kErrHeader;
    return bh;
  }
  const uint32_t total = hlit + hdist;
  uint32_t i = 0;
  while (i < total) {
    bits_fill(b, s);
    if (bits_pos(b) > s.end_bit) {
      bh.status = kErrOverrun;
      return bh;
    }
    const int c = huff_decode(cl, b);
    if (c < 0) {
      bh.status = kErrHeader;
      return bh;
    }
    if (c < 16) {
      t.lens[i++] = (uint8_t)c;
      continue;
    }
    uint32_t val = 0, rep;
    if (c == 16) {
      if (i == 0) {
        bh.status = kErrHeader;
        return bh;
      }
      val = t.lens[i - 1];
      rep = 3 + bits_take(b, 2);
    } else if (c == 17) {
      rep = 3 + bits_take(b, 3);
    } else {
      rep = 11 + bits_take(b, 7);
    }
    if (i + rep > total) {
      bh.status = kErrHeader;
      return bh;
    }
    for (uint32_t k = 0; k < rep; ++k) t.lens[i++] = (uint8_t)val;
  }
  if (t.lens[256] == 0) {
    bh.status = kErrHeader;
    return bh;
  }
  // (the distance lengths leave their place behind the literal/length ones before that table's area is written: the
  // code-length code is done with)
  int left = huff_build(t.lens, hlit, t.lit, &n_used);
  if (!code_set_ok(left, n_used, t.lit, false)) {
    bh.status = kErrHeader;
    return bh;
  }
  left = huff_build(t.lens + hlit, hdist, t.dist, &n_used);
  if (!code_set_ok(left, n_used, t.dist, true)) bh.status = kErrHeader;
  return bh;
}

// ---- the block-start probe: does a non-final dynamic block plausibly start at bit p? -------------------------------------
// Cheapest test first: the three header bits (one position in eight passes), HLIT and HDIST, the code-length code's
// Kraft sum (exactly 1), then the length sequence -- no overrun, no repeat of a previous length at its head -- with the
// Kraft sums of both codes taken on the way: literal/length complete with a code for the end of block, distances
// complete or a single code of one bit.  The code-length code is held in registers: its lengths 3 bits each in one
// word, its symbols sorted by (length, symbol) 5 bits each in two.
MSW_DF_HD inline bool probe_block_start(const Stream &s, uint64_t p) {
  if (p + 17 + 12 + 2 > s.end_bit) return false;
  uint64_t v = stream_peek(s, p);
  if ((v & 7) != 4) return false;  // BFINAL 0, BTYPE 10 (LSB first)
  const uint32_t hlit = (uint32_t)(v >> 3) & 31, hdist = (uint32_t)(v >> 8) & 31, hclen = ((uint32_t)(v >> 13) & 15) + 4;
  if (hlit > 29 || hdist > 29) return false;
  uint64_t q = p + 17;
  if (q + 3 * hclen > s.end_bit) return false;
  uint64_t cl_lens = 0, cl_count = 0;  // 3 bits per symbol; 8 bits per length
  uint32_t kraft = 0;
  for (uint32_t i = 0; i < hclen; ++i) {
    if (i % 10 == 0) v = stream_peek(s, q + 3 * i);
    const uint32_t l = (uint32_t)(v >> (3 * (i % 10))) & 7;
    if (l) {
      kraft += 128u >> l;
      cl_lens |= (uint64_t)l << (3 * cl_order(i));
      cl_count += (uint64_t)1 << (8 * l);
    }
  }
  if (kraft != 128) return false;
  q += 3 * hclen;
  uint64_t sorted0 = 0, sorted1 = 0;
  uint32_t n_sorted = 0;
  for (uint32_t l = 1; l < 8; ++l)
    for (uint32_t c = 0; c < 19; ++c)
      if (((cl_lens >> (3 * c)) & 7) == l) {
        if (n_sorted < 12) sorted0 |= (uint64_t)c << (5 * n_sorted);
        else sorted1 |= (uint64_t)c << (5 * (n_sorted - 12));
        ++n_sorted;
      }
  const uint32_t n_lit = hlit + 257, total = n_lit + hdist + 1;
  uint32_t i = 0, prev = 0, kraft_lit = 0, kraft_dist = 0, n_dist = 0, len_eob = 0;
  while (i < total) {
    if (q + 14 > s.end_bit) return false;
    v = stream_peek(s, q);
    uint32_t bits = (uint32_t)v, code = 0, first = 0, index = 0, l = 1, c = 19;
    for (; l < 8; ++l) {
      code |= bits & 1;
      bits >>= 1;
      const uint32_t cnt = (uint32_t)(cl_count >> (8 * l)) & 255;
      if (code < first + cnt) {
        const uint32_t k = index + (code - first);
        c = (uint32_t)(k < 12 ? sorted0 >> (5 * k) : sorted1 >> (5 * (k - 12))) & 31;
        break;
      }
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
    if (c > 18) return false;  // (never: the code is complete)
    q += l;
    uint32_t val = 0, rep = 1;
    if (c < 16) {
      val = c;
    } else if (c == 16) {
      if (i == 0) return false;
      val = prev;
      rep = 3 + (bits & 3);
      q += 2;
    } else if (c == 17) {
      rep = 3 + (bits & 7);
      q += 3;
    } else {
      rep = 11 + (bits & 127);
      q += 7;
    }
    if (i + rep > total) return false;
    prev = val;
    if (val) {
      const uint32_t in_lit = i >= n_lit ? 0 : (i + rep <= n_lit ? rep : n_lit - i), in_dist = rep - in_lit;
      kraft_lit += in_lit * (32768u >> val);
      kraft_dist += in_dist * (32768u >> val);
      n_dist += in_dist;
      if (i <= 256 && 256 < i + rep) len_eob = val;
      if (kraft_lit > 32768 || kraft_dist > 32768) return false;
    }
    i += rep;
  }
  if (len_eob == 0 || kraft_lit != 32768) return false;
  return kraft_dist == 32768 || (n_dist == 1 && kraft_dist == 16384);
}

// ---- the symbols of a block, into a sink ----------------------------------------------------------------------------------
// Sink: bool lit(uint32_t byte); bool copy(uint32_t len, uint32_t dist)  (false: the capacity is used up, or the distance
// reaches in front of the stream)
template <class Sink>
MSW_DF_HD inline uint32_t inflate_symbols(const Stream &s, BitIn &b, const Tables &t, Sink &sink) {
  for (;;) {  // (every pass takes at least one bit, and ends behind the payload)
    bits_fill(b, s);
    if (bits_pos(b) > s.end_bit) return kErrOverrun;
    const int c = huff_decode(t.lit, b);
    if (c < 0) return kErrSymbol;
    if (c < 256) {
      if (!sink.lit((uint32_t)c)) return sink.why;
      continue;
    }
    if (c == 256) return bits_pos(b) > s.end_bit ? kErrOverrun : kOk;
    if (c > 285) return kErrSymbol;
    const uint32_t li = (uint32_t)c - 257;
    const uint32_t len = length_base(li) + bits_take(b, defl::lit_extra_bits((uint32_t)c));
    bits_fill(b, s);
    const int d = huff_decode(t.dist, b);
    if (d < 0 || d > 29) return kErrSymbol;
    const uint32_t dist = dist_base((uint32_t)d) + bits_take(b, defl::dist_extra_bits((uint32_t)d));
    if (!sink.copy(len, dist)) return sink.why;
  }
}
template <class Sink>
MSW_DF_HD inline uint32_t inflate_stored(const Stream &s, BitIn &b, uint32_t len, Sink &sink) {
  for (uint32_t i = 0; i < len; ++i) {  // (len <= 65535, and the header saw that the bytes are there)
    if ((i & 3) == 0) bits_fill(b, s);
    if (!sink.lit(bits_take(b, 8))) return sink.why;
  }
  return kOk;
}

// The sinks serve `width` lanes that run the same decode in lock step (a wavefront on the device; one, lane 0, on the
// host): every lane holds the same count, lane 0 writes a literal, and a match is copied `width` bytes a step, lane l
// taking the bytes l, l + width, ...  Byte i of a match is byte i mod dist of the dist bytes in front of it, so no lane
// reads what the copy itself writes.
// pass (a): counts, and keeps the last 32 Ki bytes as entries of a ring that starts out as the markers 0 ... 32767
struct WindowSink {
  uint16_t *ring;
  uint64_t count, cap;
  uint32_t why;
  bool first;  // the stream's first owner: nothing lies in front of it
  uint32_t lane, width;
  MSW_DF_HD bool lit(uint32_t byte) {
    if (count >= cap) {
      why = kErrCapacity;
      return false;
    }
    if (lane == 0) ring[count & kWinMask] = (uint16_t)byte;
    ++count;
    return true;
  }
  MSW_DF_HD bool copy(uint32_t len, uint32_t dist) {
    if (count + len > cap) {
      why = kErrCapacity;
      return false;
    }
    if (first && dist > count) {
      why = kErrDistance;
      return false;
    }
    for (uint32_t i = lane; i < len; i += width)
      ring[(count + i) & kWinMask] = ring[(count - dist + (i < dist ? i : i % dist)) & kWinMask];
    count += len;
    return true;
  }
};
// pass (b): bytes to out[0 .. cap); the ring starts out as the resolved window in front of the owner
struct FinalSink {
  uint8_t *ring, *out;
  uint64_t count, cap;
  uint32_t why;
  bool first;
  uint32_t lane, width;
  MSW_DF_HD bool lit(uint32_t byte) {
    if (count >= cap) {
      why = kErrCapacity;
      return false;
    }
    if (lane == 0) {
      ring[count & kWinMask] = (uint8_t)byte;
      out[count] = (uint8_t)byte;
    }
    ++count;
    return true;
  }
  MSW_DF_HD bool copy(uint32_t len, uint32_t dist) {
    if (count + len > cap) {
      why = kErrCapacity;
      return false;
    }
    if (first && dist > count) {
      why = kErrDistance;
      return false;
    }
    for (uint32_t i = lane; i < len; i += width) {
      const uint8_t v = ring[(count - dist + (i < dist ? i : i % dist)) & kWinMask];
      ring[(count + i) & kWinMask] = v;
      out[count + i] = v;
    }
    count += len;
    return true;
  }
};

// what an owner's decode leaves: the status, the bit behind its last block, whether that block was the final one
struct OwnerEnd {
  uint32_t status, final;
  uint64_t end_bit;
};
// block after block from bit `start`, up to the first block boundary at or behind `stop` (kNoStart: to the final block)
template <class Sink>
MSW_DF_HD inline OwnerEnd inflate_owner(const Stream &s, uint64_t start, uint64_t stop, const Tables &t, Sink &sink) {
  OwnerEnd e = {kOk, 0, start};
  BitIn b;
  bits_open(b, s, start);
  for (;;) {  // (every block takes at least three bits)
    e.end_bit = bits_pos(b);
    if (e.end_bit >= stop) return e;
    const BlockHead bh = read_block_head(s, b, t);
    e.status = bh.status;
    if (e.status == kOk) e.status = bh.type == 0 ? inflate_stored(s, b, bh.stored_len, sink) : inflate_symbols(s, b, t, sink);
    e.end_bit = bits_pos(b);
    if (e.status != kOk) return e;
    if (bh.final) {
      e.final = 1;
      return e;
    }
  }
}

// window k (markers) read through the resolved window k - 1
MSW_DF_HD inline uint8_t resolve_entry(uint16_t e, const uint8_t *prev) { return (e & kMarker) ? prev[e & kWinMask] : (uint8_t)e; }

// ---- files of members that declare their own lengths: BGZF (htslib's blocked gzip, what bgzip writes) -------------------
// A BGZF member's header carries an extra subfield 'B' 'C' of two bytes, BSIZE = the member's length - 1; its trailer
// states CRC-32 and length of at most 64 KiB of text; it starts with an empty window.  So a walk over headers and trailers
// alone gives every member's payload and its place in the text before anything is decoded: one decode per member, side
// by side, checked per member (inflate_member_kernels.hpp; members_reference below runs the same steps on one thread).
constexpr uint32_t kMemberMaxText = 65536;
struct MemberEntry {
  uint64_t first_bit, end_bit;  // the payload's first bit; the bit behind its last byte (the trailer's first bit)
  uint64_t text_off;            // exclusive prefix sum of the members' ISIZE
  uint32_t crc, isize;          // the trailer
};
// BSIZE of the header in p[0 .. avail): magic, CM 8, FEXTRA, and the subfield 'B' 'C' of length 2 found by walking the
// extra field's subfields, which must fill it exactly
MSW_DF_HD inline bool member_bsize(const uint8_t *p, uint64_t avail, uint32_t *bsize) {
  if (avail < 12 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4) || (p[3] & 0xe0)) return false;
  const uint64_t end = 12 + (p[10] | (uint64_t)p[11] << 8);
  if (end > avail) return false;
  bool found = false;
  uint64_t at = 12;
  while (at < end) {  // (every subfield takes at least four bytes)
    if (at + 4 > end) return false;
    const uint64_t slen = p[at + 2] | (uint64_t)p[at + 3] << 8;
    if (at + 4 + slen > end) return false;
    if (!found && p[at] == 66 && p[at + 1] == 67 && slen == 2) {
      *bsize = p[at + 4] | (uint32_t)p[at + 5] << 8;
      found = true;
    }
    at += 4 + slen;
  }
  return found;
}
// a member's stream ends at its own trailer: nothing behind it is read as payload (words from there on read as zero)
MSW_DF_HD inline Stream member_stream(const uint32_t *w, uint64_t n_words, const MemberEntry &m) {
  const uint64_t own = (m.end_bit + 31) / 32;
  return Stream{w, own < n_words ? own : n_words, m.end_bit};
}
// what a member's decode (inflate_owner from first_bit to the final block, FinalSink with cap = ISIZE and first = true)
// must have left, in front of the CRC: kWhyNone, or the reason the host path serves the file
MSW_DF_HD inline int32_t member_verdict(const OwnerEnd &e, uint64_t count, const MemberEntry &m) {
  if (e.status != kOk || !e.final) return kWhyStatus;
  if ((e.end_bit + 7) / 8 * 8 != m.end_bit) return kWhyTrailing;  // the final block ends in the member's last payload byte
  if (count != m.isize) return kWhyCrc;
  return kWhyNone;
}
// (host code from here on, under either compiler)
struct MemberTable {
  std::vector<MemberEntry> members;
  uint64_t text_bytes = 0, payload_bytes = 0;  // sum of ISIZE; sum of the DEFLATE payloads' bytes
};
// bytes in memory as the walk's source (a file: pread, host_inflate_members.inc)
struct BufferFetch {
  const uint8_t *p;
  uint64_t n;
  bool operator()(uint64_t off, size_t len, uint8_t *dst) const {
    if (off > n || len > n - off) return false;
    std::memcpy(dst, p + off, len);
    return true;
  }
};
// The member table of a file of n bytes, or false: "not BGZF".  fetch(off, len, dst) reads len bytes at off (off + len
// <= n).  Every member must qualify -- member_bsize's header with the other optional fields as parse_member takes them,
// BSIZE + 1 >= header + 8, the member inside the file, ISIZE <= 64 KiB -- and the walk (next member at offset + BSIZE + 1)
// must land exactly on the end of the file: a plain member anywhere, trailing bytes or a cut last member refuse the whole
// file.  Members of ISIZE 0 (BGZF's end-of-file marker, at the end or inside a concatenation) are ordinary members.
// Only headers and trailers are read: a trailer and the header behind it in one fetch.
template <class Fetch>
inline bool walk_members(Fetch &&fetch, uint64_t n, MemberTable &T) {
  T.members.clear();
  T.text_bytes = T.payload_bytes = 0;
  constexpr uint64_t kAhead = 8 + 32;  // a trailer and the usual header (18 bytes) behind it
  std::vector<uint8_t> win((size_t)kAhead);
  uint64_t win_off = 0, win_len = 0;
  auto view = [&](uint64_t off, uint64_t len) -> const uint8_t * {  // (off + len <= n)
    if (off < win_off || off + len > win_off + win_len) {
      uint64_t want = len > kAhead ? len : kAhead;
      if (want > n - off) want = n - off;
      if (win.size() < want) win.resize((size_t)want);
      if (!fetch(off, (size_t)want, win.data())) return nullptr;
      win_off = off, win_len = want;
    }
    return win.data() + (off - win_off);
  };
  uint64_t off = 0;
  while (off < n) {
    if (n - off < 18 + 8) return false;
    uint64_t avail = n - off < 32 ? n - off : 32;
    const uint8_t *p = view(off, avail);
    if (!p) return false;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
    // an extra field longer than the usual one, or names / a header CRC behind it: the whole header (a member is at
    // most 64 KiB)
    if (12 + (p[10] | (uint64_t)p[11] << 8) > avail || (p[3] & 0x1a)) {
      avail = n - off < 65536 ? n - off : 65536;
      if (!(p = view(off, avail))) return false;
    }
    uint32_t bsize = 0;
    if (!member_bsize(p, avail, &bsize)) return false;
    const uint64_t msize = (uint64_t)bsize + 1;
    if (msize > n - off) return false;
    static const uint8_t no_trailer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const Member m = parse_member(p, avail < msize ? avail : msize, msize, no_trailer);  // (n >= 18, payload <= n - 8)
    if (!m.ok) return false;
    const uint8_t *tr = view(off + msize - 8, 8);  // (p is gone from here on)
    if (!tr) return false;
    const uint32_t crc = le32(tr), isize = le32(tr + 4);
    if (isize > kMemberMaxText) return false;
    T.members.push_back(MemberEntry{8 * (off + m.payload), 8 * (off + msize - 8), T.text_bytes, crc, isize});
    T.text_bytes += isize;
    T.payload_bytes += msize - 8 - m.payload;
    off += msize;
  }
  return !T.members.empty();
}

#if !defined(__HIPCC__)
// ---- the plain reference: the kernels' steps, one thread ----------------------------------------------------------------
struct Reference {
  int32_t why = kWhyNone;      // kWhyNone: `text` is the member's text and has the trailer's CRC-32 and length
  std::vector<uint8_t> text;
  std::vector<uint64_t> starts;  // per chunk: the start the probe found, or kNoStart
  uint32_t n_chunks = 0, n_starts = 0;
  uint32_t bad_status = 0;
};
inline uint32_t crc32_plain(const uint8_t *p, size_t n) {
  static uint32_t table[256];
  if (!table[1])
    for (uint32_t i = 0; i < 256; ++i) table[i] = defl::crc_word(0, i, 1);
  uint32_t r = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) r = table[(r ^ p[i]) & 0xff] ^ (r >> 8);
  return ~r;
}
inline Reference inflate_reference(const uint8_t *gz, size_t n, size_t chunk = kDefaultChunk) {
  Reference R;
  const Member m = parse_member(gz, n);
  if (!m.ok) {
    R.why = kWhyHeader;
    return R;
  }
  std::vector<uint32_t> words((n + 3) / 4 + 4, 0);
  std::memcpy(words.data(), gz, n);
  const Stream s = {words.data(), words.size(), 8 * (uint64_t)(n - 8)};
  const uint64_t first_bit = 8 * m.payload, payload = n - 8 - m.payload;
  if (chunk < kMinChunk) chunk = kMinChunk;
  R.n_chunks = (uint32_t)std::max<uint64_t>(1, (payload + chunk - 1) / chunk);
  R.starts.assign(R.n_chunks, kNoStart);
  R.starts[0] = first_bit;
  for (uint32_t c = 1; c < R.n_chunks; ++c) {
    const uint64_t lo = first_bit + 8 * (uint64_t)c * chunk, hi = std::min<uint64_t>(lo + 8 * (uint64_t)chunk, s.end_bit);
    for (uint64_t p = lo; p < hi; ++p)
      if (probe_block_start(s, p)) {
        R.starts[c] = p;
        break;
      }
  }
  struct Own {
    uint64_t start, stop, bytes;
    OwnerEnd end;
  };
  std::vector<Own> own;
  for (uint64_t st : R.starts)
    if (st != kNoStart) own.push_back(Own{st, kNoStart, 0, {}});
  R.n_starts = (uint32_t)own.size();
  for (size_t k = 0; k + 1 < own.size(); ++k) own[k].stop = own[k + 1].start;
  // pass (a)
  std::vector<uint16_t> ws(kWsSize), ring(kWindow);
  const Tables t = tables_in(ws.data());
  std::vector<std::vector<uint16_t>> windows(own.size());
  const uint64_t cap = (uint64_t)1 << 40;
  for (size_t k = 0; k < own.size(); ++k) {
    for (uint32_t i = 0; i < kWindow; ++i) ring[i] = (uint16_t)(kMarker | i);
    WindowSink sink = {ring.data(), 0, cap, kOk, k == 0, 0, 1};
    own[k].end = inflate_owner(s, own[k].start, own[k].stop, t, sink);
    own[k].bytes = sink.count;
    if (own[k].end.status != kOk) {
      R.why = kWhyStatus;
      R.bad_status = own[k].end.status;
      return R;
    }
    const bool last = k + 1 == own.size();
    if (!last && own[k].end.final) {  // the member ends in front of the last owner: what follows is not its payload
      R.why = kWhyTrailing;
      return R;
    }
    if (last ? !own[k].end.final : own[k].end.end_bit != own[k].stop) {
      R.why = kWhyProbe;
      return R;
    }
    windows[k].resize(kWindow);
    for (uint32_t j = 0; j < kWindow; ++j) windows[k][j] = ring[(sink.count + j) & kWinMask];
  }
  if ((own.back().end.end_bit + 7) / 8 * 8 != s.end_bit) {
    R.why = kWhyTrailing;
    return R;
  }
  // offsets; the window chain
  std::vector<uint64_t> off(own.size() + 1, 0);
  for (size_t k = 0; k < own.size(); ++k) off[k + 1] = off[k] + own[k].bytes;
  std::vector<std::vector<uint8_t>> resolved(own.size(), std::vector<uint8_t>(kWindow, 0));
  std::vector<uint8_t> zeros(kWindow, 0);
  for (size_t k = 0; k < own.size(); ++k)
    for (uint32_t j = 0; j < kWindow; ++j) resolved[k][j] = resolve_entry(windows[k][j], k ? resolved[k - 1].data() : zeros.data());
  // pass (b)
  R.text.assign(off.back(), 0);
  std::vector<uint8_t> ring8(kWindow);
  for (size_t k = 0; k < own.size(); ++k) {
    std::memcpy(ring8.data(), k ? resolved[k - 1].data() : zeros.data(), kWindow);
    FinalSink sink = {ring8.data(), R.text.data() + off[k], 0, own[k].bytes, kOk, k == 0, 0, 1};
    const OwnerEnd e = inflate_owner(s, own[k].start, own[k].stop, t, sink);
    if (e.status != kOk || sink.count != own[k].bytes || e.end_bit != own[k].end.end_bit) {
      R.why = kWhyStatus;
      R.bad_status = e.status ? e.status : kErrDiffers;
      R.text.clear();
      return R;
    }
  }
  if (crc32_plain(R.text.data(), R.text.size()) != m.crc || (uint32_t)R.text.size() != m.isize) {
    R.why = kWhyCrc;
    R.text.clear();
  }
  return R;
}

// ---- the plain reference for a file of members: the member kernel's steps, one thread -----------------------------------
struct MembersReference {
  int32_t why = kWhyNone;  // kWhyNone: `text` is the file's text, every member's with its trailer's CRC-32 and length
  std::vector<uint8_t> text;
  uint32_t n_members = 0;
  uint32_t bad_member = 0, bad_status = 0;  // the first member that failed, and its decode's status
  uint64_t payload_bytes = 0;
};
inline MembersReference members_reference(const uint8_t *gz, size_t n) {
  MembersReference R;
  MemberTable T;
  if (!walk_members(BufferFetch{gz, n}, n, T)) {
    R.why = kWhyHeader;  // not BGZF
    return R;
  }
  R.n_members = (uint32_t)T.members.size();
  R.payload_bytes = T.payload_bytes;
  std::vector<uint32_t> words((n + 3) / 4 + 4, 0);
  std::memcpy(words.data(), gz, n);
  std::vector<uint16_t> ws(kWsSize);
  const Tables t = tables_in(ws.data());
  std::vector<uint8_t> ring(kWindow);
  R.text.assign(T.text_bytes, 0);
  for (size_t k = 0; k < T.members.size(); ++k) {
    const MemberEntry &m = T.members[k];
    const Stream s = member_stream(words.data(), words.size(), m);
    FinalSink sink = {ring.data(), R.text.data() + m.text_off, 0, m.isize, kOk, true, 0, 1};
    const OwnerEnd e = inflate_owner(s, m.first_bit, kNoStart, t, sink);
    int32_t why = member_verdict(e, sink.count, m);
    if (why == kWhyNone && crc32_plain(R.text.data() + m.text_off, m.isize) != m.crc) why = kWhyCrc;
    if (why != kWhyNone) {
      R.why = why;
      R.bad_member = (uint32_t)k;
      R.bad_status = e.status;
      R.text.clear();
      return R;
    }
  }
  return R;
}
#endif

}  // namespace infl
}  // namespace msw
