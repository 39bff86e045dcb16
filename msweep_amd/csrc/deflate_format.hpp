// deflate_format.hpp -- what a DEFLATE stream (RFC 1951) inside a gzip member (RFC 1952) is made of, for both sides:
// __host__ __device__ under hipcc (the gzip kernels, deflate_kernels.hpp), plain C++ under g++
// (tests/cpp/deflate_format_test.cpp).  The length and distance codes of 3.2.5, code lengths limited to 15 bits from a
// histogram, canonical codes from code lengths (3.2.2), the dynamic block header (3.2.7), the bit order (3.1.1), the
// token of the LZ77 parse, and CRC-32 arithmetic (values of pieces combined with x^(8 n) mod P).
//
// Framing of the stream the kernels write (host_gzip.inc; pigz's independent blocks):
//   gzip header (10 bytes) | per chunk of kChunk bytes of text: one non-final block -- dynamic, or stored where that is
//   not larger -- then an empty stored block (3 zero bits, padding to a byte, 00 00 ff ff): every chunk starts on a
//   byte | final empty fixed block 03 00 | CRC-32 and ISIZE of the text, little-endian.
// No match reaches back across a chunk.  The dynamic header sends all 286 + 30 code lengths as 4-bit codes of a flat
// code-length code (sixteen symbols of length 4: complete, as zlib demands; no run-length symbols): 1338 bits a chunk,
// 0.5 % of 32 KiB.
//
// Nothing here indexes a local array with a run-time index: work areas are passed in (LDS on the device), so the
// kernels stay free of scratch memory (tests/test_deflate_kernel_resources.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MSW_DF_HD __host__ __device__
#else
#define MSW_DF_HD
#include <vector>
#endif

namespace msw {
namespace defl {

constexpr uint32_t kChunk = 32768;  // bytes of text per independently compressed chunk (distances stay below it)
constexpr int kMinMatch = 4, kMaxMatch = 258;
constexpr int kHashBits = 12;       // single-entry buckets keyed by 4 bytes
constexpr int kBatch = 64;          // positions the parse looks up at a time (a wavefront)
constexpr int kNumLit = 286, kNumDist = 30, kNumSyms = kNumLit + kNumDist;
constexpr int kEob = 256;
constexpr int kMaxBits = 15;
// the dynamic header: BFINAL 0, BTYPE 10, HLIT 29 (286 codes), HDIST 29 (30 codes), HCLEN 15 (19 lengths) -- 17 bits,
// LSB first; the 19 code-length code lengths, 3 bits each, in the order 16 17 18 0 8 7 ...: 0 0 0, then sixteen 4s
constexpr uint32_t kHeaderPrefix = 0u | 2u << 1 | 29u << 3 | 29u << 8 | 15u << 13;
constexpr int kHeaderPrefixBits = 17;
constexpr int kHeaderClBits = 19 * 3;
constexpr int kHeaderBits = kHeaderPrefixBits + kHeaderClBits + 4 * kNumSyms;  // 1338
MSW_DF_HD inline uint32_t header_cl_len(int i) { return i < 3 ? 0u : 4u; }  // i-th of the 19, in the order above

// RFC 1951 3.2.5
constexpr uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct Sym {  // a length or distance as the stream carries it: the code's symbol, and `nbits` extra bits of value `extra`
  uint32_t sym, nbits, extra;
};
// the tables above as arithmetic (the kernels keep no table behind a run-time index)
MSW_DF_HD inline Sym length_sym(uint32_t len) {  // 3 ... 258
  if (len == 258) return Sym{285, 0, 0};
  const uint32_t l = len - 3;
  if (l < 8) return Sym{257 + l, 0, 0};
  const uint32_t e = 29u - (uint32_t)__builtin_clz(l);  // floor(log2 l) - 2
  return Sym{257 + 4 * (e + 1) + ((l >> e) - 4), e, l & ((1u << e) - 1)};
}
MSW_DF_HD inline Sym dist_sym(uint32_t dist) {  // 1 ... 32768
  const uint32_t d = dist - 1;
  if (d < 4) return Sym{d, 0, 0};
  const uint32_t e = 30u - (uint32_t)__builtin_clz(d);  // floor(log2 d) - 1
  return Sym{2 * (e + 1) + ((d >> e) & 1), e, d & ((1u << e) - 1)};
}
MSW_DF_HD inline uint32_t lit_extra_bits(uint32_t sym) {  // extra bits of literal/length symbol sym
  return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2;
}
MSW_DF_HD inline uint32_t dist_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

// ---- a token of the parse: a literal byte, or bit 31 | (length - 3) << 16 | (distance - 1)
MSW_DF_HD inline uint32_t token_match(uint32_t len, uint32_t dist) { return 0x80000000u | (len - 3) << 16 | (dist - 1); }
MSW_DF_HD inline bool token_is_match(uint32_t t) { return (t >> 31) != 0; }
MSW_DF_HD inline uint32_t token_len(uint32_t t) { return ((t >> 16) & 0xff) + 3; }
MSW_DF_HD inline uint32_t token_dist(uint32_t t) { return (t & 0x7fff) + 1; }
MSW_DF_HD inline uint32_t hash4(uint32_t four_bytes) { return (four_bytes * 2654435761u) >> (32 - kHashBits); }

// Huffman codes are packed starting from their most significant bit, everything else from the least (3.1.1): a code
// is kept bit-reversed, so that every field goes into the stream LSB first
MSW_DF_HD inline uint32_t reverse_bits(uint32_t code, uint32_t n) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; ++i) r |= ((code >> i) & 1u) << (n - 1 - i);
  return r;
}

// ---- code lengths of at most `limit` bits from a histogram -----------------------------------------------------------
// lens[0 .. n) <- the lengths of a Huffman code for freq[0 .. n) (every freq < 2^23, n <= 512), made to fit `limit`
// bits the way zlib's gen_bitlen does: over-long leaves move up, one leaf of the deepest full level moves down for
// every two.  No symbol used: all zero.  One: length 1.  Two or more: a complete code (Kraft sum exactly 1).
// ws: 5 n + 32 words of work area.
constexpr size_t build_lengths_ws(size_t n) { return 5 * n + 32; }
MSW_DF_HD inline void build_lengths(const uint32_t *freq, int n, int limit, uint8_t *lens, uint32_t *ws) {
  uint32_t *key = ws, *w = ws + n, *par = ws + 3 * n, *cnt = ws + 5 * n;  // w, par: 2 n nodes; cnt: 32
  int m = 0;
  for (int s = 0; s < n; ++s) {
    lens[s] = 0;
    if (freq[s]) key[m++] = freq[s] << 9 | (uint32_t)s;
  }
  if (m == 0) return;
  if (m == 1) {
    lens[key[0] & 511] = 1;
    return;
  }
  for (int i = 1; i < m; ++i) {  // ascending by (frequency, symbol)
    const uint32_t k = key[i];
    int j = i;
    for (; j > 0 && key[j - 1] > k; --j) key[j] = key[j - 1];
    key[j] = k;
  }
  for (int i = 0; i < m; ++i) w[i] = key[i] >> 9;
  // two queues: the sorted leaves and the internal nodes in the order they were made; a leaf wins a tie
  int leaf = 0, node = m;
  for (int next = m; next < 2 * m - 1; ++next) {
    uint32_t sum = 0;
    for (int pick = 0; pick < 2; ++pick) {
      int take;
      if (leaf < m && (node >= next || w[leaf] <= w[node])) take = leaf++;
      else take = node++;
      sum += w[take];
      par[take] = (uint32_t)next;
    }
    w[next] = sum;
  }
  // from here w holds depths, clamped on the way down; every node that was deeper counts, internal ones included
  for (int b = 0; b <= limit; ++b) cnt[b] = 0;
  int overflow = 0;
  w[2 * m - 2] = 0;
  for (int i = 2 * m - 3; i >= 0; --i) {
    uint32_t d = w[par[i]] + 1;
    if (d > (uint32_t)limit) {
      d = (uint32_t)limit;
      ++overflow;
    }
    w[i] = d;
    if (i < m) ++cnt[d];
  }
  while (overflow > 0) {
    int bits = limit - 1;
    while (cnt[bits] == 0) --bits;
    --cnt[bits];
    cnt[bits + 1] += 2;
    --cnt[limit];
    overflow -= 2;
  }
  int i = 0;  // the rarest symbols get the longest codes
  for (int bits = limit; bits >= 1; --bits)
    for (uint32_t k = 0; k < cnt[bits]; ++k) lens[key[i++] & 511] = (uint8_t)bits;
}

// ---- canonical codes (3.2.2): table[s] = bit-reversed code | length << 16; ws: 2 * 16 words -----------------------------
MSW_DF_HD inline void assign_codes(const uint8_t *lens, int n, uint32_t *table, uint32_t *ws) {
  uint32_t *count = ws, *next = ws + 16;
  for (int b = 0; b < 16; ++b) count[b] = 0;
  for (int s = 0; s < n; ++s) ++count[lens[s]];
  count[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) {
    code = (code + count[b - 1]) << 1;
    next[b] = code;
  }
  for (int s = 0; s < n; ++s) {
    const uint32_t l = lens[s];
    table[s] = l ? reverse_bits(next[l]++, l) | l << 16 : 0u;
  }
}

// bits of a chunk as one dynamic block (header, tokens, end of block), from the histogram and the lengths
MSW_DF_HD inline uint32_t symbol_bits(uint32_t sym, uint32_t len) {  // sym: 0 ... 285 literal/length, 286 + d distance
  return len + (sym < (uint32_t)kNumLit ? lit_extra_bits(sym) : dist_extra_bits(sym - kNumLit));
}
// bytes of a chunk of n bytes of text in the stream, the empty stored block behind it included
MSW_DF_HD inline uint32_t dynamic_bytes(uint32_t block_bits) { return (block_bits + 3 + 7) / 8 + 4; }
MSW_DF_HD inline uint32_t stored_bytes(uint32_t n) { return (n > 65535 ? 10 : 5) + n + 5; }

// ---- CRC-32 (reflected, P = 0xedb88320) ---------------------------------------------------------------------------------
// R(s, M): the register after the bytes M from the state s, without the customary inversions.  R is linear:
// R(s, M) = s x^(8 |M|) + R(0, M), so pieces are summed after a multiplication each; crc32(M) = ~R(~0, M).
constexpr uint32_t kCrcPoly = 0xedb88320u;
MSW_DF_HD inline uint32_t crc_word(uint32_t r, uint32_t data, int nbytes) {  // R(r, the low nbytes bytes of data)
  r ^= data;
  for (int i = 0; i < 8 * nbytes; ++i) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
  return r;
}
MSW_DF_HD inline uint32_t gf2_mul(uint32_t a, uint32_t b) {  // a b mod P; x^0 is bit 31
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
// pow8[j] = x^(8 * 2^j) mod P, j < 40
MSW_DF_HD inline void crc_pow_table(uint32_t *pow8) {
  uint32_t p = 0x00800000u;  // x^8
  for (int j = 0; j < 40; ++j) {
    pow8[j] = p;
    p = gf2_mul(p, p);
  }
}
MSW_DF_HD inline uint32_t crc_shift(uint32_t r, uint64_t nbytes, const uint32_t *pow8) {  // r x^(8 nbytes)
  for (int j = 0; nbytes; ++j, nbytes >>= 1)
    if (nbytes & 1) r = gf2_mul(pow8[j], r);
  return r;
}

#if !defined(__HIPCC__)
// ---- host reference encoder (tests): the same parse, codes, header and framing, written plainly ----------------------------
struct BitWriter {
  std::vector<uint8_t> out;
  uint64_t acc = 0;
  int n = 0;
  void put(uint32_t v, int bits) {
    acc |= (uint64_t)v << n;
    n += bits;
    while (n >= 8) {
      out.push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void align() {
    if (n) put(0, 8 - n);
  }
};

inline uint32_t load4(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// The parse of one chunk as the kernel runs it: kBatch positions are looked up at a time against the table as it stood
// before the batch; the positions in front of the first hit are literals, the hit is extended as far as it goes (258
// at most), and every position passed enters the table, where the latest position of a bucket stays.
inline void parse_chunk(const uint8_t *d, uint32_t m, std::vector<uint32_t> &tokens, uint32_t *hist) {
  std::vector<uint32_t> table(1u << kHashBits, 0);
  for (int s = 0; s < kNumSyms; ++s) hist[s] = 0;
  hist[kEob] = 1;
  uint32_t p = 0;
  while (p < m) {
    uint32_t k = m - p < (uint32_t)kBatch ? m - p : (uint32_t)kBatch, src = 0;
    bool hit = false;
    for (uint32_t l = 0; l < k && !hit; ++l) {
      const uint32_t q = p + l;
      if (q + 4 > m) break;
      const uint32_t c = table[hash4(load4(d + q))];
      if (c && q - (c - 1) <= 32768 && load4(d + c - 1) == load4(d + q)) {  // (the distance: always, in chunks of kChunk)
        hit = true;
        k = l;
        src = c - 1;
      }
    }
    for (uint32_t l = 0; l < k; ++l) {
      const uint32_t q = p + l;
      tokens.push_back(d[q]);
      ++hist[d[q]];
      if (q + 4 <= m) table[hash4(load4(d + q))] = q + 1;
    }
    p += k;
    if (!hit) continue;
    const uint32_t maxlen = m - p < (uint32_t)kMaxMatch ? m - p : (uint32_t)kMaxMatch;
    uint32_t len = 4;
    while (len < maxlen && d[src + len] == d[p + len]) ++len;
    tokens.push_back(token_match(len, p - src));
    ++hist[length_sym(len).sym];
    ++hist[kNumLit + dist_sym(p - src).sym];
    for (uint32_t i = 0; i < len; ++i)
      if (p + i + 4 <= m) table[hash4(load4(d + p + i))] = p + i + 1;
    p += len;
  }
}

inline void put_stored(BitWriter &bw, const uint8_t *d, uint32_t n) {
  bw.put(0, 3);
  bw.align();
  bw.put(n, 16);
  bw.put(~n & 0xffffu, 16);
  for (uint32_t i = 0; i < n; ++i) bw.put(d[i], 8);
}

// one chunk (any length below 2^23) and the empty stored block behind it
inline void encode_chunk(BitWriter &bw, const uint8_t *d, uint32_t m, bool stored_only = false) {
  std::vector<uint32_t> tokens, ws(build_lengths_ws(kNumLit));
  uint32_t hist[kNumSyms], table[kNumSyms];
  uint8_t lens[kNumSyms];
  uint32_t bits = kHeaderBits;
  if (!stored_only) {
    parse_chunk(d, m, tokens, hist);
    build_lengths(hist, kNumLit, kMaxBits, lens, ws.data());
    build_lengths(hist + kNumLit, kNumDist, kMaxBits, lens + kNumLit, ws.data());
    assign_codes(lens, kNumLit, table, ws.data());
    assign_codes(lens + kNumLit, kNumDist, table + kNumLit, ws.data());
    for (int s = 0; s < kNumSyms; ++s) bits += hist[s] * symbol_bits((uint32_t)s, lens[s]);
  }
  if (stored_only || dynamic_bytes(bits) >= stored_bytes(m)) {
    const uint32_t first = m < 65535 ? m : 65535;  // two stored blocks where one cannot hold the chunk
    put_stored(bw, d, first);
    if (first < m) put_stored(bw, d + first, m - first);
  } else {
    bw.put(kHeaderPrefix, kHeaderPrefixBits);
    for (int i = 0; i < 19; ++i) bw.put(header_cl_len(i), 3);
    for (int s = 0; s < kNumSyms; ++s) bw.put(reverse_bits(lens[s], 4), 4);
    for (uint32_t t : tokens) {
      if (!token_is_match(t)) {
        bw.put(table[t] & 0xffff, (int)(table[t] >> 16));
        continue;
      }
      const Sym l = length_sym(token_len(t)), ds = dist_sym(token_dist(t));
      bw.put(table[l.sym] & 0xffff, (int)(table[l.sym] >> 16));
      bw.put(l.extra, (int)l.nbits);
      bw.put(table[kNumLit + ds.sym] & 0xffff, (int)(table[kNumLit + ds.sym] >> 16));
      bw.put(ds.extra, (int)ds.nbits);
    }
    bw.put(table[kEob] & 0xffff, (int)(table[kEob] >> 16));
  }
  put_stored(bw, d, 0);
}

// the raw DEFLATE stream of n bytes cut into chunks of `chunk` bytes, closed by the final empty fixed block
inline std::vector<uint8_t> encode(const uint8_t *d, size_t n, uint32_t chunk = kChunk, bool stored_only = false) {
  BitWriter bw;
  for (size_t o = 0; o < n; o += chunk) encode_chunk(bw, d + o, (uint32_t)(n - o < chunk ? n - o : chunk), stored_only);
  bw.put(3, 10);  // 03 00
  bw.align();
  return bw.out;
}
#endif

}  // namespace defl
}  // namespace msw
