// deflate_kernels.hpp -- gzip on the device (msw_core_gzip_* / msw_core_text_block_gzip, host_gzip.inc): with
// --compress z the file's bytes are the compressed ones, so the compressor runs where the text lies (a block's finished
// text, text_kernels.hpp, or uploaded host bytes) and only its output crosses the link.  Format, framing and the arithmetic shared with the host: deflate_format.hpp.
//
// The text is cut into chunks of 32 KiB that are compressed independently, a wavefront each (wave64: __ballot is 64 bits
// wide), in the text kernels' length pass / scan / write pass:
//   k_gz_parse  the chunk in LDS; greedy LZ77 through single-entry hash buckets keyed by 4 bytes: the wavefront looks up
//               64 positions at a time against the table as it stood before the batch, the positions in front of the
//               first hit are literals, the hit is extended 64 bytes a step (258 at most), and every position passed
//               enters the table with atomicMax -- the latest position of a bucket stays, whatever the order.  Tokens go
//               to a device scratch (4 bytes each, at most one per byte of text); the histograms, the code lengths
//               (15 bits at most) and the canonical codes follow on lane 0 with the routines the host tests, and the
//               exact size of the chunk as a dynamic block decides between that and a stored one.
//   (host: exclusive scan of the chunks' byte lengths -> byte offset of every chunk, rocprim)
//   k_gz_emit   header and codes at the chunk's offset: a wave scan of the token widths gives every token its bit
//               position, the bits are ORed into an LDS image of the chunk's output (OR commutes), and the image
//               leaves as whole dwords (text_flush).
//   k_gz_crc    CRC-32 of the text: the register value of every 256-byte piece from a zero state, multiplied by
//               x^(8 n) mod P for the n bytes behind it, all XORed together.
// The compressed bytes are a function of the text, the chunk size and the call boundaries alone.  No kernel uses
// scratch memory; the parse holds 51 KiB of LDS (three workgroups a CU), the emit pass 34 KiB
// (tests/test_deflate_kernel_resources.py).
#pragma once
#include "common.hpp"
#include "deflate_format.hpp"
#include "text_kernels.hpp"

namespace msw {

constexpr uint32_t kGzChunk = defl::kChunk;
constexpr int kGzSyms = defl::kNumSyms;
constexpr int kGzCrcPiece = 256;
static_assert(kGzChunk % 4 == 0 && kGzChunk <= 32768, "distances and stored lengths of a chunk fit their fields");
static_assert(defl::kBatch == kWave, "the parse looks up a wavefront of positions at a time");
static_assert(defl::build_lengths_ws(defl::kNumLit) <= (1u << defl::kHashBits), "the hash table is the builder's work area");

struct GzChunk {  // what the parse leaves for the emit pass
  uint32_t n_tok, stored;
};

// LDS image of a chunk: dwords, the text little-endian in them
__device__ inline uint32_t gz_load4(const uint32_t *data, uint32_t q) {
  const uint32_t i = q >> 2;
  return (uint32_t)(((uint64_t)data[i + 1] << 32 | data[i]) >> (8 * (q & 3)));
}
__device__ inline uint32_t gz_byte(const uint32_t *data, uint32_t q) { return (data[q >> 2] >> (8 * (q & 3))) & 0xffu; }

__global__ __launch_bounds__(kWave) void k_gz_parse(const uint8_t *__restrict__ text, uint64_t n, uint32_t n_chunks, int stored_only,
                                                    uint32_t *__restrict__ tokens, uint32_t *__restrict__ tables,
                                                    GzChunk *__restrict__ meta, uint32_t *__restrict__ byte_len) {
  using namespace defl;
  __shared__ uint32_t data[kGzChunk / 4 + 2];
  __shared__ uint32_t table[1u << kHashBits];  // position + 1 of the latest entry of a bucket; later the builder's work area
  __shared__ uint32_t hist[kGzSyms];
  __shared__ uint32_t codes[kGzSyms];
  __shared__ uint8_t lens[kGzSyms + 4];
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t o = (uint64_t)c * kGzChunk;
    const uint32_t m = (uint32_t)min((uint64_t)kGzChunk, n - o);
    if (stored_only) {
      if (lane == 0) {
        meta[c] = GzChunk{0, 1};
        byte_len[c] = stored_bytes(m);
      }
      continue;
    }
    text_wave_sync();  // the previous chunk's tables are out
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(text + o);
    const uint32_t nd = (m + 3) / 4;
    for (uint32_t i = lane; i < kGzChunk / 4 + 2; i += kWave) {
      uint32_t v = i < nd ? src32[i] : 0u;
      if (i + 1 == nd && (m & 3)) v &= (1u << (8 * (m & 3))) - 1u;
      data[i] = v;
    }
    for (uint32_t i = lane; i < (1u << kHashBits); i += kWave) table[i] = 0;
    for (uint32_t i = lane; i < (uint32_t)kGzSyms; i += kWave) hist[i] = i == (uint32_t)kEob ? 1u : 0u;
    text_wave_sync();

    uint32_t *tk = tokens + o;
    uint32_t p = 0, ntok = 0;
    while (p < m) {
      const uint32_t q = p + lane;
      const bool can = q + 4 <= m;
      const uint32_t v = can ? gz_load4(data, q) : 0u;
      const uint32_t hsh = hash4(v);
      const uint32_t cand = can ? table[hsh] : 0u;
      const bool ok = cand != 0 && gz_load4(data, cand - 1) == v;
      const uint64_t hits = __ballot(ok);
      const uint32_t k = hits ? (uint32_t)__builtin_ctzll(hits) : min((uint32_t)kWave, m - p);
      if (lane < k) {
        const uint32_t b = gz_byte(data, q);
        tk[ntok + lane] = b;
        atomicAdd(&hist[b], 1u);
        if (can) atomicMax(&table[hsh], q + 1);
      }
      ntok += k;
      p += k;
      if (hits) {
        const uint32_t src = (uint32_t)__shfl((int)cand, (int)k) - 1;
        const uint32_t maxlen = min((uint32_t)kMaxMatch, m - p);
        uint32_t len = kMinMatch;
        while (len < maxlen) {
          const uint32_t i = len + lane;
          const bool differs = i >= maxlen || gz_byte(data, src + i) != gz_byte(data, p + i);
          const uint64_t stop = __ballot(differs);
          if (stop) {
            len += (uint32_t)__builtin_ctzll(stop);
            break;
          }
          len += kWave;
        }
        if (lane == 0) {
          tk[ntok] = token_match(len, p - src);
          atomicAdd(&hist[length_sym(len).sym], 1u);
          atomicAdd(&hist[kNumLit + dist_sym(p - src).sym], 1u);
        }
        for (uint32_t i = lane; i < len; i += kWave)
          if (p + i + 4 <= m) atomicMax(&table[hash4(gz_load4(data, p + i))], p + i + 1);
        ++ntok;
        p += len;
      }
      text_wave_sync();  // the next batch reads the table this one wrote
    }

    if (lane == 0) {
      build_lengths(hist, kNumLit, kMaxBits, lens, table);
      build_lengths(hist + kNumLit, kNumDist, kMaxBits, lens + kNumLit, table);
      assign_codes(lens, kNumLit, codes, table);
      assign_codes(lens + kNumLit, kNumDist, codes + kNumLit, table);
    }
    text_wave_sync();
    uint32_t bits = 0;
    for (uint32_t s = lane; s < (uint32_t)kGzSyms; s += kWave) {
      bits += hist[s] * symbol_bits(s, lens[s]);
      tables[(size_t)c * kGzSyms + s] = codes[s];
    }
    for (int d = 1; d < kWave; d <<= 1) bits += __shfl_xor(bits, d);
    if (lane == 0) {
      const uint32_t dyn = dynamic_bytes(bits + kHeaderBits), st = stored_bytes(m);
      meta[c] = GzChunk{ntok, dyn >= st ? 1u : 0u};
      byte_len[c] = dyn >= st ? st : dyn;
    }
  }
}

// w bits of v into the image at bit position pos (w <= 28)
__device__ inline void gz_put(uint32_t *stage, uint32_t pos, uint32_t v, uint32_t w) {
  if (w == 0) return;
  const uint64_t x = (uint64_t)v << (pos & 31);
  atomicOr(&stage[pos >> 5], (uint32_t)x);
  if (x >> 32) atomicOr(&stage[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(kWave) void k_gz_emit(const uint8_t *__restrict__ text, uint64_t n, uint32_t n_chunks,
                                                   const uint32_t *__restrict__ tokens, const uint32_t *__restrict__ tables,
                                                   const GzChunk *__restrict__ meta, const uint64_t *__restrict__ off,
                                                   uint8_t *__restrict__ out) {
  using namespace defl;
  // the chunk's bytes in the stream at the alignment they have in the output: at most 3 + 10 + kGzChunk of them
  __shared__ uint32_t stage[(kGzChunk + 16) / 4 + 2];
  __shared__ uint32_t codes[kGzSyms];
  uint8_t *stage8 = reinterpret_cast<uint8_t *>(stage);
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t o = (uint64_t)c * kGzChunk;
    const uint32_t m = (uint32_t)min((uint64_t)kGzChunk, n - o);
    const uint64_t base = off[c];
    const uint32_t nbytes = (uint32_t)(off[c + 1] - base), a = (uint32_t)(base & 3);
    const GzChunk mc = meta[c];
    if (nbytes > kGzChunk + 10) continue;  // (never: a chunk is stored where coding it would take more)
    text_wave_sync();  // the previous chunk's image is out
    for (uint32_t i = lane; 4 * i < a + nbytes + 4; i += kWave) stage[i] = 0;
    for (uint32_t s = lane; s < (uint32_t)kGzSyms; s += kWave) codes[s] = tables[(size_t)c * kGzSyms + s];
    text_wave_sync();
    if (mc.stored) {
      // 000 and padding, LEN, NLEN, the text; then the empty stored block
      if (lane == 0) {
        stage8[a + 1] = (uint8_t)m;
        stage8[a + 2] = (uint8_t)(m >> 8);
        stage8[a + 3] = (uint8_t)~m;
        stage8[a + 4] = (uint8_t)(~m >> 8);
        stage8[a + 5 + m + 3] = 0xff;
        stage8[a + 5 + m + 4] = 0xff;
      }
      for (uint32_t i = lane; i < m; i += kWave) stage8[a + 5 + i] = text[o + i];
    } else {
      const uint32_t bit0 = 8 * a;
      if (lane == 0) gz_put(stage, bit0, kHeaderPrefix, kHeaderPrefixBits);
      if (lane < 19) gz_put(stage, bit0 + kHeaderPrefixBits + 3 * lane, header_cl_len((int)lane), 3);
      for (uint32_t s = lane; s < (uint32_t)kGzSyms; s += kWave)
        gz_put(stage, bit0 + kHeaderPrefixBits + kHeaderClBits + 4 * s, reverse_bits(codes[s] >> 16, 4), 4);
      uint32_t cur = bit0 + kHeaderBits;
      const uint32_t *tk = tokens + o;
      for (uint32_t t0 = 0; t0 < mc.n_tok; t0 += kWave) {
        const uint32_t t = t0 + lane;
        const bool active = t < mc.n_tok;
        const uint32_t tok = active ? tk[t] : 0u;
        uint32_t v1, w1, v2 = 0, w2 = 0;
        if (!token_is_match(tok)) {
          const uint32_t e = codes[tok & 0xff];
          v1 = e & 0xffff;
          w1 = e >> 16;
        } else {
          const Sym l = length_sym(token_len(tok)), d = dist_sym(token_dist(tok));
          const uint32_t el = codes[l.sym], ed = codes[kNumLit + d.sym];
          v1 = (el & 0xffff) | l.extra << (el >> 16);
          w1 = (el >> 16) + l.nbits;
          v2 = (ed & 0xffff) | d.extra << (ed >> 16);
          w2 = (ed >> 16) + d.nbits;
        }
        const uint32_t mine = active ? w1 + w2 : 0u;
        uint32_t incl = mine;
        for (int s = 1; s < kWave; s <<= 1) {
          const uint32_t u = __shfl_up(incl, s);
          if ((int)lane >= s) incl += u;
        }
        if (active) {
          gz_put(stage, cur + incl - mine, v1, w1);
          gz_put(stage, cur + incl - mine + w1, v2, w2);
        }
        cur += __shfl(incl, kWave - 1);
      }
      if (lane == 0) {
        gz_put(stage, cur, codes[kEob] & 0xffff, codes[kEob] >> 16);
        // the empty stored block: 000, padding to a byte, 00 00 ff ff
        const uint32_t tail = (cur + (codes[kEob] >> 16) + 3 + 7) / 8;
        gz_put(stage, 8 * (tail + 2), 0xffff, 16);
      }
    }
    text_wave_sync();
    text_flush(stage, out, base, nbytes, (int)lane);
  }
}

__global__ __launch_bounds__(256) void k_gz_crc(const uint8_t *__restrict__ text, uint64_t n, const uint32_t *__restrict__ pow8,
                                                uint32_t *__restrict__ result) {
  using namespace defl;
  __shared__ uint32_t pw[40];
  if (threadIdx.x < 40) pw[threadIdx.x] = pow8[threadIdx.x];
  __syncthreads();
  const uint64_t n_pieces = (n + kGzCrcPiece - 1) / kGzCrcPiece;
  uint32_t acc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pieces; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o = i * kGzCrcPiece;
    const uint32_t len = (uint32_t)min((uint64_t)kGzCrcPiece, n - o);
    const uint4 *p = reinterpret_cast<const uint4 *>(text + o);
    uint32_t r = 0;
    for (uint32_t k = 0; k < len / 16; ++k) {
      const uint4 v = p[k];
      r = crc_word(crc_word(crc_word(crc_word(r, v.x, 4), v.y, 4), v.z, 4), v.w, 4);
    }
    for (uint32_t b = len & ~15u; b < len; ++b) r = crc_word(r, text[o + b], 1);
    acc ^= crc_shift(r, n - o - len, pw);
  }
  for (int d = 1; d < kWave; d <<= 1) acc ^= __shfl_xor(acc, d);
  if (threadIdx.x % kWave == 0 && acc) atomicXor(result, acc);
}

}  // namespace msw
