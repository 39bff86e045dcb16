// likelihood_text_kernels.hpp -- device side of --read-likelihood (include/Likelihood.hpp:224-253): the text of a
// likelihood file, already in device memory (host_reader.inc: upload_text, plain / gzip / BGZF), becomes the read counts
// and the dense matrix without a cell crossing the link.  Host side: host_likelihood_file.inc.
//
// The device serves ONE grammar and judges nothing else -- a text outside it raises a flag and the drivers' own
// parsers read the file (their result or their message stands):
//   line   = count '\t' cell ('\t' cell){G-1} '\n'         (the last line may lack its '\n')
//   count  = 1 to 18 digits;  cell: dec_parse.hpp (inf / nan words, or -?digits(.digits)?(e[+-]?digits)?, <= 24 bytes)
// A TOKEN starts at byte 0 and behind every '\t' and '\n' and ends in front of the next of them, so blank lines and
// doubled tabs are (empty, bad) tokens.  Same two passes over 4 KB tiles, 16 bytes per thread, as the Themisto reader
// (reader_kernels.hpp):
//   pass 1   k_lik_count   per tile: tokens that start in it, line feeds; byte classes; no token beyond 24 bytes
//   (scans)                exclusive sums of both counts; host: tokens == lines * (G + 1)
//   pass 2   k_lik_parse   at every line feed: (l + 1)(G + 1) tokens have started in front of it -- so token t is column
//                          t % (G + 1) of line t / (G + 1), no per-line index --; every token parsed by the thread in
//                          whose segment it starts; counts[j], Lt[j][g] (EC-major: consecutive tokens, consecutive
//                          doubles); cells outside Clinger's case listed for the host's strtod
//   k_lik_transpose        [E][G] -> the [G][E] stage msw_core_set_dense_logl continues from
// A thread reads 24 bytes behind its segment (the text is padded with line feeds by a whole tile).
#pragma once
#include "dec_parse.hpp"
#include "reader_kernels.hpp"

namespace msw {

// LikCtr::flags
constexpr uint32_t kLikBadByte = 1u;    // a byte no token of the grammar holds ('\r', blanks, upper case, ...)
constexpr uint32_t kLikBadToken = 2u;   // bytes of the grammar in an order it does not have; a cell beyond 24 bytes
constexpr uint32_t kLikColumns = 4u;    // a line feed that does not have (l + 1)(G + 1) tokens in front of it
constexpr uint32_t kLikHostOver = 8u;   // more cells for the host than its list takes
constexpr uint32_t kLikHostCap = 1u << 16;  // listed cells per file

struct LikCtr {
  uint32_t flags;
  uint32_t n_host;   // cells met for the list (beyond kLikHostCap: not stored, kLikHostOver raised)
};
struct LikHostCell {
  uint64_t cell;     // j * G + g: where the value goes in the EC-major matrix
  uint64_t off;      // the token's first byte in the text
  uint32_t len, pad;
  uint64_t b[3];     // its bytes (<= 24)
};

// 40 bytes from the thread's segment on, as five words, and the masks of the bytes that end a token
struct LikSeg {
  uint64_t W[5];
  uint64_t sep;      // bit i: byte i is '\t' or '\n' (40 bits)
  uint32_t nl;       // bit i: byte i of the segment is '\n', inside the text
  uint32_t starts;   // bit i: a token starts at byte i of the segment, inside the text
  uint32_t valid;
};
__device__ __forceinline__ void lik_load(const unsigned char *txt, uint64_t n, uint64_t at, LikSeg &s) {
  // (the buffer is padded with line feeds by one tile beyond the last: at + 48 stays inside it)
  const uint4 v0 = *reinterpret_cast<const uint4 *>(txt + at), v1 = *reinterpret_cast<const uint4 *>(txt + at + 16);
  const uint2 v2 = *reinterpret_cast<const uint2 *>(txt + at + 32);
  s.W[0] = (uint64_t)v0.y << 32 | v0.x, s.W[1] = (uint64_t)v0.w << 32 | v0.z;
  s.W[2] = (uint64_t)v1.y << 32 | v1.x, s.W[3] = (uint64_t)v1.w << 32 | v1.z;
  s.W[4] = (uint64_t)v2.y << 32 | v2.x;
  uint64_t sep = 0;
  uint32_t nl = 0;
#pragma unroll
  for (int j = 0; j < 40; ++j) {
    const uint32_t b = (uint32_t)(s.W[j >> 3] >> (8 * (j & 7))) & 0xffu;
    sep |= (uint64_t)(b == '\t' || b == '\n') << j;
    if (j < kSegBytes) nl |= (uint32_t)(b == '\n') << j;
  }
  // bytes beyond the text are line feeds (the padding), which is what ends a last line without one
  s.valid = n - at >= (uint64_t)kSegBytes ? 0xffffu : (1u << (uint32_t)(n - at)) - 1u;
  const uint32_t prev_sep = at ? (uint32_t)(txt[at - 1] == '\t' || txt[at - 1] == '\n') : 1u;
  s.sep = sep;
  s.nl = nl & s.valid;
  s.starts = (((uint32_t)sep << 1 | prev_sep) & 0xffffu) & s.valid;
}
// length of the token that starts at byte i of the segment: 0 .. 24, or 25 for anything longer
__device__ __forceinline__ int lik_token_len(const LikSeg &s, int i) {
  const uint64_t m = (s.sep >> i) & ((1ull << 25) - 1ull);
  return m ? __ffsll((unsigned long long)m) - 1 : 25;
}
// bytes the grammar's tokens are made of, and the two separators
__device__ __forceinline__ bool lik_byte_ok(uint32_t b) {
  // 0 .. 63: '\t' '\n' '+' '-' '.' '0'-'9';  64 .. 127: 'a' 'e' 'f' 'i' 'n'
  const uint64_t lo = 1ull << '\t' | 1ull << '\n' | 1ull << '+' | 1ull << '-' | 1ull << '.' | 0x3ffull << '0';
  const uint64_t hi = 1ull << ('a' - 64) | 1ull << ('e' - 64) | 1ull << ('f' - 64) | 1ull << ('i' - 64) | 1ull << ('n' - 64);
  return b < 128u && (((b < 64u ? lo : hi) >> (b & 63u)) & 1ull) != 0;
}

// Pass 1: cnt_tok[tile] = tokens that START in the tile, cnt_nl[tile] = its line feeds; byte and length checks.
__global__ __launch_bounds__(kTileThreads) void k_lik_count(const unsigned char *txt, uint64_t n, uint32_t *cnt_tok,
                                                             uint32_t *cnt_nl, LikCtr *ctr) {
  __shared__ uint32_t sh[8];
  const uint64_t at = ((uint64_t)blockIdx.x * kTileThreads + threadIdx.x) * kSegBytes;
  uint32_t ntok = 0, nnl = 0, bad = 0;
  if (at < n) {
    LikSeg s;
    lik_load(txt, n, at, s);
    ntok = __popc(s.starts);
    nnl = __popc(s.nl);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kSegBytes; ++j) {
      const uint32_t b = (uint32_t)(s.W[j >> 3] >> (8 * (j & 7))) & 0xffu;
      ok = ok && (lik_byte_ok(b) || !((s.valid >> j) & 1u));
    }
    if (!ok) bad |= kLikBadByte;
    uint32_t q = s.starts;
    while (q) {
      const int i = __ffs(q) - 1;
      q &= q - 1;
      const int len = lik_token_len(s, i);
      if (len == 0 || len > dec::kDecMaxToken) bad |= kLikBadToken;
    }
  }
  uint32_t tot = 0;
  const uint32_t packed = ntok | nnl << 16;  // (<= 16 of either per thread, 4096 per tile)
  (void)tile_scan_incl(packed, sh, &tot);
  bad = wave_or(bad);
  if (threadIdx.x == 0) {
    cnt_tok[blockIdx.x] = tot & 0xffffu;
    cnt_nl[blockIdx.x] = tot >> 16;
  }
  if (bad && (threadIdx.x & 63) == 0) atomicOr(&ctr->flags, bad);
}

// Pass 2.  base_tok[tile], base_nl[tile]: tokens / line feeds in front of the tile.  The caller has checked that the
// text holds n_lines * cols tokens (cols = G + 1), so line = t / cols < n_lines for every token: every store below is
// inside counts[n_lines] or Lt[n_lines * G], whatever the text looks like.
__global__ __launch_bounds__(kTileThreads) void k_lik_parse(const unsigned char *txt, uint64_t n, const uint64_t *base_tok,
                                                             const uint64_t *base_nl, uint32_t cols, uint64_t n_tokens,
                                                             uint64_t *counts, double *Lt, LikHostCell *host, LikCtr *ctr) {
  __shared__ uint32_t sh[8];
  const uint64_t at = ((uint64_t)blockIdx.x * kTileThreads + threadIdx.x) * kSegBytes;
  LikSeg s;
  s.starts = 0, s.nl = 0, s.sep = 0, s.valid = 0;
  s.W[0] = s.W[1] = s.W[2] = s.W[3] = s.W[4] = 0;
  if (at < n) lik_load(txt, n, at, s);
  uint32_t tot = 0;
  const uint32_t mine = (uint32_t)__popc(s.starts) | (uint32_t)__popc(s.nl) << 16;
  const uint32_t incl = tile_scan_incl(mine, sh, &tot);
  const uint32_t excl = incl - mine;
  const uint64_t tk0 = base_tok[blockIdx.x] + (excl & 0xffffu);
  const uint64_t l0 = base_nl[blockIdx.x] + (excl >> 16);
  uint32_t bad = 0;
  // every line feed closes a line of exactly `cols` tokens: the tokens that have started up to it are (l + 1) * cols
  uint32_t q = s.nl, ln = 0;
  while (q) {
    const int i = __ffs(q) - 1;
    q &= q - 1;
    const uint64_t before = tk0 + (uint32_t)__popc(s.starts & ((2u << i) - 1u));
    if (before != (l0 + ln + 1) * (uint64_t)cols) bad |= kLikColumns;
    ++ln;
  }
  const uint32_t G = cols - 1u;
  uint64_t t = tk0;
  q = s.starts;
  while (q) {
    const int i = __ffs(q) - 1;
    q &= q - 1;
    const uint64_t tok = t++;
    if (tok >= n_tokens) break;  // (cannot happen: the scans count these same starts)
    const int len = lik_token_len(s, i);
    // the 24 bytes from byte i on, by shifts (no indexed register array)
    const bool up = i >= 8;
    const uint32_t shb = (uint32_t)(i & 7) * 8u;
    const uint64_t A = up ? s.W[1] : s.W[0], B = up ? s.W[2] : s.W[1], C = up ? s.W[3] : s.W[2], D = up ? s.W[4] : s.W[3];
    dec::Words24 w;
    w.w0 = shb ? A >> shb | B << (64u - shb) : A;
    w.w1 = shb ? B >> shb | C << (64u - shb) : B;
    w.w2 = shb ? C >> shb | D << (64u - shb) : C;
    const uint64_t line = tok / cols;
    const uint32_t col = (uint32_t)(tok - line * cols);
    if (col == 0) {
      uint64_t c = 0;
      if (dec::parse_count(w, len, &c) != dec::kDecided) bad |= kLikBadToken;
      counts[line] = c;
    } else {
      double v = 0.0;
      const int r = len <= dec::kDecMaxToken ? dec::parse_cell(w, len, &v) : dec::kBad;
      const uint64_t cell = line * G + (col - 1u);
      if (r == dec::kBad) {
        bad |= kLikBadToken;
      } else if (r == dec::kUndecided) {
        const uint32_t k = atomicAdd(&ctr->n_host, 1u);
        if (k < kLikHostCap) {
          LikHostCell hc;
          hc.cell = cell, hc.off = at + (uint32_t)i, hc.len = (uint32_t)len, hc.pad = 0;
          hc.b[0] = w.w0, hc.b[1] = w.w1, hc.b[2] = w.w2;
          host[k] = hc;
        } else {
          bad |= kLikHostOver;
        }
      }
      Lt[cell] = v;
    }
  }
  bad = wave_or(bad);
  if (bad && (threadIdx.x & 63) == 0) atomicOr(&ctr->flags, bad);
}

// [E][G] -> [G][E] through LDS: k_transpose of dense_kernels.hpp with the dimensions swapped, in 32 x 32 tiles (8.4 KB of
// LDS); the long dimension, E, on the grid's x, the group tiles strided over its y.
__global__ __launch_bounds__(256) void k_lik_transpose(const double *src, uint32_t E, uint32_t G, double *dst) {
  __shared__ double tile[32][33];
  const uint32_t j0 = blockIdx.x * 32u;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (uint32_t g0 = blockIdx.y * 32u; g0 < G; g0 += gridDim.y * 32u) {
    for (int r = ty; r < 32; r += 8) {
      const uint32_t j = j0 + r, g = g0 + tx;
      tile[r][tx] = (j < E && g < G) ? src[(size_t)j * G + g] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const uint32_t g = g0 + r, j = j0 + tx;
      if (g < G && j < E) dst[(size_t)g * E + j] = tile[tx][r];
    }
    __syncthreads();
  }
}
// out[i] = src[idx[i]]: the cells compress_dense samples for its background, from the stage (host_compress.inc)
__global__ void k_lik_gather(const double *src, const uint64_t *idx, uint32_t n, double *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}

// dst[idx[i]] = val[i]: the cells the host converted, back into the EC-major matrix (n_cells: its size)
__global__ void k_lik_scatter(const double *val, const uint64_t *idx, uint32_t n, uint64_t n_cells, double *dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && idx[i] < n_cells) dst[idx[i]] = val[i];
}

}  // namespace msw
