// text_kernels.hpp -- the text of the matrix outputs on the device (msw_core_text_block / msw_core_format_g6,
// host_text.inc): --write-probs, --write-likelihood and --write-likelihood-bitseq turn the G x w block that
// gamma_kernels.hpp materialises into the file's bytes where it lies; only the bytes cross the link.  The mirror image
// of the device reader (reader_kernels.hpp).
//
// The block is group-major, val[g * w + jj]; the text is line-major, one line per EC, cells of 1 ... 13 bytes
// (g6_format.hpp).  Two passes that both convert:
//   k_text_len    one lane per EC, a loop over the groups (lanes along jj: coalesced 8-byte reads): the length of line jj.
//   (host: exclusive scan of the lengths -> byte offset of every line, rocprim)
//   k_text_write  a workgroup per 64 ECs, chunks of 32 groups.  Convert: every wavefront takes rows of the chunk, lanes
//                 along jj (the same coalesced reads), and leaves 16 bytes per cell in an LDS tile.  Assemble: every
//                 wavefront takes lines, lanes along the groups of the chunk: a wave scan of the cell widths places
//                 the cells in the wavefront's LDS staging area at the alignment the line has in the output, and the
//                 stretch leaves as whole dwords (single bytes only for the ragged first and last dword, which belong
//                 in part to the neighbouring stretch).
// Converting twice costs a second read of the block (8 bytes per cell) and a second run of an integer-only routine; a
// single conversion through a 16-byte-per-cell scratch in device memory would write and read 32 bytes per cell instead.
// No kernel here uses scratch memory (tests/test_text_kernel_resources.py): the text of a cell lives in two 64-bit
// registers, digits in nibbles, never in an indexed array.
//
// A value the formatter cannot decide (g6::kUndecided: too close to a half where the power of ten is inexact) gets 13
// blanks, and its (byte offset, bits) goes to a list: the host prints those cells (text_cells.hpp) and
//   k_text_close  puts them in: every stretch between them moves down by the slack accumulated in front of it, and the
//                 finished text lies on the device for either sink, the copy to the host or the compressor (host_gzip.inc).
#pragma once
#include "common.hpp"
#include "g6_format.hpp"
#include "text_cells.hpp"

namespace msw {

enum { kTextProbs = 0, kTextLogl = 1, kTextBitseq = 2, kTextPlain = 3 };  // the first three: MSW_TEXT_* of the ABI

constexpr int kTextLines = 64;     // ECs per workgroup tile of k_text_write (a wavefront wide: lanes along jj)
constexpr int kTextGroups = 32;    // groups per chunk (the LDS tile holds kTextGroups x kTextLines cells)
constexpr int kTextThreads = 256;
constexpr int kTextWaves = kTextThreads / kWave;
// staging area of a wavefront: the longest stretch is a line prefix (20 digits + 1) and kTextGroups cells of at most
// 10 + 1 + 13 + 1 bytes (BitSeq: group number, blank, value, blank), shifted by up to 3 bytes of alignment
constexpr int kTextStageBytes = 1024;
static_assert(3 + 21 + kTextGroups * 25 <= kTextStageBytes, "a stretch must fit the staging area");
constexpr int kTextSuffixPiece = 512;  // bytes of a line's suffix staged at a time

struct TextJob {
  const double *val;       // G x w, group-major
  uint32_t G, w;
  uint64_t id0;            // PROBS: the id of line 0
  const uint64_t *prefix;  // LOGL: the number that starts line jj
  uint32_t n_zero;         // PROBS: "\t0" columns after the groups
};

__device__ inline uint32_t text_dec_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 10) {
    v /= 10;
    ++n;
  }
  return n;
}
// the decimal digits of v at p[0 .. n), n = text_dec_len(v)
__device__ inline void text_put_dec(uint8_t *p, uint64_t v, uint32_t n) {
  for (uint32_t i = n; i-- > 0;) {
    p[i] = (uint8_t)('0' + v % 10);
    v /= 10;
  }
}

template <int WHAT>
__device__ inline uint64_t text_cell_bits(double v) {
  return (uint64_t)__double_as_longlong(WHAT == kTextProbs ? exp(v) : v);
}
template <int WHAT>
__device__ inline uint64_t text_line_number(const TextJob &J, uint32_t jj) {
  return WHAT == kTextProbs ? J.id0 + jj : (WHAT == kTextLogl ? J.prefix[jj] : (uint64_t)J.G + 1);
}
template <int WHAT>
__device__ inline uint32_t text_prefix_len(const TextJob &J, uint32_t jj) {
  if (WHAT == kTextPlain) return 0;
  return text_dec_len(text_line_number<WHAT>(J, jj)) + (WHAT == kTextBitseq ? 1 : 0);
}
// what a cell of group g adds around the value's own text
template <int WHAT>
__device__ inline uint32_t text_cell_extra(uint32_t g) {
  return WHAT == kTextPlain ? 0 : (WHAT == kTextBitseq ? text_dec_len((uint64_t)g + 1) + 2 : 1);
}
template <int WHAT>
__device__ inline uint32_t text_suffix_len(const TextJob &J) {
  return WHAT == kTextProbs ? 2 * J.n_zero + 1 : (WHAT == kTextBitseq ? 12 : 1);
}
template <int WHAT>
__device__ inline uint8_t text_suffix_byte(uint32_t i, uint32_t n) {
  if (WHAT == kTextBitseq) {
    // "0 -10000.00\n" as three little-endian words: no array of characters behind a dynamic index
    const uint32_t w = i < 4 ? 0x312d2030u : (i < 8 ? 0x30303030u : 0x0a30302eu);
    return (uint8_t)(w >> (8 * (i & 3)));
  }
  return i + 1 == n ? '\n' : ((i & 1) ? '0' : '\t');
}

template <int WHAT>
__global__ __launch_bounds__(256) void k_text_len(TextJob J, uint32_t *__restrict__ len) {
  for (size_t jj = (size_t)blockIdx.x * blockDim.x + threadIdx.x; jj < J.w; jj += (size_t)gridDim.x * blockDim.x) {
    uint32_t n = text_prefix_len<WHAT>(J, (uint32_t)jj) + text_suffix_len<WHAT>(J);
    for (uint32_t g = 0; g < J.G; ++g) {
      g6::Text t;
      g6::format(text_cell_bits<WHAT>(J.val[(size_t)g * J.w + jj]), t);
      n += t.len + text_cell_extra<WHAT>(g);
    }
    len[jj] = n;
  }
}

// PROBS on a block the host formats itself (the list of undecided cells overflowed): the values the device formats
__global__ __launch_bounds__(256) void k_text_exp(double *__restrict__ val, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    val[i] = exp(val[i]);
}

__device__ inline void text_wave_sync() {  // orders a wavefront's own LDS traffic (its staging area is private to it)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// n staged bytes, stage[a ... a + n) with a = base & 3, to out[base ... base + n): whole dwords where the stretch covers
// them, single bytes in the ragged first and last dword
__device__ inline void text_flush(const uint32_t *stage, uint8_t *__restrict__ out, uint64_t base, uint32_t n, int lane) {
  const uint32_t a = (uint32_t)(base & 3);
  uint8_t *aligned = out + (base - a);
  const uint8_t *s8 = reinterpret_cast<const uint8_t *>(stage);
  for (uint32_t d = lane; 4 * d < a + n; d += kWave) {
    if (4 * d >= a && 4 * d + 4 <= a + n) {
      reinterpret_cast<uint32_t *>(aligned)[d] = stage[d];
    } else {
      for (uint32_t i = 4 * d; i < 4 * d + 4; ++i)
        if (i >= a && i < a + n) aligned[i] = s8[i];
    }
  }
}

template <int WHAT>
__global__ __launch_bounds__(kTextThreads) void k_text_write(TextJob J, const uint64_t *__restrict__ off,
                                                             uint8_t *__restrict__ out, TextHostCell *__restrict__ list,
                                                             uint32_t *__restrict__ n_list, uint32_t list_cap) {
  // a cell: its text in x, y, z and the low 3 bytes of w (an undecided one: the value's bits in x, y); byte 15 = the
  // length, bit 7 of it set for an undecided cell.  Rows padded by one cell: the assemble phase reads a column
  // (lanes along the rows) without bank conflicts.
  __shared__ uint4 tile[kTextGroups][kTextLines + 1];
  __shared__ uint32_t stage_all[kTextWaves][kTextStageBytes / 4];
  __shared__ uint32_t cur[kTextLines];  // bytes of every line written so far
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  uint32_t *stage = stage_all[wave];
  uint8_t *stage8 = reinterpret_cast<uint8_t *>(stage);
  const uint32_t n_tiles = (J.w + kTextLines - 1) / kTextLines;
  constexpr int kLinesPerWave = kTextLines / kTextWaves;

  for (uint32_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const uint32_t j0 = tl * kTextLines;
    __syncthreads();  // the previous tile's lines are out
    if (tid < kTextLines) cur[tid] = 0;
    for (uint32_t g0 = 0; g0 < J.G; g0 += kTextGroups) {
      // ---- convert: rows of the chunk by wavefront, lanes along the ECs
      for (uint32_t r = wave; r < (uint32_t)kTextGroups; r += kTextWaves) {
        const uint32_t g = g0 + r, jj = j0 + lane;
        if (g < J.G && jj < J.w) {
          const uint64_t bits = text_cell_bits<WHAT>(J.val[(size_t)g * J.w + jj]);
          g6::Text t;
          const bool und = g6::format(bits, t) == g6::kUndecided;
          const uint64_t lo = und ? bits : t.lo, hi = und ? 0 : t.hi;
          tile[r][lane] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi,
                                     (uint32_t)(hi >> 32) | (t.len | (und ? 0x80u : 0u)) << 24);
        }
      }
      __syncthreads();
      // ---- assemble: lines by wavefront, lanes along the groups of the chunk
      const uint32_t ng = min((uint32_t)kTextGroups, J.G - g0);
      for (int li = 0; li < kLinesPerWave; ++li) {
        const uint32_t lj = wave * kLinesPerWave + li, jj = j0 + lj;
        if (jj >= J.w) break;  // (uniform in the wavefront)
        const bool active = (uint32_t)lane < ng;
        const uint32_t g = g0 + lane;
        uint4 c = make_uint4(0, 0, 0, 0);
        if (active) c = tile[lane][lj];
        const uint32_t tlen = (c.w >> 24) & 0x7f;
        const bool und = (c.w >> 31) != 0;
        const uint32_t pre = (g0 == 0 && lane == 0) ? text_prefix_len<WHAT>(J, jj) : 0;
        const uint32_t mine = active ? pre + text_cell_extra<WHAT>(g) + tlen : 0;
        uint32_t incl = mine;
        for (int o = 1; o < kWave; o <<= 1) {
          const uint32_t u = __shfl_up(incl, o);
          if (lane >= o) incl += u;
        }
        const uint32_t total = __shfl(incl, kWave - 1);
        const uint64_t base = off[jj] + cur[lj];
        const uint32_t a = (uint32_t)(base & 3);
        if (active) {
          uint8_t *p = stage8 + a + (incl - mine);
          if (pre) {
            text_put_dec(p, text_line_number<WHAT>(J, jj), text_dec_len(text_line_number<WHAT>(J, jj)));
            if (WHAT == kTextBitseq) p[pre - 1] = ' ';
            p += pre;
          }
          if (WHAT == kTextBitseq) {
            const uint32_t nd = text_dec_len((uint64_t)g + 1);
            text_put_dec(p, (uint64_t)g + 1, nd);
            p[nd] = ' ';
            p += nd + 1;
          } else if (WHAT != kTextPlain) {
            *p++ = '\t';
          }
          if (und) {
            const uint32_t k = atomicAdd(n_list, 1u);
            if (k < list_cap) list[k] = TextHostCell{base + (uint64_t)(p - (stage8 + a)), (uint64_t)c.x | (uint64_t)c.y << 32};
            for (uint32_t i = 0; i < tlen; ++i) p[i] = ' ';
          } else {
            const uint64_t lo = (uint64_t)c.x | (uint64_t)c.y << 32, hi = (uint64_t)c.z | (uint64_t)c.w << 32;
            for (uint32_t i = 0; i < tlen; ++i) p[i] = (uint8_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xff);
          }
          if (WHAT == kTextBitseq) p[tlen] = ' ';
        }
        text_wave_sync();
        text_flush(stage, out, base, total, lane);
        text_wave_sync();  // the staging area is written again for the next line
        if (lane == 0) cur[lj] += total;
      }
      __syncthreads();  // the tile is written again for the next chunk
    }
    // ---- the suffix of every line
    const uint32_t ns = text_suffix_len<WHAT>(J);
    for (int li = 0; li < kLinesPerWave; ++li) {
      const uint32_t lj = wave * kLinesPerWave + li, jj = j0 + lj;
      if (jj >= J.w) break;
      const uint64_t line = off[jj] + cur[lj];
      for (uint32_t s0 = 0; s0 < ns; s0 += kTextSuffixPiece) {
        const uint32_t n = min((uint32_t)kTextSuffixPiece, ns - s0);
        const uint64_t base = line + s0;
        const uint32_t a = (uint32_t)(base & 3);
        for (uint32_t i = lane; i < n; i += kWave) stage8[a + i] = text_suffix_byte<WHAT>(s0 + i, ns);
        text_wave_sync();
        text_flush(stage, out, base, n, lane);
        text_wave_sync();
      }
    }
  }
}

// dst <- src[0 .. total) with every listed cell's 13 blanks replaced by its text; cells sorted by offset
__global__ __launch_bounds__(256) void k_text_close(const uint8_t *__restrict__ src, uint64_t total, const TextFilledCell *__restrict__ cells,
                                                    uint32_t n_cells, uint8_t *__restrict__ dst) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = n_cells;  // lo <- the cells that start at or before byte i
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (cells[mid].off <= i) lo = mid + 1;
      else hi = mid;
    }
    uint64_t slack = 0;
    if (lo) {
      const TextFilledCell *c = &cells[lo - 1];
      const uint64_t j = i - c->off;
      if (j < (uint64_t)g6::kMaxLen) {
        if (j < c->len) dst[c->off - c->slack + j] = (uint8_t)c->s[j];
        continue;
      }
      slack = (uint64_t)c->slack + ((uint32_t)g6::kMaxLen - c->len);
    }
    dst[i - slack] = src[i];
  }
}

}  // namespace msw
