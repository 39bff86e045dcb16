// fastq_kernels.hpp -- device side of --extract-reads (host_fastq.inc): the records of a FASTQ file, resident in device
// memory as upload_text leaves it (host_reader.inc: padded with line feeds to whole tiles plus one), are indexed,
// checked against the strict four-line grammar (fastq_host.hpp) and gathered by read id.
//
// Index.  Line feeds per 4 KB tile (k_fq_count), an exclusive scan of the counts, then every line's start and -- lines
// are counted modulo 4, '@' is never searched for -- every fourth one as a record's start (k_fq_index).  A line longer
// than a tile is a tile without line feeds: it adds zero to the scan and nothing else.
// Validation.  One thread per record reads the starts of its four lines (k_fq_validate); the smallest offending record
// comes back through one atomicMin.  It runs before any gather: the gather's loop bounds all come from rec_off.
// Gather.  The selected records, ascending by id, are laid out one behind the other (k_fq_gather): the OUTPUT is cut
// into chunks of 16 KB, a workgroup each, and every thread writes 16-byte vectors of it -- the work is balanced by output
// bytes, so a read of 10 000 bases is spread over 40 threads' worth of stores like any other 10 KB.  The source of a
// vector has no alignment in common with it: five aligned dwords are read and v_alignbyte_b32 shifts them into place.
// No kernel waits for another, and no loop runs on data the index has not bounded.
#pragma once
#include "common.hpp"
#include "reader_kernels.hpp"
#include "prim_ops.hpp"

namespace msw {

constexpr int kFqGatherThreads = 256;
constexpr int kFqGatherIters = 4;                                                 // 16-byte vectors per thread
constexpr uint64_t kFqGatherChunk = 16ull * kFqGatherThreads * kFqGatherIters;    // output bytes per workgroup
constexpr unsigned long long kFqNoBad = ~0ull;                                    // fastq_host.hpp: fq::kNoBad

// line feeds of the tile's bytes in front of byte n
__global__ __launch_bounds__(kTileThreads) void k_fq_count(const unsigned char *txt, uint64_t n, uint32_t *cnt_nl) {
  __shared__ uint32_t sh[8];
  const uint64_t at = ((uint64_t)blockIdx.x * kTileThreads + threadIdx.x) * kSegBytes;
  uint32_t nnl = 0;
  if (at < n) {
    unsigned char c[kSegBytes];
    load_seg(txt, at, c);
    const uint32_t valid = n - at >= (uint64_t)kSegBytes ? 0xffffu : (1u << (uint32_t)(n - at)) - 1u;
    nnl = __popc(seg_masks(c, valid).nl);
  }
  uint32_t tot = 0;
  (void)tile_scan_incl(nnl, sh, &tot);
  if (threadIdx.x == 0) cnt_nl[blockIdx.x] = tot;
}

// base_nl[tile] = line feeds in front of the tile.  Line l + 1 starts behind the l-th line feed (l from 0):
// line_off[l + 1], and rec_off[(l + 1) / 4] where l + 1 is a multiple of 4.  line_off has n_lines + 1 entries and
// rec_off n_lines / 4 + 1; entry 0 of both, and the last of both, are the host's to write.
__global__ __launch_bounds__(kTileThreads) void k_fq_index(const unsigned char *txt, uint64_t n, const uint64_t *base_nl,
                                                            uint64_t n_lines, uint64_t *line_off, uint64_t *rec_off) {
  __shared__ uint32_t sh[8];
  const uint64_t at = ((uint64_t)blockIdx.x * kTileThreads + threadIdx.x) * kSegBytes;
  uint32_t nls = 0;
  if (at < n) {
    unsigned char c[kSegBytes];
    load_seg(txt, at, c);
    const uint32_t valid = n - at >= (uint64_t)kSegBytes ? 0xffffu : (1u << (uint32_t)(n - at)) - 1u;
    nls = seg_masks(c, valid).nl;
  }
  uint32_t tot = 0;
  const uint32_t mine = (uint32_t)__popc(nls);
  const uint32_t incl = tile_scan_incl(mine, sh, &tot);
  uint64_t l = base_nl[blockIdx.x] + (incl - mine) + 1;  // the line that starts behind this thread's next line feed
  uint32_t q = nls;
  while (q) {  // (at most 16 bits)
    const int i = __ffs(q) - 1;
    q &= q - 1;
    if (l <= n_lines) {
      line_off[l] = at + (uint64_t)i + 1;
      if ((l & 3) == 0) rec_off[l >> 2] = at + (uint64_t)i + 1;
    }
    ++l;
  }
}

// One thread per record: line 0 begins with '@', line 2 with '+', lines 1 and 3 have the same length.  line_off[4 r + 4]
// is the byte behind the record's last line feed (for a last line without one: n + 1, the padding's line feed), so every
// byte read lies inside the padded text.  *bad: the smallest record << 2 | (reason - 2) (fastq_host.hpp: fq::bad_code).
__global__ void k_fq_validate(const unsigned char *txt, const uint64_t *line_off, uint64_t n_records, unsigned long long *bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long mine = kFqNoBad;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_records; r += stride) {
    const uint64_t s0 = line_off[4 * r], s1 = line_off[4 * r + 1], s2 = line_off[4 * r + 2], s3 = line_off[4 * r + 3],
                   s4 = line_off[4 * r + 4];
    unsigned long long code = kFqNoBad;
    if (txt[s0] != '@') code = r << 2;
    else if (txt[s2] != '+') code = r << 2 | 1u;
    else if (s2 - s1 != s4 - s3) code = r << 2 | 2u;
    mine = min(mine, code);
  }
  if (mine != kFqNoBad) atomicMin(bad, mine);
}

// (FqLen, the length of the i-th selected record: prim_ops.hpp)

// the largest r in [lo, hi) with off[r] <= D, given off[lo] <= D (at most 64 steps: hi - lo halves)
__device__ __forceinline__ uint64_t fq_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t D) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= D) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The bytes [out_off[r_lo], out_off[r_hi]) of the selection -- records r_lo .. r_hi - 1 of it, `len` bytes -- to out[0 .. len).
// Record i of the selection is text bytes [rec_off[ids[i]], rec_off[ids[i] + 1]), and out_off rises strictly (validated
// records are not empty).  out is 16-byte aligned; txt is 4-byte aligned and readable for 4 bytes beyond every record
// (the padding).  Whole vectors are stored as 16 bytes, the bytes of a last partial vector one by one: nothing is
// written beyond out[len).
__global__ __launch_bounds__(kFqGatherThreads) void k_fq_gather(const unsigned char *txt, const uint64_t *rec_off,
                                                                 const uint32_t *ids, const uint64_t *out_off, uint64_t r_lo,
                                                                 uint64_t r_hi, uint64_t len, unsigned char *out) {
  const uint64_t B0 = out_off[r_lo];
  const uint64_t c0 = (uint64_t)blockIdx.x * kFqGatherChunk;
  if (c0 >= len) return;
  const uint64_t c1 = min(c0 + kFqGatherChunk, len);
  // the records the chunk touches (the same search in every thread: the loads are uniform)
  const uint64_t r_first = fq_find(out_off, r_lo, r_hi, B0 + c0);
  const uint64_t r_last = fq_find(out_off, r_first, r_hi, B0 + c1 - 1);
#pragma unroll 1
  for (int it = 0; it < kFqGatherIters; ++it) {
    const uint64_t d = c0 + ((uint64_t)it * kFqGatherThreads + threadIdx.x) * 16;
    if (d >= c1) continue;
    const uint64_t D = B0 + d;
    uint64_t r = fq_find(out_off, r_first, r_last + 1, D);
    const uint64_t o0 = out_off[r];
    uint64_t o1 = out_off[r + 1];
    uint4 v;
    if (D + 16 <= o1) {
      // the vector lies inside one record: five aligned dwords of the source, shifted into place
      const uint64_t src = rec_off[ids[r]] + (D - o0);
      const uint32_t *w = reinterpret_cast<const uint32_t *>(txt + (src & ~(uint64_t)3));
      const uint32_t sh = (uint32_t)(src & 3);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
      v.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
      v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
      v.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
      v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
      *reinterpret_cast<uint4 *>(out + d) = v;
      continue;
    }
    // a record ends inside the vector (or the output does): byte by byte, moving on to the next record where one ends
    const uint32_t nvalid = (uint32_t)min((uint64_t)16, len - d);
    uint64_t base = rec_off[ids[r]] - o0;  // source = base + position in the selection (mod 2^64)
    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      if (j < nvalid) {
        const uint64_t Dj = D + j;
        while (Dj >= o1 && r + 1 < r_hi) {  // (r rises to r_last at most)
          ++r;
          base = rec_off[ids[r]] - out_off[r];
          o1 = out_off[r + 1];
        }
        wd[j >> 2] |= (uint32_t)txt[base + Dj] << (8 * (j & 3));
      }
    }
    if (nvalid == 16) {
      v.x = wd[0], v.y = wd[1], v.z = wd[2], v.w = wd[3];
      *reinterpret_cast<uint4 *>(out + d) = v;
    } else {
      // the output's last, partial vector: its whole dwords, then the up to three bytes behind them
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        if (4 * k + 4 <= nvalid) {
          *reinterpret_cast<uint32_t *>(out + d + 4 * k) = wd[k];
        } else {
#pragma unroll
          for (uint32_t j = 4 * k; j < 4 * k + 4; ++j)
            if (j < nvalid) out[d + j] = (unsigned char)(wd[k] >> (8 * (j & 3)));
        }
      }
    }
  }
}

}  // namespace msw
