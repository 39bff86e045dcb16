// inflate_kernels.hpp -- gzip pseudoalignment input inflated on the device (host_inflate.inc), in front of the reader's
// token kernels: only the compressed bytes cross the link, and the one serial host stage of the input path is gone.
// Format, probe, block headers and both symbol loops are inflate_format.hpp's -- the code the host tests hold against
// zlib -- and the steps are those of its plain reference:
//   k_inf_probe   a wavefront per chunk of the payload: 64 consecutive bit positions a step through the block-start
//                 probe; the first position that passes is the chunk's start (chunk 0: the payload's first bit).
//   (host: the chunks with a start are the owners; each stops where the next begins)
//   k_inf_window  pass (a), a wavefront per owner: block after block against an unknown window -- the byte count, the
//                 end bit, a status word, and the last 32 Ki bytes as 16-bit entries (a byte, or a marker).
//   (rocprim: exclusive scan of the byte counts -> every owner's offset in the text, and the total)
//   k_inf_chain   one workgroup walks the owners in order: window k read through resolved window k - 1, which it keeps
//                 in LDS (two halves of 32 KiB, in turn).  Ordered by barriers of that workgroup: no kernel waits on
//                 another workgroup's progress.
//   k_inf_write   pass (b), a wavefront per owner: the same decode, bytes to the text at the owner's offset;
//                 back-references in front of the owner read the resolved window, which starts out the wavefront's ring.
//   (k_gz_crc of deflate_kernels.hpp over the text; the host compares CRC-32 and length with the member's trailer)
// Lane mapping: a DEFLATE stream is decoded symbol by symbol, every symbol's position known only once the one before it
// is read, so within an owner there is one thread of control.  All 64 lanes of the owner's wavefront run it in lock step
// -- the same bit positions, the same table reads (LDS broadcasts), the same values in every lane -- so that a match,
// the common symbol of this text, is copied 64 bytes a step through the LDS ring (a match's source is at most 32 KiB
// back: never global memory) and leaves as one coalesced store; literals are lane 0's.  The parallelism is across
// owners -- 5 000 of them per GB of text at 64 KiB chunks -- and a workgroup is one wavefront, so that a CU holds as many
// owners as its LDS allows: two in pass (a) (68 KiB: the ring is 16 bits wide there), four in pass (b) (36 KiB).
// The lock step IS the synchronisation: the 64 lanes bump the same LDS words without atomics (++count[], sym[offs[]++]
// in huff_build: every lane reads the same old value and writes the same new one) and read ring bytes that other lanes
// wrote one instruction earlier with no barrier in between.  That is correct only because a wave64 executes ONE
// instruction stream and its LDS accesses complete in order -- so the decode kernels' workgroup must be exactly one
// wavefront of 64 lanes (the static_assert and __launch_bounds__(kWave) below; host_inflate.inc launches dim3(kWave)).
// A larger block, or a wave32 target, needs barriers and atomics there.
// Decode tables, code lengths and rings live in LDS; no kernel uses scratch memory
// (tests/test_inflate_kernel_resources.py).  Every loop is bounded by the payload's bit length or the owner's byte
// capacity; a wavefront that would leave either sets the owner's status and stops.
#pragma once
#include "common.hpp"
#include "inflate_format.hpp"
#include "prim_ops.hpp"  // InfOwner

namespace msw {

constexpr int kInfChainThreads = 1024;
static_assert(kWave == 64, "the decode kernels run one wave64 per workgroup in lock step: no barrier orders their LDS traffic");

__global__ __launch_bounds__(kWave) void k_inf_probe(const uint32_t *__restrict__ words, uint64_t n_words, uint64_t first_bit,
                                                     uint64_t end_bit, uint64_t chunk_bits, uint32_t n_chunks,
                                                     uint64_t *__restrict__ start) {
  const infl::Stream s = {words, n_words, end_bit};
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    uint64_t found = infl::kNoStart;
    if (c == 0) {
      found = first_bit;
    } else {
      const uint64_t lo = first_bit + (uint64_t)c * chunk_bits, hi = min(lo + chunk_bits, end_bit);
      for (uint64_t p0 = lo; p0 < hi; p0 += kWave) {  // (at most chunk_bits / 64 steps)
        const uint64_t p = p0 + lane;
        const bool ok = p < hi && infl::probe_block_start(s, p);
        const uint64_t hits = __ballot(ok);
        if (hits) {
          found = p0 + (uint64_t)__builtin_ctzll(hits);
          break;
        }
      }
    }
    if (lane == 0) start[c] = found;
  }
}

__global__ __launch_bounds__(kWave) void k_inf_window(const uint32_t *__restrict__ words, uint64_t n_words, uint64_t end_bit,
                                                      uint64_t cap, uint32_t n_owners, InfOwner *__restrict__ owners,
                                                      uint16_t *__restrict__ windows) {
  __shared__ uint16_t ring[infl::kWindow];
  __shared__ uint16_t ws[infl::kWsSize];
  __shared__ uint64_t count_sh;
  const infl::Stream s = {words, n_words, end_bit};
  const uint32_t lane = threadIdx.x;
  for (uint32_t k = blockIdx.x; k < n_owners; k += gridDim.x) {
    __syncthreads();  // the previous owner's window is out
    for (uint32_t i = lane; i < infl::kWindow; i += kWave) ring[i] = (uint16_t)(infl::kMarker | i);
    __syncthreads();
    // (all 64 lanes run the decode in lock step -- the same addresses, the same values -- so that a match is one step)
    infl::WindowSink sink = {ring, 0, cap, infl::kOk, k == 0, lane, (uint32_t)kWave};
    const infl::OwnerEnd e = infl::inflate_owner(s, owners[k].start, owners[k].stop, infl::tables_in(ws), sink);
    if (lane == 0) {
      owners[k].end_bit = e.end_bit;
      owners[k].bytes = sink.count;
      owners[k].status = e.status;
      owners[k].final = e.final;
      count_sh = sink.count;
    }
    __syncthreads();
    const uint64_t count = count_sh;
    uint16_t *w = windows + (size_t)k * infl::kWindow;
    for (uint32_t j = lane; j < infl::kWindow; j += kWave) w[j] = ring[(count + j) & infl::kWinMask];
  }
}

// resolved[k] = windows[k] read through resolved[k - 1] (k = 0: nothing lies in front of the stream), k < n
__global__ __launch_bounds__(kInfChainThreads) void k_inf_chain(const uint16_t *__restrict__ windows, uint32_t n,
                                                                uint8_t *__restrict__ resolved) {
  __shared__ uint8_t win[2][infl::kWindow];
  const uint32_t t = threadIdx.x;
  for (uint32_t j = t; j < infl::kWindow; j += kInfChainThreads) win[1][j] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < n; ++k) {
    const uint8_t *prev = win[(k & 1) ^ 1];
    uint8_t *cur = win[k & 1];
    const uint2 *src = reinterpret_cast<const uint2 *>(windows + (size_t)k * infl::kWindow);
    uint32_t *dst = reinterpret_cast<uint32_t *>(resolved + (size_t)k * infl::kWindow);
    for (uint32_t q = t; q < infl::kWindow / 4; q += kInfChainThreads) {  // four entries a thread and step
      const uint2 e = src[q];
      const uint32_t v = (uint32_t)infl::resolve_entry((uint16_t)(e.x & 0xffff), prev) |
                         (uint32_t)infl::resolve_entry((uint16_t)(e.x >> 16), prev) << 8 |
                         (uint32_t)infl::resolve_entry((uint16_t)(e.y & 0xffff), prev) << 16 |
                         (uint32_t)infl::resolve_entry((uint16_t)(e.y >> 16), prev) << 24;
      reinterpret_cast<uint32_t *>(cur)[q] = v;
      dst[q] = v;
    }
    __syncthreads();  // window k is whole before k + 1 reads it (and k - 1 is read no more before it is written again)
  }
}

__global__ __launch_bounds__(kWave) void k_inf_write(const uint32_t *__restrict__ words, uint64_t n_words, uint64_t end_bit,
                                                     uint32_t n_owners, InfOwner *__restrict__ owners,
                                                     const uint64_t *__restrict__ offset, const uint8_t *__restrict__ resolved,
                                                     uint8_t *__restrict__ text) {
  __shared__ uint32_t ring32[infl::kWindow / 4];
  __shared__ uint16_t ws[infl::kWsSize];
  uint8_t *ring = reinterpret_cast<uint8_t *>(ring32);
  const infl::Stream s = {words, n_words, end_bit};
  const uint32_t lane = threadIdx.x;
  for (uint32_t k = blockIdx.x; k < n_owners; k += gridDim.x) {
    __syncthreads();
    const uint32_t *prev = k ? reinterpret_cast<const uint32_t *>(resolved + (size_t)(k - 1) * infl::kWindow) : nullptr;
    for (uint32_t i = lane; i < infl::kWindow / 4; i += kWave) ring32[i] = prev ? prev[i] : 0u;
    __syncthreads();
    infl::FinalSink sink = {ring, text + offset[k], 0, owners[k].bytes, infl::kOk, k == 0, lane, (uint32_t)kWave};
    const infl::OwnerEnd e = infl::inflate_owner(s, owners[k].start, owners[k].stop, infl::tables_in(ws), sink);
    uint32_t st = e.status;
    if (st == infl::kOk && (sink.count != owners[k].bytes || e.end_bit != owners[k].end_bit)) st = infl::kErrDiffers;
    if (lane == 0) owners[k].status_b = st;
  }
}

}  // namespace msw
