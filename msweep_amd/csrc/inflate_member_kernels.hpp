// inflate_member_kernels.hpp -- BGZF (bgzip) pseudoalignment input inflated on the device, per member
// (host_inflate_members.inc).  A BGZF file is thousands of small gzip members, each stating its compressed length in its
// header and CRC-32 and length of its text (at most 64 KiB) in its trailer, each starting with an empty window: the host
// walks headers and trailers (infl::walk_members) and knows every member's payload and its offset in the text before a
// kernel runs.  What inflate_kernels.hpp needs for one long member -- a probe for block starts, a pass against an unknown
// window, the window chain, a second pass -- has nothing to do here:
//   k_infm_decode  a wavefront per member: infl::inflate_owner from the member's first payload bit to its final block,
//                  the bytes to the text at the member's offset; then the member's trailer check in the same wavefront:
//                  the final block ends in the member's last payload byte, the byte count is ISIZE, and the CRC-32 of the
//                  bytes just written (each lane a 64th of them, the pieces joined by crc_shift) is the trailer's.
// The check is fused into the decode because it is small beside it and needs what the decode has at hand: by instruction
// count the 64 lanes take tens of microseconds over 64 KiB (~100 operations a word, 256 words a lane) that the same
// wavefront took ~8 ms to decode, the text is still in the CU's cache, and a second kernel would read the table and the
// text again and be handed end bit and count through memory to come to the same words.  Only a count of bad members and the first
// of them (index, reason, decode status) come back; the text stays where the token kernels read it.
// Lane mapping and lock step are those of k_inf_write (inflate_kernels.hpp): one thread of control per member, run by all
// 64 lanes with the same values, so that a match is copied 64 bytes a step through the 32 KiB ring in LDS and leaves as
// one coalesced store; literals are lane 0's.  The lock step IS the synchronisation -- the lanes bump the same LDS words
// without atomics and read ring bytes other lanes wrote one instruction earlier with no barrier in between -- which is
// correct only because a wave64 executes one instruction stream and its LDS accesses complete in order: the workgroup
// must be exactly one wavefront of 64 lanes (the static_assert and __launch_bounds__(kWave) below;
// host_inflate_members.inc launches dim3(kWave)).  The CRC part is per lane and needs no lock step; one barrier of the
// (one-wavefront) workgroup puts the decode's stores in front of its loads.
// The member's Stream ends at its own trailer (infl::member_stream), so a damaged member cannot read into its
// neighbour; every loop is bounded by the member's bit length or by cap = ISIZE <= 64 KiB, which also bounds the stores:
// host_inflate_members.inc allocates the sum of ISIZE and hands every member its prefix sum.  The ring starts empty and is
// not initialised: with first = true a distance beyond the bytes written is an error, so nothing unwritten is read.
// Decode tables, code lengths and the ring live in LDS (36.4 KiB: four workgroups share a CU's 160 KiB); no scratch
// memory is used (tests/test_inflate_member_kernel_resources.py).
#pragma once
#include "common.hpp"
#include "inflate_format.hpp"

namespace msw {

static_assert(kWave == 64, "the member decode runs one wave64 per workgroup in lock step: no barrier orders its LDS traffic");

// what comes back: bad[0] = the smallest (member index << 32 | decode status << 8 | reason) of the members that failed
// (kInfmAllGood: none did), bad[1] = how many failed
constexpr unsigned long long kInfmAllGood = ~0ull;

__global__ __launch_bounds__(kWave) void k_infm_decode(const uint32_t *__restrict__ words, uint64_t n_words,
                                                       const infl::MemberEntry *__restrict__ members, uint32_t n_members,
                                                       const uint32_t *__restrict__ pow8, uint8_t *__restrict__ text,
                                                       unsigned long long *__restrict__ bad) {
  __shared__ uint32_t ring32[infl::kWindow / 4];
  __shared__ uint16_t ws[infl::kWsSize];
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (k >= n_members) return;
  const infl::MemberEntry m = members[k];
  const infl::Stream s = infl::member_stream(words, n_words, m);
  uint8_t *out = text + m.text_off;
  // (all 64 lanes run the decode in lock step -- the same addresses, the same values -- so that a match is one step)
  infl::FinalSink sink = {reinterpret_cast<uint8_t *>(ring32), out, 0, m.isize, infl::kOk, true, lane, (uint32_t)kWave};
  const infl::OwnerEnd e = infl::inflate_owner(s, m.first_bit, infl::kNoStart, infl::tables_in(ws), sink);
  int32_t why = infl::member_verdict(e, sink.count, m);
  __syncthreads();  // the wavefront's stores to its text are in front of the loads below
  if (why == infl::kWhyNone) {
    // CRC-32 of out[0 .. ISIZE): lane l takes bytes [lo, hi) from a zero register, single bytes up to a word boundary
    const uint32_t n = m.isize, piece = (n + kWave - 1) / kWave;
    const uint32_t lo = min(n, lane * piece), hi = min(n, lo + piece);
    uint32_t r = 0, i = lo;
    for (; i < hi && (reinterpret_cast<uintptr_t>(out + i) & 3); ++i) r = defl::crc_word(r, out[i], 1);
    for (; i + 4 <= hi; i += 4) r = defl::crc_word(r, *reinterpret_cast<const uint32_t *>(out + i), 4);
    for (; i < hi; ++i) r = defl::crc_word(r, out[i], 1);
    uint32_t acc = defl::crc_shift(r, n - hi, pow8);
    for (int d = 1; d < kWave; d <<= 1) acc ^= __shfl_xor(acc, d);
    if (~(defl::crc_shift(0xffffffffu, n, pow8) ^ acc) != m.crc) why = infl::kWhyCrc;
  }
  if (why != infl::kWhyNone && lane == 0) {
    atomicMin(&bad[0], (unsigned long long)k << 32 | (unsigned long long)(e.status & 0xffffffu) << 8 | (unsigned long long)why);
    atomicAdd(&bad[1], 1ull);
  }
}

}  // namespace msw
