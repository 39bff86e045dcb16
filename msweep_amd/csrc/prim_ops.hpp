// prim_ops.hpp -- the element types and length functors that the rocPRIM scans of prim.hip read.  They stand here, not
// in the kernel headers that use them (inflate_kernels.hpp, bin_kernels.hpp, fastq_kernels.hpp include this file), so
// that prim.hip can name them without holding those headers' kernels a second time.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace msw {

struct InfOwner {       // one owner: what the host sets, what pass (a) leaves, what pass (b) adds
  uint64_t start, stop;  // first bit; the next owner's first bit (infl::kNoStart: to the final block)
  uint64_t end_bit, bytes;
  uint32_t status, final, status_b, pad;
};

// read count of the i-th sorted pair (0 for the spare element i = n: the exclusive scan's total)
struct BinPairLen {
  const uint32_t *ec;
  const uint64_t *rptr;
  size_t n;
  __host__ __device__ uint64_t operator()(size_t i) const { return i < n ? rptr[ec[i] + 1] - rptr[ec[i]] : 0; }
};

// length of the i-th selected record; i == m: the spare zero behind them (the scan's total)
struct FqLen {
  const uint32_t *ids;
  const uint64_t *rec_off;
  size_t m;
  __host__ __device__ uint64_t operator()(size_t i) const {
    if (i >= m) return 0;
    const uint64_t id = ids[i];
    return rec_off[id + 1] - rec_off[id];
  }
};

}  // namespace msw
