// subset_kernels.hpp -- device side of msw_alignment_subset (host side: host_subset.inc): a resident alignment restricted
// to a set of reads and a set of target sequences, collapsed into equivalence classes again without leaving HBM.
//
// The work is done per CLASS of the source alignment wherever it can be: every class's target list is filtered and
// renumbered once (k_subset_filter, two passes: lengths, then the lists), hashed once (k_subset_hash: the reference's
// recurrence over the renumbered ids, one lane per class as in k_hash_reads), and the selected reads only carry their
// class's index to the sort (k_subset_mark, k_subset_keys).  No atomic decides an order: the bitmap's atomic OR only
// says whether an id was there before, and the smallest repeated id is taken with a min.
#pragma once
#include "reader_kernels.hpp"

namespace msw {

// A class's target list is filtered by ONE LANE up to kSubsetLaneMax targets, by its WAVEFRONT beyond (a ballot and a
// prefix count per kSubsetWaveChunk targets), which LOOPS over lists longer than one chunk.
constexpr uint32_t kSubsetLaneMax = 32;
constexpr uint32_t kSubsetWaveChunk = 64;

struct SubsetCtr {
  uint32_t dup_min;   // smallest read id listed twice (0xffffffff: none)
  uint32_t n_dup;     // flag: an id was listed twice
};

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int lane) {
  return (uint64_t)(uint32_t)__shfl((uint32_t)(v >> 32), lane) << 32 | (uint32_t)__shfl((uint32_t)v, lane);
}

// keep[t] != 0 as a word per target, for the scan that ranks the kept targets
__global__ void k_subset_keep_flags(const uint8_t *keep, uint64_t n, uint32_t *flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    flag[i] = keep[i] != 0;
}

// Every class's target list without the dropped targets, the kept ones as their rank among the kept.
// WRITE = false: flen[e] = the new length.  WRITE = true: the list itself at ftgt[fptr[e] ..] (fptr: the scan of flen).
// A wavefront takes 64 classes at a time: the short lists one per lane, then the long ones one after the other.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_subset_filter(const uint64_t *tptr, const uint32_t *tgt, uint64_t E, const uint32_t *keepf,
                                                       const uint64_t *rank, uint32_t *flen, const uint64_t *fptr, uint32_t *ftgt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e0 = t0 & ~63ull; e0 < E; e0 += step) {
    const uint64_t e = e0 + lane;
    uint64_t b = 0;
    uint32_t len = 0;
    if (e < E) {
      b = tptr[e];
      len = (uint32_t)(tptr[e + 1] - b);
    }
    if (e < E && len <= kSubsetLaneMax) {
      const uint64_t d = WRITE ? fptr[e] : 0;
      uint32_t n = 0;
      for (uint32_t k = 0; k < len; ++k) {
        const uint32_t t = tgt[b + k];
        if (!keepf[t]) continue;
        if (WRITE) ftgt[d + n] = (uint32_t)rank[t];
        ++n;
      }
      if (!WRITE) flen[e] = n;
    }
    uint64_t longs = __ballot(e < E && len > kSubsetLaneMax);
    while (longs) {  // (the same in every lane)
      const int l = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const uint64_t rb = shfl_u64(b, l);
      const uint32_t rlen = (uint32_t)__shfl(len, l);
      const uint64_t d = WRITE ? fptr[e0 + l] : 0;
      uint32_t n = 0;
      for (uint32_t c = 0; c < rlen; c += kSubsetWaveChunk) {
        const uint32_t k = c + lane;
        bool kp = false;
        uint32_t t = 0;
        if (k < rlen) {
          t = tgt[rb + k];
          kp = keepf[t] != 0;
        }
        const uint64_t m = __ballot(kp);
        if (WRITE && kp) ftgt[d + n + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = (uint32_t)rank[t];
        n += (uint32_t)__popcll(m);
      }
      if (!WRITE && lane == 0) flen[e0 + l] = n;
    }
  }
}

// the reference's hash of every filtered list (include/mSWEEP_alignment.hpp:152-156, over the renumbered ids)
__global__ void k_subset_hash(const uint64_t *fptr, const uint32_t *ftgt, uint64_t E, uint64_t *hkey) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t h = 0;
    for (uint64_t k = fptr[e]; k < fptr[e + 1]; ++k) h ^= (uint64_t)ftgt[k] + 0x517cc1b727220a95ull + (h << 6) + (h >> 2);
    hkey[e] = h;
  }
}

// bits: one per read id of [0, largest selected id]; an id whose bit was set before is listed twice
__global__ void k_subset_bitmap(const uint32_t *ids, uint64_t n, uint32_t *bits, SubsetCtr *ctr) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i], bit = 1u << (id & 31);
    if (atomicOr(&bits[id >> 5], bit) & bit) {
      atomicMin(&ctr->dup_min, id);
      ctr->n_dup = 1u;
    }
  }
}

// Per aligned read of the source: selected, and its class keeps a target?  Then flag[id] = 1 and cls[id] = its class
// (the last e with rptr[e] <= k).  A read id is in one class only: no two threads write the same entry.
// n_space: the largest selected id + 1 (the bitmap's and the tables' extent).
__global__ void k_subset_mark(const uint64_t *rptr, const uint32_t *reads, uint64_t K, uint64_t E, const uint32_t *bits,
                              uint64_t n_space, const uint32_t *flen, uint32_t *flag, uint32_t *cls) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t id = reads[k];
    if (id >= n_space || !(bits[id >> 5] >> (id & 31) & 1u)) continue;
    uint64_t lo = 0, hi = E;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (rptr[mid] <= k) lo = mid;
      else hi = mid;
    }
    if (!flen[lo]) continue;
    flag[id] = 1u;
    cls[id] = (uint32_t)lo;
  }
}

// the flagged reads in ascending id order (idx: the scan of flag), keyed by their class's new hash
__global__ void k_subset_keys(const uint32_t *flag, const uint64_t *idx, const uint32_t *cls, const uint64_t *hkey,
                              uint64_t n_space, uint64_t *keys, uint32_t *ids) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_space; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!flag[i]) continue;
    keys[idx[i]] = hkey[cls[i]];
    ids[idx[i]] = (uint32_t)i;
  }
}

// k_ec_meta / k_ec_rows of the reader with the representative's row taken from its class's filtered list
__global__ void k_subset_meta(const uint32_t *head, const uint64_t *eidx, const uint32_t *ids, const uint32_t *cls,
                              const uint32_t *flen, uint64_t K, uint64_t *rptr, uint32_t *tlen) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (uint64_t)gridDim.x * blockDim.x) {
    if (!head[k]) continue;
    const uint64_t e = eidx[k];
    rptr[e] = k;
    tlen[e] = flen[cls[ids[k]]];
  }
}
__global__ __launch_bounds__(256) void k_subset_rows(const uint64_t *rptr, const uint32_t *ids, const uint32_t *cls,
                                                     const uint64_t *fptr, const uint32_t *ftgt, const uint64_t *tptr, uint64_t E,
                                                     uint64_t *counts, uint32_t *out) {
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e0 = t0 & ~63ull; e0 < E; e0 += step) {
    const uint64_t e = e0 + (threadIdx.x & 63);
    uint64_t so = 0, d0 = 0;
    uint32_t len = 0;
    if (e < E) {
      counts[e] = rptr[e + 1] - rptr[e];
      so = fptr[cls[ids[rptr[e]]]];
      d0 = tptr[e];
      len = (uint32_t)(tptr[e + 1] - d0);
    }
    wave_copy_rows(ftgt, so, out, d0, len);
  }
}

}  // namespace msw
