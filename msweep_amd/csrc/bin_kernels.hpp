// bin_kernels.hpp -- the mGEMS binning step on the device (src/mSWEEP.cpp:437-469, mGEMS::BinFromMatrix): the read
// ids of every target group's bin, without the G x E responsibility matrix anywhere.
#pragma once
#include "gamma_kernels.hpp"
#include "prim_ops.hpp"

namespace msw {

// ---------------------------------------------------------------------------------------
// Read-to-bin rule ([UPSTREAM-UNVERIFIED]): the reads of EC j go to the bin of target k when
// gamma(g_k, j) >= log t_k, t_k = 1 - theta_k (log t_k formed once on the host).  gamma is formed with
// gamma_kernels.hpp's expressions, so the bins equal that rule applied to msw_core_gamma_block's output, bit for bit.
//
// Passes (host_bin.inc):
//   count   a thread per permuted position p, EC j = perm[p]: lse_j (kept, 8 B per EC), the passing targets among the
//           EC's listed cells, then -- only when lse_j could let one through (prefilter below) -- the background
//           targets; cnt[j] = how many passed.
//   write   the same visit again on the kept lse_j, the (target slot, j) pairs written at the exclusive scan of cnt in
//           EC order.  A stable radix sort by slot (host) leaves every target's pairs in EC order.
//   scatter the reads of every sorted pair to its output offset (the exclusive scan of the pairs' read counts).
// ---------------------------------------------------------------------------------------
constexpr uint32_t kNoSlot = 0xffffffffu;
constexpr uint32_t kBinLdsGroups = 12288;  // slot map in LDS up to this many groups (48 KB), in global memory beyond

struct BinTargets {
  const uint32_t *slot_of;  // [G] target slot of every group (kNoSlot: not a target)
  const uint32_t *grp;      // [n] group of every target slot
  const double *logt;       // [n] log t_k
  uint32_t n;
  // Background prefilter: c_k = a logzi + u[g_k] - log t_k, cmax = max_k c_k.  An EC with lse_j - cmax > margin has no
  // passing background target; every EC the prefilter lets through is tested with the exact expression, so it only
  // decides which ECs skip the loop, never a pass.  margin is a large multiple of the rounding of both sides.
  double cmax, margin;
};

// The slot map the kernels read: a copy in LDS (LDS = true) or the global array
template <bool LDS>
__device__ __forceinline__ const uint32_t *bin_slot_map(const BinTargets &B, uint32_t G, uint32_t *lds) {
  if constexpr (LDS) {
    for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) lds[g] = B.slot_of[g];
    __syncthreads();
    return lds;
  } else {
    return B.slot_of;
  }
}

// f(k) for every target slot k that EC p (normaliser lse) passes: its listed cells first, in cell order, then the
// background targets in slot order.  Count and write pass both visit through here: the same passes, the same number.
template <int ENC, class F>
__device__ __forceinline__ void bin_visit(const SellDev &S, uint32_t p, double a, double logzi, const double *u,
                                          const uint32_t *slot_of, const BinTargets &B, double lse, F f) {
  for_each_cell<ENC>(S, p, [&](uint32_t g, double T) {
    const uint32_t k = slot_of[g];
    if (k != kNoSlot && gamma_cell(a, T, u[g], lse) >= B.logt[k]) f(k);
  });
  if (lse - B.cmax > B.margin * (1.0 + fabs(lse))) return;  // no background target can pass (NaN: visited)
  for (uint32_t k = 0; k < B.n; ++k) {
    const uint32_t g = B.grp[k];
    if (!(gamma_cell(a, logzi, u[g], lse) >= B.logt[k])) continue;
    bool listed = false;
    for_each_cell<ENC>(S, p, [&](uint32_t gg, double) { listed |= gg == g; });
    if (!listed) f(k);
  }
}

// count pass: lse_p[p] = lse of the EC at position p, cnt[perm[p]] = its passing targets
template <int ENC, bool LDS>
__global__ __launch_bounds__(256) void k_bin_count(SellDev S, double a, double logzi, double tref, const double *u,
                                                  BinTargets B, double *lse_p, uint32_t *cnt) {
  __shared__ double sh[32];
  extern __shared__ uint32_t bin_lds[];
  double M, U;
  gamma_norm_consts(S.n_groups, u, sh, M, U);
  const uint32_t *slot_of = bin_slot_map<LDS>(B, S.n_groups, bin_lds);
  const double p0 = exp(a * (logzi - tref));
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_ecs; p += gridDim.x * blockDim.x) {
    const double lse = gamma_lse<ENC>(S, p, a, tref, u, M, U, p0);
    uint32_t n = 0;
    bin_visit<ENC>(S, p, a, logzi, u, slot_of, B, lse, [&](uint32_t) { ++n; });
    lse_p[p] = lse;
    cnt[S.perm[p]] = n;
  }
}

// write pass: the pairs of EC j at [off[j], off[j + 1]) (the visit of the count pass again, on its lse)
template <int ENC, bool LDS>
__global__ __launch_bounds__(256) void k_bin_write(SellDev S, double a, double logzi, const double *u, BinTargets B,
                                                  const double *lse_p, const uint64_t *off, uint32_t *key,
                                                  uint32_t *val) {
  extern __shared__ uint32_t bin_lds[];
  const uint32_t *slot_of = bin_slot_map<LDS>(B, S.n_groups, bin_lds);
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_ecs; p += gridDim.x * blockDim.x) {
    const uint32_t j = S.perm[p];
    uint64_t o = off[j];
    const uint64_t end = off[j + 1];
    bin_visit<ENC>(S, p, a, logzi, u, slot_of, B, lse_p[p], [&](uint32_t k) {
      if (o < end) {
        key[o] = k;
        val[o] = j;
      }
      ++o;
    });
  }
}

// (BinPairLen, the read count of the i-th sorted pair: prim_ops.hpp)

// bin_ptr[k] = output offset of the first pair of slot k (k = n_targets: the total); keys sorted ascending
__global__ __launch_bounds__(256) void k_bin_ptr(const uint32_t *key, size_t n, const uint64_t *roff, uint32_t n_targets,
                                                uint64_t *bin_ptr) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_targets) return;
  size_t lo = 0, hi = n;  // lower_bound of k
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (key[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  bin_ptr[k] = roff[lo];
}

// scatter: a wavefront takes 64 sorted pairs at a time; a lane copies the reads of a short EC itself, the whole
// wavefront copies each long one in turn
constexpr uint64_t kBinShortEc = 16;
__global__ __launch_bounds__(256) void k_bin_scatter(const uint32_t *ec, size_t n, const uint64_t *rptr,
                                                    const uint32_t *reads, const uint64_t *roff, uint32_t *out) {
  const uint32_t lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t base = wave * 64; base < n; base += n_waves * 64) {
    const size_t i = base + lane;
    unsigned long long b = 0, len = 0, o = 0;
    if (i < n) {
      const uint32_t j = ec[i];
      b = rptr[j];
      len = rptr[j + 1] - b;
      o = roff[i];
    }
    const bool lng = len > kBinShortEc;
    if (!lng)
      for (unsigned long long t = 0; t < len; ++t) out[o + t] = reads[b + t];
    unsigned long long m = __ballot(lng);
    while (m) {
      const int l = __ffsll(m) - 1;
      m &= m - 1;
      const unsigned long long bl = __shfl(b, l, 64), ll = __shfl(len, l, 64), ol = __shfl(o, l, 64);
      for (unsigned long long t = lane; t < ll; t += 64) out[ol + t] = reads[bl + t];
    }
  }
}

}  // namespace msw
