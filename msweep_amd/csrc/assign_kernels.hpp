// assign_kernels.hpp -- what `mGEMS bin` gives beyond the target bins, on the device: every EC judged
// against ALL estimated groups (how many claim it), the bin of the reads no group claims, and the read x target
// assignment table as text.  Builds on bin_kernels.hpp: the same gamma expressions, slot map, sort and scatter.
#pragma once
#include "bin_kernels.hpp"

namespace msw {

// ---------------------------------------------------------------------------------------
// Rule ([UPSTREAM-UNVERIFIED]): pass(g, j) <=> gamma(g, j) >= log t_g for EVERY estimated group g, log t_g
// formed once on the host; n_assigned[j] = the groups that pass.  The pairs of an EC are its passing TARGETS (slot_of),
// and -- when the unassigned bin is wanted -- one pair with slot n_targets for an EC nobody claims: that slot sorts last
// under bin_kernels.hpp's stable sort, so offsets, k_bin_ptr and k_bin_scatter run unchanged with one more slot.
//
// Passes (host_assign.inc):
//   count   a thread per permuted position: lse_j (kept), the visit, n_assigned[j] and the EC's pair count
//   write   the visit again on the kept lse_j: the pairs at the exclusive scan of the counts (a CSR by EC: the table's 1s)
//   expand  (table only) the EC of every read position; a sort by read id gives the table's rows
//   table   length of every row, exclusive scan, then the rows: the constant "\t0" pattern in 4-byte stores, several
//           lanes per row, the 1s from the EC's pair list
// ---------------------------------------------------------------------------------------
struct AssignGroups {
  const uint32_t *slot_of;  // [G] target slot of every group (kNoSlot: not a target)
  const double *logt;       // [G] log t_g of every estimated group
  uint32_t n_targets;
  uint32_t unassigned;      // 1: an EC with n_assigned == 0 gives the pair (n_targets, j)
  // Background prefilter as BinTargets', but over ALL G groups: over the targets alone it would skip an EC whose only
  // passing group is a background group that is no target.
  double cmax, margin;
};

// f(g) for every group g that EC p (normaliser lse) passes: its listed cells first, in cell order, then the background
// groups in group order.  The count and the write pass both visit through here.
template <int ENC, class F>
__device__ __forceinline__ void assign_visit(const SellDev &S, uint32_t p, double a, double logzi, const double *u,
                                             const AssignGroups &A, double lse, F f) {
  for_each_cell<ENC>(S, p, [&](uint32_t g, double T) {
    if (gamma_cell(a, T, u[g], lse) >= A.logt[g]) f(g);
  });
  if (lse - A.cmax > A.margin * (1.0 + fabs(lse))) return;  // no background group can pass (NaN: visited)
  for (uint32_t g = 0; g < S.n_groups; ++g) {
    if (!(gamma_cell(a, logzi, u[g], lse) >= A.logt[g])) continue;
    bool listed = false;
    for_each_cell<ENC>(S, p, [&](uint32_t gg, double) { listed |= gg == g; });
    if (!listed) f(g);
  }
}

template <bool LDS>
__device__ __forceinline__ const uint32_t *assign_slot_map(const AssignGroups &A, uint32_t G, uint32_t *lds) {
  const BinTargets B{A.slot_of, nullptr, nullptr, 0, 0.0, 0.0};
  return bin_slot_map<LDS>(B, G, lds);
}

// count pass: lse_p[p], n_assigned[perm[p]] = the passing groups, cnt[perm[p]] = the EC's pairs
template <int ENC, bool LDS>
__global__ __launch_bounds__(256) void k_assign_count(SellDev S, double a, double logzi, double tref, const double *u,
                                                     AssignGroups A, double *lse_p, uint32_t *n_assigned, uint32_t *cnt) {
  __shared__ double sh[32];
  extern __shared__ uint32_t assign_lds[];
  double M, U;
  gamma_norm_consts(S.n_groups, u, sh, M, U);
  const uint32_t *slot_of = assign_slot_map<LDS>(A, S.n_groups, assign_lds);
  const double p0 = exp(a * (logzi - tref));
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_ecs; p += gridDim.x * blockDim.x) {
    const double lse = gamma_lse<ENC>(S, p, a, tref, u, M, U, p0);
    uint32_t n = 0, nt = 0;
    assign_visit<ENC>(S, p, a, logzi, u, A, lse, [&](uint32_t g) {
      ++n;
      nt += slot_of[g] != kNoSlot;
    });
    const uint32_t j = S.perm[p];
    lse_p[p] = lse;
    n_assigned[j] = n;
    cnt[j] = nt + (A.unassigned && n == 0 ? 1u : 0u);
  }
}

// write pass: the pairs of EC j at [off[j], off[j + 1])
template <int ENC, bool LDS>
__global__ __launch_bounds__(256) void k_assign_write(SellDev S, double a, double logzi, const double *u, AssignGroups A,
                                                     const double *lse_p, const uint64_t *off, uint32_t *key,
                                                     uint32_t *val) {
  extern __shared__ uint32_t assign_lds[];
  const uint32_t *slot_of = assign_slot_map<LDS>(A, S.n_groups, assign_lds);
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_ecs; p += gridDim.x * blockDim.x) {
    const uint32_t j = S.perm[p];
    uint64_t o = off[j];
    const uint64_t end = off[j + 1];
    uint32_t n = 0;
    auto put = [&](uint32_t k) {
      if (o < end) {
        key[o] = k;
        val[o] = j;
      }
      ++o;
    };
    assign_visit<ENC>(S, p, a, logzi, u, A, lse_p[p], [&](uint32_t g) {
      ++n;
      const uint32_t k = slot_of[g];
      if (k != kNoSlot) put(k);
    });
    if (A.unassigned && n == 0) put(A.n_targets);
  }
}

// out[c] += the reads in the ECs claimed by c = 0 / 1 / >= 2 groups (integer sums: any order gives the same value)
__global__ __launch_bounds__(256) void k_assign_class_reads(const uint32_t *n_assigned, const uint64_t *rptr, uint32_t E,
                                                           unsigned long long *out) {
  unsigned long long s0 = 0, s1 = 0, s2 = 0;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < E; j += gridDim.x * blockDim.x) {
    const unsigned long long len = rptr[j + 1] - rptr[j];
    const uint32_t n = n_assigned[j];
    s0 += n == 0 ? len : 0;
    s1 += n == 1 ? len : 0;
    s2 += n >= 2 ? len : 0;
  }
  for (int d = 32; d > 0; d >>= 1) {
    s0 += __shfl_down(s0, d, 64);
    s1 += __shfl_down(s1, d, 64);
    s2 += __shfl_down(s2, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (s0) atomicAdd(out + 0, s0);
    if (s1) atomicAdd(out + 1, s1);
    if (s2) atomicAdd(out + 2, s2);
  }
}

// reads-by-id index, before its sort: id[i] = reads[i], ec[i] = the EC that holds read position i (the last j with
// rptr[j] <= i: empty ECs are stepped over)
__global__ __launch_bounds__(256) void k_assign_expand(const uint64_t *rptr, const uint32_t *reads, uint32_t E, uint64_t n_rows,
                                                      uint32_t *id, uint32_t *ec) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t lo = 0, hi = E;  // rptr[lo] <= i < rptr[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rptr[mid] <= i) lo = mid;
      else hi = mid;
    }
    id[i] = reads[i];
    ec[i] = lo;
  }
}

// ---- the table: row i of a block = dec(id) then "\t0" or "\t1" per target, then '\n' ---------------------------------------
struct AssignTable {
  const uint32_t *id, *ec;  // the rows of the block: read id and EC, ascending id
  const uint64_t *off;      // [E + 1] the ECs' pairs as the write pass left them ...
  const uint32_t *key;      // ... their target slots (slot n_targets, the unassigned bin's, is no column)
  uint32_t n_targets;
  uint32_t n;               // rows of the block
};

__device__ __forceinline__ uint32_t assign_digits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
         (v >= 100000000u) + (v >= 1000000000u);
}

__global__ __launch_bounds__(256) void k_assign_table_len(AssignTable T, uint32_t *len) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < T.n; i += gridDim.x * blockDim.x)
    len[i] = assign_digits(T.id[i]) + 2u * T.n_targets + 1u;
}

// byte b of a row of nd digits and len bytes
__device__ __forceinline__ uint8_t assign_row_byte(uint32_t id, uint32_t nd, uint32_t len, uint32_t b) {
  if (b + 1 == len) return '\n';
  if (b >= nd) return ((b - nd) & 1u) ? '0' : '\t';
  uint32_t v = id;
  for (uint32_t t = nd - 1 - b; t > 0; --t) v /= 10u;
  return (uint8_t)('0' + v % 10u);
}

// write pass: 2^lanes_log2 lanes per row (256 >> lanes_log2 rows per workgroup at a time).  A lane takes every
// 2^lanes_log2-th aligned 4-byte word of the row: a word inside the "\t0" pattern is one of two constants, the words
// that hold digits, the line end or a neighbour's bytes are put together byte by byte (a row writes its own bytes only).
// Then, behind a barrier, the 1s of the row's EC: one byte per pair of a target.  toff: the rows' byte offsets.
__global__ __launch_bounds__(256) void k_assign_table_write(AssignTable T, const uint64_t *toff, uint32_t lanes_log2, uint8_t *out) {
  const uint32_t L = 1u << lanes_log2, sub = threadIdx.x >> lanes_log2, lane = threadIdx.x & (L - 1u);
  const uint32_t rows = 256u >> lanes_log2;
  for (uint64_t base = (uint64_t)blockIdx.x * rows; base < T.n; base += (uint64_t)gridDim.x * rows) {  // (uniform per workgroup)
    const uint64_t i = base + sub;
    const bool live = i < T.n;
    uint32_t id = 0, nd = 0, len = 0;
    uint64_t o = 0;
    if (live) {
      id = T.id[i];
      nd = assign_digits(id);
      len = nd + 2u * T.n_targets + 1u;
      o = toff[i];
      const uint64_t w1 = (o + len + 3u) & ~(uint64_t)3;
      for (uint64_t w = (o & ~(uint64_t)3) + 4u * lane; w < w1; w += 4u * L) {
        if (w >= o + nd && w + 4u <= o + len - 1u) {
          *reinterpret_cast<uint32_t *>(out + w) = ((w - o - nd) & 1u) ? 0x09300930u : 0x30093009u;
        } else {
          for (uint32_t q = 0; q < 4u; ++q)
            if (w + q >= o && w + q < o + len) out[w + q] = assign_row_byte(id, nd, len, (uint32_t)(w + q - o));
        }
      }
    }
    __syncthreads();  // the pattern is in memory before a 1 goes over it
    if (live) {
      const uint32_t j = T.ec[i];
      for (uint64_t t = T.off[j] + lane; t < T.off[j + 1]; t += L) {
        const uint32_t k = T.key[t];
        if (k < T.n_targets) out[o + nd + 2u * (uint64_t)k + 1u] = '1';
      }
    }
  }
}

}  // namespace msw
