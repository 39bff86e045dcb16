// gamma_cell.hpp -- the expressions of gamma(g, j) = a*L(g, j) + u_g - lse_j as device functions, for every unit whose
// kernels judge or print a cell: k_gamma_block (gamma_kernels.hpp), the bin and assign passes (bin_kernels.hpp,
// assign_kernels.hpp) and the sparse probabilities (sparse_probs_kernels.hpp) all form gamma with these, so each works on
// the bits msw_core_gamma_block returns.  No kernel is defined here.
#pragma once
#include "device_util.hpp"
#include "guard.hpp"
#include "sell.hpp"

namespace msw {

// The per-EC normaliser of gamma and the value of one cell, shared by k_gamma_block and the bin pass
// (bin_kernels.hpp): both compute gamma(g, j) with these very expressions, so a read binned on the device is binned
// by the same bits msw_core_gamma_block returns.  gamma_norm_consts: M = max_g u_g and U = sum_g exp(u_g - M) over
// the block (256 threads: the order of block_sum's additions depends on the block size); p0 = exp(a (logzi - tref)).
__device__ __forceinline__ void gamma_norm_consts(uint32_t G, const double *u, double *sh, double &M, double &U) {
  const int tid = threadIdx.x;
  double m = -INFINITY;
  for (uint32_t g = tid; g < G; g += blockDim.x) m = fmax(m, u[g]);
  M = block_max(m, sh);
  double su = 0.0;
  for (uint32_t g = tid; g < G; g += blockDim.x) su += exp(u[g] - M);
  U = block_sum(su, sh);
}
// lse_j of the EC at permuted position p: every exp(a T) relative to tref (the table value with the largest a T, log zi
// included): <= 1
template <int ENC>
__device__ __forceinline__ double gamma_lse(const SellDev &S, uint32_t p, double a, double tref, const double *u,
                                            double M, double U, double p0) {
  double zs = 0.0;
  for_each_cell<ENC>(S, p, [&](uint32_t g, double T) { zs += exp(u[g] - M) * (exp(a * (T - tref)) - p0); });
  double Z = p0 * U + zs;
  if (!(Z >= p0 * U * kGuardRatio)) {  // guarded EC (guard.hpp): every group visited instead
    Z = 0.0;
    for (uint32_t g = 0; g < S.n_groups; ++g) {
      double xg = p0;
      for_each_cell<ENC>(S, p, [&](uint32_t gg, double T) { if (gg == g) xg = exp(a * (T - tref)); });
      Z += exp(u[g] - M) * xg;
    }
  }
  return M + log(Z) + a * tref;
}
// gamma of one cell: T = the listed value, or log zi for the background
__device__ __forceinline__ double gamma_cell(double a, double T, double ug, double lse) { return a * T + ug - lse; }

}  // namespace msw
