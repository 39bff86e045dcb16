// guard.hpp -- the guarded ECs of the sweeps: deferral queue, walk over an EC's listed and unlisted groups, tail limbs.
#pragma once
#include <type_traits>

#include "device_util.hpp"
#include "sell.hpp"

namespace msw {

// ---------------------------------------------------------------------------------------
// Guarded ECs (SURVEY.md 7.3 ii).  The sweeps form Z_j = p0 * U + sum_listed e_g (x_gj - p0): when
// the listed groups hold nearly all of U and their cells sit far below the background (x << p0:
// an isolate's read that hits the dominant lineage with one k-mer, priors << 1) the two parts cancel
// and Z_j, r_j = c_j / Z_j and the listed groups' column sums lose their digits -- or their sign.
// An EC whose Z_j comes out below 2^-8 of the background sum (the unguarded relative error is thus
// at most 2^-45; with the reference's WOR21 tables, whose values stay within e^-1 of log(zi) up to
// groups of 400 sequences, no EC comes near it) is set aside by the sweep (its position appended to the workgroup's list) and
// evaluated WITHOUT the background trick at the end of the workgroup, a wavefront per EC:
// Z_j = sum_listed e_g x_gj + p0 * (sum over the groups NOT listed, one by one), and every group's
// share of c_j added directly.  O(G) per guarded EC; none exist in ordinary inputs.
//
// The protocol, once for the three sweeps (k_passA, k_passB, the fp32 EM sweep):
//   * list: a workgroup's sweep appends (GuardQueue::defer), its own wavefronts read the entries back behind a barrier
//     (count, entry).  The count lives in LDS and is reset at the head of every sweep: nothing is carried between launches.
//   * bits: one bitmap of listed groups per wavefront, zeroed by the host with the solver state and all zero between any
//     two ECs: guard_walk sets the bits of the EC it evaluates, and the wavefront clears the words it read before it
//     leaves the EC on EVERY exit (the Z <= 0 one: guard_clear).  Nobody may leave a bit set.
//   * tail: the guarded ECs' shares per group (pass B and the fp32 sweep: guard_share_add).  Zeroed by the host with the
//     solver state and by whoever consumes it: k_redfin, or k_colsum of an EC-sharded solve (which hands the limbs on).
//   * err: 1 = an EC has no probability under any group (Z = 0 with every group visited: reported, not divided by);
//     2 = more ECs set aside than a workgroup's list holds (cannot happen while guard_cap mirrors the sweeps' stride).
//   * visits (msw_core_guarded_visits): counted by pass B and the fp32 sweep only -- pass A sets aside the same ECs of
//     the same iteration: counting there too would report each twice -- and, as the ECs are evaluated, only in the first
//     run of a pass B that runs once per range of groups (mode 4).
// ---------------------------------------------------------------------------------------
constexpr double kGuardRatio = 0x1p-8;
struct GuardDev {
  uint32_t *list;          // [workgroups * cap] positions of the ECs set aside, per workgroup
  uint32_t *bits;          // [workgroups * 16 * words] one bitmap of listed groups per wavefront
  unsigned long long *tail;  // [2 * G] the guarded ECs' shares per group, two fixed-point limbs (pass B)
  const double *lut_area;  // table value of every slot-area entry
  int *err;                // set when an EC has no probability under any group
  unsigned long long *visits;  // ECs pass B has taken through the guard path so far (reporting: msw_core_guarded_visits)
  uint32_t cap, words;
};
// The workgroup's count of deferred ECs: double 16 of the reduction scratch at scratch_off of the LDS image (sell.hpp).
// Around it pass A uses doubles 0..15 (block sums) and 18, 19 (background moments); pass B none of the first 32 (its
// block sums take 32..79, over the slice geometry); the fp32 sweep 8..55, in its block sums BEHIND the guard section.
constexpr uint32_t kGuardCountByte = 128;

// Setting an EC aside.  T = the arithmetic of the sweep's own test Z >= threshold(): double, or float (fp32 EM sweep).
template <class T>
struct GuardQueue {
  typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
  const GuardDev &GD;
  uint32_t cnt_off;  // LDS byte address of the count
  T zbase;           // the background sum p0 * U
  __device__ __forceinline__ GuardQueue(const GuardDev &gd, uint32_t scratch_off, T zb)
      : GD(gd), cnt_off(scratch_off + kGuardCountByte), zbase(zb) {}
  __device__ __forceinline__ T threshold() const {  // ECs whose Z falls below it are set aside (Z = 0 too: reported)
    if constexpr (std::is_same<T, float>::value) return fmaxf(zbase * (float)kGuardRatio, 1.17549435e-38f);
    else return fmax(zbase * kGuardRatio, 2.2250738585072014e-308);
  }
  __device__ __forceinline__ void reset(int tid) const { if (tid == 0) *(lds_u32_t *)(size_t)cnt_off = 0u; }  // head of the sweep
  __device__ __forceinline__ void defer(uint32_t pos) const {
    const uint32_t i = __hip_atomic_fetch_add((lds_u32_t *)(size_t)cnt_off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (i < GD.cap) GD.list[(size_t)blockIdx.x * GD.cap + i] = pos;
    else *GD.err = 2;
  }
  __device__ __forceinline__ uint32_t count() const { return min(*(lds_u32_t *)(size_t)cnt_off, GD.cap); }  // behind a barrier
  __device__ __forceinline__ uint32_t entry(uint32_t i) const { return GD.list[(size_t)blockIdx.x * GD.cap + i]; }
  __device__ __forceinline__ uint32_t *bits(uint32_t wv) const { return GD.bits + (size_t)(blockIdx.x * 16 + wv) * GD.words; }
};

// Every group of the EC at position p, for a whole wavefront: listed(g, T) for the groups of its cells (a cell per
// lane and step), unlisted(g) for every other group < G.  MARK: set the listed groups' bits first (the first walk
// over an EC; a second one finds them set); CLEAR: clear the words read (the last walk over an EC).
template <int ENC, bool MARK, bool CLEAR, class FL, class FU>
__device__ __forceinline__ void guard_walk(const SellDev &S, const GuardDev &GD, uint32_t *bits, uint32_t p, uint32_t lane,
                                           uint32_t G, FL listed, FU unlisted) {
  wave_cells<ENC>(S, p, lane, [&](uint32_t g, double T) {
    listed(g, T);
    if (MARK) atomicOr(&bits[g >> 5], 1u << (g & 31));
  });
  if (MARK) __builtin_amdgcn_s_waitcnt(0);  // the bitmap updates have reached memory before it is read back
  for (uint32_t w0 = lane; w0 < GD.words; w0 += 64) {
    const uint32_t set = CLEAR ? atomicAnd(&bits[w0], 0u) : atomicOr(&bits[w0], 0u);  // (read and clear / read)
    for (uint32_t b = 0; b < 32; ++b)
      if (w0 * 32 + b < G && !((set >> b) & 1u)) unlisted(w0 * 32 + b);
  }
}
// ... and for the exit that does not walk a second time
__device__ __forceinline__ void guard_clear(uint32_t *bits, uint32_t lane, uint32_t words) {
  for (uint32_t w0 = lane; w0 < words; w0 += 64) atomicAnd(&bits[w0], 0u);
}

// A group's share of a guarded EC, in reads, goes to two global 64-bit fixed-point accumulators: tail[2 g] in units of
// 2^-t reads, tail[2 g + 1] of 2^-(t + 36) (2^t = Scalars::fx_tscale, 2^-t = fx_tinv).  Such a share can exceed any bound
// the group's own exponent allows for (c e_g p0 / Z with Z far below the background sum), while the shares of one EC
// always add up to c_j.  Global integer atomics: rare path.  k_redfin joins the limbs back into reads.
__device__ __forceinline__ void guard_share_add(unsigned long long *tail, uint32_t g, double share, double tscale) {
  const double vh = fma(share, tscale, kFxMagic);
  const double qh = vh - kFxMagic;                     // rint(share * 2^t), exact
  const double ql = fma(share, tscale, -qh) * 0x1p36;  // remainder, |.| <= 2^35
  atomicAdd(&tail[2 * (size_t)g], fx_bits(1.0, qh));
  atomicAdd(&tail[2 * (size_t)g + 1], fx_bits(1.0, ql));
}
__device__ __forceinline__ double guard_share_join(long long hi, long long lo, double tinv) {
  return (double)hi * tinv + (double)lo * (tinv * 0x1p-36);
}

// Pass B's evaluation of the guarded EC at position p: Z over every group, then each group's share of c_j to the tail
// limbs -- listed: c e_g x / Z, not listed: c e_g p0 / Z -- and the EC stays out of W = sum r_j (the background share
// of the ordinary ECs).  The first lane hands elbo(c, Z, r, H) what the sweep's ELBO sums need.  F32 = the fp32 EM
// sweep's form, which differs in three ways only: a = 1, T rounded through float, no H term.
template <int ENC, bool F32, class FE>
__device__ __forceinline__ void guard_eval_B(const SellDev &S, const GuardDev &GD, uint32_t *bits, uint32_t p, uint32_t lane,
                                             uint32_t G, const double *e_g, double a, double tref, double p0, double logzi,
                                             double tscale, FE elbo) {
  auto X = [&](double T) { return F32 ? exp((double)(float)T - tref) : exp(a * (T - tref)); };
  const double c = S.cvec[p];
  double z = 0.0, h = 0.0, r0 = 0.0;
  guard_walk<ENC, true, false>(S, GD, bits, p, lane, G, [&](uint32_t g, double T) {
    const double q = e_g[g] * X(T);
    z += q;
    if constexpr (!F32) h = fma(q, T, h);
  }, [&](uint32_t g) { r0 += e_g[g]; });
  z = wave_sum(z), r0 = wave_sum(r0);
  if constexpr (!F32) h = wave_sum(h);
  const double Z = fma(p0, r0, z), H = fma(p0 * logzi, r0, h);
  if (Z > 0.0) {
    const double rj = c / Z;
    if (lane == 0) elbo(c, Z, rj, H);
    guard_walk<ENC, false, true>(S, GD, bits, p, lane, G, [&](uint32_t g, double T) { guard_share_add(GD.tail, g, e_g[g] * rj * X(T), tscale); },
                    [&](uint32_t g) { guard_share_add(GD.tail, g, e_g[g] * (rj * p0), tscale); });
  } else {
    if (lane == 0) *GD.err = 1;  // no probability under any group: the solve reports it
    guard_clear(bits, lane, GD.words);
  }
}

}  // namespace msw
