// sweep_launch.hpp -- launch of the templated CSR sweeps (sweep_kernels.hpp) and the dispatch over their instantiations,
// for the sweep_<encoding>.hip units: a launch function sits in the unit that holds the instantiations it launches, so that the
// kernel pointer, prepare_sweep's attribute calls and the launch see one registered kernel.
#pragma once
#include "host_api.hpp"
#include "sweep_kernels.hpp"

namespace {

// ---- launch helpers for the templated sweeps ----------------------------------------------
// The sweeps address their LDS image by absolute ds addresses taken from the records: the image
// must start at LDS address 0, i.e. the kernels must not own static __shared__ memory.
template <class K>
void prepare_sweep(K k, size_t lds, size_t &lds_set) {
  if (lds > lds_set) {  // raise the dynamic-LDS limit of this instantiation only when it grows
    hipFuncAttributes fa;
    MSW_HIP(hipFuncGetAttributes(&fa, (const void *)k));
    if (fa.sharedSizeBytes != 0) throw Fail("internal: sweep kernel owns static LDS");
    grant_dynamic_lds((const void *)k, lds);  // (process wide and only ever raised: another handle's smaller layout does not lower it)
    lds_set = lds;
  }
}
template <int ENC, bool GL, bool TL>
void launch_passA_t(const Resident &L, Solver &s) {
  const size_t lds = pass_lds_bytes(GL ? 1 : 0, L.n_tab_lds, L.G, true, ENC == kEncIndex);
  // ML: some slices hold ECs over several lanes (sell.hpp slice classes) -- an instantiation of its own: the few
  // scalar operations and branches the classes cost per slice are 2-3 % of a sweep over short slices (cfg3, cfg5)
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  auto k = ml ? k_passA<ENC, GL, TL, true> : k_passA<ENC, GL, TL, false>;
  prepare_sweep(k, lds, s.lds_attr[0][(ml ? 40 : 0) + ENC * 4 + (GL ? 2 : 0) + (TL ? 1 : 0)]);
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_A<ENC>()), lds, s.stream, s.sc.p, sell_view(L, s),
                     s.ew.p, s.tabA.p, s.partA.p, s.partR.p, (int)((L.G + kRedfinGroups - 1) / kRedfinGroups),
                     guard_view(L, s));
}
template <int ENC, int GM, bool TL>
void launch_passB_t(const Resident &L, Solver &s) {
  const size_t lds = pass_lds_bytes(GM, L.n_tab_lds, L.G, false, ENC == kEncIndex);
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  if constexpr (ENC == kEncNarrow) {
    if (L.passB_rc8 && !ml) {  // (nearly) every slice at most 8 rows: 16 wavefronts per workgroup (finish_sell)
      auto k8 = k_passB<ENC, GM, TL, false, 8>;
      prepare_sweep(k8, lds, s.lds_attr[2][2 * GM + (TL ? 1 : 0)]);
      const auto rg_of = [&](uint32_t g0) {
        return GM == 4 ? RangeB{g0, std::min<uint32_t>(kRangeGroups, L.G - g0), g0 == 0 ? 1 : 0} : RangeB{0, 0, 1};
      };
      for (uint32_t g0 = 0; g0 < (GM == 4 ? L.G : 1u); g0 += kRangeGroups)
        hipLaunchKernelGGL(k8, dim3(L.nblk), dim3(pass_threads_B<ENC, GM, TL, 8>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                           s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p, rg_of(g0), guard_view(L, s));
      return;
    }
  }
  auto k = ml ? k_passB<ENC, GM, TL, true> : k_passB<ENC, GM, TL, false>;
  prepare_sweep(k, lds, s.lds_attr[1][(ml ? 40 : 0) + ENC * 10 + 2 * GM + (TL ? 1 : 0)]);
  if (GM == 4) {  // one run per range of groups; the first also delivers the ELBO terms
    for (uint32_t g0 = 0; g0 < L.G; g0 += kRangeGroups)
      hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_B<ENC, GM, TL>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                         s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p,
                         RangeB{g0, std::min<uint32_t>(kRangeGroups, L.G - g0), g0 == 0 ? 1 : 0}, guard_view(L, s));
    return;
  }
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_B<ENC, GM, TL>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                     s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p, RangeB{0, 0, 1}, guard_view(L, s));
}

#define MSW_DISPATCH3(fn, ...)                                                       \
  do {                                                                               \
    const int key = L.enc * 4 + (L.glds ? 2 : 0) + (L.tlds ? 1 : 0);              \
    switch (key) {                                                                   \
      case 0: fn<kEncNarrow, false, false>(__VA_ARGS__); break;                      \
      case 1: fn<kEncNarrow, false, true>(__VA_ARGS__); break;                       \
      case 2: fn<kEncNarrow, true, false>(__VA_ARGS__); break;                       \
      case 3: fn<kEncNarrow, true, true>(__VA_ARGS__); break;                        \
      case 4: fn<kEncWide, false, false>(__VA_ARGS__); break;                        \
      case 5: fn<kEncWide, false, true>(__VA_ARGS__); break;                         \
      case 6: fn<kEncWide, true, false>(__VA_ARGS__); break;                         \
      case 7: fn<kEncWide, true, true>(__VA_ARGS__); break;                          \
      case 8: fn<kEncIndex, false, false>(__VA_ARGS__); break;                       \
      case 10: fn<kEncIndex, true, false>(__VA_ARGS__); break;                       \
      case 12: fn<kEncValue, false, false>(__VA_ARGS__); break;                      \
      case 14: fn<kEncValue, true, false>(__VA_ARGS__); break;                       \
      default: throw Fail("internal: no sweep for this layout");                     \
    }                                                                                \
  } while (0)
#define MSW_DISPATCH_B(fn, ...)                                                      \
  do {                                                                               \
    const int key = L.enc * 10 + 2 * L.gmodeB + (L.tlds ? 1 : 0);                 \
    switch (key) {                                                                   \
      case 0: fn<kEncNarrow, 0, false>(__VA_ARGS__); break;                          \
      case 1: fn<kEncNarrow, 0, true>(__VA_ARGS__); break;                           \
      case 2: fn<kEncNarrow, 1, false>(__VA_ARGS__); break;                          \
      case 3: fn<kEncNarrow, 1, true>(__VA_ARGS__); break;                           \
      case 4: fn<kEncNarrow, 2, false>(__VA_ARGS__); break;                          \
      case 5: fn<kEncNarrow, 2, true>(__VA_ARGS__); break;                           \
      case 6: fn<kEncNarrow, 3, false>(__VA_ARGS__); break;                          \
      case 7: fn<kEncNarrow, 3, true>(__VA_ARGS__); break;                           \
      case 8: fn<kEncNarrow, 4, false>(__VA_ARGS__); break;                          \
      case 9: fn<kEncNarrow, 4, true>(__VA_ARGS__); break;                           \
      case 10: fn<kEncWide, 0, false>(__VA_ARGS__); break;                           \
      case 11: fn<kEncWide, 0, true>(__VA_ARGS__); break;                            \
      case 12: fn<kEncWide, 1, false>(__VA_ARGS__); break;                           \
      case 13: fn<kEncWide, 1, true>(__VA_ARGS__); break;                            \
      case 14: fn<kEncWide, 2, false>(__VA_ARGS__); break;                           \
      case 15: fn<kEncWide, 2, true>(__VA_ARGS__); break;                            \
      case 16: fn<kEncWide, 3, false>(__VA_ARGS__); break;                           \
      case 17: fn<kEncWide, 3, true>(__VA_ARGS__); break;                            \
      case 18: fn<kEncWide, 4, false>(__VA_ARGS__); break;                           \
      case 19: fn<kEncWide, 4, true>(__VA_ARGS__); break;                            \
      case 20: fn<kEncIndex, 0, false>(__VA_ARGS__); break;                          \
      case 22: fn<kEncIndex, 1, false>(__VA_ARGS__); break;                          \
      case 24: fn<kEncIndex, 2, false>(__VA_ARGS__); break;                          \
      case 26: fn<kEncIndex, 3, false>(__VA_ARGS__); break;                          \
      case 28: fn<kEncIndex, 4, false>(__VA_ARGS__); break;                          \
      case 30: fn<kEncValue, 0, false>(__VA_ARGS__); break;                          \
      case 32: fn<kEncValue, 1, false>(__VA_ARGS__); break;                          \
      case 34: fn<kEncValue, 2, false>(__VA_ARGS__); break;                          \
      case 36: fn<kEncValue, 3, false>(__VA_ARGS__); break;                          \
      case 38: fn<kEncValue, 4, false>(__VA_ARGS__); break;                          \
      default: throw Fail("internal: no sweep for this layout");                     \
    }                                                                                \
  } while (0)

}  // namespace

// The CSR sweeps are cut by record encoding, pass A and pass B of an encoding together: a unit instantiates
// launch_passA_t / launch_passB_t for the encodings it holds (MINE) and leaves the other cases of the dispatch macros,
// which the outer switch on enc (host_solve.inc launch_passA / launch_passB) never sends here.
#define MSW_SWEEP_UNIT(name, MINE)                                                                     \
  MSW_UNIT_WARM(sweep_##name)                                                                          \
  MSW_UNIT_STAMPS(sweep_##name)                                                                        \
  namespace {                                                                                          \
  template <int ENC, bool GL, bool TL>                                                                 \
  void launch_passA_unit(const Resident &L, Solver &s) {                                               \
    if constexpr (MINE) launch_passA_t<ENC, GL, TL>(L, s);                                             \
    else throw Fail("internal: no sweep for this layout");                                             \
  }                                                                                                    \
  template <int ENC, int GM, bool TL>                                                                  \
  void launch_passB_unit(const Resident &L, Solver &s) {                                               \
    if constexpr (MINE) launch_passB_t<ENC, GM, TL>(L, s);                                             \
    else throw Fail("internal: no sweep for this layout");                                             \
  }                                                                                                    \
  }                                                                                                    \
  void msw::host::passA_##name(const Resident &L, Solver &s) { MSW_DISPATCH3(launch_passA_unit, L, s); } \
  void msw::host::passB_##name(const Resident &L, Solver &s) { MSW_DISPATCH_B(launch_passB_unit, L, s); }
