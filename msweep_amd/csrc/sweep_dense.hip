// sweep_dense.hip -- translation unit of the dense sweeps (dense_kernels.hpp) and of --emprecision float's kernels
// (em_f32_kernels.hpp), with their launches; k_transpose lives in dense_kernels.hpp and is launched from here too.
#include "sweep_launch.hpp"
#include "dense_kernels.hpp"
#include "em_f32_kernels.hpp"

MSW_UNIT_WARM(sweep_dense)

namespace {

template <int NREG>
void launch_dense_A(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_passA<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.u.p, s.w.p, s.partA.p);
}
template <int NREG>
void launch_dense_B(const Resident &L, Solver &s) {
  const size_t lds = (32 + 4 * (size_t)L.G) * sizeof(double);
  hipLaunchKernelGGL(k_dense_passB<NREG>, dim3(L.nblk_dense), dim3(256), lds, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.cvec.p, s.u.p, s.partAcc.p, s.partS.p);
}
template <int NREG>
void launch_dense_big_A(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_big_passA<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.u.p, s.w.p, s.partA.p);
}
template <int NREG>
void launch_dense_big_B(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_big_passB<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.cvec.p, s.u.p, s.partAcc.p, s.partS.p);
}
#define MSW_DISPATCH_NREG(fn, fnbig, ...)                \
  do {                                                   \
    switch (L.nreg) {                                   \
      case 1: fn<1>(__VA_ARGS__); break;                 \
      case 2: fn<2>(__VA_ARGS__); break;                 \
      case 4: fn<4>(__VA_ARGS__); break;                 \
      case 8: fn<8>(__VA_ARGS__); break;                 \
      case 16: fn<16>(__VA_ARGS__); break;               \
      case 32: fnbig<32>(__VA_ARGS__); break;            \
      case 64: fnbig<64>(__VA_ARGS__); break;            \
      default: fnbig<128>(__VA_ARGS__); break;           \
    }                                                    \
  } while (0)

}  // namespace

// --emprecision float: the fp32 sweeps of em_f32_kernels.hpp (run_em decides; one persistent workgroup per CU).
// Served: one GPU, the CSR flavour, the group vectors in LDS, at most kStepRegs * 1024 groups, and either offset records
// with the whole slot table in LDS or index records (the hybrid area, whatever part of it the fp64 images hold) whose
// FLOAT image -- 4 bytes per entry of the whole area, 12 per group -- fits LDS.
bool msw::host::em_f32_layout_ok(const Resident &L, const Solver &s) {
  if (!kFx || L.flavor != 0 || !L.glds || s.comm() || L.G > (uint32_t)(kStepRegs * 1024)) return false;
  if (getenv("MSWEEP_EM_FLOAT_AS_DOUBLE")) return false;  // (developer switch: the fp64 kernels under MSW_PREC_FLOAT, as until round 4)
  if (L.enc == kEncNarrow)
    return L.tlds && L.n_tab_lds == L.n_area && em_f32_lds_bytes(L.n_tab_lds, L.G) <= kLdsMax;
  // (shift <= 30: the two shifts that leave 4 * entry of a record, em_f32_kernels.hpp F32Form)
  if (L.hybrid()) return L.dec.shift <= 30 && em_f32_idx_lds_bytes(L.n_area, L.G) <= kLdsMax;
  return false;
}
void msw::host::em_passB_f32(const Resident &L, Solver &s) {
  const bool idx = L.hybrid();
  const size_t lds = idx ? em_f32_idx_lds_bytes(L.n_area, L.G) : em_f32_lds_bytes(L.n_tab_lds, L.G);
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  auto k = idx ? (ml ? k_em_passB_f32_idx<true> : k_em_passB_f32_idx<false>)
               : (ml ? k_em_passB_f32<true> : k_em_passB_f32<false>);
  prepare_sweep(k, lds, s.lds_attr[2][30 + (idx ? 2 : 0) + (ml ? 1 : 0)]);
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(1024), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p, s.e32.p, s.tab32.p,
                     s.partAcc.p, s.partS.p, guard_view(L, s));
}

void msw::host::dense_passA(const Resident &L, Solver &s) { MSW_DISPATCH_NREG(launch_dense_A, launch_dense_big_A, L, s); }
void msw::host::dense_passB(const Resident &L, Solver &s) { MSW_DISPATCH_NREG(launch_dense_B, launch_dense_big_B, L, s); }
void msw::host::em_f32_prep(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_em_f32_prep, dim3(1), dim3(1024), 0, s.stream, s.sc.p, (int)L.G, (int)L.n_area, L.lut_area.p, s.e.p,
                     s.e32.p, s.tab32.p);
}
void msw::host::transpose_launch(dim3 grid, hipStream_t st, const double *src, size_t ld, int G, uint32_t E, double *dst) {
  hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, st, src, ld, G, E, dst);
}
