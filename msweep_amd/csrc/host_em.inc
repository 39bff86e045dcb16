// host_em.inc -- EM driver (included by solve.hip).  `prec` (--emprecision, src/mSWEEP.cpp:129,202): double runs
// k_passB + k_em_fin per iteration; float (round 5) runs the fp32 sweeps of em_f32_kernels.hpp where the layout allows
// (em_f32_layout_ok: offset records with the table in LDS, index records whose float image fits) and the fp64 kernels
// elsewhere -- msw_timing::em_float_kernels reports which.
namespace {

void run_em(const Resident &L, Solver &s, size_t max_iters, int prec) {
  const int G = (int)L.G, n_lut = L.n_tab_inline();
  TraceDev tr{s.tr_bound.p, s.tr_newnorm.p, s.tr_beta.p, s.tr_theta.p, s.tr_reset.p};
  hipLaunchKernelGGL(k_em_init, dim3(1), dim3(1024), 0, s.stream, s.sc.p, G, n_lut, s.u.p, L.lut_area.p,
                     s.e.p, s.tabs());
  launch_tables(L, s);  // a = 1 throughout: built once, every later call returns at once
  const bool f32 = prec == MSW_PREC_FLOAT && em_f32_layout_ok(L, s);
  struct Flag {  // (launch_passB reads it; cleared on every way out)
    Solver &s;
    ~Flag() { s.em_f32 = false; }
  } flag{s};
  s.em_f32 = f32;
  s.timing.em_float_kernels = f32 ? 1 : 0;
  if (f32) {
    s.e32.alloc((size_t)G + kSentinels);
    s.tab32.alloc(std::max<uint32_t>(L.n_area, 1));  // (every entry of the slot area, in its order: lut_area -- a hybrid area's too)
    em_f32_prep(L, s);  // (k_em_f32_prep: sweep_dense.hip)
  }
  size_t enq = 0;
  while (enq < max_iters) {
    const size_t batch = std::min<size_t>(kIterBatch, max_iters - enq);
    for (size_t b = 0; b < batch; ++b) {
      launch_passB(L, s);
      hipLaunchKernelGGL(k_em_fin, dim3(1), dim3(1024), 0, s.stream, s.sc.p, G, n_lut, fin_npartS(L, s), fin_partS(L, s),
                         s.Nc.p, s.alpha0.p, s.u.p, s.logth.p, L.lut_area.p, s.e.p, s.tabs(), tr,
                         f32 ? s.e32.p : (float *)nullptr);
    }
    MSW_HIP(hipGetLastError());
    enq += batch;
    poll(s);
    if (s.sc_host->done) break;
  }
  // s.logth now holds theta of the last M-step; u = log(theta) stays in s.u for gamma
}

}  // namespace
