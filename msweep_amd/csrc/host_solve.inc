// host_solve.inc -- a solver's buffers, the launches of one iteration and the RCG driver (included by solve.hip).  The
// sweeps themselves are launched by the sweep_*.hip units (host_api.hpp).

// a solver's buffers for the likelihood resident in L (they only grow: a bootstrap worker gets ready by this call)
void msw::host::alloc_solve_state(const Resident &L, Solver &s) {
  const uint32_t G = L.G, E = L.E;
  for (DevBuf<double> *b : {&s.alpha0, &s.u, &s.os_u, &s.step_u, &s.w, &s.e, &s.N, &s.Nc,
                            &s.Acc, &s.logth})
    b->alloc((size_t)G + kSentinels);
  s.ew.alloc((size_t)G + kSentinels);
  // entries G.. of e / ew are the sentinel groups of SELL padding records: zero, never rewritten
  s.e.zero(s.stream);
  s.ew.zero(s.stream);
  s.cvec.alloc(E);
  s.c8.alloc((size_t)E + 64);
  s.c8s.alloc((size_t)L.nslices * 64 + 64);  // lanes without an EC stay 0: no EC
  s.c8s.zero(s.stream);
  s.logc_d.alloc(E);
  s.tabA.alloc((size_t)std::max<uint32_t>(L.n_area, 1));
  s.tabB.alloc((size_t)std::max<uint32_t>(L.n_area, 1));
  s.tab_built.alloc(2);
  const int nb = std::max(L.nblk, std::max(L.nblk_dense, L.npart_rows()));
  s.partA.alloc(std::max(nb, 1024));
  s.partS.alloc(4 * (size_t)std::max(nb, 1024));
  s.partR.alloc(kRedfinParts * ((size_t)G / kRedfinGroups + 2));
  s.totS.alloc(4);
  s.commA.alloc(1);
  s.commB.alloc(3 * (size_t)G + 4);  // column sums, two limbs of the guarded ECs' shares, ELBO terms
  s.partAcc.alloc((size_t)std::max(nb, 1) * G);
  s.partC.alloc(1024);
  if (L.flavor == 0) {
    const uint32_t nb0 = (uint32_t)std::max(L.nblk, 1);
    s.guard_list.alloc((size_t)nb0 * L.guard_cap());
    s.guard_bits.alloc((size_t)nb0 * 16 * L.guard_words());
    s.guard_bits.zero(s.stream);
    s.guard_tail.alloc(2 * (size_t)G);
    s.guard_tail.zero(s.stream);
  }
  s.guard_err.alloc(1);
  s.guard_err.zero(s.stream);
  s.guard_visits.alloc(1);
  s.guard_visits.zero(s.stream);
  s.sc.alloc(1);
  s.tr_bound.alloc(kMaxTrace);
  s.tr_newnorm.alloc(kMaxTrace);
  s.tr_beta.alloc(kMaxTrace);
  s.tr_reset.alloc(kMaxTrace);
  if (!s.sc_host) MSW_HIP(hipHostMalloc((void **)&s.sc_host, sizeof(Scalars)));
  if (!s.ev0) {
    MSW_HIP(hipEventCreate(&s.ev0));
    MSW_HIP(hipEventCreate(&s.ev1));
  }
}

namespace {

void launch_passA(const Resident &L, Solver &s) {
  std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
  if (s.profiling) {
    ev = &next_pair(s.evA, s.evA_used);
    MSW_HIP(hipEventRecord(ev->first, s.stream));
  }
  if (L.flavor != 0) dense_passA(L, s);
  else switch (L.enc) {  // the unit that holds this encoding's instantiations; MSW_DISPATCH3 there (sweep_launch.hpp)
      case kEncNarrow: passA_narrow(L, s); break;
      case kEncWide: passA_wide(L, s); break;
      default: passA_index(L, s); break;
    }
  MSW_HIP(hipGetLastError());
  if (ev) MSW_HIP(hipEventRecord(ev->second, s.stream));
  s.timing.passA_launches++;
}

void launch_passB(const Resident &L, Solver &s) {
  std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
  if (s.profiling) {
    ev = &next_pair(s.evB, s.evB_used);
    MSW_HIP(hipEventRecord(ev->first, s.stream));
  }
  if (L.flavor == 0 && s.em_f32) {
    em_passB_f32(L, s);
  } else if (L.flavor == 0) {
    if (L.gmodeB == 0) MSW_HIP(hipMemsetAsync(s.Acc.p, 0, ((size_t)L.G + kSentinels) * sizeof(double), s.stream));
    switch (L.enc) {  // as launch_passA: MSW_DISPATCH_B in the unit of this encoding
      case kEncNarrow: passB_narrow(L, s); break;
      case kEncWide: passB_wide(L, s); break;
      default: passB_index(L, s); break;
    }
  } else {
    dense_passB(L, s);
  }
  MSW_HIP(hipGetLastError());
  if (ev) MSW_HIP(hipEventRecord(ev->second, s.stream));
  s.timing.passB_launches++;
  // column sums across workgroups + N_g / lgamma / digamma, spread over G/16 workgroups
  const bool partials = (L.flavor == 1) || L.gmodeB > 0 || s.em_f32;
  const int nb = L.npart_rows();
  // the CSR sweeps leave fixed-point integer rows (kFx); 2: the fp32 EM sweep's, without the per-group factor
  const int fxrows = L.flavor == 0 ? (s.em_f32 ? 2 : 1) : 0;
  if (s.comm()) {
    // EC-sharded: local column sums + ELBO terms -> one all-reduce -> k_redfin on the totals.  The
    // fixed-point column sums are all-reduced as INTEGERS: exact, so the totals -- and with them every
    // N_g -- are the same bits whatever the number of ranks the ECs are spread over.
    const size_t G3 = 3 * (size_t)L.G;
    std::pair<hipEvent_t, hipEvent_t> *evc = nullptr;
    if (s.profiling) {
      evc = &next_pair(s.evC, s.evC_used);
      MSW_HIP(hipEventRecord(evc->first, s.stream));
    }
    hipLaunchKernelGGL(k_colsum, dim3((L.G + 63) / 64), dim3(1024), 0, s.stream, s.sc.p, (int)L.G,
                       partials ? nb : 0, fxrows, nb, s.partAcc.p, s.Acc.p, s.partS.p,
                       fxrows ? s.guard_tail.p : nullptr, s.commB.p);
    if (kFx && fxrows) {
      s.comm()->allreduce_mixed(reinterpret_cast<uint64_t *>(s.commB.p), G3, s.commB.p + G3, 4, s.stream);
    } else {  // fp64 column sums (dense flavour, MSW_FX=0 builds): doubles, then the integer limbs
      s.comm()->allreduce(s.commB.p, (size_t)L.G, s.stream);
      s.comm()->allreduce_mixed(reinterpret_cast<uint64_t *>(s.commB.p) + L.G, 2 * (size_t)L.G, s.commB.p + G3, 4,
                               s.stream);
    }
    if (evc) MSW_HIP(hipEventRecord(evc->second, s.stream));
    hipLaunchKernelGGL(k_redfin, dim3((L.G + kRedfinGroups - 1) / kRedfinGroups), dim3(kRedfinThreads), 0, s.stream,
                       s.sc.p, (int)L.G, 0, fxrows, reinterpret_cast<unsigned long long *>(s.commB.p) + L.G, 0, 1,
                       s.partAcc.p, s.commB.p, s.commB.p + G3, s.e.p, s.u.p,
                       s.alpha0.p, s.Nc.p, s.N.p, s.w.p, s.ew.p, s.partR.p, s.totS.p);
    return;
  }
  hipLaunchKernelGGL(k_redfin, dim3((L.G + kRedfinGroups - 1) / kRedfinGroups), dim3(kRedfinThreads), 0, s.stream,
                     s.sc.p, (int)L.G, partials ? nb : 0, fxrows, fxrows ? s.guard_tail.p : nullptr, 1, nb,
                     s.partAcc.p, s.Acc.p, s.partS.p, s.e.p,
                     s.u.p, s.alpha0.p, s.Nc.p, s.N.p, s.w.p, s.ew.p, s.partR.p, s.totS.p);
}

// partS as seen by k_fin / k_em_fin: the all-reduced totals when sharded
const double *fin_partS(const Resident &L, Solver &s) { return s.comm() ? s.commB.p + 3 * (size_t)L.G : s.partS.p; }
int fin_npartS(const Resident &L, Solver &s) { return s.comm() ? 1 : L.npart_rows(); }

// slot areas beyond kTabInline entries: the tables are rebuilt by their own kernel after every
// kernel that may have moved a (it returns at once when they are current)
void launch_tables(const Resident &L, Solver &s) {
  if (L.flavor != 0 || L.n_area <= (uint32_t)kTabInline) return;
  const unsigned nb = std::min<unsigned>((L.n_area + 255) / 256, (unsigned)s.n_cu * 8);
  hipLaunchKernelGGL(k_tables, dim3(nb), dim3(256), 0, s.stream, s.sc.p, (int)L.n_area, L.lut_area.p, s.tabs(),
                     s.tab_built.p);
}

// the verdict on the pending evaluation + the next step (state_kernels.hpp k_finstep); mode 1: the verdict alone
void launch_finstep(const Resident &L, Solver &s, int mode) {
  TraceDev tr{s.tr_bound.p, s.tr_newnorm.p, s.tr_beta.p, s.tr_theta.p, s.tr_reset.p};
  const double *pA = s.partA.p;
  int npA = L.flavor == 0 ? L.nblk : L.nblk_dense;
  if (s.comm()) {  // |g|^2 summed over the EC shards (run_rcg)
    pA = s.commA.p;
    npA = 1;
  }
  hipLaunchKernelGGL(k_finstep, dim3(1), dim3(1024), 0, s.stream, s.sc.p, mode, (int)L.G, L.n_tab_inline(), npA, pA,
                     (int)((L.G + kRedfinGroups - 1) / kRedfinGroups), s.totS.p, s.partR.p, s.Nc.p, s.w.p, s.u.p,
                     s.os_u.p, s.step_u.p, L.lut_area.p, s.e.p, s.tabs(), tr);
  launch_tables(L, s);
}

}  // namespace

void msw::host::poll(Solver &s) {
  MSW_HIP(hipMemcpyAsync(s.sc_host, s.sc.p, sizeof(Scalars), hipMemcpyDeviceToHost, s.stream));
  MSW_HIP(hipStreamSynchronize(s.stream));
  if (s.comm()) s.comm()->check();
}

namespace {
// Inputs of one solve: c_j (from log counts or from bootstrap counts already on the device) and
// the prior.  Leaves per-block partial sums of c in partC for k_init_state.
constexpr int kCvecBlocks = 512;
void prepare_inputs(const Resident &L, Solver &s, const double *logc_host, const uint32_t *counts_dev,
                    const double *alpha0_host) {
  if (L.flavor < 0) throw Fail("no likelihood resident: call msw_core_set_csr / set_dense_logl first");
  const uint32_t E = L.E, G = L.G;
  if (counts_dev) {
    hipLaunchKernelGGL(k_cvec_from_counts, dim3(kCvecBlocks), dim3(256), 0, s.stream, counts_dev,
                       L.flavor == 0 ? L.perm.p : nullptr, E, s.cvec.p, s.c8.p, s.partC.p, L.cls, L.n_long,
                       L.flavor == 0 ? s.c8s.p : nullptr);
  } else {
    const double *src = s.logc_d.p;
    if (logc_host) {
      MSW_HIP(hipMemcpyAsync(s.logc_d.p, logc_host, E * sizeof(double), hipMemcpyHostToDevice, s.stream));
    } else {  // the log counts msw_core_build_likelihood left on the device: no 8 * E byte upload
      if (!L.have_logc_res) throw Fail("null logc: only a likelihood built by msw_core_build_likelihood keeps its log counts");
      src = L.logc_res.p;
    }
    hipLaunchKernelGGL(k_cvec_from_logc, dim3(kCvecBlocks), dim3(256), 0, s.stream, src,
                       L.flavor == 0 ? L.perm.p : nullptr, E, s.cvec.p, s.c8.p, s.partC.p, L.cls, L.n_long,
                       L.flavor == 0 ? s.c8s.p : nullptr);
  }
  if (alpha0_host)
    MSW_HIP(hipMemcpyAsync(s.alpha0.p, alpha0_host, G * sizeof(double), hipMemcpyHostToDevice, s.stream));
  MSW_HIP(hipGetLastError());
  // logc_host / alpha0_host may be pageable caller memory: finish the copies before returning
  MSW_HIP(hipStreamSynchronize(s.stream));
  s.prepared = true;
}

// argument / state errors of a solve: thrown BEFORE anything that a peer of a sharded solve could wait for
void validate_solve(size_t max_iters, int algo, int prec) {
  if (algo != MSW_ALGO_RCG && algo != MSW_ALGO_EM) throw Fail("unknown algorithm id");
  if (prec != MSW_PREC_DOUBLE && prec != MSW_PREC_FLOAT) throw Fail("unknown precision id");
  if (max_iters == 0 || max_iters > (size_t)std::numeric_limits<int32_t>::max())
    throw Fail("max_iters out of range");
}

void begin_solve(const Resident &L, Solver &s, double tol, size_t max_iters) {
  const uint32_t G = L.G;
  if (s.trace_theta) s.tr_theta.alloc(s.trace_theta * G);
  const double *cpart = s.partC.p;
  int ncpart = kCvecBlocks;
  if (s.comm()) {  // global sum of the EC counts (bound constant, theta normalisation)
    s.comm()->rendezvous();  // the ranks' calls may be seconds apart on the host: meet before the device-side waits
    hipLaunchKernelGGL(k_sum_scalar, dim3(1), dim3(1024), 0, s.stream, s.sc.p, 0, kCvecBlocks, s.partC.p,
                       s.commA.p);
    s.comm()->allreduce(s.commA.p, 1, s.stream);
    cpart = s.commA.p;
    ncpart = 1;
  }
  hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1024), 0, s.stream, s.sc.p, (int)G, ncpart,
                     cpart, s.alpha0.p, s.u.p, s.os_u.p, s.step_u.p, tol, (int)max_iters,
                     s.fixed_iters ? 1 : 0, (int)s.trace_theta, L.flavor, L.logzi, s.opts, s.tab_built.p,
                     L.trange.p);
  MSW_HIP(hipGetLastError());
}

// iters_start > 0: the solve on the handle is continued (msw_core_continue) -- no initial evaluation
void run_rcg(const Resident &L, Solver &s, size_t max_iters, size_t iters_start = 0) {
  const int G = (int)L.G, n_lut = L.n_tab_inline();
  if (iters_start > 0 && s.comm()) s.comm()->rendezvous();  // msw_core_continue: as begin_solve
  if (iters_start == 0) {
    // initial update_N_k on gamma = log(1/G): the first slot's k_finstep finds it as Scalars::have_eval = 2
    hipLaunchKernelGGL(k_prepB, dim3(1), dim3(1024), 0, s.stream, s.sc.p, G, n_lut, s.u.p, L.lut_area.p,
                       s.e.p, s.tabs());
    launch_tables(L, s);
    launch_passB(L, s);
    s.timing.passB_launches--;  // the initial evaluation is not an iteration
    if (s.profiling && s.evB_used) s.evB_used--;
  }
  const int nbA = L.flavor == 0 ? L.nblk : L.nblk_dense;
  // Slots (state_kernels.hpp k_finstep): k_passA -> k_finstep -> k_passB (+ k_redfin); one per iteration plus one per
  // rejected step.  The verdict on a slot's evaluation is taken by the NEXT slot's k_finstep, so the iteration count
  // the host polls lags the evaluations by one: enqueue as many slots as iterations are still missing, poll, repeat;
  // slots enqueued past the end return at once (Scalars::done), and a verdict-only launch closes the run where the
  // count, not the tolerance, ends it.
  size_t iters_done = iters_start;
  for (;;) {
    // fixed-iteration runs know how many slots are missing; otherwise poll every kIterBatch
    const size_t missing = std::max<size_t>(1, max_iters - std::min(max_iters, iters_done));
    const size_t batch = s.fixed_iters ? std::min<size_t>(256, missing) : std::min<size_t>(kIterBatch, missing);
    for (size_t b = 0; b < batch; ++b) {
      launch_passA(L, s);
      if (s.comm()) {  // |g|^2 summed over the EC shards
        std::pair<hipEvent_t, hipEvent_t> *evc = nullptr;
        if (s.profiling) {
          evc = &next_pair(s.evC, s.evC_used);
          MSW_HIP(hipEventRecord(evc->first, s.stream));
        }
        hipLaunchKernelGGL(k_sum_scalar, dim3(1), dim3(1024), 0, s.stream, s.sc.p, 1, nbA, s.partA.p,
                           s.commA.p);
        s.comm()->allreduce(s.commA.p, 1, s.stream);
        if (evc) MSW_HIP(hipEventRecord(evc->second, s.stream));
      }
      launch_finstep(L, s, 0);
      launch_passB(L, s);
    }
    MSW_HIP(hipGetLastError());
    poll(s);
    if (s.sc_host->done) break;
    if (s.sc_host->have_eval && (size_t)s.sc_host->iter + 1 >= max_iters) {  // the last evaluation's verdict ends the run
      launch_finstep(L, s, 1);
      MSW_HIP(hipGetLastError());
      poll(s);
      if (s.sc_host->done) break;
    }
    iters_done = (size_t)s.sc_host->iter;
  }
}

void finish_solve(const Resident &L, Solver &s, double *theta_out, size_t *iters_out, double *bound_out) {
  poll(s);
  const uint32_t G = L.G;
  int gerr = 0;
  MSW_HIP(hipMemcpy(&gerr, s.guard_err.p, sizeof gerr, hipMemcpyDeviceToHost));
  if (gerr) {
    MSW_HIP(hipMemset(s.guard_err.p, 0, sizeof gerr));
    if (gerr == 2) throw Fail("internal: a workgroup's list of guarded equivalence classes overflowed");
    throw NumericFail("likelihood underflow: an equivalence class has zero probability under every group "
                      "(exp(a * log-likelihood) and the group weights underflow fp64 together)");
  }
  // (an EM run that was asked for no iteration leaves its initial bound, -inf: nothing is wrong)
  if (s.sc_host->iter > 0 && !std::isfinite(s.sc_host->bound))
    throw NumericFail("the evidence lower bound is not finite: the likelihood or the prior counts are out of range");
  if (theta_out) {
    if (s.last_algo == MSW_ALGO_EM) {
      MSW_HIP(hipMemcpy(theta_out, s.logth.p, G * sizeof(double), hipMemcpyDeviceToHost));  // theta of the last M-step
    } else {
      std::vector<double> nc(G);
      MSW_HIP(hipMemcpy(nc.data(), s.Nc.p, G * sizeof(double), hipMemcpyDeviceToHost));
      const double csum = s.sc_host->csum;
      for (uint32_t g = 0; g < G; ++g) theta_out[g] = nc[g] / csum;
    }
  }
  if (iters_out) *iters_out = (size_t)s.sc_host->iter;
  if (bound_out) *bound_out = s.sc_host->bound;
  s.have_solution = true;
}

void collect_timing(const Resident &L, Solver &s) {
  float ms = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms, s.ev0, s.ev1));
  s.timing.solve_ms = ms;
  s.timing.passA_ms = s.timing.passB_ms = 0.0;
  if (s.profiling) {
    // launches enqueued after `done` was set return immediately; they are still counted
    for (size_t i = 0; i < s.evA_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evA[i].first, s.evA[i].second));
      s.timing.passA_ms += ms;
    }
    for (size_t i = 0; i < s.evB_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evB[i].first, s.evB[i].second));
      s.timing.passB_ms += ms;
    }
    s.timing.collective_ms = 0.0;
    for (size_t i = 0; i < s.evC_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evC[i].first, s.evC[i].second));
      s.timing.collective_ms += ms;
    }
    s.timing.collectives = s.evC_used;
  }
  s.timing.iters = (uint64_t)s.sc_host->iter;
  const uint64_t recsz = L.enc == kEncValue ? 12 : (L.wide() ? 8 : 4);
  if (L.flavor == 0) {
    // algorithmic bytes (DESIGN.md 5): every real cell record once + the per-EC count vector in
    // pass B; SELL padding, slice offsets and the L2-served second read of pass B are not counted
    // (slot tables that do not fit LDS are read from memory: every used 16-byte entry at least once per sweep)
    // (a hybrid area: the entries beyond its LDS-resident head)
    const uint64_t tab = L.tlds ? 0ull : 16ull * (L.n_area - L.n_tab_lds);
    s.timing.bytes_passA = L.nnz * recsz + tab;
    s.timing.bytes_passB = L.nnz * recsz + 1ull * L.E + tab;  // + one byte per EC (its multiplicity)
  } else {
    s.timing.bytes_passA = 8ull * L.E * L.G;
    s.timing.bytes_passB = 8ull * L.E * L.G + 8ull * L.E;
  }
}

void run_em(const Resident &L, Solver &s, size_t max_iters, int prec);

// n more iterations of the fixed-iteration RCG solve that last ran on the handle: the state carries on
// where it stood (no re-initialisation, no initial evaluation) -- what a benchmark's "W warm-up steps,
// then exactly K timed steps" means for an iterative solver.
void continue_impl(const Resident &L, Solver &s, size_t n_iters, double *theta_out, size_t *iters_out, double *bound_out) {
  if (!s.have_solution || !s.fixed_iters || s.last_algo != MSW_ALGO_RCG)
    throw Fail("msw_core_continue: needs a fixed-iteration RCG solve on the handle (msw_core_set_fixed_iters, msw_core_run)");
  const size_t start = (size_t)s.sc_host->iter;
  if (n_iters == 0 || start + n_iters > (size_t)std::numeric_limits<int32_t>::max()) throw Fail("msw_core_continue: iteration count out of range");
  s.timing = {};
  s.evA_used = s.evB_used = s.evC_used = 0;
  CollectiveScope cs(s.collective);
  hipLaunchKernelGGL(k_extend, dim3(1), dim3(1), 0, s.stream, s.sc.p, (int)n_iters);
  MSW_HIP(hipEventRecord(s.ev0, s.stream));
  run_rcg(L, s, start + n_iters, start);
  MSW_HIP(hipEventRecord(s.ev1, s.stream));
  finish_solve(L, s, theta_out, iters_out, bound_out);
  collect_timing(L, s);
  s.timing.iters = (uint64_t)s.sc_host->iter - start;
  cs.leave();
}

void run_impl(const Resident &L, Solver &s, double tol, size_t max_iters, int algo, int prec, double *theta_out,
              size_t *iters_out, double *bound_out) {
  validate_solve(max_iters, algo, prec);
  if (!s.prepared) throw Fail("msw_core_run: inputs not prepared (call msw_core_prepare)");
  s.timing = {};
  s.evA_used = s.evB_used = s.evC_used = 0;
  CollectiveScope cs(s.collective);  // from here on a failure strands the peers of a sharded solve (guarded())
  begin_solve(L, s, tol, max_iters);
  MSW_HIP(hipEventRecord(s.ev0, s.stream));
  if (algo == MSW_ALGO_RCG) run_rcg(L, s, max_iters);
  else run_em(L, s, max_iters, prec);
  MSW_HIP(hipEventRecord(s.ev1, s.stream));
  s.last_algo = algo;
  finish_solve(L, s, theta_out, iters_out, bound_out);
  collect_timing(L, s);
  cs.leave();
}

}  // namespace
