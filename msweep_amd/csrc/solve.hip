// solve.hip -- translation unit of the solve: the state kernels, the RCG and EM drivers, the bootstrap and the communicators,
// with the C ABI entries of those families.  The sweeps are launched through host_api.hpp.
#include "host_api.hpp"

#include "state_kernels.hpp"
#include "em_kernels.hpp"
#include "bootstrap_kernels.hpp"
#include "stream_kernels.hpp"
#include "shm_comm.hpp"
#include "peer_comm.hpp"

// (this unit's first launch is k_warm of stream_kernels.hpp itself)
void msw::host::warm_solve(hipStream_t st) { hipLaunchKernelGGL(k_warm, dim3(1), dim3(1), 0, st, (int *)nullptr); }
MSW_UNIT_STAMPS(solve)
void msw::host::minmax_launch(unsigned nb, hipStream_t st, const double *v, uint64_t n, int pairs, double *out) {
  hipLaunchKernelGGL(k_minmax, dim3(nb), dim3(1024), 0, st, v, n, pairs, out);
}

#include "host_solve.inc"
#include "host_em.inc"
#include "host_mtjump.inc"
#include "host_bootstrap.inc"

extern "C" {

int msw_core_shape(msw_handle h, size_t *n_groups, size_t *n_ecs, size_t *nnz) {
  return guarded(h, [&] {
    if (h->lik.flavor < 0) throw Fail("no likelihood resident");
    if (n_groups) *n_groups = h->lik.G;
    if (n_ecs) *n_ecs = h->lik.E;
    if (nnz) *nnz = h->lik.flavor == 0 ? h->lik.nnz : (size_t)h->lik.G * h->lik.E;
  });
}

int msw_core_solve(msw_handle h, const double *logc, const double *alpha0, double tol, size_t max_iters,
                   int algo, int prec, double *theta_out, size_t *iters_out, double *bound_out) {
  return guarded(h, [&] {
    if (!alpha0) throw Fail("msw_core_solve: null alpha0");
    h->drop_kept();  // (the kept assignment table belongs to the solve before: host_assign.inc)
    prepare_inputs(h->lik, h->solver, logc, nullptr, alpha0);
    run_impl(h->lik, h->solver, tol, max_iters, algo, prec, theta_out, iters_out, bound_out);
  });
}

int msw_core_prepare(msw_handle h, const double *logc, const double *alpha0) {
  return guarded(h, [&] {
    if (!alpha0) throw Fail("msw_core_prepare: null alpha0");
    h->drop_kept();
    prepare_inputs(h->lik, h->solver, logc, nullptr, alpha0);
  });
}

int msw_core_run(msw_handle h, double tol, size_t max_iters, int algo, int prec, double *theta_out,
                 size_t *iters_out, double *bound_out) {
  return guarded(h, [&] {
    h->drop_kept();
    run_impl(h->lik, h->solver, tol, max_iters, algo, prec, theta_out, iters_out, bound_out);
  });
}

int msw_core_continue(msw_handle h, size_t n_iters, double *theta_out, size_t *iters_out, double *bound_out) {
  return guarded(h, [&] {
    h->drop_kept();
    continue_impl(h->lik, h->solver, n_iters, theta_out, iters_out, bound_out);
  });
}

int msw_core_set_trace_theta(msw_handle h, size_t n_iters) {
  return guarded(h, [&] {
    if (n_iters > (size_t)kMaxTrace) throw Fail("trace_theta: at most 4096 iterations");
    h->solver.trace_theta = n_iters;
  });
}

int msw_core_trace(msw_handle h, size_t n, double *bound, double *newnorm, double *beta,
                   int32_t *didreset, double *theta_trace, size_t *n_out) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_trace: no solve has run on this handle");
    size_t have = std::min<size_t>((size_t)h->solver.sc_host->iter, kMaxTrace);
    n = std::min(n, have);
    if (bound) MSW_HIP(hipMemcpy(bound, h->solver.tr_bound.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (newnorm) MSW_HIP(hipMemcpy(newnorm, h->solver.tr_newnorm.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta) MSW_HIP(hipMemcpy(beta, h->solver.tr_beta.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (didreset) MSW_HIP(hipMemcpy(didreset, h->solver.tr_reset.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (theta_trace) {
      const size_t nt = std::min(n, h->solver.trace_theta);
      if (nt) MSW_HIP(hipMemcpy(theta_trace, h->solver.tr_theta.p, nt * h->lik.G * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = n;
  });
}

int msw_core_bootstrap(msw_handle h, const uint32_t *ec_counts, int32_t seed, size_t bootstrap_count,
                       size_t rep_begin, size_t rep_end, const double *alpha0, double tol,
                       size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out) {
  return guarded(h, [&] {
    h->drop_kept();
    bootstrap_impl(h, ec_counts, seed, bootstrap_count, rep_begin, rep_end, alpha0, tol, max_iters,
                   algo, prec, theta_out, iters_out);
  });
}

int msw_core_resample_counts(msw_handle h, const uint32_t *ec_counts, size_t n_ecs, int32_t seed,
                             size_t bootstrap_count, size_t rep_begin, size_t rep_end,
                             uint32_t *counts_out) {
  return guarded(h, [&] {
    resample_impl(h, ec_counts, n_ecs, seed, bootstrap_count, rep_begin, rep_end, counts_out);
  });
}

int msw_core_bootstrap_dist(msw_handle h, msw_comm_t comm, const uint32_t *ec_counts, int32_t seed,
                            size_t bootstrap_count, size_t n_replicates, const double *alpha0, double tol,
                            size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out) {
  // (a rank whose block fails still joins the all-gather and reports through its status word: every rank
  // returns non-zero, none is left waiting, and the communicator stays usable -- host_bootstrap.inc)
  return guarded(h, [&] {
    h->drop_kept();
    bootstrap_dist_impl(h, comm, ec_counts, seed, bootstrap_count, n_replicates, alpha0, tol, max_iters, algo,
                        prec, theta_out, iters_out);
  });
}

const char *msw_comm_last_error(void) { return g_create_error.c_str(); }

int msw_comm_size(msw_comm_t c, int *nranks, int *rank) {
  if (!c) {
    g_create_error = "msw_comm_size: null communicator";
    return 1;
  }
  if (nranks) *nranks = c->size();
  if (rank) *rank = c->rank();
  return 0;
}

int msw_comm_rccl_count(msw_comm_t c, int *count) {
  if (!c || !count) {
    g_create_error = "msw_comm_rccl_count: null argument";
    return 1;
  }
  if (const PeerComm *pc = dynamic_cast<const PeerComm *>(c)) c = pc->base.get();
  const RcclComm *rc = dynamic_cast<const RcclComm *>(c);
  *count = rc ? rc->count() : 0;
  return 0;
}

int msw_comm_allgather(msw_comm_t c, const double *send, size_t n, double *recv) {
  if (!c || (n && (!send || !recv))) {
    g_create_error = "msw_comm_allgather: null argument";
    return 1;
  }
  try {
    c->allgather_host(send, n, recv);
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    c->abort();
    return 1;
  }
}

int msw_comm_allreduce(msw_comm_t c, uint64_t *ints, size_t ni, double *reals, size_t nr, int repeats, double *ms_per_call) {
  if (!c || (ni && !ints) || (nr && !reals) || repeats < 1) {
    g_create_error = "msw_comm_allreduce: bad arguments";
    return 1;
  }
  hipStream_t st = nullptr;
  try {
    MSW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf<double> buf, work;
    buf.alloc(ni + nr + 1);
    work.alloc(ni + nr + 1);
    if (ni) MSW_HIP(hipMemcpyAsync(buf.p, ints, ni * 8, hipMemcpyHostToDevice, st));
    if (nr) MSW_HIP(hipMemcpyAsync(buf.p + ni, reals, nr * 8, hipMemcpyHostToDevice, st));
    // repeats > 1: the same message again and again (timing; the sums of the last one are returned)
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < repeats; ++k) {
      MSW_HIP(hipMemcpyAsync(work.p, buf.p, (ni + nr) * 8, hipMemcpyDeviceToDevice, st));
      c->allreduce_mixed(reinterpret_cast<uint64_t *>(work.p), ni, work.p + ni, nr, st);
    }
    MSW_HIP(hipStreamSynchronize(st));
    c->check();
    if (ms_per_call)
      *ms_per_call = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
    if (ni) MSW_HIP(hipMemcpyAsync(ints, work.p, ni * 8, hipMemcpyDeviceToHost, st));
    if (nr) MSW_HIP(hipMemcpyAsync(reals, work.p + ni, nr * 8, hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st);
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    if (st) (void)hipStreamDestroy(st);
    c->abort();
    return 1;
  }
}

int msw_comm_unique_id(unsigned char id_out[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  const ncclResult_t rc = ncclGetUniqueId(&id);
  if (rc != ncclSuccess) {
    g_create_error = std::string("ncclGetUniqueId: ") + ncclGetErrorString(rc);
    return 1;
  }
  std::memcpy(id_out, &id, 128);
  return 0;
}

int msw_comm_create_rccl(const unsigned char id[128], int rank, int nranks, int device, msw_comm_t *out) {
  if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) {
    g_create_error = "msw_comm_create_rccl: bad arguments";
    return 1;
  }
  try {
    MSW_HIP(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    std::unique_ptr<msw_comm> c(new RcclComm(uid, rank, nranks));
    if (peer_allreduce_requested() && nranks > 1) c.reset(new PeerComm(std::move(c), /*ipc=*/true));
    *out = c.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    return 1;
  }
}

int msw_comm_create_local(int nranks, msw_comm_t *out) {
  if (!out || nranks < 1) {
    g_create_error = "msw_comm_create_local: bad arguments";
    return 1;
  }
  try {
    const bool peer = peer_allreduce_requested() && nranks > 1;
    auto grp = std::make_shared<LocalGroup>(nranks);
    for (int r = 0; r < nranks; ++r) out[r] = nullptr;
    for (int r = 0; r < nranks; ++r) {
      std::unique_ptr<msw_comm> c(new LocalComm(grp, r));
      if (peer) c.reset(new PeerComm(std::move(c), /*ipc=*/false));
      out[r] = c.release();
    }
    return 0;
  } catch (const std::exception &ex) {
    for (int r = 0; r < nranks; ++r) delete out[r];
    g_create_error = ex.what();
    return 1;
  }
}

int msw_comm_create_shm(const char *name, int rank, int nranks, int device, msw_comm_t *out) {
  if (!out || !name || nranks < 1 || rank < 0 || rank >= nranks) {
    g_create_error = "msw_comm_create_shm: bad arguments";
    return 1;
  }
  try {
    MSW_HIP(hipSetDevice(device));
    std::unique_ptr<msw_comm> c(new ShmComm(name, rank, nranks));
    if (peer_allreduce_requested() && nranks > 1) c.reset(new PeerComm(std::move(c), /*ipc=*/true));
    *out = c.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    return 1;
  }
}

void msw_comm_destroy(msw_comm_t c) { delete c; }

int msw_core_set_comm(msw_handle h, msw_comm_t comm) {
  return guarded(h, [&] { h->comm = comm; });
}

int msw_core_set_profiling(msw_handle h, int enabled) {
  return guarded(h, [&] { h->solver.profiling = enabled != 0; });
}

int msw_core_set_fixed_iters(msw_handle h, int enabled) {
  return guarded(h, [&] { h->solver.fixed_iters = enabled != 0; });
}

int msw_core_set_option(msw_handle h, int option, double value) {
  return guarded(h, [&] {
    switch (option) {
      case MSW_OPT_CHECK_EVERY:
        if (!(value >= 1.0 && value <= 65536.0) || value != std::floor(value)) throw Fail("MSW_OPT_CHECK_EVERY: an integer in [1, 65536]");
        h->solver.opts.check_every = (int32_t)value;
        break;
      case MSW_OPT_INIT_BOUND:
        if (std::isnan(value) || value == INFINITY) throw Fail("MSW_OPT_INIT_BOUND: a number below +inf");
        h->solver.opts.init_bound = value;
        break;
      case MSW_OPT_EM_PRIOR:
        if (value != 0.0 && value != 1.0) throw Fail("MSW_OPT_EM_PRIOR: 0 (MAP) or 1 (ML)");
        h->solver.opts.em_prior = (int32_t)value;
        break;
      case MSW_OPT_EM_STOP:
        if (value != 0.0 && value != 1.0) throw Fail("MSW_OPT_EM_STOP: 0 (log-likelihood gain) or 1 (largest move of a weight)");
        h->solver.opts.em_stop = (int32_t)value;
        break;
      default: throw Fail("msw_core_set_option: unknown option id");
    }
  });
}

int msw_core_get_option(msw_handle h, int option, double *value) {
  return guarded(h, [&] {
    if (!value) throw Fail("null out");
    switch (option) {
      case MSW_OPT_CHECK_EVERY: *value = h->solver.opts.check_every; break;
      case MSW_OPT_INIT_BOUND: *value = h->solver.opts.init_bound; break;
      case MSW_OPT_EM_PRIOR: *value = h->solver.opts.em_prior; break;
      case MSW_OPT_EM_STOP: *value = h->solver.opts.em_stop; break;
      default: throw Fail("msw_core_get_option: unknown option id");
    }
  });
}

int msw_core_last_timing(msw_handle h, msw_timing *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    *out = h->solver.timing;
  });
}

#ifdef MSW_STAMPS
// diagnostic build only (tools/chain_timeline.py): the phase stamps of the last <= 64 iterations; clear = 1 zeroes them
int msw_debug_stamps(msw_handle h, uint64_t *out, int clear) {
  return guarded(h, [&] {
    MSW_HIP(hipStreamSynchronize(h->stream));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "stamps are 64-bit words");
    unsigned long long *newest = reinterpret_cast<unsigned long long *>(out);
    if (newest) std::fill(newest, newest + 64 * 40, 0ull);
    for (auto stamps : {stamps_solve, stamps_sweep_narrow, stamps_sweep_wide, stamps_sweep_index}) stamps(newest, clear);
  });
}
#endif

int msw_core_guarded_visits(msw_handle h, uint64_t *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    if (h->lik.flavor != 0) throw Fail("msw_core_guarded_visits: no CSR-of-ECs likelihood resident");
    unsigned long long v = 0;
    MSW_HIP(hipStreamSynchronize(h->stream));
    MSW_HIP(hipMemcpy(&v, h->solver.guard_visits.p, sizeof v, hipMemcpyDeviceToHost));
    *out = v;
  });
}

int msw_core_last_bootstrap_timing(msw_handle h, msw_bootstrap_timing *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    *out = h->btiming;
  });
}

int msw_core_hbm_stream_rates(msw_handle h, size_t n_bytes, int reps, double *read_gbs, double *triad_gbs) {
  return guarded(h, [&] {
    if (!read_gbs || !triad_gbs) throw Fail("null out");
    if (n_bytes < (1u << 20) || reps < 1) throw Fail("msw_core_hbm_stream_rates: at least 1 MiB and one repetition");
    const size_t n = n_bytes / sizeof(double2);
    DevBuf<double2> a, b, c;
    DevBuf<double> sink;
    a.alloc(n);
    b.alloc(n);
    c.alloc(n);
    sink.alloc(1);
    MSW_HIP(hipMemsetAsync(a.p, 0, n * sizeof(double2), h->stream));
    MSW_HIP(hipMemsetAsync(b.p, 0, n * sizeof(double2), h->stream));
    MSW_HIP(hipMemsetAsync(c.p, 0, n * sizeof(double2), h->stream));
    hipEvent_t e0, e1;
    MSW_HIP(hipEventCreate(&e0));
    MSW_HIP(hipEventCreate(&e1));
    // the rate depends on the launch shape by +-10 %: the best of a few shapes is the ceiling
    const int shapes[7][2] = {{256, 512}, {256, 1024}, {512, 256}, {512, 1024}, {1024, 512}, {2048, 1024}, {8192, 1024}};
    double best_r = 0.0, best_t = 0.0;
    for (int r = 0; r < reps + 2; ++r) {  // the first two rounds warm the clocks and the TLB
      for (const auto &sh : shapes) {
        float ms = 0.f;
        MSW_HIP(hipEventRecord(e0, h->stream));
        k_stream_read<<<sh[0], sh[1], 0, h->stream>>>(a.p, n, sink.p);
        MSW_HIP(hipEventRecord(e1, h->stream));
        MSW_HIP(hipEventSynchronize(e1));
        MSW_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) best_r = std::max(best_r, (double)(n * sizeof(double2)) / (ms * 1e-3) / 1e9);
        MSW_HIP(hipEventRecord(e0, h->stream));
        k_stream_triad<<<sh[0], sh[1], 0, h->stream>>>(a.p, b.p, c.p, n);
        MSW_HIP(hipEventRecord(e1, h->stream));
        MSW_HIP(hipEventSynchronize(e1));
        MSW_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) best_t = std::max(best_t, (double)(3 * n * sizeof(double2)) / (ms * 1e-3) / 1e9);
      }
    }
    MSW_HIP(hipGetLastError());
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *read_gbs = best_r;
    *triad_gbs = best_t;
  });
}

}  // extern "C"
