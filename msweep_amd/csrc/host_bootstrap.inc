// host_bootstrap.inc -- bootstrap driver (included by solve.hip): replaces
// BootstrapSample::init_bootstrap / resample_counts (src/BootstrapSample.cpp:33-73) and the
// replicate loop of main() (src/mSWEEP.cpp:496-518).
namespace {

// fn(t) for t in [0, n) on n host threads (memory-bound helpers of the table below)
template <class F>
void cp_threads(size_t n, F &&fn) {
  std::vector<std::thread> pool;
  for (size_t t = 1; t < n; ++t) pool.emplace_back([&fn, t] { fn(t); });
  fn((size_t)0);
  for (auto &th : pool) th.join();
}

// libstdc++ discrete_distribution::param_type::_M_initialize: p_i = double(w_i) / sum with a
// sequential sum, partial sums, last entry forced to 1.0.  Sequential fp64 adds define the
// table bit for bit, so it is formed on the host and kept on the device -- ACROSS calls: mSWEEP
// resamples the same EC counts `--iters` times (src/BootstrapSample.cpp:33-44 builds the distribution
// once per sample), so the handle keeps a copy of the counts the resident table was made from and a
// call that brings the same counts again only compares them (threads over 1 M-entry chunks: < 1 ms for
// cfg3's 9.4 M ECs against 34 ms for the table).
void upload_cp(msw_core *h, const uint32_t *ec_counts, size_t E) {
  const size_t nthr = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::thread::hardware_concurrency(), (E + (1u << 20) - 1) >> 20}));
  h->cp_hit = false;
  if (h->cp.p && h->cp.n >= E && h->cp_counts.size() == E && !getenv("MSWEEP_CP_NOCACHE")) {
    std::vector<char> diff(nthr, 0);
    cp_threads(nthr, [&](size_t t) {
      const size_t a = E * t / nthr, b = E * (t + 1) / nthr;
      diff[t] = std::memcmp(h->cp_counts.data() + a, ec_counts + a, (b - a) * sizeof(uint32_t)) != 0;
    });
    if (std::none_of(diff.begin(), diff.end(), [](char c) { return c != 0; })) {
      h->cp_hit = true;
      return;
    }
  }
  h->cp_counts.clear();  // (no stale key should the work below throw)
  std::vector<double> cp(E);
  double sum = 0.0;
  for (size_t i = 0; i < E; ++i) sum += (double)ec_counts[i];
  if (!(sum > 0.0)) throw Fail("bootstrap: the EC counts sum to zero");
  double run = 0.0;
  for (size_t i = 0; i < E; ++i) {
    run += (double)ec_counts[i] / sum;
    cp[i] = run;
  }
  cp[E - 1] = 1.0;
  h->cp.alloc(E);
  MSW_HIP(hipMemcpy(h->cp.p, cp.data(), E * sizeof(double), hipMemcpyHostToDevice));
  std::vector<uint32_t> keep(E);
  cp_threads(nthr, [&](size_t t) {
    const size_t a = E * t / nthr, b = E * (t + 1) / nthr;
    std::memcpy(keep.data() + a, ec_counts + a, (b - a) * sizeof(uint32_t));
  });
  h->cp_counts.swap(keep);
}

constexpr uint64_t kMtJumpMin = 1ull << 27;  // words from which the host jump beats stepping on the device

// Positions the device Mersenne-Twister stream at word `target` (re-seeding when it has to
// move backwards or the seed changed).
void mt_seek(Resampler &r, int32_t seed, uint64_t target, hipStream_t st) {
  r.mt.alloc(1);
  bool reseed = !r.mt_valid || r.mt_seed != seed || r.mt_pos > target;
  if (reseed) {
    // std::mt19937_64(int32 seed): the seed converts to uint64 (sign-extends)
    hipLaunchKernelGGL(k_mt64_seed, dim3(1), dim3(64), 0, st, r.mt.p, (uint64_t)(int64_t)seed);
    r.mt_pos = 0;
    r.mt_seed = seed;
    r.mt_valid = true;
  }
  // far targets (a rank of a multi-GPU bootstrap seeks to its first replicate): GF(2) jump-ahead on
  // the host, ~0.3 s whatever the distance, instead of 2 ns per word on the device
  if (target - r.mt_pos >= kMtJumpMin && !getenv("MSWEEP_MT_NOJUMP")) {
    MtState hs;
    MSW_HIP(hipMemcpyAsync(&hs, r.mt.p, sizeof hs, hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    std::array<uint64_t, mtjump::kN> w;
    std::copy(hs.mt, hs.mt + mtjump::kN, w.begin());
    mtjump::jump(w, target - r.mt_pos);
    std::copy(w.begin(), w.end(), hs.mt);
    hs.produced += target - r.mt_pos;
    MSW_HIP(hipMemcpyAsync(r.mt.p, &hs, sizeof hs, hipMemcpyHostToDevice, st));
    MSW_HIP(hipStreamSynchronize(st));
    r.mt_pos = target;
  }
  if (r.mt_pos < target) {
    hipLaunchKernelGGL(k_mt64, dim3(1), dim3(256), 0, st, r.mt.p, target - r.mt_pos, (uint64_t)0,
                       (uint64_t *)nullptr);
    r.mt_pos = target;
  }
  MSW_HIP(hipGetLastError());
}

// Replicate b of the stream into `counts` (device, uint32[E]), enqueued on stream `st`; cp: the handle's table.
void resample_one(Resampler &r, const double *cp, int n_cu, size_t E, int32_t seed, size_t draws, size_t b,
                  uint32_t *counts, hipStream_t st) {
  MSW_HIP(hipMemsetAsync(counts, 0, E * sizeof(uint32_t), st));
  if (E == 1) {
    // a single weight: libstdc++ returns 0 without consuming a random number
    r.one_count = (uint32_t)draws;
    MSW_HIP(hipMemcpyAsync(counts, &r.one_count, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    return;
  }
  mt_seek(r, seed, (uint64_t)b * draws, st);
  r.mtwords.alloc(draws);
  hipLaunchKernelGGL(k_mt64, dim3(1), dim3(256), 0, st, r.mt.p, (uint64_t)0, (uint64_t)draws, r.mtwords.p);
  r.mt_pos += draws;
  const unsigned nb = (unsigned)std::min<size_t>((draws + 255) / 256, (size_t)n_cu * 16);
  hipLaunchKernelGGL(k_resample, dim3(std::max(nb, 1u)), dim3(256), 0, st, r.mtwords.p, (uint64_t)draws,
                     cp, (uint32_t)E, counts);
  MSW_HIP(hipGetLastError());
}

void check_bootstrap_args(size_t E, size_t draws, size_t rep_begin, size_t rep_end) {
  if (E == 0 || E >= 0xffffffffull) throw Fail("bootstrap: n_ecs out of range");
  if (draws == 0 || draws > 0xffffffffull) throw Fail("bootstrap: bootstrap_count must be in [1, 2^32-1]");
  if (rep_end < rep_begin) throw Fail("bootstrap: rep_end < rep_begin");
}

void resample_impl(msw_core *h, const uint32_t *ec_counts, size_t E, int32_t seed, size_t draws,
                   size_t rep_begin, size_t rep_end, uint32_t *counts_out) {
  if (!ec_counts || !counts_out) throw Fail("msw_core_resample_counts: null argument");
  check_bootstrap_args(E, draws, rep_begin, rep_end);
  upload_cp(h, ec_counts, E);
  Resampler &r = h->resampler;
  r.bcounts.alloc(E);
  for (size_t b = rep_begin; b < rep_end; ++b) {
    resample_one(r, h->cp.p, h->n_cu, E, seed, draws, b, r.bcounts.p, h->stream);
    MSW_HIP(hipMemcpyAsync(counts_out + (b - rep_begin) * E, r.bcounts.p, E * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
  }
}

// Replicates [b0, b1) on worker w, on the likelihood resident in h: resampling of replicate b + 1 (sequential
// Mersenne-Twister stream, one workgroup) runs on a second stream underneath the solve of replicate b; two count
// buffers in ping-pong.
void bootstrap_range(const msw_core &h, Worker &w, int32_t seed, size_t draws, size_t b0, size_t b1, const double *alpha0,
                     double tol, size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out) {
  MSW_HIP(hipSetDevice(h.device));
  const Resident &L = h.lik;
  Solver &s = w.s;
  Resampler &r = w.r;
  const size_t E = L.E, G = L.G;
  MSW_HIP(hipMemcpyAsync(s.alpha0.p, alpha0, G * sizeof(double), hipMemcpyHostToDevice, s.stream));
  if (!r.stream2) MSW_HIP(hipStreamCreateWithFlags(&r.stream2, hipStreamNonBlocking));
  for (auto &ev : r.ev_counts)
    if (!ev) MSW_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  r.bcounts.alloc(E);
  r.bcounts2.alloc(E);
  uint32_t *buf[2] = {r.bcounts.p, r.bcounts2.p};
  if (b0 < b1) {
    MSW_HIP(hipStreamSynchronize(s.stream));
    resample_one(r, h.cp.p, h.n_cu, E, seed, draws, b0, buf[0], r.stream2);
    MSW_HIP(hipEventRecord(r.ev_counts[0], r.stream2));
  }
  for (size_t b = b0; b < b1; ++b) {
    const int cur = (int)((b - b0) & 1);
    MSW_HIP(hipStreamWaitEvent(s.stream, r.ev_counts[cur], 0));
    prepare_inputs(L, s, nullptr, buf[cur], nullptr);  // synchronises: buf[cur] is free afterwards
    if (b + 1 < b1) {
      resample_one(r, h.cp.p, h.n_cu, E, seed, draws, b + 1, buf[cur ^ 1], r.stream2);
      MSW_HIP(hipEventRecord(r.ev_counts[cur ^ 1], r.stream2));
    }
    size_t it = 0;
    try {
      run_impl(L, s, tol, max_iters, algo, prec, theta_out + b * G, &it, nullptr);
    } catch (const NumericFail &) {
      // a replicate whose solve fails NUMERICALLY (likelihood underflow, non-finite bound: the reference returns
      // NaN weights there) is reported as a row of NaN; the other replicates are unaffected.  Everything else --
      // device errors, internal errors, bad arguments (validated before the workers start) -- propagates.
      std::fill(theta_out + b * G, theta_out + (b + 1) * G, std::numeric_limits<double>::quiet_NaN());
      it = (size_t)s.sc_host->iter;
    }
    if (iters_out) iters_out[b] = it;
  }
  MSW_HIP(hipStreamSynchronize(r.stream2));
}

// How many replicates to run at a time.  Up to a few million reads an iteration is a chain of short
// kernels and launch gaps (36 us whatever the size): four replicates side by side give 2.2 x the
// replicates per second at 100 k reads, 1.3 x at 1 M, 1.07 x at 3 M x 5 k groups.  At 10 M reads the sweeps
// fill every CU (one 1024-thread workgroup with 150 KB of LDS each) and a second replicate only gets in their
// way: 43.9 ms per replicate one at a time, 49.3 with two in flight, 50.4 with four
// (tools/bootstrap_streams_timing.py, round 2; the next replicate's resampling runs under the solve either way).
int bootstrap_streams(const Resident &L, size_t n_reps) {
  int n = L.nnz < 30000000ull || L.flavor != 0 ? 4 : 1;
  if (const char *e = getenv("MSWEEP_BOOTSTRAP_STREAMS")) n = std::max(1, std::min(16, atoi(e)));
  return (int)std::min<size_t>((size_t)n, std::max<size_t>(n_reps, 1));
}

void bootstrap_impl(msw_core *h, const uint32_t *ec_counts, int32_t seed, size_t draws, size_t rep_begin,
                    size_t rep_end, const double *alpha0, double tol, size_t max_iters, int algo,
                    int prec, double *theta_out, size_t *iters_out) {
  const Resident &L = h->lik;
  if (L.flavor < 0) throw Fail("msw_core_bootstrap: no likelihood resident");
  if (h->comm)
    throw Fail("msw_core_bootstrap: replicates shard over GPUs as whole solves (rep_begin / rep_end, or "
               "msw_core_bootstrap_dist); detach the EC-sharding communicator first");
  if (!ec_counts || !alpha0 || !theta_out) throw Fail("msw_core_bootstrap: null argument");
  const size_t E = L.E, G = L.G;
  check_bootstrap_args(E, draws, rep_begin, rep_end);
  validate_solve(max_iters, algo, prec);  // bad arguments fail the whole call (never a table of NaN)
  const auto t_begin = std::chrono::steady_clock::now();
  upload_cp(h, ec_counts, E);
  const auto t_table = std::chrono::steady_clock::now();
  const size_t n_reps = rep_end - rep_begin;
  const int n_ctx = bootstrap_streams(L, n_reps);
  // contiguous blocks of replicates per worker, like ranks of a multi-GPU run (each seeks -- or jumps -- to its
  // first replicate of the one sequential stream once)
  // Every replicate runs on a worker's solver: the handle's own solver keeps the solution of the un-resampled
  // estimate, so msw_core_gamma / msw_core_trace after the bootstrap still describe it (the reference writes those
  // probabilities, src/mSWEEP.cpp:437-493).  Of the handle's settings a worker takes the solver options only: the
  // replicates solve to tol, unprofiled and untraced, whatever fixed_iters, profiling and trace_theta say.
  while ((int)h->workers.size() < n_ctx) h->workers.emplace_back(new Worker(h->n_cu));
  for (int i = 0; i < n_ctx; ++i) {
    Worker &w = *h->workers[i];
    w.s.opts = h->solver.opts;
    w.s.fixed_iters = w.s.profiling = false;
    w.s.trace_theta = 0;
    w.r.mt_valid = false;
    alloc_solve_state(L, w.s);
  }
  MSW_HIP(hipStreamSynchronize(h->stream));
  double *theta0 = theta_out - rep_begin * G;  // rows are indexed by replicate below
  size_t *iters0 = iters_out ? iters_out - rep_begin : nullptr;
  std::vector<std::string> errs(n_ctx);
  std::vector<std::thread> workers;
  const msw_core &shared = *h;  // what the workers share (the resident likelihood, the table): read-only
  auto work = [&](int i) {
    const size_t b0 = rep_begin + n_reps * i / n_ctx, b1 = rep_begin + n_reps * (i + 1) / n_ctx;
    try {
      bootstrap_range(shared, *h->workers[i], seed, draws, b0, b1, alpha0, tol, max_iters, algo, prec, theta0, iters0);
    } catch (const std::exception &ex) {
      errs[i] = ex.what();
      (void)hipGetLastError();
    }
  };
  for (int i = 1; i < n_ctx; ++i) workers.emplace_back(work, i);
  work(0);
  for (auto &w : workers) w.join();
  for (auto &e : errs)
    if (!e.empty()) throw Fail(e);
  const auto t_end = std::chrono::steady_clock::now();
  h->btiming = {};
  h->btiming.table_ms = std::chrono::duration<double, std::milli>(t_table - t_begin).count();
  h->btiming.solve_ms = std::chrono::duration<double, std::milli>(t_end - t_table).count();
  h->btiming.replicates = n_reps;
  h->btiming.table_reused = h->cp_hit ? 1 : 0;
  if (iters_out)
    for (size_t b = 0; b < n_reps; ++b) h->btiming.iterations += iters_out[b];
}

// All n_reps replicates over the ranks of `comm`: rank r solves the contiguous block
// [n_reps * r / P, n_reps * (r + 1) / P) of the one sequential stream, then one all-gather leaves the
// whole n_reps x G block, in replicate order, on every rank (bootstrap_results, include/Sample.hpp:157,180).
void bootstrap_dist_impl(msw_core *h, msw_comm *comm, const uint32_t *ec_counts, int32_t seed, size_t draws,
                         size_t n_reps, const double *alpha0, double tol, size_t max_iters, int algo, int prec,
                         double *theta_out, size_t *iters_out) {
  if (!comm) throw Fail("msw_core_bootstrap_dist: null communicator");
  if (!theta_out) throw Fail("msw_core_bootstrap_dist: null output");
  const size_t P = (size_t)comm->size(), r = (size_t)comm->rank(), G = h->lik.G;
  const size_t b0 = n_reps * r / P, b1 = n_reps * (r + 1) / P;
  // a rank's message: its rows {theta, iteration count}, then ONE status word -- a rank whose block fails still
  // takes part in the all-gather (its peers would wait in it for ever otherwise) and every rank learns of it
  const size_t maxb = (n_reps + P - 1) / P, row = G + 1, msg = maxb * row + 1;
  std::vector<double> mine(msg, 0.0), all(P * msg);
  std::string my_err;
  h->btiming = {};
  if (b0 < b1) {  // more ranks than replicates leave some ranks an empty block: nothing to solve, still gathered
    std::vector<double> th((b1 - b0) * G);
    std::vector<size_t> it(b1 - b0);
    try {
      bootstrap_impl(h, ec_counts, seed, draws, b0, b1, alpha0, tol, max_iters, algo, prec, th.data(), it.data());
      for (size_t b = 0; b < b1 - b0; ++b) {
        std::copy(th.begin() + b * G, th.begin() + (b + 1) * G, mine.begin() + b * row);
        mine[b * row + G] = (double)it[b];
      }
    } catch (const std::exception &ex) {
      my_err = ex.what();
      (void)hipGetLastError();
      mine[msg - 1] = 1.0;
    }
  } else if (h->lik.flavor < 0 || !ec_counts || !alpha0) {
    my_err = "msw_core_bootstrap_dist: no likelihood resident or null argument";
    mine[msg - 1] = 1.0;
  }
  const auto t_gather = std::chrono::steady_clock::now();
  try {
    comm->allgather_host(mine.data(), msg, all.data());
    h->btiming.gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_gather).count();
  } catch (...) {
    comm->abort();  // the exchange itself failed on this rank: its peers must not wait in it
    throw;
  }
  if (!my_err.empty()) throw Fail(my_err);
  for (size_t q = 0; q < P; ++q)
    if (all[q * msg + msg - 1] != 0.0)
      throw Fail("msw_core_bootstrap_dist: rank " + std::to_string(q) + " failed on its block of replicates");
  for (size_t q = 0; q < P; ++q) {
    const size_t q0 = n_reps * q / P, q1 = n_reps * (q + 1) / P;
    for (size_t b = q0; b < q1; ++b) {
      const double *src = all.data() + q * msg + (b - q0) * row;
      std::copy(src, src + G, theta_out + b * G);
      if (iters_out) iters_out[b] = (size_t)src[G];
    }
  }
}

}  // namespace
