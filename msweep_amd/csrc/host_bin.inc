// host_bin.inc -- msw_core_bin_reads / _aln (included by build.hip): the mGEMS binning step of
// src/mSWEEP.cpp:437-469 on the device (bin_kernels.hpp).  Device memory: O(E) (lse, counts, offsets) plus
// O(pairs) (one (target slot, EC) pair per passing EC and target) plus the output; nothing is sized G x E or
// n_targets x E, and the output is sized from the count pass before it is allocated.  No atomics: every order is
// fixed by scans and one stable sort, the same bins run to run.
namespace {

// hipMalloc that names what failed and how many bytes it wanted (an out-of-memory result is an error, never a fault)
template <class T>
void bin_alloc(DevBuf<T> &b, size_t count, const char *what) {
  named_alloc(b, count, "msw_core_bin_reads", what);
}

template <int ENC, bool LDS>
void launch_bin_passes(msw_core *h, const GammaState &gs, const BinTargets &B, double *lse_p, uint32_t *cnt,
                       const uint64_t *off, uint32_t *key, uint32_t *val, bool write) {
  const Resident &L = h->lik;
  const size_t lds = LDS ? (size_t)L.G * sizeof(uint32_t) : 0;
  const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)L.E + 255) / 256, (size_t)h->n_cu * 8));
  if (!write)
    hipLaunchKernelGGL((k_bin_count<ENC, LDS>), dim3(nb), dim3(256), lds, h->stream, sell_view(L, h->solver), gs.a, L.logzi,
                       gs.tref, gs.u, B, lse_p, cnt);
  else
    hipLaunchKernelGGL((k_bin_write<ENC, LDS>), dim3(nb), dim3(256), lds, h->stream, sell_view(L, h->solver), gs.a, L.logzi, gs.u,
                       B, lse_p, off, key, val);
  MSW_HIP(hipGetLastError());
}
template <bool LDS>
void launch_bin_enc(msw_core *h, const GammaState &gs, const BinTargets &B, double *lse_p, uint32_t *cnt,
                    const uint64_t *off, uint32_t *key, uint32_t *val, bool write) {
  const Resident &L = h->lik;
  if (L.enc == kEncValue) launch_bin_passes<kEncValue, LDS>(h, gs, B, lse_p, cnt, off, key, val, write);
  else if (L.wide()) launch_bin_passes<kEncWide, LDS>(h, gs, B, lse_p, cnt, off, key, val, write);
  else if (L.hybrid()) launch_bin_passes<kEncIndex, LDS>(h, gs, B, lse_p, cnt, off, key, val, write);
  else launch_bin_passes<kEncNarrow, LDS>(h, gs, B, lse_p, cnt, off, key, val, write);
}

// the slot map goes to LDS when it fits; MSWEEP_BIN_LDS=0 keeps it in global memory (tests cover both paths)
bool bin_slots_in_lds(uint32_t G) {
  const char *e = getenv("MSWEEP_BIN_LDS");
  return G <= kBinLdsGroups && !(e && e[0] == '0');
}

void bin_reads_impl(msw_core *h, const uint64_t *rptr, const uint32_t *reads, size_t n_ecs, bool on_device,
                    const uint32_t *targets, const double *thresholds, size_t n_targets, uint64_t *bin_ptr,
                    uint32_t *reads_out, double *log_thr_out) {
  const Resident &L = h->lik;
  if (!h->solver.have_solution) throw Fail("msw_core_bin_reads: no solve has run on this handle");
  if (h->comm) throw Fail("msw_core_bin_reads: not available on an EC-sharded handle (a communicator is set)");
  if (L.flavor != 0)
    throw Fail("msw_core_bin_reads: the resident likelihood has the dense flavour; binning needs the CSR-of-ECs layout");
  if (n_ecs != L.E)
    throw Fail("msw_core_bin_reads: " + std::to_string(n_ecs) + " equivalence classes given, the handle holds " +
               std::to_string(L.E));
  if (!bin_ptr) throw Fail("msw_core_bin_reads: null bin_ptr");
  if (n_targets && (!targets || !thresholds)) throw Fail("msw_core_bin_reads: null targets or thresholds");
  if (n_targets >= (size_t)kNoSlot) throw Fail("msw_core_bin_reads: too many targets");
  const uint32_t G = L.G, E = L.E;
  std::vector<uint32_t> slot_of(G, kNoSlot);
  std::vector<double> logt(n_targets);
  for (size_t k = 0; k < n_targets; ++k) {
    if (targets[k] >= G)
      throw Fail("msw_core_bin_reads: target " + std::to_string(targets[k]) + " out of range (" + std::to_string(G) +
                 " groups)");
    if (slot_of[targets[k]] != kNoSlot)
      throw Fail("msw_core_bin_reads: group " + std::to_string(targets[k]) + " is a target twice");
    slot_of[targets[k]] = (uint32_t)k;
    const double t = thresholds[k];
    if (!(t >= 0.0 && t <= 1.0)) throw Fail("msw_core_bin_reads: threshold of target " + std::to_string(k) + " not in [0, 1]");
    logt[k] = std::log(t);
  }
  if (!rptr || (!reads && n_ecs && !on_device)) throw Fail("msw_core_bin_reads: null ec_rptr or ec_reads");
  if (log_thr_out && n_targets) std::memcpy(log_thr_out, logt.data(), n_targets * sizeof(double));
  std::fill(bin_ptr, bin_ptr + n_targets + 1, (uint64_t)0);
  if (n_targets == 0) return;
  hipStream_t st = h->stream;

  // the reads of every class where the kernels can read them
  DevBuf<uint64_t> d_rptr_own;
  DevBuf<uint32_t> d_reads_own;
  const uint64_t *d_rptr = rptr;
  const uint32_t *d_reads = reads;
  if (!on_device) {
    if (rptr[0] != 0) throw Fail("msw_core_bin_reads: ec_rptr[0] != 0");
    for (size_t j = 0; j < n_ecs; ++j)
      if (rptr[j + 1] < rptr[j]) throw Fail("msw_core_bin_reads: ec_rptr is not ascending");
    bin_alloc(d_rptr_own, n_ecs + 1, "ec_rptr");
    bin_alloc(d_reads_own, rptr[n_ecs], "ec_reads");
    MSW_HIP(hipMemcpyAsync(d_rptr_own.p, rptr, (n_ecs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (rptr[n_ecs])
      MSW_HIP(hipMemcpyAsync(d_reads_own.p, reads, rptr[n_ecs] * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_rptr = d_rptr_own.p;
    d_reads = d_reads_own.p;
  }

  // targets, thresholds and the background prefilter (bin_kernels.hpp: BinTargets)
  const GammaState gs = gamma_state(h->solver);
  std::vector<double> u(G);
  MSW_HIP(hipMemcpyAsync(u.data(), gs.u, G * sizeof(double), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  double cmax = -INFINITY, mag = 0.0;
  for (size_t k = 0; k < n_targets; ++k) {
    const double x = gs.a * L.logzi, ug = u[targets[k]];
    const double c = x + ug - logt[k];
    cmax = std::isnan(c) ? INFINITY : std::max(cmax, c);
    for (double v : {x, ug, logt[k]})
      if (std::isfinite(v)) mag = std::max(mag, std::fabs(v));
  }
  DevBuf<uint32_t> d_slot, d_grp;
  DevBuf<double> d_logt;
  bin_alloc(d_slot, G, "the slot map");
  bin_alloc(d_grp, n_targets, "the targets");
  bin_alloc(d_logt, n_targets, "the thresholds");
  MSW_HIP(hipMemcpyAsync(d_slot.p, slot_of.data(), G * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(d_grp.p, targets, n_targets * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(d_logt.p, logt.data(), n_targets * sizeof(double), hipMemcpyHostToDevice, st));
  const BinTargets B{d_slot.p, d_grp.p, d_logt.p, (uint32_t)n_targets, cmax, 1e-9 * (1.0 + mag)};
  const bool lds = bin_slots_in_lds(G);

  // count pass, exclusive scan of the counts in EC order (cnt[E] = 0: off[E] = the number of pairs)
  DevBuf<double> lse_p;
  DevBuf<uint32_t> cnt;
  DevBuf<uint64_t> off;
  bin_alloc(lse_p, E, "the normalisers");
  bin_alloc(cnt, (size_t)E + 1, "the pair counts");
  bin_alloc(off, (size_t)E + 1, "the pair offsets");
  MSW_HIP(hipMemsetAsync(cnt.p + E, 0, sizeof(uint32_t), st));
  if (lds) launch_bin_enc<true>(h, gs, B, lse_p.p, cnt.p, nullptr, nullptr, nullptr, false);
  else launch_bin_enc<false>(h, gs, B, lse_p.p, cnt.p, nullptr, nullptr, nullptr, false);
  size_t tmp_bytes = 0;
  MSW_HIP(prim_scan(nullptr, tmp_bytes, cnt.p, off.p, (size_t)E + 1, st));
  DevBuf<uint8_t> tmp;
  bin_alloc(tmp, tmp_bytes, "scan storage");
  MSW_HIP(prim_scan(tmp.p, tmp_bytes, cnt.p, off.p, (size_t)E + 1, st));
  uint64_t n_pairs = 0;
  MSW_HIP(hipMemcpyAsync(&n_pairs, off.p + E, sizeof n_pairs, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  if (n_pairs == 0) return;

  // write pass, then the pairs by target slot (stable: each target's ECs stay in EC order)
  DevBuf<uint32_t> key, val, key2, val2;
  bin_alloc(key, n_pairs, "the (target, class) pairs");
  bin_alloc(val, n_pairs, "the (target, class) pairs");
  bin_alloc(key2, n_pairs, "the sorted pairs");
  bin_alloc(val2, n_pairs, "the sorted pairs");
  if (lds) launch_bin_enc<true>(h, gs, B, lse_p.p, nullptr, off.p, key.p, val.p, true);
  else launch_bin_enc<false>(h, gs, B, lse_p.p, nullptr, off.p, key.p, val.p, true);
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < n_targets) ++bits;
  MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, key.p, key2.p, val.p, val2.p, (size_t)n_pairs, bits, st));
  bin_alloc(tmp, tmp_bytes, "sort storage");
  MSW_HIP(prim_sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, val2.p, (size_t)n_pairs, bits, st));

  // output offsets of the sorted pairs (roff[n_pairs] = the reads in all bins) and bin_ptr
  DevBuf<uint64_t> roff, d_bin_ptr;
  bin_alloc(roff, n_pairs + 1, "the output offsets");
  bin_alloc(d_bin_ptr, n_targets + 1, "bin_ptr");
  const BinPairLen lens{val2.p, d_rptr, (size_t)n_pairs};
  MSW_HIP(prim_scan(nullptr, tmp_bytes, lens, roff.p, (size_t)n_pairs + 1, st));
  bin_alloc(tmp, tmp_bytes, "scan storage");
  MSW_HIP(prim_scan(tmp.p, tmp_bytes, lens, roff.p, (size_t)n_pairs + 1, st));
  hipLaunchKernelGGL(k_bin_ptr, dim3((unsigned)((n_targets + 1 + 255) / 256)), dim3(256), 0, st, key2.p, (size_t)n_pairs,
                     roff.p, (uint32_t)n_targets, d_bin_ptr.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipMemcpyAsync(bin_ptr, d_bin_ptr.p, (n_targets + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  const uint64_t total = bin_ptr[n_targets];
  if (!reads_out || total == 0) return;

  // the reads themselves
  DevBuf<uint32_t> out;
  bin_alloc(out, total, "the binned read ids");
  const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_pairs + 255) / 256, (uint64_t)h->n_cu * 16));
  hipLaunchKernelGGL(k_bin_scatter, dim3(nb), dim3(256), 0, st, val2.p, (size_t)n_pairs, d_rptr, d_reads, roff.p, out.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipMemcpyAsync(reads_out, out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
}

}  // namespace
