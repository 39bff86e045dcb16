// host_build.inc -- device build of the likelihood from the pseudoalignment (included by
// build.hip): replaces LL_WOR21::fill_ll_mat + fill_ec_counts
// (include/Likelihood.hpp:109-195).  K0-K2 run on the device; the host computes the O(G) mask /
// size-class bookkeeping; the SELL-64 packing runs on the device too (pack_kernels.hpp).
namespace {

// exclusive scan of nd[0..n) in place on the device -> offsets; returns the total
uint64_t device_scan_u32(msw_core *h, uint32_t *d, uint64_t n, DevBuf<uint32_t> &tot, DevBuf<uint64_t> &gt) {
  const uint32_t nblocks = (uint32_t)((n + kScanChunk - 1) / kScanChunk);
  tot.alloc(nblocks + 1);
  gt.alloc(1);
  hipLaunchKernelGGL(k_scan_local, dim3(nblocks), dim3(256), 0, h->stream, d, n, d, tot.p);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(256), 0, h->stream, tot.p, nblocks, gt.p);
  hipLaunchKernelGGL(k_scan_add, dim3(nblocks), dim3(256), 0, h->stream, d, n, tot.p);
  MSW_HIP(hipGetLastError());
  uint64_t total = 0;
  MSW_HIP(hipMemcpyAsync(&total, gt.p, sizeof total, hipMemcpyDeviceToHost, h->stream));
  MSW_HIP(hipStreamSynchronize(h->stream));
  return total;
}

void build_likelihood_impl(msw_core *h, const uint64_t *ec_tptr, const uint32_t *ec_targets, size_t E,
                           const uint32_t *target_group, size_t T, const uint64_t *group_sizes,
                           size_t G, const uint64_t *ec_counts, double q, double e, double zi,
                           size_t min_hits, size_t *n_groups_out, uint8_t *mask_out, double *logc_out,
                           bool on_device, uint64_t dev_hits) {
  Resident &L = h->lik;
  // on_device: ec_tptr / ec_targets / ec_counts are DEVICE pointers (msw_alignment_read_device) and dev_hits =
  // ec_tptr[E]; they are read where they lie
  // EC-sharded build (a communicator is attached): a rank whose OWN block is bad -- arguments, ec_tptr, target ids,
  // an EC that hits more sequences than its group holds -- must not leave its peers waiting in the --min-hits
  // all-reduce or in the first collective of the solve that follows.  The rank-local stages therefore run under
  // try / catch and end in an all-reduce of ONE status word: every rank fails together, none is stranded, and the
  // communicator stays usable (as msw_core_bootstrap_dist does).  Only a failure between the collectives of the
  // --min-hits stage itself aborts the communicator (guarded(), in_collective).
  DevBuf<unsigned long long> d_status;
  auto sync_status = [&](const std::string &my_err) {
    if (!h->comm) {
      if (!my_err.empty()) throw Fail(my_err);
      return;
    }
    CollectiveScope cs(&h->in_collective);
    const unsigned long long flag = my_err.empty() ? 0ull : 1ull;
    unsigned long long total = 0;
    d_status.alloc(1);
    MSW_HIP(hipMemcpyAsync(d_status.p, &flag, sizeof flag, hipMemcpyHostToDevice, h->stream));
    h->comm->allreduce_u64(reinterpret_cast<uint64_t *>(d_status.p), 1, h->stream);
    MSW_HIP(hipMemcpyAsync(&total, d_status.p, sizeof total, hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
    cs.leave();
    if (!my_err.empty()) throw Fail(my_err);
    if (total) throw Fail("msw_core_build_likelihood: another rank of the sharded build failed on its block of equivalence classes");
  };
  auto local_stage = [&](auto &&stage) {  // run a rank-local stage; sharded: every rank learns whether all got through
    if (!h->comm) {
      stage();
      return;
    }
    std::string err;
    try {
      stage();
    } catch (const std::exception &ex) {
      err = ex.what();
      (void)hipGetLastError();
    }
    sync_status(err);
  };
  StageTimer tm(h->stream);
  hipStream_t st = h->stream;
  // The multiplicities (8 E bytes: 7 ms of PCIe at cfg5) are first needed by K2: they travel on the handle's second
  // stream while the first pass of K1 runs on `st`.  The guard drains that stream on every way out: the copy reads
  // the caller's buffer.
  if (!h->resampler.stream2) MSW_HIP(hipStreamCreateWithFlags(&h->resampler.stream2, hipStreamNonBlocking));
  if (!h->resampler.ev_counts[0]) MSW_HIP(hipEventCreateWithFlags(&h->resampler.ev_counts[0], hipEventDisableTiming));
  struct DrainGuard {
    hipStream_t s;
    ~DrainGuard() { (void)hipStreamSynchronize(s); }
  } drain_side{h->resampler.stream2};
  DevBuf<uint64_t> tptr_up, ecc_up, gt;
  DevBuf<uint32_t> targets_up, d_tgroup, d_mid, d_long, d_ctr, d_rowptr, d_grp, d_cnt, tot;
  // the pseudoalignment on the device: the caller's arrays (on_device) or the copies uploaded below
  const uint64_t *d_tptr = ec_tptr, *d_ecc = ec_counts;
  const uint32_t *d_targets = ec_targets;
  uint64_t nnz = 0;
  local_stage([&] {
  if (!ec_tptr || !target_group || !group_sizes || !ec_counts) throw Fail("msw_core_build_likelihood: null argument");
  if (E == 0 || G == 0 || T == 0) throw Fail("msw_core_build_likelihood: empty input");
  if (E >= 0xffffffffull || G > 0x7fffffffull || T >= 0xffffffffull)
    throw Fail("msw_core_build_likelihood: dimensions exceed 32 bits");
  if (!(zi > 0.0 && zi < 1.0)) throw Fail("msw_core_build_likelihood: zero_inflation must be in (0, 1)");
  if (!on_device && ec_tptr[0] != 0) throw Fail("msw_core_build_likelihood: ec_tptr[0] must be 0");
  const uint64_t ntot = on_device ? dev_hits : ec_tptr[E];
  if (ntot > 0 && !ec_targets) throw Fail("msw_core_build_likelihood: null ec_targets");
  // shape checks the kernels rely on (ec_tptr monotone and the target ids in range: checked by K1 on the device,
  // which reads them anyway -- the host walking 495 M target ids cost a third of the cfg5 build)
  if (ntot >= (1ull << 40)) throw Fail("msw_core_build_likelihood: ec_tptr[n_ecs] is not a hit count (ec_tptr not monotone?)");
  for (size_t t = 0; t < T; ++t)
    if (target_group[t] >= G) throw Fail("msw_core_build_likelihood: group indicator out of range");
  for (size_t g = 0; g < G; ++g)
    if (group_sizes[g] == 0 || group_sizes[g] > 0x7fffffffull) throw Fail("msw_core_build_likelihood: bad group size");
  reset_likelihood(h);
  if (!on_device) {
    tptr_up.upload(ec_tptr, E + 1, st);
    targets_up.upload(ec_targets, ntot, st);
    d_tptr = tptr_up.p;
    d_targets = targets_up.p;
  }
  d_tgroup.upload(target_group, T, st);
  if (!on_device) {
    ecc_up.alloc(E);
    d_ecc = ecc_up.p;
  }
  d_mid.alloc(E);   // ECs of 17..64 hits / of more than 64: listed by the first pass of K1
  d_long.alloc(E);
  d_ctr.alloc(kBuildCtrs);
  d_ctr.zero(st);
  d_rowptr.alloc(E + 1);
  MSW_HIP(hipMemsetAsync(d_rowptr.p, 0, (E + 1) * sizeof(uint32_t), st));
  tm.mark("uploads");

  // ---- K1: count distinct groups per EC, scan, emit (group, count) ----------------------------
  const unsigned nbt = (unsigned)std::min<size_t>((E + 255) / 256, (size_t)h->n_cu * 32);
  hipLaunchKernelGGL(k_ec_groups_thread<false>, dim3(nbt), dim3(256), 0, st, d_tptr, d_targets, d_tgroup.p, (uint32_t)E,
                     (uint32_t)T, ntot, d_rowptr.p, (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                     d_mid.p, d_long.p, d_ctr.p);
  MSW_HIP(hipGetLastError());
  if (!on_device) ecc_up.upload(ec_counts, E, h->resampler.stream2);  // under the kernel just launched
  MSW_HIP(hipEventRecord(h->resampler.ev_counts[0], h->resampler.stream2));
  MSW_HIP(hipStreamWaitEvent(st, h->resampler.ev_counts[0], 0));  // (whatever follows on `st` sees the counts)
  uint32_t ctr[kBuildCtrs] = {};
  auto read_ctr = [&] {
    MSW_HIP(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    if (ctr[kCtrBad] & kBadTptr) throw Fail("msw_core_build_likelihood: ec_tptr not monotone");
    if (ctr[kCtrBad] & kBadTarget) throw Fail("msw_core_build_likelihood: target id out of range");
  };
  read_ctr();
  const uint32_t n_mid = ctr[kCtrMid], n_long = ctr[kCtrLong];
  const unsigned nbw = (unsigned)std::min<size_t>(((size_t)n_mid + 3) / 4, (size_t)h->n_cu * 32);
  const bool hist_lds = G * sizeof(uint32_t) <= 128 * 1024;
  const unsigned nbl = n_long ? std::min<uint32_t>(n_long, hist_lds ? 1024u : 64u) : 0u;
  DevBuf<uint32_t> scratch;
  if (n_long && !hist_lds) scratch.alloc((size_t)nbl * G);
  const size_t lds_long = hist_lds ? G * sizeof(uint32_t) : 0;
  if (n_long && hist_lds) {
    grant_dynamic_lds((const void *)k_ec_groups_long<false>, lds_long);
    grant_dynamic_lds((const void *)k_ec_groups_long<true>, lds_long);
  }
  if (n_mid)
    hipLaunchKernelGGL(k_ec_groups_wave<false>, dim3(nbw), dim3(256), 0, st, d_mid.p, n_mid, d_tptr, d_targets,
                       d_tgroup.p, (uint32_t)T, d_rowptr.p, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                       (uint32_t *)nullptr, d_ctr.p);
  if (n_long)
    hipLaunchKernelGGL(k_ec_groups_long<false>, dim3(nbl), dim3(256), lds_long, st, d_long.p, n_long, d_tptr,
                       d_targets, d_tgroup.p, (uint32_t)G, (uint32_t)T, hist_lds ? nullptr : scratch.p, d_rowptr.p,
                       (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, d_ctr.p);
  MSW_HIP(hipGetLastError());
  nnz = device_scan_u32(h, d_rowptr.p, E + 1, tot, gt);
  if (n_mid || n_long) read_ctr();  // target ids of the longer ECs
  tm.mark("K1 count + scan");
  if (nnz >= 0xffffffffull) throw Fail("msw_core_build_likelihood: more than 2^32-1 nonzero cells");
  d_grp.alloc(nnz);
  d_cnt.alloc(nnz);
  hipLaunchKernelGGL(k_ec_groups_thread<true>, dim3(nbt), dim3(256), 0, st, d_tptr, d_targets, d_tgroup.p, (uint32_t)E,
                     (uint32_t)T, ntot, (uint32_t *)nullptr, d_rowptr.p, d_grp.p, d_cnt.p, (uint32_t *)nullptr,
                     (uint32_t *)nullptr, d_ctr.p);
  if (n_mid)
    hipLaunchKernelGGL(k_ec_groups_wave<true>, dim3(nbw), dim3(256), 0, st, d_mid.p, n_mid, d_tptr, d_targets,
                       d_tgroup.p, (uint32_t)T, (uint32_t *)nullptr, d_rowptr.p, d_grp.p, d_cnt.p, d_ctr.p);
  if (n_long)
    hipLaunchKernelGGL(k_ec_groups_long<true>, dim3(nbl), dim3(256), lds_long, st, d_long.p, n_long, d_tptr,
                       d_targets, d_tgroup.p, (uint32_t)G, (uint32_t)T, hist_lds ? nullptr : scratch.p,
                       (uint32_t *)nullptr, d_rowptr.p, d_grp.p, d_cnt.p, d_ctr.p);
  MSW_HIP(hipGetLastError());
  if (h->comm) MSW_HIP(hipStreamSynchronize(st));  // sharded: a device fault of this stage surfaces inside it
  });  // local stage 1

  tm.mark("K1 emit");
  // ---- K2: --min-hits mask (include/Likelihood.hpp:141-171) -----------------------------------
  std::vector<uint8_t> mask(G, 1);
  std::vector<int32_t> pos(G);
  size_t Gk = G;
  const unsigned nbe = (unsigned)std::min<size_t>((E + 255) / 256, (size_t)h->n_cu * 16);
  std::vector<unsigned long long> hits;
  DevBuf<unsigned long long> d_hits;
  if (min_hits > 0) {
    // from here to the all-reduce of the group hits the peers of a sharded build wait for this rank (guarded())
    h->in_collective = h->comm != nullptr;
    d_hits.alloc(G);
    MSW_HIP(hipMemsetAsync(d_hits.p, 0, G * sizeof(unsigned long long), st));
    grant_dynamic_lds((const void *)k_group_hits, kHitsGroups * sizeof(unsigned long long));
    for (uint32_t g0 = 0; g0 < G; g0 += kHitsGroups) {
      const uint32_t ng = (uint32_t)std::min<size_t>(kHitsGroups, G - g0);
      hipLaunchKernelGGL(k_group_hits, dim3((unsigned)std::min<size_t>((E + 1023) / 1024, (size_t)h->n_cu)), dim3(1024),
                         ng * sizeof(unsigned long long), st, d_rowptr.p, d_grp.p, (uint32_t)E, d_ecc, g0, ng, d_hits.p);
    }
    // EC-sharded build (a communicator is attached: this handle holds one rank's block of ECs): the hits of a
    // group are summed over ALL ECs (include/Likelihood.hpp:146-163) -- one all-reduce of G integers, after
    // which every rank derives the same mask and the same compaction
    if (h->comm) h->comm->allreduce_u64(reinterpret_cast<uint64_t *>(d_hits.p), G, st);
    h->in_collective = false;
    hits.resize(G);
    MSW_HIP(hipMemcpyAsync(hits.data(), d_hits.p, G * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
  }
  local_stage([&] {  // local stage 2: mask / compaction, lookup table, packing
  if (min_hits > 0) {
    Gk = 0;
    for (size_t g = 0; g < G; ++g) {
      mask[g] = hits[g] >= min_hits;
      pos[g] = mask[g] ? (int32_t)Gk++ : -1;
    }
    if (Gk == 0) throw Fail("msw_core_build_likelihood: --min-hits removed every group");
    if (Gk < G) {
      DevBuf<int32_t> d_pos;
      DevBuf<uint32_t> d_rowptr2, d_grp2, d_cnt2;
      d_pos.upload(pos.data(), G, st);
      d_rowptr2.alloc(E + 1);
      MSW_HIP(hipMemsetAsync(d_rowptr2.p, 0, (E + 1) * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_compact_count, dim3(nbe), dim3(256), 0, st, d_rowptr.p, d_grp.p, (uint32_t)E, d_pos.p, d_rowptr2.p);
      const uint64_t nnz2 = device_scan_u32(h, d_rowptr2.p, E + 1, tot, gt);
      d_grp2.alloc(nnz2);
      d_cnt2.alloc(nnz2);
      hipLaunchKernelGGL(k_compact_emit, dim3(nbe), dim3(256), 0, st, d_rowptr.p, d_grp.p, d_cnt.p, (uint32_t)E,
                         d_pos.p, d_rowptr2.p, d_grp2.p, d_cnt2.p);
      MSW_HIP(hipGetLastError());
      MSW_HIP(hipStreamSynchronize(st));
      std::swap(d_rowptr.p, d_rowptr2.p); std::swap(d_rowptr.n, d_rowptr2.n);
      std::swap(d_grp.p, d_grp2.p); std::swap(d_grp.n, d_grp2.n);
      std::swap(d_cnt.p, d_cnt2.p); std::swap(d_cnt.n, d_cnt2.n);
      nnz = nnz2;
    }
  } else {
    for (size_t g = 0; g < G; ++g) pos[g] = (int32_t)g;
  }

  tm.mark("K2 min-hits + compaction");
  // ---- K0: size classes of the kept groups and their lookup table ------------------------------
  std::vector<uint32_t> ksize(Gk), lut_off(Gk), class_size;
  uint64_t max_size = 0;
  for (size_t g = 0; g < G; ++g)
    if (mask[g]) {
      ksize[pos[g]] = (uint32_t)group_sizes[g];
      max_size = std::max<uint64_t>(max_size, group_sizes[g]);
    }
  const uint64_t ld = max_size + 1;
  {
    std::unordered_map<uint32_t, uint32_t> cls;
    for (size_t g = 0; g < Gk; ++g) {
      auto it = cls.find(ksize[g]);
      if (it == cls.end()) {
        it = cls.emplace(ksize[g], (uint32_t)class_size.size()).first;
        class_size.push_back(ksize[g]);
      }
      const uint64_t off = (uint64_t)it->second * ld;
      if (off + ld > 0x7fffffffull) throw Fail("msw_core_build_likelihood: lookup table too large");
      lut_off[g] = (uint32_t)off;
    }
  }
  const uint64_t n_lut = class_size.size() * ld;
  DevBuf<uint32_t> d_csize, d_lutoff, d_ksize, d_idx;
  DevBuf<int> d_bad;
  d_csize.upload(class_size.data(), class_size.size(), st);
  d_lutoff.upload(lut_off.data(), Gk, st);
  d_ksize.upload(ksize.data(), Gk, st);
  L.lut.alloc(n_lut);
  hipLaunchKernelGGL(k_lut_build, dim3((unsigned)((n_lut + 255) / 256)), dim3(256), 0, st, d_csize.p,
                     (uint32_t)class_size.size(), (uint32_t)ld, q, e, zi, L.lut.p);
  d_idx.alloc(nnz);
  d_bad.alloc(1);
  MSW_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), st));
  if (nnz)
    hipLaunchKernelGGL(k_cell_lutidx, dim3((unsigned)std::min<uint64_t>((nnz + 255) / 256, (uint64_t)h->n_cu * 32)),
                       dim3(256), 0, st, d_grp.p, d_cnt.p, nnz, d_lutoff.p, d_ksize.p, d_idx.p, d_bad.p);
  DevBuf<double> &d_logc = L.logc_res;  // stays resident: msw_core_solve(logc = NULL) uses it
  d_logc.alloc(E);
  hipLaunchKernelGGL(k_log_counts, dim3(nbe), dim3(256), 0, st, d_ecc, (uint32_t)E, d_logc.p);
  MSW_HIP(hipGetLastError());

  // ---- pack into SELL-64: on the device (pack_kernels.hpp); MSWEEP_HOST_PACK=1 takes the CSR to the
  // host packer instead ---------------------------------------------------------------------------
  int bad = 0;
  MSW_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
  if (logc_out) MSW_HIP(hipMemcpyAsync(logc_out, d_logc.p, E * sizeof(double), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  tm.mark("K0 table, slots, log counts");
  if (bad) throw Fail("msw_core_build_likelihood: an EC hits more sequences of a group than the group holds");
  L.G = (uint32_t)Gk;
  L.E = (uint32_t)E;
  L.nnz = nnz;
  L.n_lut = (uint32_t)n_lut;
  L.logzi = std::log(zi);
  if (getenv("MSWEEP_HOST_PACK")) {
    std::vector<uint32_t> rp(E + 1), hg(nnz + 1), hi(nnz + 1);
    MSW_HIP(hipMemcpyAsync(rp.data(), d_rowptr.p, (E + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (nnz) {
      MSW_HIP(hipMemcpyAsync(hg.data(), d_grp.p, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      MSW_HIP(hipMemcpyAsync(hi.data(), d_idx.p, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    MSW_HIP(hipStreamSynchronize(st));
    upload_sell(h, rp.data(), hg.data(), hi.data());
  } else {
    sell_from_device(h, d_rowptr.p, d_grp.p, d_idx.p);
  }
  tm.mark("pack (total)");
  L.have_logc_res = true;
  });  // local stage 2
  if (n_groups_out) *n_groups_out = Gk;
  if (mask_out) std::memcpy(mask_out, mask.data(), G);
}

}  // namespace
