// host_pack.inc -- driver of the device SELL packer (pack_kernels.hpp); included by
// build.hip after host_likelihood.inc.
namespace {

uint64_t device_scan_u32(msw_core *h, uint32_t *d, uint64_t n, DevBuf<uint32_t> &tot, DevBuf<uint64_t> &gt);

// Value records (sell.hpp): no slot area; the group vectors in LDS when they fit.
void choose_value_layout(Resident &L) {
  L.enc = kEncValue;
  L.tlds = false;
  L.n_area = 0;
  L.n_tab_lds = 0;
  L.dec.shift = 0;
  L.dec.mask = 0;
  L.dec.bhi = L.dec.bhiA = 0;
  const char *force = getenv("MSWEEP_FORCE_LDS");  // developer switch: first digit = group vectors in LDS or not
  const bool want_glds = !(force && strlen(force) == 2 && force[0] == '0');
  L.glds = want_glds && pass_lds_bytes(1, 0, L.G, true, false) <= kLdsMax && passB_mode(L, true, 0, false) >= 0;
  L.gmodeB = passB_mode(L, L.glds, 0, false);
  if (L.gmodeB < 0) throw Fail("internal: no LDS configuration fits");
  if (8ull * ((uint64_t)L.G + kSentinels) >= (1ull << 31)) throw Fail("likelihood too large: group offsets exceed the record field");
}

// CSR-of-ECs in HBM (32-bit row pointers, per-cell group and LUT slot) -> the resident SELL-64
// likelihood of handle h.  L.G, E, nnz, n_lut are set by the caller.
// cell_val != nullptr: value records -- d_idx[k] is then cell k's position in cell_val (its log-likelihood).
void sell_from_device(msw_core *h, const uint32_t *d_rowptr, const uint32_t *d_grp, const uint32_t *d_idx,
                      const double *cell_val /* = nullptr */) {
  Resident &L = h->lik;
  const uint32_t E = L.E, n_lut = L.n_lut;
  const uint64_t nnz = L.nnz;
  hipStream_t st = h->stream;
  StageTimer tm(st);
  SlotPlan sp;
  DevBuf<uint32_t> d_canon, d_hot;
  DevBuf<double> mm_part;
  if (cell_val) {
    choose_value_layout(L);
    L.area_slot.alloc(1);
    L.lut_area.alloc(1);
    MSW_HIP(hipMemsetAsync(L.area_slot.p, 0, sizeof(uint32_t), st));
    MSW_HIP(hipMemcpyAsync(L.lut_area.p, &L.logzi, sizeof(double), hipMemcpyHostToDevice, st));
    L.trange.alloc(2);  // {max, min} of the cells' values: what the sweeps scale their exponentials by
    {  // (up to 5e8 cells at cfg2's shape: every CU reads its share, then one workgroup the partial pairs)
      const uint64_t nv = std::max<uint64_t>(nnz, 1);
      const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nv + 8191) / 8192, (uint64_t)h->n_cu * 4));
      mm_part.alloc(2 * (size_t)nb);
      minmax_launch(nb, st, nnz ? cell_val : L.lut_area.p, nv, 0, mm_part.p);  // (k_minmax: solve.hip)
      minmax_launch(1, st, mm_part.p, (uint64_t)nb, 1, L.trange.p);
      MSW_HIP(hipGetLastError());
    }
  } else {
  // ---- slot statistics -> slot area, LDS mode, record encoding (host decisions on n_lut numbers) --
  DevBuf<unsigned long long> d_freq;
  d_freq.alloc(std::max<uint32_t>(n_lut, 1));
  d_freq.zero(st);
  if (nnz) {
    const size_t lds = n_lut <= 16384 ? (size_t)n_lut * sizeof(unsigned int) : 0;
    hipLaunchKernelGGL(k_slot_hist, dim3((unsigned)std::min<uint64_t>((nnz + 4095) / 4096, (uint64_t)h->n_cu * 8)), dim3(256),
                       lds, st, d_idx, nnz, n_lut, d_freq.p);
  }
  std::vector<unsigned long long> f(std::max<uint32_t>(n_lut, 1), 0);
  MSW_HIP(hipMemcpyAsync(f.data(), d_freq.p, f.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  const std::vector<uint64_t> freq(f.begin(), f.end());
  sp = plan_slot_area(h, freq);
  d_canon.upload(sp.canon.data(), sp.canon.size(), st);
  d_hot.upload(sp.hot_rank.data(), sp.hot_rank.size(), st);
  }
  tm.mark("  pack: slot plan");
  // ---- EC order: stable radix sort of the (length, cold class) keys ------------------------------
  DevBuf<uint32_t> key, key2, val, cnt;
  key.alloc(E);
  key2.alloc(E);
  val.alloc(E);
  L.perm.alloc(E);
  cnt.alloc(1 + kSliceClasses);
  MSW_HIP(hipMemsetAsync(cnt.p, 0, (1 + kSliceClasses) * sizeof(uint32_t), st));
  const unsigned nbe = (unsigned)std::min<size_t>(((size_t)E + 255) / 256, (size_t)h->n_cu * 16);
  hipLaunchKernelGGL(k_pack_keys, dim3(nbe), dim3(256), 0, st, d_rowptr, E, L.long_row, multilane() ? 1 : 0, d_idx,
                     L.hybrid() ? d_canon.p : (const uint32_t *)nullptr, L.n_tab_lds, key.p, val.p, cnt.p);
  size_t tmp_bytes = 0;
  MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, key.p, key2.p, val.p, L.perm.p, (size_t)E, kPackKeyBits, st));
  DevBuf<unsigned char> tmp;
  tmp.alloc(tmp_bytes);
  MSW_HIP(prim_sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, L.perm.p, (size_t)E, kPackKeyBits, st));
  uint32_t counts[1 + kSliceClasses] = {};
  MSW_HIP(hipMemcpyAsync(counts, cnt.p, sizeof counts, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  tm.mark("  pack: keys + sort");
  const uint32_t n_long = counts[0];
  // ---- geometry: slice classes (sell.hpp), long-EC pointers and slice offsets --------------------
  const uint32_t n_sell = E - n_long;
  L.cls = make_slice_classes(counts + 1);
  const uint32_t nslices = L.cls.s0[kSliceClasses];
  L.long_ptr.alloc((size_t)n_long + 1);
  L.slice_off.alloc((size_t)nslices + 1);
  MSW_HIP(hipMemsetAsync(L.long_ptr.p, 0, ((size_t)n_long + 1) * sizeof(uint32_t), st));
  MSW_HIP(hipMemsetAsync(L.slice_off.p, 0, ((size_t)nslices + 1) * sizeof(uint32_t), st));
  const uint32_t nmax = std::max(n_long, nslices);
  if (nmax)
    hipLaunchKernelGGL(k_pack_lens, dim3((nmax + 255) / 256), dim3(256), 0, st, d_rowptr, L.perm.p, n_long, nslices,
                       odd_slices(L.enc) ? 0 : 1, L.cls, L.long_ptr.p, L.slice_off.p);
  DevBuf<uint32_t> tot;
  DevBuf<uint64_t> gt;
  const uint64_t n_long_cells = device_scan_u32(h, L.long_ptr.p, (uint64_t)n_long + 1, tot, gt);
  const uint64_t n_rows = device_scan_u32(h, L.slice_off.p, (uint64_t)nslices + 1, tot, gt);
  if (n_rows > 0xffffffffull || n_long_cells > 0xffffffffull)
    throw Fail("msw_core_set_csr: likelihood too large for 32-bit slice offsets");
  uint64_t hyb_rows_max = 1ull << kGeoHotShift;
  if (const char *e = getenv("MSWEEP_HYBRID_MAX_ROWS")) hyb_rows_max = std::min<uint64_t>(hyb_rows_max, strtoull(e, nullptr, 10));  // developer switch (tests)
  if (L.hybrid() && n_rows >= hyb_rows_max) {
    // the hot-segment split rides above the slice offset (27 bits): plan again without the hybrid area -- index
    // records need it -- i.e. with all-memory tables and wide records, rather than refuse the upload
    if (h->no_hybrid) throw Fail("msw_core_set_csr: likelihood too large for the hybrid slot area's slice geometry");
    h->no_hybrid = true;
    try {
      sell_from_device(h, d_rowptr, d_grp, d_idx, cell_val);
    } catch (...) {
      h->no_hybrid = false;
      throw;
    }
    h->no_hybrid = false;
    return;
  }
  const size_t nslots = (size_t)n_rows * 64;
  if (L.hybrid()) L.slice_hot.alloc(std::max<uint32_t>(nslices, 1));
  L.rec.alloc(rec_words(L.enc, nslots + 64) + 2);  // + one spare row behind the last slice
  L.rec_long.alloc(rec_words(L.enc, (size_t)n_long_cells + 64) + 2);
  MSW_HIP(hipMemsetAsync(L.rec.p + rec_words(L.enc, nslots), 0, (rec_words(L.enc, 64) + 2) * sizeof(uint32_t), st));
  // (rec_words rounds up to whole rows of 64 cells: the tail behind the last long EC's cells is read by nobody but
  // msw_core_layout_hash, which must not see uninitialised memory)
  MSW_HIP(hipMemsetAsync(L.rec_long.p, 0, (rec_words(L.enc, (size_t)n_long_cells + 64) + 2) * sizeof(uint32_t), st));
  tm.mark("  pack: geometry + alloc");
  // ---- records ------------------------------------------------------------------------------------
  const PackEnc pe{d_canon.p, d_hot.p, sp.rep_base, L.G, sp.sentinel_slot, L.dec, L.n_tab_lds, L.slice_hot.p,
                   cell_val, L.logzi};
  if (n_long) {
    auto k = L.enc == kEncValue ? k_pack_long<kEncValue>
                                 : (L.wide() ? k_pack_long<kEncWide> : (L.hybrid() ? k_pack_long<kEncIndex> : k_pack_long<kEncNarrow>));
    hipLaunchKernelGGL(k, dim3(std::min<uint32_t>(n_long, (uint32_t)h->n_cu * 32)), dim3(64), 0, st, d_rowptr, d_grp, d_idx,
                       L.perm.p, L.long_ptr.p, n_long, pe, L.rec_long.p);
  }
  if (nslices) {
    auto k = L.enc == kEncValue ? k_pack_slices<kEncValue>
                                 : (L.wide() ? k_pack_slices<kEncWide> : (L.hybrid() ? k_pack_slices<kEncIndex> : k_pack_slices<kEncNarrow>));
    hipLaunchKernelGGL(k, dim3(std::min<uint32_t>(nslices, (uint32_t)h->n_cu * 64)), dim3(64), 0, st, d_rowptr, d_grp,
                       d_idx, L.perm.p, L.slice_off.p, n_long, n_sell, nslices, L.cls, pe, h->pack_schedule ? 1 : 0, L.rec.p);
  }
  MSW_HIP(hipGetLastError());
  tm.mark("  pack: records");
  L.n_long = n_long;
  L.nslices = nslices;
  L.nslots = nslots;
  finish_sell(h);  // synchronises: the temporaries above die at return
  tm.mark("  pack: solver state");
}

// FNV-1a over the resident SELL layout (records, EC order, geometry): lets the tests hold the device
// packer against the host packer byte for byte.
uint64_t layout_hash(const Resident &L) {
  if (L.flavor != 0) throw Fail("msw_core_layout_hash: no CSR-of-ECs likelihood resident");
  uint64_t hash = 1469598103934665603ull;
  auto eat = [&](const uint32_t *d, size_t n) {
    std::vector<uint32_t> v(n);
    if (n) MSW_HIP(hipMemcpy(v.data(), d, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < n * 4; ++i) hash = (hash ^ p[i]) * 1099511628211ull;
  };
  std::vector<uint32_t> lp(L.n_long + 1);
  MSW_HIP(hipMemcpy(lp.data(), L.long_ptr.p, lp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  eat(L.perm.p, L.E);
  eat(L.slice_off.p, (size_t)L.nslices + 1);
  eat(L.long_ptr.p, (size_t)L.n_long + 1);
  eat(L.rec.p, rec_words(L.enc, L.nslots));
  eat(L.rec_long.p, rec_words(L.enc, (size_t)lp[L.n_long]));
  eat(L.area_slot.p, L.n_area);
  for (int c = 0; c <= kSliceClasses; ++c) {  // the slice classes
    const uint32_t w[2] = {L.cls.s0[c], L.cls.p0[c]};
    const unsigned char *pb = reinterpret_cast<const unsigned char *>(w);
    for (size_t i = 0; i < sizeof w; ++i) hash = (hash ^ pb[i]) * 1099511628211ull;
  }
  if (L.hybrid()) {  // rows of the hot segments
    std::vector<uint8_t> sh(L.nslices);
    if (L.nslices) MSW_HIP(hipMemcpy(sh.data(), L.slice_hot.p, L.nslices, hipMemcpyDeviceToHost));
    for (uint8_t b : sh) hash = (hash ^ b) * 1099511628211ull;
  }
  return hash;
}

}  // namespace
