// host_assign.inc -- msw_core_assign_reads / _aln and msw_core_assign_table_* (included by build.hip, behind host_bin.inc):
// what `mGEMS bin` gives beyond the target bins (assign_kernels.hpp, DESIGN.md 7h).  The assign pass judges every EC
// against all estimated groups; its pairs go through host_bin.inc's sort, offsets and scatter with one more slot for the
// reads nobody claims.  With MSW_ASSIGN_KEEP_TABLE the pairs as written (a CSR by EC) and an index of the reads by id stay
// on the handle, and the table's text is formatted from them block by block: only bytes come to the host.
// Device memory: O(E) + O(pairs) + O(aligned reads) + the output or the text of a block; nothing is sized by G x E,
// n_targets x E or reads x n_targets.  No atomics decide an order: scans and stable sorts do.
namespace {

constexpr size_t kAssignMaxBytes = (size_t)1 << 30;  // worst-case text of one table call

template <class T>
void assign_alloc(DevBuf<T> &b, size_t count, const char *what) {
  named_alloc(b, count, "msw_core_assign_reads", what);
}

struct AssignPassArgs {
  double *lse_p;
  uint32_t *n_assigned, *cnt;
  const uint64_t *off;
  uint32_t *key, *val;
};

template <int ENC, bool LDS>
void launch_assign_passes(msw_core *h, const GammaState &gs, const AssignGroups &A, const AssignPassArgs &P, bool write) {
  const Resident &L = h->lik;
  const size_t lds = LDS ? (size_t)L.G * sizeof(uint32_t) : 0;
  const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)L.E + 255) / 256, (size_t)h->n_cu * 8));
  if (!write)
    hipLaunchKernelGGL((k_assign_count<ENC, LDS>), dim3(nb), dim3(256), lds, h->stream, sell_view(L, h->solver), gs.a, L.logzi,
                       gs.tref, gs.u, A, P.lse_p, P.n_assigned, P.cnt);
  else
    hipLaunchKernelGGL((k_assign_write<ENC, LDS>), dim3(nb), dim3(256), lds, h->stream, sell_view(L, h->solver), gs.a, L.logzi,
                       gs.u, A, P.lse_p, P.off, P.key, P.val);
  MSW_HIP(hipGetLastError());
}
template <bool LDS>
void launch_assign_enc(msw_core *h, const GammaState &gs, const AssignGroups &A, const AssignPassArgs &P, bool write) {
  const Resident &L = h->lik;
  if (L.enc == kEncValue) launch_assign_passes<kEncValue, LDS>(h, gs, A, P, write);
  else if (L.wide()) launch_assign_passes<kEncWide, LDS>(h, gs, A, P, write);
  else if (L.hybrid()) launch_assign_passes<kEncIndex, LDS>(h, gs, A, P, write);
  else launch_assign_passes<kEncNarrow, LDS>(h, gs, A, P, write);
}

}  // namespace

// The index of the (read id, EC) pairs by id: id[i], ec[i] = the i-th pair in the stable sort by read id -- the rows of the
// assignment table, and of msw_core_sparse_probs_* by read (host_sparse_probs.inc).  rptr / reads: device memory.
void msw::host::reads_by_id(msw_core *h, const uint64_t *d_rptr, const uint32_t *d_reads, uint32_t E, uint64_t n_rows,
                            DevBuf<uint32_t> &id, DevBuf<uint32_t> &ec, const char *who) {
  if (!n_rows) return;
  hipStream_t st = h->stream;
  auto alloc = [&](auto &b, size_t count, const char *what) { named_alloc(b, count, who, what); };
  DevBuf<uint32_t> id0, ec0;
  DevBuf<uint8_t> tmp;
  alloc(id0, n_rows, "the read positions");
  alloc(ec0, n_rows, "the read positions");
  alloc(id, n_rows, "the reads by id");
  alloc(ec, n_rows, "the reads by id");
  const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_rows + 255) / 256, (uint64_t)h->n_cu * 16));
  hipLaunchKernelGGL(k_assign_expand, dim3(nb), dim3(256), 0, st, d_rptr, d_reads, E, n_rows, id0.p, ec0.p);
  MSW_HIP(hipGetLastError());
  size_t tmp_bytes = 0;
  MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, id0.p, id.p, ec0.p, ec.p, (size_t)n_rows, 32u, st));
  alloc(tmp, tmp_bytes, "sort storage");
  MSW_HIP(prim_sort_pairs(tmp.p, tmp_bytes, id0.p, id.p, ec0.p, ec.p, (size_t)n_rows, 32u, st));
  MSW_HIP(hipStreamSynchronize(st));
}

namespace {

void assign_reads_impl(msw_core *h, const uint64_t *rptr, const uint32_t *reads, size_t n_ecs, bool on_device,
                       const double *thresholds, const uint32_t *targets, size_t n_targets, unsigned flags, uint64_t *bin_ptr,
                       uint32_t *reads_out, uint32_t *n_assigned_out, uint64_t *class_reads_out) {
  const Resident &L = h->lik;
  AssignState &K = h->assign;
  if (!h->solver.have_solution) throw Fail("msw_core_assign_reads: no solve has run on this handle");
  if (h->comm) throw Fail("msw_core_assign_reads: not available on an EC-sharded handle (a communicator is set)");
  if (L.flavor != 0)
    throw Fail("msw_core_assign_reads: the resident likelihood has the dense flavour; binning needs the CSR-of-ECs layout");
  if (n_ecs != L.E)
    throw Fail("msw_core_assign_reads: " + std::to_string(n_ecs) + " equivalence classes given, the handle holds " +
               std::to_string(L.E));
  if (flags & ~(unsigned)(MSW_ASSIGN_UNASSIGNED | MSW_ASSIGN_KEEP_TABLE))
    throw Fail("msw_core_assign_reads: unknown flags " + std::to_string(flags));
  if (!bin_ptr) throw Fail("msw_core_assign_reads: null bin_ptr");
  if (!thresholds) throw Fail("msw_core_assign_reads: null thresholds");
  if (n_targets && !targets) throw Fail("msw_core_assign_reads: null targets");
  if (n_targets >= (size_t)kNoSlot - 1) throw Fail("msw_core_assign_reads: too many targets");
  const uint32_t G = L.G, E = L.E;
  const bool unassigned = (flags & MSW_ASSIGN_UNASSIGNED) != 0, keep = (flags & MSW_ASSIGN_KEEP_TABLE) != 0;
  const size_t n_slots = n_targets + (unassigned ? 1 : 0);
  std::vector<uint32_t> slot_of(G, kNoSlot);
  for (size_t k = 0; k < n_targets; ++k) {
    if (targets[k] >= G)
      throw Fail("msw_core_assign_reads: target " + std::to_string(targets[k]) + " out of range (" + std::to_string(G) +
                 " groups)");
    if (slot_of[targets[k]] != kNoSlot)
      throw Fail("msw_core_assign_reads: group " + std::to_string(targets[k]) + " is a target twice");
    slot_of[targets[k]] = (uint32_t)k;
  }
  std::vector<double> logt(G);
  for (uint32_t g = 0; g < G; ++g) {
    const double t = thresholds[g];
    if (!(t >= 0.0 && t <= 1.0)) throw Fail("msw_core_assign_reads: threshold of group " + std::to_string(g) + " not in [0, 1]");
    logt[g] = std::log(t);
  }
  if (!rptr || (!reads && n_ecs && !on_device)) throw Fail("msw_core_assign_reads: null ec_rptr or ec_reads");
  if (!on_device) {
    if (rptr[0] != 0) throw Fail("msw_core_assign_reads: ec_rptr[0] != 0");
    for (size_t j = 0; j < n_ecs; ++j)
      if (rptr[j + 1] < rptr[j]) throw Fail("msw_core_assign_reads: ec_rptr is not ascending");
  }
  K.drop();  // the arguments stand: what an earlier call kept goes with this one
  std::fill(bin_ptr, bin_ptr + n_slots + 1, (uint64_t)0);
  hipStream_t st = h->stream;

  // the reads of every class where the kernels can read them
  DevBuf<uint64_t> d_rptr_own;
  DevBuf<uint32_t> d_reads_own;
  const uint64_t *d_rptr = rptr;
  const uint32_t *d_reads = reads;
  uint64_t n_rows = 0;
  if (!on_device) {
    n_rows = rptr[n_ecs];
    assign_alloc(d_rptr_own, n_ecs + 1, "ec_rptr");
    assign_alloc(d_reads_own, n_rows, "ec_reads");
    MSW_HIP(hipMemcpyAsync(d_rptr_own.p, rptr, (n_ecs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (n_rows) MSW_HIP(hipMemcpyAsync(d_reads_own.p, reads, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_rptr = d_rptr_own.p;
    d_reads = d_reads_own.p;
  } else {
    MSW_HIP(hipMemcpyAsync(&n_rows, rptr + n_ecs, sizeof n_rows, hipMemcpyDeviceToHost, st));
  }

  // every group's threshold, the target slots and the background prefilter over ALL groups (assign_kernels.hpp)
  const GammaState gs = gamma_state(h->solver);
  std::vector<double> u(G);
  MSW_HIP(hipMemcpyAsync(u.data(), gs.u, G * sizeof(double), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  double cmax = -INFINITY, mag = 0.0;
  for (uint32_t g = 0; g < G; ++g) {
    const double x = gs.a * L.logzi;
    const double c = x + u[g] - logt[g];
    cmax = std::isnan(c) ? INFINITY : std::max(cmax, c);
    for (double v : {x, u[g], logt[g]})
      if (std::isfinite(v)) mag = std::max(mag, std::fabs(v));
  }
  DevBuf<uint32_t> d_slot;
  DevBuf<double> d_logt;
  assign_alloc(d_slot, G, "the slot map");
  assign_alloc(d_logt, G, "the thresholds");
  MSW_HIP(hipMemcpyAsync(d_slot.p, slot_of.data(), G * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(d_logt.p, logt.data(), G * sizeof(double), hipMemcpyHostToDevice, st));
  const AssignGroups A{d_slot.p, d_logt.p, (uint32_t)n_targets, unassigned ? 1u : 0u, cmax, 1e-9 * (1.0 + mag)};
  const bool lds = bin_slots_in_lds(G);

  // count pass, exclusive scan of the pair counts in EC order (cnt[E] = 0: off[E] = the number of pairs)
  DevBuf<double> lse_p;
  DevBuf<uint32_t> n_asg, cnt;
  DevBuf<uint64_t> off_own;
  DevBuf<uint64_t> &off = keep ? K.off : off_own;
  assign_alloc(lse_p, E, "the normalisers");
  assign_alloc(n_asg, E, "the groups per class");
  assign_alloc(cnt, (size_t)E + 1, "the pair counts");
  assign_alloc(off, (size_t)E + 1, "the pair offsets");
  MSW_HIP(hipMemsetAsync(cnt.p + E, 0, sizeof(uint32_t), st));
  AssignPassArgs P{lse_p.p, n_asg.p, cnt.p, nullptr, nullptr, nullptr};
  if (lds) launch_assign_enc<true>(h, gs, A, P, false);
  else launch_assign_enc<false>(h, gs, A, P, false);
  size_t tmp_bytes = 0;
  MSW_HIP(prim_scan(nullptr, tmp_bytes, cnt.p, off.p, (size_t)E + 1, st));
  DevBuf<uint8_t> tmp;
  assign_alloc(tmp, tmp_bytes, "scan storage");
  MSW_HIP(prim_scan(tmp.p, tmp_bytes, cnt.p, off.p, (size_t)E + 1, st));
  uint64_t n_pairs = 0;
  MSW_HIP(hipMemcpyAsync(&n_pairs, off.p + E, sizeof n_pairs, hipMemcpyDeviceToHost, st));
  if (n_assigned_out && E) MSW_HIP(hipMemcpyAsync(n_assigned_out, n_asg.p, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (class_reads_out) {
    DevBuf<unsigned long long> d_cls;
    assign_alloc(d_cls, 3, "the class sums");
    MSW_HIP(hipMemsetAsync(d_cls.p, 0, 3 * sizeof(unsigned long long), st));
    const unsigned nbc = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)E + 255) / 256, (size_t)h->n_cu * 8));
    hipLaunchKernelGGL(k_assign_class_reads, dim3(nbc), dim3(256), 0, st, n_asg.p, d_rptr, E, d_cls.p);
    MSW_HIP(hipGetLastError());
    unsigned long long cls[3] = {0, 0, 0};
    MSW_HIP(hipMemcpyAsync(cls, d_cls.p, sizeof cls, hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < 3; ++c) class_reads_out[c] = cls[c];
  }
  MSW_HIP(hipStreamSynchronize(st));

  // write pass, then the pairs by slot (stable: each bin's ECs stay in EC order; the unassigned slot sorts last).  The
  // pairs as written stay where they are: the table reads them by EC.
  DevBuf<uint32_t> key_own, val, key2, val2;
  DevBuf<uint32_t> &key = keep ? K.key : key_own;
  assign_alloc(key, n_pairs, "the (target, class) pairs");
  if (n_pairs) {
    assign_alloc(val, n_pairs, "the (target, class) pairs");
    assign_alloc(key2, n_pairs, "the sorted pairs");
    assign_alloc(val2, n_pairs, "the sorted pairs");
    P.off = off.p;
    P.key = key.p;
    P.val = val.p;
    if (lds) launch_assign_enc<true>(h, gs, A, P, true);
    else launch_assign_enc<false>(h, gs, A, P, true);
    unsigned bits = 1;
    while (bits < 32 && ((size_t)1 << bits) < n_slots) ++bits;
    MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, key.p, key2.p, val.p, val2.p, (size_t)n_pairs, bits, st));
    assign_alloc(tmp, tmp_bytes, "sort storage");
    MSW_HIP(prim_sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, val.p, val2.p, (size_t)n_pairs, bits, st));

    // output offsets of the sorted pairs (roff[n_pairs] = the reads in all bins) and bin_ptr
    DevBuf<uint64_t> roff, d_bin_ptr;
    assign_alloc(roff, n_pairs + 1, "the output offsets");
    assign_alloc(d_bin_ptr, n_slots + 1, "bin_ptr");
    const BinPairLen lens{val2.p, d_rptr, (size_t)n_pairs};
    MSW_HIP(prim_scan(nullptr, tmp_bytes, lens, roff.p, (size_t)n_pairs + 1, st));
    assign_alloc(tmp, tmp_bytes, "scan storage");
    MSW_HIP(prim_scan(tmp.p, tmp_bytes, lens, roff.p, (size_t)n_pairs + 1, st));
    hipLaunchKernelGGL(k_bin_ptr, dim3((unsigned)((n_slots + 1 + 255) / 256)), dim3(256), 0, st, key2.p, (size_t)n_pairs, roff.p,
                       (uint32_t)n_slots, d_bin_ptr.p);
    MSW_HIP(hipGetLastError());
    MSW_HIP(hipMemcpyAsync(bin_ptr, d_bin_ptr.p, (n_slots + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    const uint64_t total = bin_ptr[n_slots];
    if (reads_out && total) {
      DevBuf<uint32_t> out;
      assign_alloc(out, total, "the binned read ids");
      const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_pairs + 255) / 256, (uint64_t)h->n_cu * 16));
      hipLaunchKernelGGL(k_bin_scatter, dim3(nb), dim3(256), 0, st, val2.p, (size_t)n_pairs, d_rptr, d_reads, roff.p, out.p);
      MSW_HIP(hipGetLastError());
      MSW_HIP(hipMemcpyAsync(reads_out, out.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      MSW_HIP(hipStreamSynchronize(st));
    }
  }
  if (!keep) return;

  // the reads by id: (read id, EC) of every read position, in a stable sort by id
  reads_by_id(h, d_rptr, d_reads, E, n_rows, K.id, K.ec, "msw_core_assign_reads");
  K.n_rows = n_rows;
  K.n_targets = (uint32_t)n_targets;
  K.have = true;
}

void assign_reads_aln_impl(msw_core *h, msw_alignment *a, const double *thresholds, const uint32_t *targets, size_t n_targets,
                           unsigned flags, uint64_t *bin_ptr, uint32_t *reads_out, uint32_t *n_assigned_out,
                           uint64_t *class_reads_out) {
  if (!a) throw Fail("msw_core_assign_reads_aln: null alignment");
  if (a->on_device && a->device == h->device) {
    // the reader's classes are read where they lie
    assign_reads_impl(h, a->d_rptr.p, a->d_reads.p, a->E, true, thresholds, targets, n_targets, flags, bin_ptr, reads_out,
                      n_assigned_out, class_reads_out);
  } else {
    a->to_host(msw_alignment::kAlnRptr | msw_alignment::kAlnReads);
    assign_reads_impl(h, a->ec_rptr.data(), a->ec_reads.data(), a->ec_rptr.empty() ? 0 : a->ec_rptr.size() - 1, false,
                      thresholds, targets, n_targets, flags, bin_ptr, reads_out, n_assigned_out, class_reads_out);
  }
}

// ---- the table --------------------------------------------------------------------------------------------------------
void assign_table_check(msw_core *h, const char *who, size_t r0, size_t r1) {
  const AssignState &K = h->assign;
  if (!K.have)
    throw Fail(std::string(who) + ": no assignment table is kept on this handle (msw_core_assign_reads with "
               "MSW_ASSIGN_KEEP_TABLE; a new likelihood, a solve or a bootstrap drops it)");
  if (r0 > r1 || r1 > K.n_rows) throw Fail(std::string(who) + ": row range out of bounds (" + std::to_string(K.n_rows) + " rows)");
  const size_t per_row = 11 + 2 * (size_t)K.n_targets;  // ten digits, "\t0" per target, the line end
  if ((unsigned __int128)per_row * (r1 - r0) > kAssignMaxBytes)
    throw Fail(std::string(who) + ": the text of " + std::to_string(r1 - r0) + " rows can exceed 1 GiB; at most " +
               std::to_string(kAssignMaxBytes / per_row) + " rows of " + std::to_string(K.n_targets) + " targets fit one call");
}

// The text of the rows [r0, r1) into K.text (16-byte aligned, readable up to the next multiple of 4): length pass, scan,
// write pass.  Returns its length, the stream synchronised.
size_t assign_table_text(msw_core *h, size_t r0, size_t r1) {
  AssignState &K = h->assign;
  hipStream_t st = h->stream;
  const size_t n = r1 - r0;
  if (n == 0) return 0;
  assign_alloc(K.len, n + 1, "the row lengths");
  assign_alloc(K.toff, n + 1, "the row offsets");
  const AssignTable T{K.id.p + r0, K.ec.p + r0, K.off.p, K.key.p, K.n_targets, (uint32_t)n};
  MSW_HIP(hipMemsetAsync(K.len.p + n, 0, sizeof(uint32_t), st));
  const unsigned nbl = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 8));
  hipLaunchKernelGGL(k_assign_table_len, dim3(nbl), dim3(256), 0, st, T, K.len.p);
  MSW_HIP(hipGetLastError());
  size_t tmp_bytes = 0;
  MSW_HIP(prim_scan(nullptr, tmp_bytes, K.len.p, K.toff.p, n + 1, st));
  assign_alloc(K.tmp, tmp_bytes, "scan storage");
  MSW_HIP(prim_scan(K.tmp.p, tmp_bytes, K.len.p, K.toff.p, n + 1, st));
  uint64_t total = 0;
  MSW_HIP(hipMemcpyAsync(&total, K.toff.p + n, sizeof total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  assign_alloc(K.text, (total + 3) & ~(uint64_t)3, "the text");
  // lanes per row: a lane takes about two 4-byte words of the widest row (1 ... 64 lanes, a power of two)
  const size_t words = (11 + 2 * (size_t)K.n_targets + 3) / 4;
  uint32_t lg = 0;
  while (lg < 6 && ((size_t)2 << lg) < words) ++lg;
  const size_t rows = (size_t)256 >> lg;
  const unsigned nbw = (unsigned)std::max<size_t>(1, std::min<size_t>((n + rows - 1) / rows, (size_t)h->n_cu * 16));
  hipLaunchKernelGGL(k_assign_table_write, dim3(nbw), dim3(256), 0, st, T, K.toff.p, lg, K.text.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(st));
  return (size_t)total;
}

void assign_table_plain(msw_core *h, size_t r0, size_t r1, const char **text_out, size_t *len_out) {
  if (!text_out || !len_out) throw Fail("msw_core_assign_table_block: null text_out or len_out");
  assign_table_check(h, "msw_core_assign_table_block", r0, r1);
  const size_t total = assign_table_text(h, r0, r1);
  PinnedBuf &B = h->text.pinned;
  pinned_reserve(B, std::max<size_t>(total, 1), 0);  // an empty text still points somewhere
  if (total) {
    MSW_HIP(hipMemcpyAsync(B.p, h->assign.text.p, total, hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
  }
  *text_out = B.p;
  *len_out = total;
}

void assign_table_gzip(msw_core *h, size_t r0, size_t r1, const char **out, size_t *len_out, size_t *text_len_out) {
  if (!out || !len_out) throw Fail("msw_core_assign_table_block_gzip: null out or len_out");
  gz_require_open(h, "msw_core_assign_table_block_gzip");
  assign_table_check(h, "msw_core_assign_table_block_gzip", r0, r1);
  size_t used = 0, total = 0;
  if (h->gz.host) {  // MSWEEP_HOST_GZIP=1: the plain text through zlib
    const char *text = nullptr;
    assign_table_plain(h, r0, r1, &text, &total);
    if (total) used = gz_host_deflate(h, text, total, Z_NO_FLUSH, 0);
  } else {
    total = assign_table_text(h, r0, r1);
    used = gz_compress_device(h, h->assign.text.p, total, 0);
  }
  gz_return(h, used, out, len_out);
  if (text_len_out) *text_len_out = total;
}

}  // namespace
