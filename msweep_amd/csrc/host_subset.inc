// host_subset.inc -- msw_alignment_subset (included by input.hip behind host_reader.inc; kernels: subset_kernels.hpp):
// an alignment restricted to a set of reads and a set of target sequences and collapsed into equivalence classes again.
// The outcome is the reader's on the text that names every selected read with the kept targets of its class, the kept
// targets renumbered by rank (include/msweep_core.h states the contract); the classes are those of collapse() /
// device_collapse over the renumbered lists.  Two paths with the same outcome, array for array
// (tests/test_gpu_alignment_subset.py): plain loops over the host arrays, and the kernels over the resident ones.
namespace {

// what both paths refuse, and n_keep
size_t subset_check_args(const msw_alignment *a, const uint32_t *read_ids, size_t n_ids, const uint8_t *keep, const void *out) {
  if (!a || !out || !keep) throw Fail("msw_alignment_subset: null argument");
  if (n_ids && !read_ids) throw Fail("msw_alignment_subset: null read_ids");
  if (n_ids > 0xffffffffull) throw Fail("msw_alignment_subset: more read ids than 32 bits name");
  size_t n_keep = 0;
  for (size_t t = 0; t < a->n_targets; ++t) n_keep += keep[t] != 0;
  if (!n_keep) throw Fail("msw_alignment_subset: keep_target keeps no target sequence");
  return n_keep;
}
[[noreturn]] void subset_fail_twice(uint32_t id) {
  throw Fail("msw_alignment_subset: read id " + std::to_string(id) + " is listed twice");
}

// ---- the host path --------------------------------------------------------------------------------------------------------
void subset_host(msw_alignment &a, const uint32_t *read_ids, size_t n_ids, const uint8_t *keep, size_t n_keep, msw_alignment &out) {
  a.to_host(31u);
  out.n_targets = n_keep;
  out.n_queries = n_ids;
  uint32_t max_id = 0;
  for (size_t i = 0; i < n_ids; ++i) max_id = std::max(max_id, read_ids[i]);
  std::vector<uint64_t> bits(n_ids ? ((size_t)max_id >> 6) + 1 : 0, 0);
  uint64_t dup_min = ~0ull;
  for (size_t i = 0; i < n_ids; ++i) {
    const uint32_t id = read_ids[i];
    const uint64_t bit = 1ull << (id & 63);
    if (bits[id >> 6] & bit) dup_min = std::min<uint64_t>(dup_min, id);
    bits[id >> 6] |= bit;
  }
  if (dup_min != ~0ull) subset_fail_twice((uint32_t)dup_min);
  std::vector<uint32_t> rank(a.n_targets, 0);
  for (size_t t = 0, r = 0; t < a.n_targets; ++t) {
    rank[t] = (uint32_t)r;
    r += keep[t] != 0;
  }
  // every class's list filtered and renumbered, and its hash
  const size_t E = a.E;
  std::vector<uint64_t> fptr(E + 1, 0), hkey(E, 0);
  for (size_t e = 0; e < E; ++e) {
    uint64_t n = 0;
    for (uint64_t k = a.ec_tptr[e]; k < a.ec_tptr[e + 1]; ++k) n += keep[a.ec_targets[k]] != 0;
    fptr[e + 1] = fptr[e] + n;
  }
  uvec<uint32_t> ftgt(fptr[E]);
  for (size_t e = 0; e < E; ++e) {
    uint64_t w = fptr[e], h = 0;
    for (uint64_t k = a.ec_tptr[e]; k < a.ec_tptr[e + 1]; ++k) {
      const uint32_t t = a.ec_targets[k];
      if (!keep[t]) continue;
      ftgt[w++] = rank[t];
      h ^= (uint64_t)rank[t] + 0x517cc1b727220a95ull + (h << 6) + (h >> 2);
    }
    hkey[e] = h;
  }
  // the selected reads whose class keeps a target, keyed by the class's new hash
  const uint64_t n_space = n_ids ? (uint64_t)max_id + 1 : 0;  // (a subset's read ids are not bounded by its n_reads)
  std::vector<uint32_t> cls(n_space, 0);
  uvec<Keyed> keyed;
  {
    size_t K = 0;
    for (int pass = 0; pass < 2; ++pass) {
      if (pass) keyed.resize(K);
      size_t w = 0;
      for (size_t e = 0; e < E; ++e) {
        if (fptr[e + 1] == fptr[e]) continue;
        for (uint64_t k = a.ec_rptr[e]; k < a.ec_rptr[e + 1]; ++k) {
          const uint32_t id = a.ec_reads[k];
          if (id >= n_space || !(bits[id >> 6] >> (id & 63) & 1u)) continue;
          if (pass) {
            keyed[w] = Keyed{hkey[e], id};
            cls[id] = (uint32_t)e;
          }
          ++w;
        }
      }
      K = w;
    }
  }
  sort_keyed(keyed, 1);
  const size_t K = keyed.size();
  size_t En = 0;
  for (size_t k = 0; k < K; ++k) En += k == 0 || keyed[k].first != keyed[k - 1].first;
  out.ec_tptr.assign(En + 1, 0);
  out.ec_rptr.assign(En + 1, 0);
  out.ec_counts.assign(En, 0);
  out.ec_reads.resize(K);
  for (size_t k = 0, e = 0; k < K; ++k) {
    out.ec_reads[k] = keyed[k].second;
    if (k == 0 || keyed[k].first != keyed[k - 1].first) {
      const uint32_t c = cls[keyed[k].second];  // the class of the representative: the smallest read id
      out.ec_rptr[e] = k;
      out.ec_tptr[e + 1] = fptr[c + 1] - fptr[c];
      ++e;
    }
  }
  out.ec_rptr[En] = K;
  for (size_t e = 0; e < En; ++e) {
    out.ec_counts[e] = out.ec_rptr[e + 1] - out.ec_rptr[e];
    out.ec_tptr[e + 1] += out.ec_tptr[e];
  }
  out.ec_targets.resize(out.ec_tptr[En]);
  for (size_t e = 0; e < En; ++e) {
    const uint32_t c = cls[out.ec_reads[out.ec_rptr[e]]];
    if (fptr[c + 1] != fptr[c])
      std::memcpy(out.ec_targets.data() + out.ec_tptr[e], ftgt.data() + fptr[c], (size_t)(fptr[c + 1] - fptr[c]) * sizeof(uint32_t));
  }
  out.E = En, out.H = out.ec_tptr[En], out.K = K;
}

// ---- the device path ------------------------------------------------------------------------------------------------------
// a failed allocation is an error that names the bytes: nothing here falls back
template <class B>
void subset_alloc(B &b, size_t count, const char *what) {
  try {
    b.alloc(count);
  } catch (const HipError &ex) {
    (void)hipGetLastError();
    throw Fail("msw_alignment_subset: cannot allocate " + std::to_string(std::max<size_t>(count, 1) * sizeof(*b.p)) +
               " bytes of device memory for " + what + " (" + ex.what() + ")");
  }
}
void subset_scan(const uint32_t *in, uint64_t *out, size_t n, ReaderCtx &cx) {
  if (!n) return;
  size_t bytes = 0;
  MSW_HIP(prim_scan(nullptr, bytes, in, out, n, cx.st));
  subset_alloc(cx.tmp, bytes, "the scan");
  MSW_HIP(prim_scan(cx.tmp.p, bytes, in, out, n, cx.st));
}

void subset_device(msw_handle h, const msw_alignment &a, const uint32_t *read_ids, size_t n_ids, const uint8_t *keep, size_t n_keep,
                   msw_alignment &out) {
  hipStream_t st = h->stream;
  MSW_HIP(hipStreamSynchronize(st));
  h->reader_pool.recycle();  // (blocks an earlier call handed back: nothing of them is in flight any more)
  ReaderCtx cx(st, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
  cx.timing = getenv("MSWEEP_BUILD_TIMING") != nullptr;
  cx.t0 = std::chrono::steady_clock::now();
  out.n_targets = n_keep;
  out.n_queries = n_ids;
  out.device = h->device;
  const uint64_t E = a.E, T = a.n_targets;
  // ---- the kept targets ranked; every class's list filtered, renumbered and hashed ----
  RBuf<uint8_t> d_keep(cx);
  RBuf<uint32_t> keepf(cx), flen(cx), ftgt(cx);
  RBuf<uint64_t> rank(cx), fptr(cx), hkey(cx);
  subset_alloc(d_keep, T, "keep_target");
  subset_alloc(keepf, T + 1, "the keep flags");
  subset_alloc(rank, T + 1, "the target ranks");
  MSW_HIP(hipMemcpyAsync(d_keep.p, keep, T, hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemsetAsync(keepf.p + T, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_subset_keep_flags, dim3(reader_grid(T, cx.n_cu)), dim3(256), 0, st, d_keep.p, T, keepf.p);
  MSW_HIP(hipGetLastError());
  subset_scan(keepf.p, rank.p, T + 1, cx);
  subset_alloc(flen, E + 1, "the filtered lengths");
  subset_alloc(fptr, E + 1, "the filtered row pointers");
  subset_alloc(hkey, E, "the class hashes");
  MSW_HIP(hipMemsetAsync(flen.p + E, 0, sizeof(uint32_t), st));
  if (E)
    hipLaunchKernelGGL(k_subset_filter<false>, dim3(reader_grid(E, cx.n_cu)), dim3(256), 0, st, a.d_tptr.p, a.d_targets.p, E, keepf.p,
                       rank.p, flen.p, (const uint64_t *)nullptr, (uint32_t *)nullptr);
  MSW_HIP(hipGetLastError());
  subset_scan(flen.p, fptr.p, E + 1, cx);
  const uint64_t FH = fetch_u64(fptr.p + E, st);
  subset_alloc(ftgt, FH, "the filtered target lists");
  if (E) {
    hipLaunchKernelGGL(k_subset_filter<true>, dim3(reader_grid(E, cx.n_cu)), dim3(256), 0, st, a.d_tptr.p, a.d_targets.p, E, keepf.p,
                       rank.p, (uint32_t *)nullptr, fptr.p, ftgt.p);
    hipLaunchKernelGGL(k_subset_hash, dim3(reader_grid(E, cx.n_cu)), dim3(256), 0, st, fptr.p, ftgt.p, E, hkey.p);
  }
  MSW_HIP(hipGetLastError());
  cx.mark("subset: filter + hash");
  // ---- the selection as a bitmap over the read ids; ids listed twice ----
  uint32_t max_id = 0;
  for (size_t i = 0; i < n_ids; ++i) max_id = std::max(max_id, read_ids[i]);
  const uint64_t n_words = n_ids ? ((uint64_t)max_id >> 5) + 1 : 1;
  const uint64_t n_space = n_ids ? (uint64_t)max_id + 1 : 0;  // (a subset's read ids are not bounded by its n_reads)
  RBuf<uint32_t> d_ids(cx), bits(cx), flag(cx), cls(cx), ids(cx), head(cx), tlen(cx);
  RBuf<uint64_t> idx(cx), keys(cx), keys2(cx), eidx(cx);
  RBuf<SubsetCtr> sctr(cx);
  subset_alloc(d_ids, n_ids, "the read ids");
  subset_alloc(bits, n_words, "the selection bitmap");
  subset_alloc(sctr, 1, "the counters");
  MSW_HIP(hipMemsetAsync(bits.p, 0, n_words * sizeof(uint32_t), st));
  const SubsetCtr c0 = {0xffffffffu, 0u};
  MSW_HIP(hipMemcpyAsync(sctr.p, &c0, sizeof c0, hipMemcpyHostToDevice, st));
  if (n_ids) {
    MSW_HIP(hipMemcpyAsync(d_ids.p, read_ids, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_subset_bitmap, dim3(reader_grid(n_ids, cx.n_cu)), dim3(256), 0, st, d_ids.p, (uint64_t)n_ids, bits.p, sctr.p);
    MSW_HIP(hipGetLastError());
  }
  SubsetCtr c1 = {};
  MSW_HIP(hipMemcpyAsync(&c1, sctr.p, sizeof c1, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  if (c1.n_dup) subset_fail_twice(c1.dup_min);
  // ---- device_collapse's sequence over the id space: flags, scan, keys, stable sort, heads, meta, rows ----
  subset_alloc(flag, n_space + 1, "the read flags");
  subset_alloc(cls, n_space + 1, "the reads' classes");
  subset_alloc(idx, n_space + 1, "the read positions");
  MSW_HIP(hipMemsetAsync(flag.p, 0, (n_space + 1) * sizeof(uint32_t), st));
  if (a.K && n_space)
    hipLaunchKernelGGL(k_subset_mark, dim3(reader_grid(a.K, cx.n_cu)), dim3(256), 0, st, a.d_rptr.p, a.d_reads.p, (uint64_t)a.K, E, bits.p,
                       n_space, flen.p, flag.p, cls.p);
  MSW_HIP(hipGetLastError());
  subset_scan(flag.p, idx.p, n_space + 1, cx);
  const uint64_t K = fetch_u64(idx.p + n_space, st);
  subset_alloc(keys, K, "the sort keys");
  subset_alloc(keys2, K, "the sorted keys");
  subset_alloc(ids, K, "the keyed read ids");
  subset_alloc(out.d_reads, K, "ec_reads");
  if (K) {
    hipLaunchKernelGGL(k_subset_keys, dim3(reader_grid(n_space, cx.n_cu)), dim3(256), 0, st, flag.p, idx.p, cls.p, hkey.p, n_space, keys.p,
                       ids.p);
    MSW_HIP(hipGetLastError());
    size_t bytes = 0;  // ascending hash; the sort is stable: read ids stay ascending inside a class
    MSW_HIP(prim_sort_pairs(nullptr, bytes, keys.p, keys2.p, ids.p, out.d_reads.p, (size_t)K, 64u, st));
    subset_alloc(cx.tmp, bytes, "the sort");
    MSW_HIP(prim_sort_pairs(cx.tmp.p, bytes, keys.p, keys2.p, ids.p, out.d_reads.p, (size_t)K, 64u, st));
  }
  cx.mark("subset: select + sort");
  subset_alloc(head, K + 1, "the class heads");
  subset_alloc(eidx, K + 1, "the class indices");
  MSW_HIP(hipMemsetAsync(head.p + K, 0, sizeof(uint32_t), st));
  if (K) hipLaunchKernelGGL(k_ec_heads, dim3(reader_grid(K, cx.n_cu)), dim3(256), 0, st, keys2.p, K, head.p);
  MSW_HIP(hipGetLastError());
  subset_scan(head.p, eidx.p, K + 1, cx);
  const uint64_t En = fetch_u64(eidx.p + K, st);
  subset_alloc(out.d_rptr, En + 1, "ec_rptr");
  subset_alloc(out.d_tptr, En + 1, "ec_tptr");
  subset_alloc(out.d_counts, En, "ec_counts");
  subset_alloc(tlen, En + 1, "the class lengths");
  MSW_HIP(hipMemsetAsync(tlen.p + En, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemcpyAsync(out.d_rptr.p + En, &K, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (K)
    hipLaunchKernelGGL(k_subset_meta, dim3(reader_grid(K, cx.n_cu)), dim3(256), 0, st, head.p, eidx.p, out.d_reads.p, cls.p, flen.p, K,
                       out.d_rptr.p, tlen.p);
  MSW_HIP(hipGetLastError());
  subset_scan(tlen.p, out.d_tptr.p, En + 1, cx);
  const uint64_t H = fetch_u64(out.d_tptr.p + En, st);  // (also: K has been read)
  subset_alloc(out.d_targets, H, "ec_targets");
  if (En)
    hipLaunchKernelGGL(k_subset_rows, dim3(reader_grid(En, cx.n_cu)), dim3(256), 0, st, out.d_rptr.p, out.d_reads.p, cls.p, fptr.p, ftgt.p,
                       out.d_tptr.p, En, out.d_counts.p, out.d_targets.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(st));
  out.E = En, out.H = H, out.K = K;
  out.on_device = true;
  out.host_have = 0u;
  cx.mark("subset: classes");
}

}  // namespace

extern "C" {

int msw_alignment_subset(msw_handle h, msw_alignment_t a, const uint32_t *read_ids, size_t n_ids, const uint8_t *keep_target,
                         msw_alignment_t *out, size_t *n_targets_out) {
  if (out) *out = nullptr;
  if (n_targets_out) *n_targets_out = 0;
  auto body = [&] {
    const size_t n_keep = subset_check_args(a, read_ids, n_ids, keep_target, out);
    if (a->on_device && !h) throw Fail("msw_alignment_subset: a device-resident alignment needs the handle of its device");
    if (a->on_device && a->device != h->device)
      throw Fail("msw_alignment_subset: the alignment is resident on device " + std::to_string(a->device) + ", the handle's is device " +
                 std::to_string(h->device));
    std::unique_ptr<msw_alignment> s(new msw_alignment);
    // MSWEEP_HOST_SUBSET=1 (developer switch, read at the call): the host loops also for a resident alignment
    const char *sw = getenv("MSWEEP_HOST_SUBSET");
    if (a->on_device && !(sw && atoi(sw) != 0)) subset_device(h, *a, read_ids, n_ids, keep_target, n_keep, *s);
    else subset_host(*a, read_ids, n_ids, keep_target, n_keep, *s);
    if (n_targets_out) *n_targets_out = n_keep;
    *out = s.release();
  };
  if (h) return guarded(h, body);
  try {  // no handle: a host-resident alignment, no GPU touched; the message is this thread's (msw_last_error(NULL))
    body();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    g_aln_error = ex.what();
    return 1;
  }
}

}  // extern "C"
