// host_sparse_probs.inc -- msw_core_sparse_probs_* (included by output.hip, behind host_text.inc and host_gzip.inc):
// the read-to-group probabilities as sparse text, "id \t g \t g6(p) \n" per cell with gamma(g, j) >= log(tau)
// (sparse_probs_kernels.hpp, DESIGN.md 7k).  begin: the groups ordered by u, the count pass, the rows (ECs, or the aligned
// reads in id order: the index host_assign.inc builds) and the exclusive scans of their candidates and kept cells.
// next: a piece of whole rows -- candidates written, sorted by (row, g), judged, measured, cut at the last row end within
// max_bytes, written as text -- and a sink as host_text.inc's: the copy to the pinned text buffer or the compressor.
// Device memory: O(E) + O(rows) + O(candidates and text of a piece); nothing is sized by G x E.  A piece: 52 bytes per
// candidate (two keys, two places, gamma, the line's length, offset and value) beside its text; its rows are chosen for
// max_bytes / kSpLine KEPT cells (known per row since begin), so a piece of the drivers' 256 MiB holds about 17 M
// candidates, 0.9 GB -- a row's candidates exceed its kept cells only by the listed cells that fail inside the prefix.
namespace {

constexpr uint64_t kSpMaxCand = (uint64_t)1 << 31;  // candidates of one piece (their places are 32-bit values of the sort)
constexpr uint64_t kSpMaxRows = (uint64_t)1 << 30;  // rows of one piece (the row takes the bits above 33 of a key)
// The line a piece's rows are chosen by: id, group and value of a by-read line take 15 ... 20 bytes.  Shorter lines leave
// the piece below max_bytes, longer ones are cut off at the last row end that fits and formed again with the next piece.
constexpr uint64_t kSpLine = 16;
constexpr size_t kSpMaxBytes = (size_t)1 << 30;

template <class T>
void sp_alloc(DevBuf<T> &b, size_t count, const char *what) {
  named_alloc(b, count, "msw_core_sparse_probs", what);
}

// device time of a stretch of launches that ends in a synchronisation: open() in front of it, close() behind the sync
struct SpClock {
  SparseProbsState &P;
  hipStream_t st;
  SpClock(SparseProbsState &P_, hipStream_t st_) : P(P_), st(st_) {
    for (auto &e : P.ev)
      if (!e) MSW_HIP(hipEventCreate(&e));
  }
  void open() { MSW_HIP(hipEventRecord(P.ev[0], st)); }
  void stop() { MSW_HIP(hipEventRecord(P.ev[1], st)); }
  void close() {
    float ms = 0.f;
    MSW_HIP(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]));
    P.kernel_ms += (double)ms;
  }
};

unsigned sp_blocks(const msw_core *h, uint64_t n, unsigned per_cu) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)h->n_cu * per_cu));
}

void sp_scan(const uint32_t *len, uint64_t *off, size_t n, DevBuf<uint8_t> &tmp, hipStream_t st) {
  size_t tmp_bytes = 0;
  MSW_HIP(prim_scan(nullptr, tmp_bytes, len, off, n + 1, st));
  sp_alloc(tmp, tmp_bytes, "scan storage");
  MSW_HIP(prim_scan(tmp.p, tmp_bytes, len, off, n + 1, st));
}

SpRule sp_rule(const msw_core *h) {
  const SparseProbsState &P = h->sparse;
  return SpRule{P.a, h->lik.logzi, P.log_thr, P.u, P.us.p, P.order.p};
}

template <int ENC>
void sp_launch(msw_core *h, bool write, uint64_t r0, uint32_t n) {
  const Resident &L = h->lik;
  SparseProbsState &P = h->sparse;
  if (!write)
    hipLaunchKernelGGL((k_sp_count<ENC>), dim3(sp_blocks(h, L.E, 8)), dim3(256), 0, h->stream, sell_view(L, h->solver), sp_rule(h),
                       P.tref, P.lse_p.p, P.idx.p, P.idx2.p);
  else
    hipLaunchKernelGGL((k_sp_write<ENC>), dim3(sp_blocks(h, n, 8)), dim3(256), 0, h->stream, sell_view(L, h->solver), sp_rule(h),
                       h->iperm.p, P.lse_p.p, P.id.p ? P.ec.p : nullptr, P.coff.p, r0, n, P.key.p, P.idx.p, P.gam.p);
  MSW_HIP(hipGetLastError());
}
void sp_launch_enc(msw_core *h, bool write, uint64_t r0, uint32_t n) {
  const Resident &L = h->lik;
  if (L.enc == kEncValue) sp_launch<kEncValue>(h, write, r0, n);
  else if (L.wide()) sp_launch<kEncWide>(h, write, r0, n);
  else if (L.hybrid()) sp_launch<kEncIndex>(h, write, r0, n);
  else sp_launch<kEncNarrow>(h, write, r0, n);
}

void sparse_probs_begin_impl(msw_core *h, msw_alignment *a, double threshold, uint64_t *n_rows_out, double *log_thr_out) {
  const char *who = "msw_core_sparse_probs_begin";
  const Resident &L = h->lik;
  SparseProbsState &P = h->sparse;
  if (!n_rows_out) throw Fail(std::string(who) + ": null n_rows_out");
  if (!h->solver.have_solution) throw Fail(std::string(who) + ": no solve has run on this handle");
  if (h->comm) throw Fail(std::string(who) + ": not available on an EC-sharded handle (a communicator is set)");
  if (L.flavor != 0)
    throw Fail(std::string(who) + ": the resident likelihood has the dense flavour; the sparse probabilities need the CSR-of-ECs layout");
  if (!(threshold > 0.0 && threshold <= 1.0)) throw Fail(std::string(who) + ": the threshold is not in (0, 1]");
  const uint32_t G = L.G, E = L.E;
  const bool resident = a && a->on_device && a->device == h->device;
  if (a) {
    if (!resident) {
      a->to_host(msw_alignment::kAlnRptr | msw_alignment::kAlnReads);
      MSW_HIP(hipSetDevice(h->device));
    }
    const size_t n_ecs = resident ? a->E : (a->ec_rptr.empty() ? 0 : a->ec_rptr.size() - 1);
    if (n_ecs != E)
      throw Fail(std::string(who) + ": the alignment holds " + std::to_string(n_ecs) + " equivalence classes, the handle " +
                 std::to_string(E));
    if (!resident && a->ec_reads.size() != a->ec_rptr.back())
      throw Fail(std::string(who) + ": the alignment's read lists do not match their offsets");
  }
  P.drop();  // the arguments stand: what an earlier begin kept goes with this one
  hipStream_t st = h->stream;
  SpClock clock(P, st);
  P.kernel_ms = 0.0;
  P.bytes = 0;
  P.n_cells = 0;

  MaterialiseArgs m;
  materialise_args(h, true, m);  // (a, tref, u) of the last solve; the inverse permutation
  P.a = m.a;
  P.tref = m.tref;
  P.u = m.u;
  P.log_thr = std::log(threshold);

  // the groups by u descending: ties in ascending g (the sort is stable)
  DevBuf<uint64_t> okey, okey2;
  DevBuf<uint32_t> ogrp;
  sp_alloc(okey, G, "the group order");
  sp_alloc(okey2, G, "the group order");
  sp_alloc(ogrp, G, "the group order");
  sp_alloc(P.order, G, "the group order");
  sp_alloc(P.us, G, "the group order");
  clock.open();
  hipLaunchKernelGGL(k_sp_order_keys, dim3((G + 255) / 256), dim3(256), 0, st, P.u, G, okey.p, ogrp.p);
  MSW_HIP(hipGetLastError());
  size_t tmp_bytes = 0;
  MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, okey.p, okey2.p, ogrp.p, P.order.p, (size_t)G, 64u, st));
  sp_alloc(P.tmp, tmp_bytes, "sort storage");
  MSW_HIP(prim_sort_pairs(P.tmp.p, tmp_bytes, okey.p, okey2.p, ogrp.p, P.order.p, (size_t)G, 64u, st));
  hipLaunchKernelGGL(k_sp_gather, dim3((G + 255) / 256), dim3(256), 0, st, P.u, P.order.p, G, P.us.p);
  MSW_HIP(hipGetLastError());

  // count pass: candidates and kept cells of every EC (in P.idx / P.idx2 until the rows have taken them)
  sp_alloc(P.lse_p, E, "the normalisers");
  sp_alloc(P.idx, E, "the candidate counts");
  sp_alloc(P.idx2, E, "the kept counts");
  sp_launch_enc(h, false, 0, 0);
  clock.stop();
  MSW_HIP(hipStreamSynchronize(st));
  clock.close();

  // the rows
  uint64_t n_rows = E;
  if (a) {
    DevBuf<uint64_t> d_rptr_own;
    DevBuf<uint32_t> d_reads_own;
    const uint64_t *d_rptr = nullptr;
    const uint32_t *d_reads = nullptr;
    if (resident) {
      d_rptr = a->d_rptr.p;
      d_reads = a->d_reads.p;
      n_rows = a->K;
    } else {
      n_rows = a->ec_rptr.back();
      if (a->ec_rptr[0] != 0) throw Fail(std::string(who) + ": ec_rptr[0] != 0");
      for (size_t j = 0; j < E; ++j)
        if (a->ec_rptr[j + 1] < a->ec_rptr[j]) throw Fail(std::string(who) + ": ec_rptr is not ascending");
      sp_alloc(d_rptr_own, (size_t)E + 1, "ec_rptr");
      sp_alloc(d_reads_own, n_rows, "ec_reads");
      MSW_HIP(hipMemcpyAsync(d_rptr_own.p, a->ec_rptr.data(), ((size_t)E + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      if (n_rows) MSW_HIP(hipMemcpyAsync(d_reads_own.p, a->ec_reads.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      MSW_HIP(hipStreamSynchronize(st));
      d_rptr = d_rptr_own.p;
      d_reads = d_reads_own.p;
    }
    sp_alloc(P.id, n_rows, "the reads by id");  // (also with no row: its pointer says "by read")
    sp_alloc(P.ec, n_rows, "the reads by id");
    reads_by_id(h, d_rptr, d_reads, E, n_rows, P.id, P.ec, who);
  }
  DevBuf<uint32_t> rc, rk;
  sp_alloc(rc, n_rows + 1, "the rows' candidate counts");
  sp_alloc(rk, n_rows + 1, "the rows' kept counts");
  sp_alloc(P.coff, n_rows + 1, "the rows' candidate offsets");
  sp_alloc(P.koff, n_rows + 1, "the rows' kept offsets");
  clock.open();
  hipLaunchKernelGGL(k_sp_rows, dim3(sp_blocks(h, n_rows + 1, 16)), dim3(256), 0, st, a ? P.ec.p : nullptr, P.idx.p, P.idx2.p, n_rows,
                     rc.p, rk.p);
  MSW_HIP(hipGetLastError());
  sp_scan(rc.p, P.coff.p, n_rows, P.tmp, st);
  sp_scan(rk.p, P.koff.p, n_rows, P.tmp, st);
  clock.stop();
  MSW_HIP(hipStreamSynchronize(st));
  clock.close();
  P.n_rows = n_rows;
  P.cur = 0;
  P.have = true;
  *n_rows_out = n_rows;
  if (log_thr_out) *log_thr_out = P.log_thr;
}

// the lines of the kept candidates [0, n_use) of a piece on the host, from what the device judged (more undecided cells
// than the list holds)
void sp_render_host(msw_core *h, uint64_t r0, uint32_t n_use, std::string &s) {
  SparseProbsState &P = h->sparse;
  std::vector<uint64_t> key(n_use), pbits(n_use);
  std::vector<uint32_t> elen(n_use), ids;
  MSW_HIP(hipMemcpy(key.data(), P.key2.p, (size_t)n_use * sizeof(uint64_t), hipMemcpyDeviceToHost));
  MSW_HIP(hipMemcpy(pbits.data(), P.pbits.p, (size_t)n_use * sizeof(uint64_t), hipMemcpyDeviceToHost));
  MSW_HIP(hipMemcpy(elen.data(), P.elen.p, (size_t)n_use * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const uint64_t rows = n_use ? (key[n_use - 1] >> kSpRowShift) + 1 : 0;
  if (P.id.p && rows) {
    ids.resize(rows);
    MSW_HIP(hipMemcpy(ids.data(), P.id.p + r0, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  char b[32];
  for (uint32_t i = 0; i < n_use; ++i) {
    if (!elen[i]) continue;
    const uint64_t row = key[i] >> kSpRowShift;
    s.append(b, text_dec(b, P.id.p ? (uint64_t)ids[row] : r0 + row));
    s.push_back('\t');
    s.append(b, text_dec(b, (uint32_t)(key[i] >> 1)));
    s.push_back('\t');
    s.append(b, (size_t)g6::format_host(pbits[i], b));
    s.push_back('\n');
  }
}

void sparse_probs_next_impl(msw_core *h, size_t max_bytes, bool gz, const char **out, size_t *len_out, uint64_t *rows_done_out,
                            uint64_t *n_cells_out, size_t *n_host_out, size_t *text_len_out) {
  const char *who = gz ? "msw_core_sparse_probs_next_gzip" : "msw_core_sparse_probs_next";
  SparseProbsState &P = h->sparse;
  if (!out || !len_out || !rows_done_out) throw Fail(std::string(who) + ": null out, len_out or rows_done_out");
  if (!P.have)
    throw Fail(std::string(who) + ": no selection on this handle (msw_core_sparse_probs_begin; a new likelihood, a solve, a "
               "bootstrap or msw_core_trim drops it)");
  if (max_bytes == 0 || max_bytes > kSpMaxBytes) throw Fail(std::string(who) + ": max_bytes is outside 1 ... 1 GiB");
  if (gz) gz_require_open(h, who);
  hipStream_t st = h->stream;
  SpClock clock(P, st);
  TextDone D;
  size_t n_host = 0;
  uint64_t n_cells = 0, r1 = P.cur;
  if (P.cur < P.n_rows) {
    const uint64_t r0 = P.cur;
    // the rows of the piece: about max_bytes of text by their kept cells, and no more candidates than a piece holds
    uint64_t span[5] = {0, 0, 0, 0, 0};
    sp_alloc(P.span, 5, "the piece");
    const uint64_t budget = std::max<uint64_t>(max_bytes / kSpLine, 1);
    clock.open();
    hipLaunchKernelGGL(k_sp_span, dim3(1), dim3(1), 0, st, P.koff.p, P.coff.p, r0, std::min(P.n_rows, r0 + kSpMaxRows), budget, kSpMaxCand,
                       P.span.p);
    MSW_HIP(hipGetLastError());
    clock.stop();
    MSW_HIP(hipMemcpyAsync(span, P.span.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    clock.close();
    const uint64_t r1p = span[0], n_cand = span[1];
    if (r1p <= r0 || r1p > P.n_rows) throw Fail(std::string(who) + ": internal: the piece's rows are out of range");
    if (n_cand > kSpMaxCand)
      throw Fail(std::string(who) + ": row " + std::to_string(r0) + " alone has " + std::to_string(n_cand) +
                 " candidate cells, more than a piece holds");
    r1 = r1p;
    if (n_cand) {
      const uint32_t nc = (uint32_t)n_cand, nr = (uint32_t)(r1p - r0);
      sp_alloc(P.key, n_cand, "the candidates");
      sp_alloc(P.key2, n_cand, "the sorted candidates");
      sp_alloc(P.idx, n_cand, "the candidates");
      sp_alloc(P.idx2, n_cand, "the sorted candidates");
      sp_alloc(P.gam, n_cand, "the candidates' values");
      sp_alloc(P.elen, n_cand + 1, "the line lengths");
      sp_alloc(P.eoff, n_cand + 1, "the line offsets");
      sp_alloc(P.pbits, n_cand, "the cells' values");
      sp_alloc(P.n_list, 1, "the undecided cells");
      sp_alloc(P.list, kTextListCap, "the undecided cells");
      clock.open();
      // (a slot the write pass leaves out -- none, unless the two passes disagree -- names no row of the piece)
      MSW_HIP(hipMemsetAsync(P.key.p, 0xff, n_cand * sizeof(uint64_t), st));
      MSW_HIP(hipMemsetAsync(P.idx.p, 0xff, n_cand * sizeof(uint32_t), st));
      sp_launch_enc(h, true, r0, nr);
      unsigned bits = kSpRowShift + 1;
      while (bits < 64 && ((uint64_t)1 << (bits - kSpRowShift)) < (uint64_t)nr) ++bits;
      size_t tmp_bytes = 0;
      MSW_HIP(prim_sort_pairs(nullptr, tmp_bytes, P.key.p, P.key2.p, P.idx.p, P.idx2.p, (size_t)n_cand, bits, st));
      sp_alloc(P.tmp, tmp_bytes, "sort storage");
      MSW_HIP(prim_sort_pairs(P.tmp.p, tmp_bytes, P.key.p, P.key2.p, P.idx.p, P.idx2.p, (size_t)n_cand, bits, st));
      const SpPiece piece{P.key2.p, P.idx2.p, nc, nr, r0, P.id.p};
      MSW_HIP(hipMemsetAsync(P.elen.p + n_cand, 0, sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_sp_len, dim3(sp_blocks(h, n_cand, 16)), dim3(256), 0, st, piece, P.gam.p, P.log_thr, P.elen.p, P.pbits.p);
      MSW_HIP(hipGetLastError());
      sp_scan(P.elen.p, P.eoff.p, n_cand, P.tmp, st);
      hipLaunchKernelGGL(k_sp_cut, dim3(1), dim3(1), 0, st, P.coff.p, P.koff.p, r0, r1p, P.eoff.p, (uint64_t)max_bytes, P.span.p);
      MSW_HIP(hipGetLastError());
      clock.stop();
      MSW_HIP(hipMemcpyAsync(span, P.span.p, sizeof span, hipMemcpyDeviceToHost, st));
      MSW_HIP(hipStreamSynchronize(st));
      clock.close();
      r1 = span[0];
      const uint64_t n_use = span[1], total = span[2];
      n_cells = span[4];
      if (r1 < r0 || r1 > r1p || n_use > n_cand || total > max_bytes) throw Fail(std::string(who) + ": internal: the piece's cut is out of range");
      if (r1 == r0)
        throw Fail(std::string(who) + ": row " + std::to_string(r0) + " has " + std::to_string(span[3]) +
                   " bytes of text, more than max_bytes = " + std::to_string(max_bytes));
      if (total) {
        const uint32_t cap = text_list_cap();
        sp_alloc(P.text, ((total + 15) & ~(uint64_t)15) + 16, "the text");
        MSW_HIP(hipMemsetAsync(P.n_list.p, 0, sizeof(uint32_t), st));
        clock.open();
        hipLaunchKernelGGL(k_sp_text, dim3(sp_blocks(h, n_use, 16)), dim3(256), 0, st, piece, (uint32_t)n_use, P.elen.p, P.eoff.p,
                           P.pbits.p, P.text.p, P.list.p, P.n_list.p, cap);
        MSW_HIP(hipGetLastError());
        clock.stop();
        uint32_t n_list = 0;
        MSW_HIP(hipMemcpyAsync(&n_list, P.n_list.p, sizeof n_list, hipMemcpyDeviceToHost, st));
        MSW_HIP(hipStreamSynchronize(st));
        clock.close();
        D.dev = P.text.p;
        D.len = total;
        if (n_list > cap) {
          D.host.reserve(total);
          sp_render_host(h, r0, (uint32_t)n_use, D.host);
          if (D.host.size() > total) throw Fail(std::string(who) + ": the host's text of a piece is longer than the device's");
          D.dev = nullptr;
          D.len = D.host.size();
          n_host = n_cells;
        } else if (n_list) {
          // the undecided cells in text order, printed here; k_text_close puts them in and closes the gaps
          std::vector<TextHostCell> cells(n_list);
          MSW_HIP(hipMemcpy(cells.data(), P.list.p, n_list * sizeof(TextHostCell), hipMemcpyDeviceToHost));
          std::sort(cells.begin(), cells.end(), [](const TextHostCell &x, const TextHostCell &y) { return x.off < y.off; });
          std::vector<TextFilledCell> filled;
          D.len = text_fill_cells(cells, total, filled);
          sp_alloc(P.cells, n_list, "the undecided cells");
          MSW_HIP(hipMemcpyAsync(P.cells.p, filled.data(), n_list * sizeof(TextFilledCell), hipMemcpyHostToDevice, st));
          MSW_HIP(hipStreamSynchronize(st));
          sp_alloc(P.closed, ((total + 15) & ~(uint64_t)15) + 16, "the text");
          hipLaunchKernelGGL(k_text_close, dim3(sp_blocks(h, total, 32)), dim3(256), 0, st, P.text.p, total, P.cells.p, n_list, P.closed.p);
          MSW_HIP(hipGetLastError());
          D.dev = P.closed.p;
          n_host = n_list;
        }
      }
    }
  }
  size_t used = 0;
  if (gz) {
    if (h->gz.host) {
      const size_t n = D.len ? text_sink_plain(h, D, 0) : 0;
      if (n) used = gz_host_deflate(h, h->text.pinned.p, n, Z_NO_FLUSH, 0);
    } else if (D.len) {
      used = text_sink_gzip(h, D, 0);
    }
    gz_return(h, used, out, len_out);
    if (text_len_out) *text_len_out = D.len;
  } else {
    if (D.len) used = text_sink_plain(h, D, 0);
    text_return(h, used, n_host, out, len_out, nullptr);
  }
  P.cur = r1;  // (only now: a piece that failed is handed out again)
  P.n_cells += n_cells;
  P.bytes += D.len;
  *rows_done_out = r1;
  if (n_cells_out) *n_cells_out = n_cells;
  if (n_host_out) *n_host_out = n_host;
}

}  // namespace
