// host_text.inc -- msw_core_text_block / msw_core_format_g6 (included by output.hip): the text of the matrix
// outputs formatted on the device (text_kernels.hpp).  One pipeline per block of ECs, shared with the gzip stream
// (host_gzip.inc): materialise the G x w values where they lie (host_likelihood.inc), the length of every line, an
// exclusive scan, the write pass -- the block's FINISHED text (text_block_finish) -- and a sink: here one copy of the
// bytes to the handle's pinned buffer, there the compressor.  The few cells the device leaves undecided come back as
// (byte offset, bits): the host prints them (text_cells.hpp), k_text_close puts them in and closes the gaps; more of
// them than the list holds: the host formats the block.  Device memory: the block, its text and O(w) offsets.
namespace {

constexpr size_t kTextMaxBytes = (size_t)1 << 30;  // worst-case text of one call
constexpr uint32_t kTextListCap = 1u << 16;        // undecided cells of a block the list holds; more: the host formats the block

// MSWEEP_TEXT_HOST_CAP=n (developer switch, tests): a smaller list, to drive the whole-block host path
uint32_t text_list_cap() {
  const char *e = getenv("MSWEEP_TEXT_HOST_CAP");
  if (e && *e) return (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), kTextListCap);
  return kTextListCap;
}

}  // namespace

// room for `need` bytes in a pinned buffer, its first `keep` bytes kept
void msw::host::pinned_reserve(PinnedBuf &B, size_t need, size_t keep) {
  if (need <= B.cap) return;
  const size_t cap = std::max(need, B.cap + B.cap / 2);
  char *p = nullptr;
  if (hipHostMalloc((void **)&p, cap, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    throw Fail(std::string(B.who) + ": cannot allocate " + std::to_string(cap) + " bytes of pinned host memory for " + B.what);
  }
  if (keep) std::memcpy(p, B.p, keep);
  if (B.p) (void)hipHostFree(B.p);
  B.p = p;
  B.cap = cap;
}

namespace {

// off[i] = len[0] + ... + len[i - 1] for i in [0, n], len[n] a spare zero; `scanned` is recorded behind the scan, and
// off[n], the total, comes back with the stream synchronised
uint64_t scan_lengths(const uint32_t *len, uint64_t *off, size_t n, DevBuf<uint8_t> &tmp, hipEvent_t scanned, hipStream_t st) {
  size_t tmp_bytes = 0;
  MSW_HIP(prim_scan(nullptr, tmp_bytes, len, off, n + 1, st));
  tmp.alloc(tmp_bytes);
  MSW_HIP(prim_scan(tmp.p, tmp_bytes, len, off, n + 1, st));
  MSW_HIP(hipEventRecord(scanned, st));
  uint64_t total = 0;
  MSW_HIP(hipMemcpyAsync(&total, off + n, sizeof total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  return total;
}

size_t text_dec(char *p, uint64_t v) { return (size_t)snprintf(p, 24, "%llu", (unsigned long long)v); }

// the lines of a block on the host, from the values the device would format (whole-block path)
void text_render_host(int what, const std::vector<double> &val, uint32_t G, size_t w, uint64_t id0, const uint64_t *prefix,
                      size_t n_zero, std::string &s) {
  char b[32];
  for (size_t jj = 0; jj < w; ++jj) {
    if (what != kTextPlain) {
      s.append(b, text_dec(b, what == kTextProbs ? id0 + jj : (what == kTextLogl ? prefix[jj] : (uint64_t)G + 1)));
      if (what == kTextBitseq) s.push_back(' ');
    }
    for (uint32_t g = 0; g < G; ++g) {
      if (what == kTextBitseq) {
        s.append(b, text_dec(b, (uint64_t)g + 1));
        s.push_back(' ');
      } else if (what != kTextPlain) {
        s.push_back('\t');
      }
      uint64_t bits;
      std::memcpy(&bits, &val[(size_t)g * w + jj], sizeof bits);
      s.append(b, (size_t)g6::format_host(bits, b));
      if (what == kTextBitseq) s.push_back(' ');
    }
    if (what == kTextProbs) for (size_t z = 0; z < n_zero; ++z) s.append("\t0");
    s.append(what == kTextBitseq ? "0 -10000.00\n" : "\n");
  }
}

template <int WHAT>
void text_launch(msw_core *h, const TextJob &J, TextState &T, uint32_t cap, bool write) {
  if (!write) {
    const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)J.w + 255) / 256, (size_t)h->n_cu * 8));
    hipLaunchKernelGGL((k_text_len<WHAT>), dim3(nb), dim3(256), 0, h->stream, J, T.len.p);
  } else {
    const size_t tiles = ((size_t)J.w + kTextLines - 1) / kTextLines;
    const unsigned nb = (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)h->n_cu * 16));
    hipLaunchKernelGGL((k_text_write<WHAT>), dim3(nb), dim3(kTextThreads), 0, h->stream, J, T.off.p, T.out.p, T.list.p,
                       T.n_list.p, cap);
  }
  MSW_HIP(hipGetLastError());
}
void text_launch_what(msw_core *h, int what, const TextJob &J, TextState &T, uint32_t cap, bool write) {
  if (what == kTextProbs) text_launch<kTextProbs>(h, J, T, cap, write);
  else if (what == kTextLogl) text_launch<kTextLogl>(h, J, T, cap, write);
  else if (what == kTextBitseq) text_launch<kTextBitseq>(h, J, T, cap, write);
  else text_launch<kTextPlain>(h, J, T, cap, write);
}

// The text of the w lines whose values lie in T.val (G x w, group-major) into T.out: length pass, scan, write pass (left
// enqueued).  Returns its length, undecided cells still 13 blanks wide.  prefix: host pointer (LOGL) or null.
uint64_t text_block_device(msw_core *h, int what, uint32_t G, size_t w, uint64_t id0, const uint64_t *prefix, size_t n_zero,
                           uint32_t cap) {
  TextState &T = h->text;
  hipStream_t st = h->stream;
  TextJob J{T.val.p, G, (uint32_t)w, id0, nullptr, (uint32_t)n_zero};
  if (what == kTextLogl) {
    T.prefix.upload(prefix, w, st);
    J.prefix = T.prefix.p;
  }
  T.len.alloc(w + 1);
  T.off.alloc(w + 1);
  T.n_list.alloc(1);
  T.list.alloc(kTextListCap);
  MSW_HIP(hipMemsetAsync(T.len.p + w, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemsetAsync(T.n_list.p, 0, sizeof(uint32_t), st));
  for (auto &e : T.ev)
    if (!e) MSW_HIP(hipEventCreate(&e));
  MSW_HIP(hipEventRecord(T.ev[0], st));
  text_launch_what(h, what, J, T, cap, false);
  const uint64_t total = scan_lengths(T.len.p, T.off.p, w, T.tmp, T.ev[1], st);
  T.out.alloc((total + 3) & ~(uint64_t)3);
  MSW_HIP(hipEventRecord(T.ev[2], st));
  text_launch_what(h, what, J, T, cap, true);
  MSW_HIP(hipEventRecord(T.ev[3], st));
  return total;
}

// the finished text of a block, every cell printed: where it lies on the device (16-byte aligned, readable up to the
// next multiple of 4; T.out or T.closed, until the next block) or, from the whole-block host render, as host bytes
struct TextDone {
  const uint8_t *dev = nullptr;  // null: `host` holds the text
  std::string host;
  size_t len = 0;
};

// The block whose values lie in T.val, finished; the cells the host printed are added to n_host.
TextDone text_block_finish(msw_core *h, int what, uint32_t G, size_t w, uint64_t id0, const uint64_t *prefix, size_t n_zero,
                           size_t &n_host) {
  TextState &T = h->text;
  hipStream_t st = h->stream;
  const uint32_t cap = text_list_cap();
  const uint64_t total = text_block_device(h, what, G, w, id0, prefix, n_zero, cap);
  uint32_t n_list = 0;
  MSW_HIP(hipMemcpyAsync(&n_list, T.n_list.p, sizeof n_list, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  float ms_len = 0.f, ms_write = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms_len, T.ev[0], T.ev[1]));
  MSW_HIP(hipEventElapsedTime(&ms_write, T.ev[2], T.ev[3]));
  T.kernel_ms += (double)ms_len + (double)ms_write;
  T.bytes += total;
  TextDone D{T.out.p, std::string(), total};
  if (n_list == 0) return D;
  if (n_list > cap) {
    // more undecided cells than the list holds: the host formats this block from the values the device formatted
    // (PROBS: the device's exp of them)
    const size_t n = (size_t)G * w;
    if (what == kTextProbs) {
      hipLaunchKernelGGL(k_text_exp, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65536)), dim3(256), 0, st, T.val.p, n);
      MSW_HIP(hipGetLastError());
    }
    std::vector<double> val(n);
    MSW_HIP(hipMemcpyAsync(val.data(), T.val.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    D.host.reserve(total);
    text_render_host(what, val, G, w, id0, prefix, n_zero, D.host);
    if (D.host.size() > total) throw Fail("msw_core_text_block: the host's text of a block is longer than the device's");
    D.dev = nullptr;
    D.len = D.host.size();
    n_host += n;
    return D;
  }
  // the undecided cells in text order, printed here; k_text_close puts them in and closes the gaps
  std::vector<TextHostCell> cells(n_list);
  MSW_HIP(hipMemcpy(cells.data(), T.list.p, n_list * sizeof(TextHostCell), hipMemcpyDeviceToHost));
  std::sort(cells.begin(), cells.end(), [](const TextHostCell &a, const TextHostCell &b) { return a.off < b.off; });
  std::vector<TextFilledCell> filled;
  D.len = text_fill_cells(cells, total, filled);
  T.cells.upload(filled.data(), n_list, st);
  MSW_HIP(hipStreamSynchronize(st));  // (`filled` is pageable and goes with this call, also on a failure)
  T.closed.alloc((total + 3) & ~(uint64_t)3);
  hipLaunchKernelGGL(k_text_close, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + 255) / 256, (uint64_t)h->n_cu * 32))),
                     dim3(256), 0, st, T.out.p, total, T.cells.p, n_list, T.closed.p);
  MSW_HIP(hipGetLastError());
  D.dev = T.closed.p;
  n_host += n_list;
  return D;
}

// the plain sink: the finished text appended to the pinned buffer at `used`; returns the bytes appended
size_t text_sink_plain(msw_core *h, const TextDone &D, size_t used) {
  TextState &T = h->text;
  pinned_reserve(T.pinned, used + D.len, used);
  if (D.dev) {
    MSW_HIP(hipMemcpyAsync(T.pinned.p + used, D.dev, D.len, hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
  } else {
    std::memcpy(T.pinned.p + used, D.host.data(), D.len);
  }
  return D.len;
}

void text_return(msw_core *h, size_t used, size_t n_host, const char **text_out, size_t *len_out, size_t *n_host_out) {
  pinned_reserve(h->text.pinned, 1, 0);  // an empty text still points somewhere
  *text_out = h->text.pinned.p;
  *len_out = used;
  if (n_host_out) *n_host_out = n_host;
}

// the refusals of msw_core_text_block
void text_block_check(msw_core *h, int what, size_t e0, size_t e1, const uint64_t *prefix, size_t n_zero) {
  const Resident &L = h->lik;
  if (what != MSW_TEXT_PROBS && what != MSW_TEXT_LOGL && what != MSW_TEXT_BITSEQ)
    throw Fail("msw_core_text_block: unknown kind of text " + std::to_string(what));
  if (L.flavor < 0) throw Fail("msw_core_text_block: no likelihood resident");
  if (what == MSW_TEXT_PROBS && !h->solver.have_solution) throw Fail("msw_core_text_block: no solve has run on this handle");
  if (what == MSW_TEXT_LOGL && !prefix && e0 != e1) throw Fail("msw_core_text_block: the likelihood lines need line_prefix (the read count of every class)");
  if (what != MSW_TEXT_LOGL && prefix) throw Fail("msw_core_text_block: line_prefix is taken by MSW_TEXT_LOGL only");
  if (what != MSW_TEXT_PROBS && n_zero) throw Fail("msw_core_text_block: n_zero_cols is taken by MSW_TEXT_PROBS only");
  const uint32_t G = L.G, E = L.E;
  if (e0 > e1 || e1 > E) throw Fail("msw_core_text_block: EC range out of bounds");
  // the worst case of a line: 20 digits, 14 bytes per cell (BitSeq: the group number and a blank on top), the zero
  // columns, 12 bytes of suffix
  const size_t cell = what == MSW_TEXT_BITSEQ ? 15 + std::to_string((uint64_t)G + 1).size() : 14;
  const unsigned __int128 per_line = (unsigned __int128)20 + (unsigned __int128)cell * G + (unsigned __int128)2 * n_zero + 12;
  if (per_line * (e1 - e0) > kTextMaxBytes) {
    const size_t fit = per_line > kTextMaxBytes ? 0 : (size_t)(kTextMaxBytes / per_line);
    throw Fail("msw_core_text_block: the text of " + std::to_string(e1 - e0) + " classes can exceed 1 GiB; at most " +
               std::to_string(fit) + " classes of " + std::to_string(G) + " groups and " + std::to_string(n_zero) +
               " zero columns fit one call");
  }
}

// run(G, w, j0, prefix of the block): once per block of classes of [e0, e1), its values materialised in T.val
template <class F>
void text_block_each(msw_core *h, int what, size_t e0, size_t e1, const uint64_t *prefix, F &&run) {
  h->text.kernel_ms = 0.0;
  h->text.bytes = 0;
  if (e0 >= e1) return;
  const uint32_t G = h->lik.G;
  const bool gamma = what == MSW_TEXT_PROBS;
  MaterialiseArgs m;
  materialise_args(h, gamma, m);
  const size_t blk = std::max<size_t>(1, std::min<size_t>(e1 - e0, ((size_t)1 << 27) / std::max<uint32_t>(G, 1)));
  h->text.val.alloc((size_t)G * blk);
  for (size_t j0 = e0; j0 < e1; j0 += blk) {
    const size_t j1 = std::min(e1, j0 + blk);
    materialise_block(h, m, gamma, j0, j1, h->text.val.p);
    run(G, j1 - j0, j0, prefix ? prefix + (j0 - e0) : nullptr);
  }
}

void text_block_impl(msw_core *h, int what, size_t e0, size_t e1, const uint64_t *prefix, size_t n_zero,
                     const char **text_out, size_t *len_out, size_t *n_host_out) {
  if (!text_out || !len_out) throw Fail("msw_core_text_block: null text_out or len_out");
  text_block_check(h, what, e0, e1, prefix, n_zero);
  size_t used = 0, n_host = 0;
  text_block_each(h, what, e0, e1, prefix, [&](uint32_t G, size_t w, size_t j0, const uint64_t *pre) {
    used += text_sink_plain(h, text_block_finish(h, what, G, w, j0, pre, n_zero, n_host), used);
  });
  text_return(h, used, n_host, text_out, len_out, n_host_out);
}

void format_g6_impl(msw_core *h, const double *x, size_t n, const char **text_out, size_t *len_out, size_t *n_host_out) {
  if (!text_out || !len_out) throw Fail("msw_core_format_g6: null text_out or len_out");
  if (n && !x) throw Fail("msw_core_format_g6: null x");
  if (n > kTextMaxBytes / 14) throw Fail("msw_core_format_g6: at most " + std::to_string(kTextMaxBytes / 14) + " values fit one call");
  size_t used = 0, n_host = 0;
  h->text.kernel_ms = 0.0;
  h->text.bytes = 0;
  const size_t blk = (size_t)1 << 24;
  for (size_t i0 = 0; i0 < n; i0 += blk) {
    const size_t w = std::min(blk, n - i0);
    h->text.val.upload(x + i0, w, h->stream);
    used += text_sink_plain(h, text_block_finish(h, kTextPlain, 1, w, 0, nullptr, 0, n_host), used);
  }
  text_return(h, used, n_host, text_out, len_out, n_host_out);
}

}  // namespace
