// host_text.inc -- msw_core_text_block / msw_core_format_g6 (included by msweep_core.hip): the text of the matrix
// outputs formatted on the device (text_kernels.hpp).  Per block of ECs: materialise the G x w values where they lie
// (host_likelihood.inc), the length of every line, an exclusive scan, the write pass, one copy of the bytes to the
// handle's pinned buffer.  Device memory: the block, its text and O(w) offsets; nothing is sized G x E.  The few cells
// the device leaves undecided come back as (byte offset, bits): the host prints them with snprintf and closes the gaps.
namespace {

constexpr size_t kTextMaxBytes = (size_t)1 << 30;  // worst-case text of one call
constexpr uint32_t kTextListCap = 1u << 16;        // undecided cells of a block the list holds; more: the host formats the block

// MSWEEP_TEXT_HOST_CAP=n (developer switch, tests): a smaller list, to drive the whole-block host path
uint32_t text_list_cap() {
  const char *e = getenv("MSWEEP_TEXT_HOST_CAP");
  if (e && *e) return (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), kTextListCap);
  return kTextListCap;
}

void text_pinned_reserve(TextState &T, size_t need, size_t used) {
  if (need <= T.pinned_cap) return;
  const size_t cap = std::max(need, T.pinned_cap + T.pinned_cap / 2);
  char *p = nullptr;
  if (hipHostMalloc((void **)&p, cap, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    throw Fail("msw_core_text_block: cannot allocate " + std::to_string(cap) + " bytes of pinned host memory for the text");
  }
  if (used) std::memcpy(p, T.pinned, used);
  if (T.pinned) (void)hipHostFree(T.pinned);
  T.pinned = p;
  T.pinned_cap = cap;
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
  auto len64 = rocprim::make_transform_iterator(T.len.p, U32ToU64{});
  size_t tmp_bytes = 0;
  MSW_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, len64, T.off.p, (uint64_t)0, w + 1, rocprim::plus<uint64_t>(), st));
  T.tmp.alloc(tmp_bytes);
  MSW_HIP(rocprim::exclusive_scan(T.tmp.p, tmp_bytes, len64, T.off.p, (uint64_t)0, w + 1, rocprim::plus<uint64_t>(), st));
  MSW_HIP(hipEventRecord(T.ev[1], st));
  uint64_t total = 0;
  MSW_HIP(hipMemcpyAsync(&total, T.off.p + w, sizeof total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  T.out.alloc((total + 3) & ~(uint64_t)3);
  MSW_HIP(hipEventRecord(T.ev[2], st));
  text_launch_what(h, what, J, T, cap, true);
  MSW_HIP(hipEventRecord(T.ev[3], st));
  return total;
}
// (after the stream has been synchronised behind text_block_device)
void text_add_timing(TextState &T, uint64_t total) {
  float ms_len = 0.f, ms_write = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms_len, T.ev[0], T.ev[1]));
  MSW_HIP(hipEventElapsedTime(&ms_write, T.ev[2], T.ev[3]));
  T.kernel_ms += (double)ms_len + (double)ms_write;
  T.bytes += total;
}
// PROBS on a block the host formats itself: the values the device formats, on the host
void text_block_values(msw_core *h, int what, uint32_t G, size_t w, std::vector<double> &val) {
  TextState &T = h->text;
  const size_t n = (size_t)G * w;
  if (what == kTextProbs) {
    hipLaunchKernelGGL(k_text_exp, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65536)), dim3(256), 0, h->stream, T.val.p, n);
    MSW_HIP(hipGetLastError());
  }
  val.resize(n);
  MSW_HIP(hipMemcpyAsync(val.data(), T.val.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  MSW_HIP(hipStreamSynchronize(h->stream));
}

// The same text appended to the pinned buffer at `used`, the undecided cells filled in; returns the bytes appended.
size_t text_block_run(msw_core *h, int what, uint32_t G, size_t w, uint64_t id0, const uint64_t *prefix, size_t n_zero,
                      size_t used, size_t &n_host) {
  TextState &T = h->text;
  hipStream_t st = h->stream;
  const uint32_t cap = text_list_cap();
  const uint64_t total = text_block_device(h, what, G, w, id0, prefix, n_zero, cap);
  text_pinned_reserve(T, used + total, used);
  uint32_t n_list = 0;
  MSW_HIP(hipMemcpyAsync(&n_list, T.n_list.p, sizeof n_list, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipMemcpyAsync(T.pinned + used, T.out.p, total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  text_add_timing(T, total);
  if (n_list == 0) return total;
  char *text = T.pinned + used;
  if (n_list > cap) {
    // more undecided cells than the list holds: the host formats this block from the values the device formatted
    std::vector<double> val;
    text_block_values(h, what, G, w, val);
    std::string s;
    s.reserve(total);
    text_render_host(what, val, G, w, id0, prefix, n_zero, s);
    if (s.size() > total) throw Fail("msw_core_text_block: the host's text of a block is longer than the device's");
    std::memcpy(text, s.data(), s.size());
    n_host += (size_t)G * w;
    return s.size();
  }
  // the undecided cells in text order: print each into its 13 blanks and move what follows up against it
  std::vector<TextHostCell> cells(n_list);
  MSW_HIP(hipMemcpy(cells.data(), T.list.p, n_list * sizeof(TextHostCell), hipMemcpyDeviceToHost));
  std::sort(cells.begin(), cells.end(), [](const TextHostCell &a, const TextHostCell &b) { return a.off < b.off; });
  size_t rp = 0, wp = 0;
  char b[32];
  for (const TextHostCell &c : cells) {
    if (c.off < rp || c.off + g6::kMaxLen > total) throw Fail("msw_core_text_block: an undecided cell lies outside its block");
    std::memmove(text + wp, text + rp, c.off - rp);
    wp += c.off - rp;
    double x;
    std::memcpy(&x, &c.bits, sizeof x);
    const int n = snprintf(b, sizeof b, "%g", x);
    std::memcpy(text + wp, b, (size_t)n);
    wp += (size_t)n;
    rp = c.off + g6::kMaxLen;
  }
  std::memmove(text + wp, text + rp, total - rp);
  wp += total - rp;
  n_host += n_list;
  return wp;
}

void text_return(msw_core *h, size_t used, size_t n_host, const char **text_out, size_t *len_out, size_t *n_host_out) {
  text_pinned_reserve(h->text, 1, 0);  // an empty text still points somewhere
  *text_out = h->text.pinned;
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
    used += text_block_run(h, what, G, w, j0, pre, n_zero, used, n_host);
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
    used += text_block_run(h, kTextPlain, 1, w, 0, nullptr, 0, used, n_host);
  }
  text_return(h, used, n_host, text_out, len_out, n_host_out);
}

}  // namespace
