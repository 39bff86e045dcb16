// host_likelihood_file.inc -- msw_core_set_dense_logl_file / _text (included by input.hip behind host_reader.inc;
// kernels: likelihood_text_kernels.hpp).  --read-likelihood (include/Likelihood.hpp:224-253) was the one file-sized stage
// of the drivers that ran on the host, a float() or std::stod per cell; here the text -- plain, gzip or BGZF, through
// upload_text -- is parsed where it lies and the resident likelihood is built from the [G][E] stage on, by the code
// msw_core_set_dense_logl runs (dense_from_stage, host_likelihood.inc).
//
// SERVED or NOT SERVED.  A served file leaves the handle in exactly the state msw_core_set_dense_logl leaves from the
// host-parsed matrix.  A file that is not served (msw_likfile_info::reason) leaves the handle as it was -- nothing is
// reset before the last check has passed; behind it only a HIP error of the resident build (whose memory the check
// counts) can fail the call, as it fails msw_core_set_dense_logl -- and the call returns 0: the drivers then run their own parsers, whose
// result or message stands.  Text outside the grammar of likelihood_text_kernels.hpp is never judged here.
//
// Cells outside Clinger's exact case (dec_parse.hpp) come back as a list of at most 65 536 tokens; strtod converts each
// on the host and a scatter kernel patches the matrix before anything reads it.  A token whose value strtod cannot
// represent at all (ERANGE with an infinite or zero result: 1e400, 1e-400) makes the file not served -- std::stod throws
// on it and Python does not, so each driver's own parser decides; an ERANGE that only reports a subnormal result keeps
// the correctly rounded double strtod returned.
namespace {

// msw_likfile_info::reason (include/msweep_core.h: MSW_LIKFILE_*)
constexpr int32_t kLikWhyForced = 1, kLikWhyOpen = 2, kLikWhyByte = 3, kLikWhyToken = 4, kLikWhyColumns = 5, kLikWhyEmpty = 6,
                  kLikWhyHostCells = 7, kLikWhyRange = 8, kLikWhyMemory = 9, kLikWhyLines = 10;
struct LikNotServed {
  int32_t reason;
};

LikCtr fetch_lik_ctr(const LikCtr *d, hipStream_t st) {
  LikCtr c = {};
  MSW_HIP(hipMemcpyAsync(&c, d, sizeof c, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  return c;
}
// text in host memory to the device, padded like upload_text pads a file's
void upload_mem(const char *mem, uint64_t n, ReaderCtx &cx, DevText &t) {
  stager_ready(cx, n);
  t.n = n;
  hipStream_t cs = cx.stage->copy;
  if (!t.done) MSW_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  const uint64_t padded = (n + kTileBytes - 1) / kTileBytes * kTileBytes + kTileBytes;
  t.txt.alloc(padded);
  MSW_HIP(hipMemsetAsync(t.txt.p + n, '\n', padded - n, cs));
  t.last = '\n';
  stage_to_device(-1, "", mem, n, t.txt.p, cx, t.last, "likelihood text");
  MSW_HIP(hipEventRecord(t.done, cs));
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() {
    MSW_HIP(hipEventCreate(&a));
    MSW_HIP(hipEventCreate(&b));
  }
  EventPair(const EventPair &) = delete;
  EventPair &operator=(const EventPair &) = delete;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// the text on the device -> counts (host) and the [G][E] stage; throws LikNotServed
void parse_likelihood_text(msw_core *h, ReaderCtx &cx, DevText &text, size_t G, DevBuf<double> &stage, std::vector<uint64_t> &counts,
                           msw_likfile_info *info) {
  hipStream_t st = h->stream;
  const uint64_t n = text.n;
  if (n == 0) throw LikNotServed{kLikWhyEmpty};
  if (n >= (1ull << 40)) throw LikNotServed{kLikWhyMemory};
  if (G == 0 || G >= 0x7fffffffull) throw LikNotServed{kLikWhyColumns};
  const uint32_t cols = (uint32_t)G + 1u;
  MSW_HIP(hipStreamWaitEvent(st, text.done, 0));
  EventPair ev;
  MSW_HIP(hipEventRecord(ev.a, st));
  RBuf<LikCtr> ctr(cx);
  ctr.alloc(1);
  ctr.zero(st);
  // ---- pass 1, scans ----
  const uint64_t n_tiles = (n + kTileBytes - 1) / kTileBytes;
  RBuf<uint32_t> cnt_tok(cx), cnt_nl(cx);
  RBuf<uint64_t> base_tok(cx), base_nl(cx);
  cnt_tok.alloc(n_tiles + 1), cnt_nl.alloc(n_tiles + 1);
  base_tok.alloc(n_tiles + 1), base_nl.alloc(n_tiles + 1);
  MSW_HIP(hipMemsetAsync(cnt_tok.p + n_tiles, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemsetAsync(cnt_nl.p + n_tiles, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_lik_count, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, text.txt.p, n, cnt_tok.p, cnt_nl.p, ctr.p);
  MSW_HIP(hipGetLastError());
  scan_u32_u64(cnt_tok.p, base_tok.p, n_tiles + 1, cx);
  scan_u32_u64(cnt_nl.p, base_nl.p, n_tiles + 1, cx);
  const uint64_t n_tok = fetch_u64(base_tok.p + n_tiles, st), n_nl = fetch_u64(base_nl.p + n_tiles, st);
  const uint32_t f1 = fetch_lik_ctr(ctr.p, st).flags;
  if (f1 & kLikBadByte) throw LikNotServed{kLikWhyByte};
  const uint64_t E = n_nl + (text.last != '\n' ? 1 : 0);
  if (E >= 0xffffffffull) throw LikNotServed{kLikWhyLines};
  // (a blank line or a doubled tab is an empty token: one column too many, which is how it is reported)
  if (E == 0 || n_tok != E * (uint64_t)cols) throw LikNotServed{kLikWhyColumns};
  if (f1 & kLikBadToken) throw LikNotServed{kLikWhyToken};
  // ---- room: the EC-major matrix and the stage side by side, beside the text; then, the EC-major matrix gone, the stage
  // and what dense_from_stage builds from it (at most another G x E doubles: the dense flavour's Lt) ----
  {
    size_t free_b = 0, total_b = 0;
    MSW_HIP(hipMemGetInfo(&free_b, &total_b));
    const long double need = 24.0L * (long double)G * (long double)E + 8.0L * (long double)E + (long double)(1u << 28);
    if (need > (long double)free_b) throw LikNotServed{kLikWhyMemory};
  }
  // ---- pass 2 ----
  DevBuf<uint64_t> d_counts;
  DevBuf<double> Lt;
  DevBuf<LikHostCell> d_host;
  d_counts.alloc(E);
  Lt.alloc(G * E);
  d_host.alloc(kLikHostCap);
  hipLaunchKernelGGL(k_lik_parse, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, text.txt.p, n, base_tok.p, base_nl.p, cols,
                     n_tok, d_counts.p, Lt.p, d_host.p, ctr.p);
  MSW_HIP(hipGetLastError());
  const LikCtr c2 = fetch_lik_ctr(ctr.p, st);
  if (c2.flags & kLikColumns) throw LikNotServed{kLikWhyColumns};
  if (c2.flags & kLikBadToken) throw LikNotServed{kLikWhyToken};
  if ((c2.flags & kLikHostOver) || c2.n_host > kLikHostCap) throw LikNotServed{kLikWhyHostCells};
  cx.drop(text.txt);
  // ---- the cells left to strtod ----
  if (c2.n_host) {
    std::vector<LikHostCell> cells(c2.n_host);
    MSW_HIP(hipMemcpyAsync(cells.data(), d_host.p, cells.size() * sizeof(LikHostCell), hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> at(cells.size());
    std::vector<double> val(cells.size());
    for (size_t i = 0; i < cells.size(); ++i) {
      char tok[dec::kDecMaxToken + 1];
      const size_t len = std::min<size_t>(cells[i].len, dec::kDecMaxToken);
      std::memcpy(tok, cells[i].b, len);
      tok[len] = 0;
      char *end = nullptr;
      errno = 0;
      const double v = strtod(tok, &end);
      if (end != tok + len) throw LikNotServed{kLikWhyToken};
      if (errno == ERANGE && (std::isinf(v) || v == 0.0)) throw LikNotServed{kLikWhyRange};
      at[i] = cells[i].cell;
      val[i] = v;
    }
    DevBuf<uint64_t> d_at;
    DevBuf<double> d_val;
    d_at.upload(at.data(), at.size(), st);
    d_val.upload(val.data(), val.size(), st);
    hipLaunchKernelGGL(k_lik_scatter, dim3((unsigned)((at.size() + 255) / 256)), dim3(256), 0, st, d_val.p, d_at.p, (uint32_t)at.size(),
                       (uint64_t)G * E, Lt.p);
    MSW_HIP(hipGetLastError());
    MSW_HIP(hipStreamSynchronize(st));  // (the host vectors die at the end of this block)
  }
  // ---- [E][G] -> the [G][E] stage ----
  stage.alloc(G * E);
  const dim3 grid((unsigned)((E + 31) / 32), (unsigned)std::min<uint64_t>((G + 31) / 32, 65535));
  hipLaunchKernelGGL(k_lik_transpose, grid, dim3(256), 0, st, Lt.p, (uint32_t)E, (uint32_t)G, stage.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(ev.b, st));
  counts.resize(E);
  MSW_HIP(hipMemcpyAsync(counts.data(), d_counts.p, E * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  info->kernel_ms = ms;  // (pass 1 through the transpose, the host's strtod of the listed cells included)
  info->n_ecs = E;
  info->n_host_cells = c2.n_host;
}

// path, or -- path null -- the n bytes at mem
void set_dense_file_impl(msw_core *h, const char *path, const char *mem, size_t n, size_t G, msw_likfile_info *info) {
  if (!info) throw Fail("msw_core_set_dense_logl_file: null info");
  *info = msw_likfile_info{};
  if (!path && !mem && n) throw Fail("msw_core_set_dense_logl_text: null text");
  const char *sw = getenv("MSWEEP_HOST_LIKELIHOOD_FILE");  // developer switch, read at the call: the drivers' own parsers
  if (sw && atoi(sw) != 0) {
    info->reason = kLikWhyForced;
    return;
  }
  MSW_HIP(hipStreamSynchronize(h->stream));
  h->reader_pool.recycle();
  DevBuf<double> stage;
  std::vector<uint64_t> counts;
  try {
    ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
    cx.inf = &h->inf;
    h->inf.last.clear();
    DevText text(cx);
    try {
      const auto t0 = std::chrono::steady_clock::now();
      try {
        if (path) upload_text(path, cx, text, "likelihood file", /*fit_stager=*/true);
        else upload_mem(mem, n, cx, text);
      } catch (const Fail &) {
        throw LikNotServed{kLikWhyOpen};
      }
      MSW_HIP(hipEventSynchronize(text.done));
      info->upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (!h->inf.last.empty()) info->inflate = h->inf.last.back();
      info->text_bytes = text.n;
      parse_likelihood_text(h, cx, text, G, stage, counts, info);
    } catch (const HipError &ex) {
      if (!strstr(ex.what(), "out of memory")) throw;
      (void)hipGetLastError();
      throw LikNotServed{kLikWhyMemory};
    }
  } catch (const LikNotServed &w) {
    MSW_HIP(hipStreamSynchronize(h->stream));
    info->reason = w.reason;
    info->n_ecs = info->n_host_cells = 0;
    info->kernel_ms = 0.0;
    h->reader_pool.trim();
    return;
  }
  h->reader_pool.trim();  // (the text's block: nothing of a likelihood file is read twice)
  // every check has passed: only now does the resident likelihood go
  reset_likelihood(h);
  dense_from_stage(h, nullptr, 0, stage.p, G, counts.size());
  h->lik_counts.swap(counts);
  info->served = 1;
}

void likfile_counts_impl(msw_core *h, uint64_t *out, size_t n_ecs) {
  if (!out && n_ecs) throw Fail("msw_core_likfile_counts: null output");
  if (n_ecs != h->lik_counts.size()) throw Fail("msw_core_likfile_counts: n_ecs is not the line count of the last served file");
  if (n_ecs) std::memcpy(out, h->lik_counts.data(), n_ecs * sizeof(uint64_t));
}

}  // namespace
