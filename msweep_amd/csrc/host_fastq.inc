// host_fastq.inc -- msw_fastq_* (included by input.hip): --extract-reads, the records of a FASTQ file by read id
// (kernels: fastq_kernels.hpp; grammar, messages and the host loops: fastq_host.hpp).  open: the file goes to the device
// through upload_text (host_reader.inc: plain, gzip and BGZF, the device inflate with zlib behind it), line feeds are
// counted per tile and scanned, every line's start is written, the records are validated, and the text with
// rec_off[n_records + 1] stays resident until close -- the text in a block of the handle's reader pool, 8 bytes per
// record beside it; the line starts (8 bytes per line) live for the validation only.  select: upload, radix sort,
// unique, range check, the records' lengths scanned into 64-bit output offsets.  next: the end of the piece by a binary
// search over those offsets, one gather kernel, and one copy of the bytes -- or, inside the gzip stream, the compressor
// on the gathered bytes where they lie (host_gzip.inc: gz_compress_device).
// MSWEEP_HOST_EXTRACT=1 (developer switch, read at open): slurp_text (zlib) and the loops of fastq_host.hpp behind the
// same calls and messages.

struct msw_fastq {
  msw_core *h = nullptr;
  bool host = false;
  std::string path;
  uint64_t n = 0, n_records = 0;
  // the device's side: the text (a block of h->reader_pool) and the index
  unsigned char *txt = nullptr;
  DevBuf<uint64_t> rec_off;
  // the host's side
  FileText ft;
  std::vector<uint64_t> h_rec_off;
  // the selection: m records, ascending; out_off[m + 1]; `cur` records of it have been handed out
  bool selected = false;
  uint64_t m = 0, total = 0, cur = 0;
  DevBuf<uint32_t> ids, sorted, sel;
  DevBuf<uint64_t> out_off, n_sel;
  DevBuf<uint8_t> tmp, out;
  std::vector<uint32_t> h_sel;
  std::vector<uint64_t> h_out_off;
};

namespace {

// hipMalloc that names what failed and how many bytes it wanted
template <class T>
void fq_alloc(DevBuf<T> &b, size_t count, const char *who, const char *what) {
  if (b.p && count <= b.n) return;
  b.release();
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc((void **)&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    throw Fail(std::string(who) + ": cannot allocate " + std::to_string(bytes) + " bytes of device memory for " + what);
  }
  b.n = std::max<size_t>(count, 1);
}

double fq_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// index and validation on the device; the text is in `text`.  Throws Fail with the grammar's message.
void fastq_index_device(msw_core *h, ReaderCtx &cx, DevText &text, msw_fastq &fq, msw_fastq_info *info) {
  hipStream_t st = h->stream;
  const uint64_t n = text.n;
  const uint64_t n_tiles = (n + kTileBytes - 1) / kTileBytes;
  RBuf<uint32_t> cnt(cx);
  RBuf<uint64_t> base(cx);
  cnt.alloc(n_tiles + 1), base.alloc(n_tiles + 1);
  MSW_HIP(hipMemsetAsync(cnt.p + n_tiles, 0, sizeof(uint32_t), st));
  if (n_tiles) hipLaunchKernelGGL(k_fq_count, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, text.txt.p, n, cnt.p);
  MSW_HIP(hipGetLastError());
  scan_u32_u64(cnt.p, base.p, n_tiles + 1, cx);
  const uint64_t n_nl = fetch_u64(base.p + n_tiles, st);
  const uint64_t n_lines = n_nl + (n && text.last != '\n' ? 1 : 0), n_records = n_lines / 4;
  if (n_records >= (1ull << 32))
    throw Fail("read file " + fq.path + ": " + std::to_string(n_records) + " records; read ids are below 2^32");
  // the line starts and the index: sized now, so an index that does not fit is an error with its bytes, never a fault
  const uint64_t need = (n_lines + 1 + n_records + 1) * sizeof(uint64_t);
  size_t free_b = 0, total_b = 0;
  MSW_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (uint64_t)free_b + h->reader_pool.idle_bytes())
    throw Fail("msw_fastq_open: the text (" + std::to_string(n) + " bytes) and the index (" + std::to_string(need) + " bytes) of read file " +
               fq.path + " do not fit in free device memory (" + std::to_string(free_b) + " bytes free)");
  RBuf<uint64_t> line_off(cx);
  line_off.alloc(n_lines + 1);
  fq_alloc(fq.rec_off, n_records + 1, "msw_fastq_open", "the record index");
  if (n_tiles)
    hipLaunchKernelGGL(k_fq_index, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, text.txt.p, n, base.p, n_lines, line_off.p,
                       fq.rec_off.p);
  MSW_HIP(hipGetLastError());
  // entry 0 and the last entry of both: a last line without its line feed ends at the padding's (n + 1)
  const uint64_t ends[3] = {0, n + (n && text.last != '\n' ? 1 : 0), n};
  MSW_HIP(hipMemcpyAsync(line_off.p + n_lines, &ends[1], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(line_off.p, &ends[0], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(fq.rec_off.p + n_records, &ends[2], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(fq.rec_off.p, &ends[0], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  RBuf<unsigned long long> bad(cx);
  bad.alloc(1);
  MSW_HIP(hipMemsetAsync(bad.p, 0xff, sizeof(unsigned long long), st));
  if (n_records)
    hipLaunchKernelGGL(k_fq_validate, dim3(reader_grid(n_records, h->n_cu)), dim3(256), 0, st, text.txt.p, line_off.p, n_records, bad.p);
  MSW_HIP(hipGetLastError());
  const uint64_t code = fetch_u64(reinterpret_cast<const uint64_t *>(bad.p), st);  // (also: `ends` has been read)
  fq.n = n;
  fq.n_records = n_records;
  info->n_records = n_records;
  if (code != fq::kNoBad) {
    info->reason = (int32_t)(code & 3) + fq::kNoAt;
    info->bad_record = code >> 2;
  } else if (n_lines % 4) {
    info->reason = fq::kLines;
    info->bad_record = n_records;
  }
  if (info->reason) throw Fail(fq::grammar_message(fq.path, info->reason, info->bad_record, n_lines));
}

void fastq_open_impl(msw_core *h, const char *path, msw_fastq_t *out, msw_fastq_info *info) {
  if (!path || !out || !info) throw Fail("msw_fastq_open: null path, out or info");
  *out = nullptr;
  *info = msw_fastq_info{};
  {
    const int fd = open(path, O_RDONLY);  // (the message of upload_text, for both sides of the switch)
    if (fd < 0) throw Fail(std::string("cannot open read file ") + path);
    close(fd);
  }
  std::unique_ptr<msw_fastq> fq(new msw_fastq());
  fq->h = h;
  fq->path = path;
  const char *sw = getenv("MSWEEP_HOST_EXTRACT");
  fq->host = sw && sw[0] == '1';
  if (fq->host) {
    const auto t0 = std::chrono::steady_clock::now();
    slurp_text(path, fq->ft);
    info->upload_ms = fq_ms_since(t0);
    info->text_bytes = fq->ft.size;
    info->inflate.text_bytes = fq->ft.size;
    const auto t1 = std::chrono::steady_clock::now();
    uint64_t n_lines = 0, bad = 0;
    const int reason = fq::host_index(fq->ft.data, fq->ft.size, fq->h_rec_off, &n_lines, &bad);
    info->index_ms = fq_ms_since(t1);
    fq->n = fq->ft.size;
    fq->n_records = info->n_records = n_lines / 4;
    if (reason) {
      info->reason = reason;
      info->bad_record = bad;
      throw Fail(fq::grammar_message(fq->path, reason, bad, n_lines));
    }
    if (fq->n_records >= (1ull << 32))
      throw Fail("read file " + fq->path + ": " + std::to_string(fq->n_records) + " records; read ids are below 2^32");
    *out = fq.release();
    return;
  }
  MSW_HIP(hipStreamSynchronize(h->stream));
  h->reader_pool.recycle();
  try {
    ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
    cx.inf = &h->inf;
    h->inf.last.clear();
    DevText text(cx);
    try {
      const auto t0 = std::chrono::steady_clock::now();
      upload_text(path, cx, text, "read file", /*fit_stager=*/true);
      MSW_HIP(hipEventSynchronize(text.done));
      info->upload_ms = fq_ms_since(t0);
      if (!h->inf.last.empty()) info->inflate = h->inf.last.back();
      info->text_bytes = text.n;
      const auto t1 = std::chrono::steady_clock::now();
      fastq_index_device(h, cx, text, *fq, info);
      info->index_ms = fq_ms_since(t1);
    } catch (const HipError &ex) {
      if (!strstr(ex.what(), "out of memory")) throw;
      (void)hipGetLastError();
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      throw Fail("msw_fastq_open: the text (" + std::to_string(text.n) + " bytes) and the index of read file " + fq->path +
                 " do not fit in free device memory (" + std::to_string(free_b) + " bytes free)");
    }
    // the text stays: its block leaves the DevText and goes back to the pool at close
    fq->txt = text.txt.p;
    text.txt.p = nullptr;
    text.txt.n = 0;
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);
    h->reader_pool.trim();  // (the failed file's text and scratch: back to the device)
    throw;
  }
  *out = fq.release();
}

void fastq_check(msw_core *h, msw_fastq *fq, const char *who) {
  if (!fq) throw Fail(std::string(who) + ": null read file");
  if (fq->h != h) throw Fail(std::string(who) + ": the read file was opened on another handle");
}

void fastq_select_impl(msw_core *h, msw_fastq *fq, const uint32_t *ids, size_t n, uint64_t *n_selected_out, uint64_t *bytes_out) {
  fastq_check(h, fq, "msw_fastq_select");
  if (n && !ids) throw Fail("msw_fastq_select: null ids");
  FastqState &F = h->fastq;
  if (fq->host) {
    uint64_t bad_id = 0;
    if (!fq::host_select(ids, n, fq->h_rec_off, fq->h_sel, fq->h_out_off, &bad_id)) throw Fail(fq::id_message(bad_id, fq->n_records));
    fq->m = fq->h_sel.size();
    fq->total = fq->h_out_off.back();
  } else {
    hipStream_t st = h->stream;
    uint64_t m = 0, total = 0;
    if (n) {
      const char *who = "msw_fastq_select";
      fq_alloc(fq->ids, n, who, "the read ids");
      fq_alloc(fq->sorted, n, who, "the sorted read ids");
      MSW_HIP(hipMemcpyAsync(fq->ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      size_t tmp_bytes = 0;
      MSW_HIP(prim_sort_keys(nullptr, tmp_bytes, fq->ids.p, fq->sorted.p, n, 32u, st));
      fq_alloc(fq->tmp, tmp_bytes, who, "sort storage");
      MSW_HIP(prim_sort_keys(fq->tmp.p, tmp_bytes, fq->ids.p, fq->sorted.p, n, 32u, st));
      uint32_t largest = 0;
      MSW_HIP(hipMemcpyAsync(&largest, fq->sorted.p + (n - 1), sizeof largest, hipMemcpyDeviceToHost, st));
      MSW_HIP(hipStreamSynchronize(st));  // (also: `ids` has been read)
      if (largest >= fq->n_records) throw Fail(fq::id_message(largest, fq->n_records));
      // from here on the selection is replaced
      fq->selected = false;
      fq_alloc(fq->sel, n, who, "the selection");
      fq_alloc(fq->n_sel, 1, who, "the selection's size");
      MSW_HIP(prim_unique(nullptr, tmp_bytes, fq->sorted.p, fq->sel.p, fq->n_sel.p, n, st));
      fq_alloc(fq->tmp, tmp_bytes, who, "select storage");
      MSW_HIP(prim_unique(fq->tmp.p, tmp_bytes, fq->sorted.p, fq->sel.p, fq->n_sel.p, n, st));
      m = fetch_u64(fq->n_sel.p, st);
      if (m > n) throw Fail("msw_fastq_select: internal: more distinct ids than ids");
    }
    fq->selected = false;
    fq_alloc(fq->out_off, m + 1, "msw_fastq_select", "the output offsets");
    if (m) {
      const FqLen lens{fq->sel.p, fq->rec_off.p, (size_t)m};
      size_t tmp_bytes = 0;
      MSW_HIP(prim_scan(nullptr, tmp_bytes, lens, fq->out_off.p, (size_t)m + 1, st));
      fq_alloc(fq->tmp, tmp_bytes, "msw_fastq_select", "scan storage");
      MSW_HIP(prim_scan(fq->tmp.p, tmp_bytes, lens, fq->out_off.p, (size_t)m + 1, st));
      total = fetch_u64(fq->out_off.p + m, st);
      if (total > fq->n) throw Fail("msw_fastq_select: internal: the selection is longer than the text");
    } else {
      MSW_HIP(hipMemsetAsync(fq->out_off.p, 0, sizeof(uint64_t), st));
      MSW_HIP(hipStreamSynchronize(st));
    }
    fq->m = m;
    fq->total = total;
  }
  fq->selected = true;
  fq->cur = 0;
  F.kernel_ms = 0.0;
  F.bytes = 0;
  if (n_selected_out) *n_selected_out = fq->m;
  if (bytes_out) *bytes_out = fq->total;
}

constexpr size_t kFqMinPiece = (size_t)1 << 20, kFqMaxPiece = (size_t)1 << 30;

void fastq_next_impl(msw_core *h, msw_fastq *fq, size_t max_bytes, bool gz, const char **out, size_t *len_out, size_t *text_len_out) {
  const char *who = gz ? "msw_fastq_next_gzip" : "msw_fastq_next";
  fastq_check(h, fq, who);
  if (!out || !len_out) throw Fail(std::string(who) + ": null out or len");
  if (max_bytes < kFqMinPiece || max_bytes > kFqMaxPiece) throw Fail(std::string(who) + ": max_bytes is outside 1 MiB ... 1 GiB");
  if (!fq->selected) throw Fail(std::string(who) + ": no selection (msw_fastq_select)");
  if (gz) gz_require_open(h, who);
  FastqState &F = h->fastq;
  hipStream_t st = h->stream;
  size_t len = 0, used = 0;
  if (fq->cur < fq->m) {
    const uint64_t r0 = fq->cur;
    auto off = [&](uint64_t r) { return fq->host ? fq->h_out_off[r] : fetch_u64(fq->out_off.p + r, st); };
    const uint64_t r1 = fq::piece_end(off, r0, fq->m, max_bytes);
    if (r1 == r0) {
      uint32_t id = 0;
      if (fq->host) {
        id = fq->h_sel[r0];
      } else {
        MSW_HIP(hipMemcpyAsync(&id, fq->sel.p + r0, sizeof id, hipMemcpyDeviceToHost, st));
        MSW_HIP(hipStreamSynchronize(st));
      }
      throw Fail(std::string(who) + ": record " + std::to_string((uint64_t)id + 1) + " of read file " + fq->path + " has " +
                 std::to_string(off(r0 + 1) - off(r0)) + " bytes, more than max_bytes = " + std::to_string(max_bytes));
    }
    len = (size_t)(off(r1) - off(r0));
    pinned_reserve(F.pinned, len, 0);
    if (fq->host) {
      const auto t0 = std::chrono::steady_clock::now();
      fq::host_gather(fq->ft.data, fq->h_rec_off, fq->h_sel, fq->h_out_off, (size_t)r0, (size_t)r1, F.pinned.p);
      F.kernel_ms += fq_ms_since(t0);
    } else {
      // (gz_compress_device reads whole dwords of a 16-byte aligned text)
      fq_alloc(fq->out, ((len + 15) & ~(size_t)15) + 16, who, "the gathered records");
      for (auto &e : F.ev)
        if (!e) MSW_HIP(hipEventCreate(&e));
      MSW_HIP(hipEventRecord(F.ev[0], st));
      const unsigned nb = (unsigned)((len + kFqGatherChunk - 1) / kFqGatherChunk);
      hipLaunchKernelGGL(k_fq_gather, dim3(nb), dim3(kFqGatherThreads), 0, st, fq->txt, fq->rec_off.p, fq->sel.p, fq->out_off.p, r0, r1,
                         (uint64_t)len, fq->out.p);
      MSW_HIP(hipGetLastError());
      MSW_HIP(hipEventRecord(F.ev[1], st));
      if (!gz || h->gz.host) MSW_HIP(hipMemcpyAsync(F.pinned.p, fq->out.p, len, hipMemcpyDeviceToHost, st));
      MSW_HIP(hipStreamSynchronize(st));
      float ms = 0.f;
      MSW_HIP(hipEventElapsedTime(&ms, F.ev[0], F.ev[1]));
      F.kernel_ms += (double)ms;
    }
    F.bytes += len;
    if (gz) {
      if (h->gz.host) used = gz_host_deflate(h, F.pinned.p, len, Z_NO_FLUSH, 0);
      else if (fq->host) used = gz_compress_host(h, F.pinned.p, len, 0);
      else used = gz_compress_device(h, fq->out.p, len, 0);
    }
    fq->cur = r1;  // (only now: a piece that failed is handed out again)
  }
  if (gz) {
    gz_return(h, used, out, len_out);
    if (text_len_out) *text_len_out = len;
  } else {
    pinned_reserve(F.pinned, 1, 0);  // an empty piece still points somewhere
    *out = F.pinned.p;
    *len_out = len;
  }
}

void fastq_close_impl(msw_fastq *fq) {
  if (!fq) return;
  if (fq->txt && fq->h) {
    (void)hipSetDevice(fq->h->device);
    (void)hipStreamSynchronize(fq->h->stream);
    fq->h->reader_pool.give(fq->txt);
    fq->h->reader_pool.trim();  // (a whole read file: back to the device, not kept for the next reader call)
  }
  delete fq;
}

}  // namespace
