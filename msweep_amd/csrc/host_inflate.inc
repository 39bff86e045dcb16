// host_inflate.inc -- gzip pseudoalignment input inflated on the device (included by input.hip behind
// host_reader.inc; kernels: inflate_kernels.hpp, format: inflate_format.hpp).  upload_text sends a gzip file's COMPRESSED
// bytes through the stager and calls inflate_device, which runs the passes on the reader's stream behind the copy's event
// and leaves the text where the token kernels read it; msw_core_inflate_gzip is the same for bytes in host memory (tests,
// diagnostics).  The trailer check is the guarantee: the device's text is used only when it has the CRC-32 and the length
// the member promises.  Whenever it cannot be vouched for -- a header the parser does not take, a probe mismatch, an
// owner's status, a CRC or length mismatch, bytes between the final block and the trailer (several members, garbage), a
// payload that does not fit the device beside its text, a stretch between two block starts too long for one wavefront to
// pay (inflate_max_span) -- the host path stands, result and messages unchanged: zlib on
// one thread (slurp_text of host_alignment.inc).  MSWEEP_HOST_INFLATE=1 (developer switch, read at the call) forces it;
// MSWEEP_INFLATE_CHUNK=n (developer switch) sets the bytes of payload per chunk.
// A file whose first member declares its own length (BGZF) takes host_inflate_members.inc's way instead: one decode per
// member, no probe, windows or chain; the reasons and the host path behind it are the same.
namespace {

// files whose first member declares its length (BGZF): host_inflate_members.inc
bool first_member_declares_length(const uint8_t *head, uint64_t avail);
int32_t upload_members_device(int fd, const char *path, uint64_t n, ReaderCtx &cx, DevText &t, msw_inflate_info &info);
int32_t inflate_members_bytes(msw_core *h, const uint8_t *gz, size_t n, const uint8_t **text_out, size_t *len_out, msw_inflate_info &info);

bool inflate_forced_to_host() {
  const char *e = getenv("MSWEEP_HOST_INFLATE");
  return e && e[0] == '1';
}
size_t inflate_chunk_bytes(size_t asked) {
  size_t c = asked;
  if (!c) {
    const char *e = getenv("MSWEEP_INFLATE_CHUNK");
    const long long v = e ? atoll(e) : 0;
    c = v > 0 ? (size_t)v : infl::kDefaultChunk;
  }
  return std::min<size_t>(std::max<size_t>(c, infl::kMinChunk), (size_t)1 << 28);
}

// The longest stretch of payload one owner may have to walk.  An owner is one wavefront, and it walks its stretch twice
// (pass a, pass b) at ~64 KiB of payload in 20 ms each (DESIGN 7a): ~1.6 MB/s along the longest stretch, whatever the
// rest of the device does, while zlib on the host inflates the WHOLE payload at 100-160 MB/s (250-400 MB/s of text).  The
// device pays while the longest stretch is below a 64th of the payload; below the floor of 256 KiB (0.16 s) neither
// path is long.  Streams in which the probe finds few starts -- fixed-Huffman or stored throughout, one very long block
// -- therefore go to the host.  MSWEEP_INFLATE_MAX_SPAN=n (developer switch, tests) sets the floor in bytes.
uint64_t inflate_max_span(uint64_t payload) {
  const char *e = getenv("MSWEEP_INFLATE_MAX_SPAN");
  const long long v = e ? atoll(e) : 0;
  const uint64_t floor_b = v > 0 ? (uint64_t)v : (uint64_t)256 << 10;
  return std::max<uint64_t>(floor_b, payload / 64);
}

// words of device memory for n bytes of a member: whole words and 16 bytes of zeros behind them
inline size_t inflate_words(uint64_t n) { return (size_t)((n + 3) / 4 + 4); }

// The passes over a member of n bytes that lies in d_gz (inflate_words(n) words, zero behind the n bytes) once `copied`
// (may be null) has happened.  Returns infl::kWhyNone with the text in `txt` (padded with line feeds as upload_text pads
// it), its length and its last byte; any other reason: nothing of `txt` counts.  Fills info but for on_device.
int32_t inflate_device(ReaderCtx &cx, const uint32_t *d_gz, uint64_t n, const infl::Member &m, size_t chunk_asked, hipEvent_t copied,
                       RBuf<unsigned char> &txt, uint64_t &total_out, unsigned char &last_out, msw_inflate_info &info) {
  InflateState &S = *cx.inf;
  hipStream_t st = cx.st;
  const uint64_t payload = n - 8 - m.payload, chunk = inflate_chunk_bytes(chunk_asked);
  const uint64_t n_chunks64 = std::max<uint64_t>(1, (payload + chunk - 1) / chunk);
  info.payload_bytes = payload;
  info.chunk_bytes = (uint32_t)chunk;
  if (n_chunks64 >= (1ull << 31)) return infl::kWhyMemory;
  const uint32_t n_chunks = (uint32_t)n_chunks64;
  info.n_chunks = n_chunks;
  const uint64_t n_words = inflate_words(n), first_bit = 8 * m.payload, end_bit = 8 * (n - 8);
  for (auto &e : S.ev)
    if (!e) MSW_HIP(hipEventCreate(&e));
  if (!S.pow8.p) {
    defl::crc_pow_table(S.pow8_host);
    S.pow8.upload(S.pow8_host, 40, st);
  }
  if (copied) MSW_HIP(hipStreamWaitEvent(st, copied, 0));
  // ---- probe: the first plausible block start of every chunk
  RBuf<uint64_t> starts(cx);
  starts.alloc(n_chunks);
  MSW_HIP(hipEventRecord(S.ev[0], st));
  hipLaunchKernelGGL(k_inf_probe, dim3(n_chunks), dim3(kWave), 0, st, d_gz, n_words, first_bit, end_bit, 8 * chunk, n_chunks, starts.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(S.ev[1], st));
  // (every stage's pair of events lies directly around its launches: no copy, synchronisation or allocation between
  // them.  A second strand's passes share the stream with the first strand's token kernels, which can land inside a pair.)
  std::vector<uint64_t> h_starts(n_chunks);
  MSW_HIP(hipMemcpyAsync(h_starts.data(), starts.p, n_chunks * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  std::vector<InfOwner> own;
  for (uint64_t s0 : h_starts)
    if (s0 != infl::kNoStart) own.push_back(InfOwner{s0, infl::kNoStart, 0, 0, 0, 0, 0, 0});
  for (size_t k = 0; k + 1 < own.size(); ++k) own[k].stop = own[k + 1].start;
  const uint32_t n_own = (uint32_t)own.size();
  info.n_starts = n_own;
  {  // no owner's stretch may be longer than one wavefront can pay for
    const uint64_t most = 8 * inflate_max_span(payload);
    for (size_t k = 0; k < own.size(); ++k)
      if ((k + 1 < own.size() ? own[k].stop : end_bit) - own[k].start > most) return infl::kWhyLongSpan;
  }
  own.push_back(InfOwner{0, 0, 0, 0, 0, 0, 0, 0});  // (a spare: the scan's last value is the total)
  // ---- pass (a): counts and windows; offsets
  size_t free_b = 0, total_b = 0;
  MSW_HIP(hipMemGetInfo(&free_b, &total_b));
  const uint64_t window_bytes = (uint64_t)n_own * infl::kWindow * 3;
  if (window_bytes + (1ull << 28) > (uint64_t)free_b + cx.pool->idle_bytes()) return infl::kWhyMemory;
  RBuf<InfOwner> owners(cx);
  RBuf<uint16_t> windows(cx);
  RBuf<uint8_t> resolved(cx);
  RBuf<uint64_t> offset(cx);
  RBuf<unsigned char> tmp(cx);
  RBuf<uint32_t> crc(cx);
  owners.alloc(n_own + 1), windows.alloc((size_t)n_own * infl::kWindow), resolved.alloc((size_t)n_own * infl::kWindow);
  offset.alloc(n_own + 1), crc.alloc(1);
  MSW_HIP(hipMemcpyAsync(owners.p, own.data(), (n_own + 1) * sizeof(InfOwner), hipMemcpyHostToDevice, st));
  {  // (the scan's temporary storage is there before the clock starts)
    size_t bytes = 0;
    MSW_HIP(prim_scan(nullptr, bytes, owners.p, offset.p, (size_t)n_own + 1, st));
    tmp.alloc(bytes);
  }
  MSW_HIP(hipEventRecord(S.ev[2], st));
  hipLaunchKernelGGL(k_inf_window, dim3(n_own), dim3(kWave), 0, st, d_gz, n_words, end_bit, (uint64_t)1 << 40, n_own, owners.p, windows.p);
  MSW_HIP(hipGetLastError());
  {
    size_t bytes = tmp.n;
    MSW_HIP(prim_scan(tmp.p, bytes, owners.p, offset.p, (size_t)n_own + 1, st));  // (the owners' byte counts)
  }
  MSW_HIP(hipEventRecord(S.ev[3], st));
  uint64_t total = 0;
  MSW_HIP(hipMemcpyAsync(own.data(), owners.p, n_own * sizeof(InfOwner), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipMemcpyAsync(&total, offset.p + n_own, sizeof total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  for (uint32_t k = 0; k < n_own; ++k) {
    if (own[k].status != infl::kOk) return infl::kWhyStatus;
    const bool last = k + 1 == n_own;
    // the final block in front of the last owner: the member ends there, and what follows is not its payload
    if (!last && own[k].final) return infl::kWhyTrailing;
    // every owner ends exactly where the next begins: anything else, and the probe took a position that starts no block
    if (last ? !own[k].final : own[k].end_bit != own[k].stop) return infl::kWhyProbe;
  }
  if ((own[n_own - 1].end_bit + 7) / 8 * 8 != end_bit) return infl::kWhyTrailing;
  if ((uint32_t)total != m.isize) return infl::kWhyCrc;
  info.text_bytes = total;
  // ---- the text: allocated now that its length is known
  const uint64_t padded = (total + kTileBytes - 1) / kTileBytes * kTileBytes + kTileBytes;
  MSW_HIP(hipMemGetInfo(&free_b, &total_b));
  if (padded + (1ull << 28) > (uint64_t)free_b + cx.pool->idle_bytes()) return infl::kWhyMemory;
  txt.alloc(padded);
  MSW_HIP(hipMemsetAsync(txt.p + total, '\n', padded - total, st));
  // ---- the window chain, pass (b), the CRC
  MSW_HIP(hipEventRecord(S.ev[4], st));
  if (n_own > 1) hipLaunchKernelGGL(k_inf_chain, dim3(1), dim3(kInfChainThreads), 0, st, windows.p, n_own - 1, resolved.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(S.ev[5], st));
  hipLaunchKernelGGL(k_inf_write, dim3(n_own), dim3(kWave), 0, st, d_gz, n_words, end_bit, n_own, owners.p, offset.p, resolved.p, txt.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(S.ev[6], st));
  MSW_HIP(hipMemsetAsync(crc.p, 0, sizeof(uint32_t), st));
  if (total) {
    gz_crc_launch(cx.n_cu, st, txt.p, total, S.pow8.p, crc.p);  // (k_gz_crc: output.hip)
    MSW_HIP(hipGetLastError());
  }
  MSW_HIP(hipEventRecord(S.ev[7], st));
  uint32_t r = 0;
  unsigned char last = '\n';
  MSW_HIP(hipMemcpyAsync(own.data(), owners.p, n_own * sizeof(InfOwner), hipMemcpyDeviceToHost, st));
  MSW_HIP(hipMemcpyAsync(&r, crc.p, sizeof r, hipMemcpyDeviceToHost, st));
  if (total) MSW_HIP(hipMemcpyAsync(&last, txt.p + total - 1, 1, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  static const int first_ev[5] = {0, 2, 4, 5, 6};  // probe; pass (a) + scan; chain; pass (b); CRC
  for (int i = 0; i < 5; ++i) MSW_HIP(hipEventElapsedTime(&ms[i], S.ev[first_ev[i]], S.ev[first_ev[i] + 1]));
  info.probe_ms = ms[0], info.window_ms = ms[1], info.chain_ms = ms[2], info.write_ms = ms[3], info.crc_ms = ms[4];
  info.kernel_ms = (double)ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
  for (uint32_t k = 0; k < n_own; ++k)
    if (own[k].status_b != infl::kOk) return infl::kWhyStatus;
  if (~(defl::crc_shift(0xffffffffu, total, S.pow8_host) ^ r) != m.crc) return infl::kWhyCrc;
  total_out = total;
  last_out = last;
  return infl::kWhyNone;
}

// inflate_device, with an allocation that fails counted as "does not fit"
int32_t inflate_device_guarded(ReaderCtx &cx, const uint32_t *d_gz, uint64_t n, const infl::Member &m, size_t chunk_asked,
                               hipEvent_t copied, RBuf<unsigned char> &txt, uint64_t &total, unsigned char &last, msw_inflate_info &info) {
  try {
    return inflate_device(cx, d_gz, n, m, chunk_asked, copied, txt, total, last, info);
  } catch (const HipError &ex) {
    if (!strstr(ex.what(), "out of memory")) throw;
    (void)hipGetLastError();
    return infl::kWhyMemory;
  }
}

// A gzip file for upload_text: true when the kernels served it (t.txt, t.n, t.last set, t.done recorded); false: the host
// path takes the file.  The file's entry of msw_alignment_last_inflate either way.
bool upload_gzip_device(int fd, const char *path, uint64_t n, ReaderCtx &cx, DevText &t) {
  msw_inflate_info info = {};
  info.fallback_reason = infl::kWhyNone;
  int32_t why = infl::kWhyNone;
  if (inflate_forced_to_host()) {
    why = infl::kWhyForced;
  } else {
    std::vector<uint8_t> head((size_t)std::min<uint64_t>(n, 1u << 17));
    uint8_t trailer[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    infl::Member m = {false, 0, 0, 0};
    if (n >= 18 && pread(fd, head.data(), head.size(), 0) == (ssize_t)head.size() && pread(fd, trailer, 8, (off_t)(n - 8)) == 8)
      m = infl::parse_member(head.data(), head.size(), n, trailer);
    if (!m.ok) {
      why = infl::kWhyHeader;
    } else if (first_member_declares_length(head.data(), head.size())) {
      why = upload_members_device(fd, path, n, cx, t, info);
    } else {
      const auto t0 = std::chrono::steady_clock::now();
      RBuf<uint32_t> gz(cx);
      bool fits = true;
      try {
        gz.alloc(inflate_words(n));
      } catch (const HipError &ex) {
        if (!strstr(ex.what(), "out of memory")) throw;
        (void)hipGetLastError();
        fits = false;
      }
      if (!fits) {
        why = infl::kWhyMemory;
      } else {
        hipStream_t cs = cx.stage->copy;
        if (!t.done) MSW_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
        unsigned char *dev = reinterpret_cast<unsigned char *>(gz.p);
        MSW_HIP(hipMemsetAsync(dev + n, 0, inflate_words(n) * 4 - n, cs));
        unsigned char last_gz = 0;
        stage_to_device(fd, path, nullptr, n, dev, cx, last_gz);
        MSW_HIP(hipEventRecord(t.done, cs));
        MSW_HIP(hipEventSynchronize(t.done));  // (the passes wait for the copy anyway: this only stops the clock)
        info.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        why = inflate_device_guarded(cx, gz.p, n, m, 0, t.done, t.txt, t.n, t.last, info);
        // (the compressed block goes back to the pool here, behind the last kernel that reads it: the stream is idle)
      }
    }
  }
  info.on_device = why == infl::kWhyNone ? 1 : 0;
  info.fallback_reason = why;
  cx.inf->last.push_back(info);
  if (why != infl::kWhyNone) return false;
  MSW_HIP(hipEventRecord(t.done, cx.st));
  return true;
}

// ---- msw_core_inflate_gzip: the same for bytes in host memory; the host path is zlib over every member -----------------
void inflate_host_members(const uint8_t *gz, size_t n, std::vector<char> &text) {
  z_stream zs;
  std::memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, 15 + 16) != Z_OK) throw Fail("msw_core_inflate_gzip: zlib's inflateInit2 failed");
  struct End {
    z_stream *z;
    ~End() { (void)inflateEnd(z); }
  } end{&zs};
  text.resize(std::max<size_t>(n * 6, (size_t)1 << 16));
  size_t used = 0, in_at = 0;
  for (;;) {
    if (used == text.size()) text.resize(text.size() * 2);
    const size_t in_now = std::min<size_t>(n - in_at, (size_t)1 << 30), room = std::min<size_t>(text.size() - used, (size_t)1 << 30);
    zs.next_in = const_cast<Bytef *>(gz + in_at);
    zs.avail_in = (uInt)in_now;
    zs.next_out = reinterpret_cast<Bytef *>(text.data() + used);
    zs.avail_out = (uInt)room;
    const int rc = ::inflate(&zs, Z_NO_FLUSH);
    in_at += in_now - zs.avail_in;
    used += room - zs.avail_out;
    if (rc == Z_STREAM_END) {
      // (gzread's rule: another member follows when the gzip magic does; anything else behind a member is ignored)
      if (n - in_at >= 2 && gz[in_at] == 0x1f && gz[in_at + 1] == 0x8b) {
        if (inflateReset(&zs) != Z_OK) throw Fail("msw_core_inflate_gzip: zlib's inflateReset failed");
        continue;
      }
      break;
    }
    if (rc == Z_BUF_ERROR && in_at == n)
      throw Fail("msw_core_inflate_gzip: cannot read gzip-compressed bytes: unexpected end of file");
    if (rc != Z_OK && rc != Z_BUF_ERROR)
      throw Fail(std::string("msw_core_inflate_gzip: cannot read gzip-compressed bytes: ") + (zs.msg ? zs.msg : "zlib error"));
    if (rc == Z_OK && in_at == n && zs.avail_out != 0)
      throw Fail("msw_core_inflate_gzip: cannot read gzip-compressed bytes: unexpected end of file");
  }
  text.resize(used);
}

void inflate_gzip_impl(msw_core *h, const uint8_t *gz, size_t n, size_t chunk_bytes, const uint8_t **text_out, size_t *len_out,
                       msw_inflate_info *info_out) {
  if (!text_out || !len_out) throw Fail("msw_core_inflate_gzip: null text_out or len_out");
  if (n && !gz) throw Fail("msw_core_inflate_gzip: null bytes");
  InflateState &S = h->inf;
  MSW_HIP(hipStreamSynchronize(h->stream));
  h->reader_pool.recycle();
  msw_inflate_info info = {};
  int32_t why = infl::kWhyNone;
  size_t len = 0;
  const infl::Member m = infl::parse_member(gz, n);
  if (inflate_forced_to_host()) {
    why = infl::kWhyForced;
  } else if (!m.ok) {
    why = infl::kWhyHeader;
  } else if (first_member_declares_length(gz, n)) {
    why = inflate_members_bytes(h, gz, n, text_out, &len, info);
  } else {
    ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
    cx.inf = &S;
    RBuf<uint32_t> d_gz(cx);
    RBuf<unsigned char> txt(cx);
    uint64_t total = 0;
    unsigned char last = '\n';
    try {
      d_gz.alloc(inflate_words(n));
      MSW_HIP(hipMemsetAsync(reinterpret_cast<unsigned char *>(d_gz.p) + n, 0, inflate_words(n) * 4 - n, h->stream));
      MSW_HIP(hipMemcpyAsync(d_gz.p, gz, n, hipMemcpyHostToDevice, h->stream));
      MSW_HIP(hipStreamSynchronize(h->stream));
      why = inflate_device_guarded(cx, d_gz.p, n, m, chunk_bytes, nullptr, txt, total, last, info);
    } catch (const HipError &ex) {
      if (!strstr(ex.what(), "out of memory")) throw;
      (void)hipGetLastError();
      why = infl::kWhyMemory;
    }
    if (why == infl::kWhyNone) {
      pinned_reserve(S.pinned, std::max<size_t>(total, 1), 0);
      if (total) MSW_HIP(hipMemcpyAsync(S.pinned.p, txt.p, total, hipMemcpyDeviceToHost, h->stream));
      MSW_HIP(hipStreamSynchronize(h->stream));
      *text_out = reinterpret_cast<const uint8_t *>(S.pinned.p);
      len = total;
    }
  }
  if (why != infl::kWhyNone) {
    inflate_host_members(gz, n, S.host_text);
    if (S.host_text.empty()) S.host_text.reserve(1);
    *text_out = reinterpret_cast<const uint8_t *>(S.host_text.data());
    len = S.host_text.size();
    info.text_bytes = len;
  }
  *len_out = len;
  info.on_device = why == infl::kWhyNone ? 1 : 0;
  info.fallback_reason = why;
  if (info_out) *info_out = info;
}

void last_inflate_impl(msw_core *h, msw_inflate_info *info, size_t max_files, size_t *n_files) {
  const std::vector<msw_inflate_info> &L = h->inf.last;
  if (n_files) *n_files = L.size();
  if (info)
    for (size_t i = 0; i < std::min(max_files, L.size()); ++i) info[i] = L[i];
}

}  // namespace
