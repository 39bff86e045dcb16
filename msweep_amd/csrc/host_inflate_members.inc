// host_inflate_members.inc -- BGZF (bgzip) pseudoalignment input inflated on the device, per member (included by
// input.hip behind host_inflate.inc, which calls in here; kernel: inflate_member_kernels.hpp, format and walk:
// inflate_format.hpp).  A gzip file whose first member carries BGZF's 'BC' subfield is walked -- headers and trailers
// only -- into the table of its members: payload bits, CRC-32, ISIZE and the text offset of each.  The text's length is
// known from the trailers, so it is allocated once, and one launch decodes every member at its offset and checks it
// against its own trailer.  No probe, no windows, no chain, no second pass; inflate_max_span does not apply: a member is
// at most 64 KiB.  The file's promise per member is the guarantee: the device's text is used only when every member ends
// in its last payload byte with the length and the CRC-32 its trailer states.  A file that starts like BGZF and does not
// walk to its end (a plain member behind BGZF ones, a damaged BSIZE, trailing bytes, a cut last member) is "header"; a
// member's decode status, framing and CRC give "chunk status", "trailing bytes" and "crc"; the host path then stands,
// result and messages unchanged (a corrupt member is zlib's error).  Files whose first member does not declare its
// length never come here: host_inflate.inc's single-member path, reasons and all, is theirs.
namespace {

static_assert(sizeof(msw_inflate_info) == 96 && offsetof(msw_inflate_info, kernel_ms) == 40 && offsetof(msw_inflate_info, n_members) == 36,
              "msw_inflate_info: n_members fills the padding behind fallback_reason; size and the other offsets stand");

// does the file start with a member that declares its length?  (head: its first bytes)
bool first_member_declares_length(const uint8_t *head, uint64_t avail) {
  uint32_t bsize = 0;
  return infl::member_bsize(head, avail, &bsize);
}

struct FileFetch {  // the walk's source for a file: pread
  int fd;
  bool operator()(uint64_t off, size_t len, uint8_t *dst) const {
    size_t got_all = 0;
    while (got_all < len) {
      const ssize_t got = pread(fd, dst + got_all, len - got_all, (off_t)(off + got_all));
      if (got <= 0) return false;
      got_all += (size_t)got;
    }
    return true;
  }
};

// The members of table T of a file of n bytes that lies in d_gz (inflate_words(n) words, zero behind the n bytes) once
// `copied` (may be null) has happened: decoded and checked.  Returns infl::kWhyNone with the text in `txt` (padded with
// line feeds as upload_text pads it), its length and its last byte; any other reason: nothing of `txt` counts.  Fills
// info but for on_device, fallback_reason and upload_ms.
int32_t inflate_members_device(ReaderCtx &cx, const uint32_t *d_gz, uint64_t n, const infl::MemberTable &T, hipEvent_t copied,
                               RBuf<unsigned char> &txt, uint64_t &total_out, unsigned char &last_out, msw_inflate_info &info) {
  InflateState &S = *cx.inf;
  hipStream_t st = cx.st;
  const uint64_t total = T.text_bytes;
  info.payload_bytes = T.payload_bytes;
  info.text_bytes = total;
  info.chunk_bytes = 0;
  if (T.members.size() >= (1ull << 31)) return infl::kWhyMemory;
  const uint32_t n_members = (uint32_t)T.members.size();
  info.n_members = info.n_chunks = info.n_starts = n_members;
  for (auto &e : S.ev)
    if (!e) MSW_HIP(hipEventCreate(&e));
  if (!S.pow8.p) {
    defl::crc_pow_table(S.pow8_host);
    S.pow8.upload(S.pow8_host, 40, st);
  }
  // ---- memory: the text and the table (the compressed bytes are there already; there are no windows)
  const uint64_t padded = (total + kTileBytes - 1) / kTileBytes * kTileBytes + kTileBytes;
  const uint64_t table_bytes = (uint64_t)n_members * sizeof(infl::MemberEntry);
  size_t free_b = 0, total_b = 0;
  MSW_HIP(hipMemGetInfo(&free_b, &total_b));
  if (padded + table_bytes + (1ull << 28) > (uint64_t)free_b + cx.pool->idle_bytes()) return infl::kWhyMemory;
  RBuf<infl::MemberEntry> members(cx);
  RBuf<unsigned long long> bad(cx);
  members.alloc(n_members), bad.alloc(2);
  txt.alloc(padded);
  MSW_HIP(hipMemsetAsync(txt.p + total, '\n', padded - total, st));
  MSW_HIP(hipMemcpyAsync(members.p, T.members.data(), table_bytes, hipMemcpyHostToDevice, st));
  static const unsigned long long none_bad[2] = {kInfmAllGood, 0};
  unsigned long long h_bad[2] = {0, 0};
  MSW_HIP(hipMemcpyAsync(bad.p, none_bad, sizeof none_bad, hipMemcpyHostToDevice, st));
  if (copied) MSW_HIP(hipStreamWaitEvent(st, copied, 0));
  // ---- decode and trailer check, a wavefront per member (the pair of events lies directly around the launch)
  MSW_HIP(hipEventRecord(S.ev[0], st));
  hipLaunchKernelGGL(k_infm_decode, dim3(n_members), dim3(kWave), 0, st, d_gz, (uint64_t)inflate_words(n), members.p, n_members,
                     S.pow8.p, txt.p, bad.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(S.ev[1], st));
  unsigned char last = '\n';
  MSW_HIP(hipMemcpyAsync(h_bad, bad.p, sizeof h_bad, hipMemcpyDeviceToHost, st));
  if (total) MSW_HIP(hipMemcpyAsync(&last, txt.p + total - 1, 1, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
  info.write_ms = ms;  // (the check is fused into the decode: crc_ms, like probe_ms, window_ms and chain_ms, stays 0)
  info.kernel_ms = ms;
  if (h_bad[1] || h_bad[0] != kInfmAllGood) return (int32_t)(h_bad[0] & 0xff);
  total_out = total;
  last_out = last;
  return infl::kWhyNone;
}

// inflate_members_device, with an allocation that fails counted as "does not fit"
int32_t inflate_members_device_guarded(ReaderCtx &cx, const uint32_t *d_gz, uint64_t n, const infl::MemberTable &T, hipEvent_t copied,
                                       RBuf<unsigned char> &txt, uint64_t &total, unsigned char &last, msw_inflate_info &info) {
  try {
    return inflate_members_device(cx, d_gz, n, T, copied, txt, total, last, info);
  } catch (const HipError &ex) {
    if (!strstr(ex.what(), "out of memory")) throw;
    (void)hipGetLastError();
    return infl::kWhyMemory;
  }
}

// A gzip file of n bytes whose first member declares its length, for upload_gzip_device: the reason the host path takes
// the file, or infl::kWhyNone with t.txt, t.n and t.last set (the caller records t.done).  The walk reads headers and
// trailers on a thread of its own while the reader's threads stage the compressed bytes.
int32_t upload_members_device(int fd, const char *path, uint64_t n, ReaderCtx &cx, DevText &t, msw_inflate_info &info) {
  const auto t0 = std::chrono::steady_clock::now();
  RBuf<uint32_t> gz(cx);
  try {
    gz.alloc(inflate_words(n));
  } catch (const HipError &ex) {
    if (!strstr(ex.what(), "out of memory")) throw;
    (void)hipGetLastError();
    return infl::kWhyMemory;
  }
  hipStream_t cs = cx.stage->copy;
  if (!t.done) MSW_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  unsigned char *dev = reinterpret_cast<unsigned char *>(gz.p);
  MSW_HIP(hipMemsetAsync(dev + n, 0, inflate_words(n) * 4 - n, cs));
  infl::MemberTable T;
  bool walked = false;
  {
    std::thread walker([&] {
      try {
        walked = infl::walk_members(FileFetch{fd}, n, T);
      } catch (const std::exception &) {  // (the table does not fit the host: not this path's file)
        walked = false;
      }
    });
    struct Join {
      std::thread &th;
      ~Join() { th.join(); }
    } join{walker};
    unsigned char last_gz = 0;
    stage_to_device(fd, path, nullptr, n, dev, cx, last_gz);
  }
  MSW_HIP(hipEventRecord(t.done, cs));
  MSW_HIP(hipEventSynchronize(t.done));  // (the decode waits for the copy anyway: this only stops the clock)
  info.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!walked) return infl::kWhyHeader;
  return inflate_members_device_guarded(cx, gz.p, n, T, t.done, t.txt, t.n, t.last, info);
  // (the compressed block goes back to the pool here, behind the kernel that reads it: the stream is idle)
}

// The same for bytes in host memory, for msw_core_inflate_gzip: the reason, or infl::kWhyNone with the text in the
// handle's pinned buffer
int32_t inflate_members_bytes(msw_core *h, const uint8_t *gz, size_t n, const uint8_t **text_out, size_t *len_out, msw_inflate_info &info) {
  InflateState &S = h->inf;
  infl::MemberTable T;
  if (!infl::walk_members(infl::BufferFetch{gz, n}, n, T)) return infl::kWhyHeader;
  ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
  cx.inf = &S;
  RBuf<uint32_t> d_gz(cx);
  RBuf<unsigned char> txt(cx);
  uint64_t total = 0;
  unsigned char last = '\n';
  int32_t why = infl::kWhyNone;
  try {
    d_gz.alloc(inflate_words(n));
    MSW_HIP(hipMemsetAsync(reinterpret_cast<unsigned char *>(d_gz.p) + n, 0, inflate_words(n) * 4 - n, h->stream));
    MSW_HIP(hipMemcpyAsync(d_gz.p, gz, n, hipMemcpyHostToDevice, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
    why = inflate_members_device_guarded(cx, d_gz.p, n, T, nullptr, txt, total, last, info);
  } catch (const HipError &ex) {
    if (!strstr(ex.what(), "out of memory")) throw;
    (void)hipGetLastError();
    why = infl::kWhyMemory;
  }
  if (why != infl::kWhyNone) return why;
  pinned_reserve(S.pinned, std::max<size_t>(total, 1), 0);
  if (total) MSW_HIP(hipMemcpyAsync(S.pinned.p, txt.p, total, hipMemcpyDeviceToHost, h->stream));
  MSW_HIP(hipStreamSynchronize(h->stream));
  *text_out = reinterpret_cast<const uint8_t *>(S.pinned.p);
  *len_out = total;
  return infl::kWhyNone;
}

}  // namespace
