// host_gzip.inc -- msw_core_gzip_* / msw_core_text_block_gzip (included by output.hip): --compress z, the gzip
// stream of a text output compressed on the device (deflate_kernels.hpp).  One stream may be open per handle; every call
// returns the bytes to append to the file in the handle's pinned buffer.  Per call: the text where it lies (a text block:
// its finished text, text_block_finish of host_text.inc, whose other sink this file is; host bytes: uploaded), the parse
// and the CRC, an exclusive scan of the chunks' byte lengths, the emit pass, one copy of the compressed bytes.  Device
// memory beside the text: 4 bytes of token scratch per byte of text, the compressed bytes, O(chunks) tables; nothing of
// that size goes to the host.  The handle keeps the running CRC register and length: a call's CRC value joins them with
// one multiplication by x^(8 n) on the host.
// MSWEEP_HOST_GZIP=1 (developer switch, read at begin): the same calls bring the plain text to the host and compress it
// with zlib at the requested level -- the reference's method (src/OutfileDesignator.cpp:30-37), the other side of the A/B.
namespace {

constexpr size_t kGzMaxBytes = (size_t)1 << 30;  // host bytes of one append

}  // namespace

// (from here to gz_host_deflate: what msw_fastq_next_gzip of input.hip also calls -- host_api.hpp)
void msw::host::gz_require_open(msw_core *h, const char *who) {
  if (!h->gz.open) throw Fail(std::string(who) + ": no gzip stream is open on this handle (msw_core_gzip_begin)");
}

void msw::host::gz_return(msw_core *h, size_t used, const char **out, size_t *len) {
  pinned_reserve(h->gz.pinned, 1, 0);  // an empty result still points somewhere
  *out = h->gz.pinned.p;
  *len = used;
  h->gz.bytes_out += used;
}

// CRC-32 pieces of n bytes of text (k_gz_crc): also what the inflate path of input.hip checks its output with
void msw::host::gz_crc_launch(int n_cu, hipStream_t st, const uint8_t *text, uint64_t n, const uint32_t *pow8, uint32_t *crc) {
  const size_t pieces = (size_t)((n + kGzCrcPiece - 1) / kGzCrcPiece);
  hipLaunchKernelGGL(k_gz_crc, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((pieces + 255) / 256, (size_t)n_cu * 32))), dim3(256),
                     0, st, text, n, pow8, crc);
}

// the chunks of the n bytes of text at d (device memory, 16-byte aligned, readable up to the next multiple of 4)
// appended to the pinned buffer at `used`; returns the bytes appended
size_t msw::host::gz_compress_device(msw_core *h, const uint8_t *d, size_t n, size_t used) {
  GzState &Z = h->gz;
  if (n == 0) return 0;
  hipStream_t st = h->stream;
  const size_t nch = (n + kGzChunk - 1) / kGzChunk;
  const bool stored_only = Z.level == 0;
  if (!stored_only) Z.tokens.alloc(nch * kGzChunk);
  Z.tables.alloc(nch * kGzSyms);
  Z.meta.alloc(nch);
  Z.len.alloc(nch + 1);
  Z.off.alloc(nch + 1);
  Z.crc.alloc(1);
  MSW_HIP(hipMemsetAsync(Z.len.p + nch, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemsetAsync(Z.crc.p, 0, sizeof(uint32_t), st));
  for (auto &e : Z.ev)
    if (!e) MSW_HIP(hipEventCreate(&e));
  MSW_HIP(hipEventRecord(Z.ev[0], st));
  hipLaunchKernelGGL(k_gz_parse, dim3((unsigned)nch), dim3(kWave), 0, st, d, (uint64_t)n, (uint32_t)nch, stored_only ? 1 : 0,
                     Z.tokens.p, Z.tables.p, Z.meta.p, Z.len.p);
  MSW_HIP(hipGetLastError());
  gz_crc_launch(h->n_cu, st, d, (uint64_t)n, Z.pow8.p, Z.crc.p);
  MSW_HIP(hipGetLastError());
  const uint64_t total = scan_lengths(Z.len.p, Z.off.p, nch, Z.tmp, Z.ev[1], st);
  if (total > n + 10 * nch) throw Fail("msw_core_gzip: the chunks' lengths exceed their stored form");
  Z.out.alloc(((total + 3) & ~(uint64_t)3) + 4);
  pinned_reserve(Z.pinned, used + total, used);
  MSW_HIP(hipEventRecord(Z.ev[2], st));
  hipLaunchKernelGGL(k_gz_emit, dim3((unsigned)nch), dim3(kWave), 0, st, d, (uint64_t)n, (uint32_t)nch, Z.tokens.p, Z.tables.p,
                     Z.meta.p, Z.off.p, Z.out.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipEventRecord(Z.ev[3], st));
  uint32_t r = 0;
  MSW_HIP(hipMemcpyAsync(&r, Z.crc.p, sizeof r, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipMemcpyAsync(Z.pinned.p + used, Z.out.p, total, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  float ms_a = 0.f, ms_b = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms_a, Z.ev[0], Z.ev[1]));
  MSW_HIP(hipEventElapsedTime(&ms_b, Z.ev[2], Z.ev[3]));
  Z.kernel_ms += (double)ms_a + (double)ms_b;
  Z.crc_reg = defl::crc_shift(Z.crc_reg, n, Z.pow8_host) ^ r;
  Z.isize += n;
  return total;
}

// the same for n bytes of pageable host memory: uploaded (16 bytes of slack behind the next multiple of 16), the copy
// complete before anything that can fail runs
size_t msw::host::gz_compress_host(msw_core *h, const char *bytes, size_t n, size_t used) {
  GzState &Z = h->gz;
  if (n == 0) return 0;
  Z.in.alloc(((n + 15) & ~(size_t)15) + 16);
  MSW_HIP(hipMemcpyAsync(Z.in.p, bytes, n, hipMemcpyHostToDevice, h->stream));
  MSW_HIP(hipStreamSynchronize(h->stream));
  return gz_compress_device(h, Z.in.p, n, used);
}

// MSWEEP_HOST_GZIP=1: n bytes of host text through zlib; what it gives out appended at `used`
size_t msw::host::gz_host_deflate(msw_core *h, const char *p, size_t n, int flush, size_t used) {
  GzState &Z = h->gz;
  z_stream &zs = *Z.zs;
  size_t got = 0, left = n;
  zs.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(p));
  do {
    const size_t in_now = std::min<size_t>(left, (size_t)1 << 30);
    zs.avail_in = (uInt)in_now;
    left -= in_now;
    do {  // (zlib's idiom: room left over means the input is used up)
      pinned_reserve(Z.pinned, used + got + ((size_t)1 << 18), used + got);
      const size_t room = std::min<size_t>(Z.pinned.cap - used - got, (size_t)1 << 30);
      zs.next_out = reinterpret_cast<Bytef *>(Z.pinned.p + used + got);
      zs.avail_out = (uInt)room;
      if (::deflate(&zs, left ? Z_NO_FLUSH : flush) == Z_STREAM_ERROR) throw Fail("msw_core_gzip: zlib's deflate failed");
      got += room - zs.avail_out;
    } while (zs.avail_out == 0);
  } while (left);
  Z.isize += n;
  return got;
}

namespace {

void gz_close(GzState &Z) {
  if (Z.zs) {
    (void)deflateEnd(Z.zs.get());
    Z.zs.reset();
  }
  Z.open = false;
}

void gzip_begin_impl(msw_core *h, int level, const char **out, size_t *len) {
  GzState &Z = h->gz;
  if (!out || !len) throw Fail("msw_core_gzip_begin: null out or len");
  if (Z.open) throw Fail("msw_core_gzip_begin: a gzip stream is open on this handle already (msw_core_gzip_end closes it)");
  if (level < 0 || level > 9) throw Fail("msw_core_gzip_begin: compression level " + std::to_string(level) + " is outside 0 ... 9");
  const char *e = getenv("MSWEEP_HOST_GZIP");
  Z.host = e && e[0] == '1';
  Z.level = level;
  Z.crc_reg = 0xffffffffu;
  Z.isize = 0;
  Z.kernel_ms = 0.0;
  Z.bytes_out = 0;
  size_t used = 0;
  if (Z.host) {
    Z.zs.reset(new z_stream());
    if (deflateInit2(Z.zs.get(), level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) {
      Z.zs.reset();
      throw Fail("msw_core_gzip_begin: zlib's deflateInit2 failed");
    }
  } else {
    if (!Z.pow8.p) {
      defl::crc_pow_table(Z.pow8_host);
      Z.pow8.upload(Z.pow8_host, 40, h->stream);
      MSW_HIP(hipStreamSynchronize(h->stream));
    }
    // RFC 1952: magic, CM 8, no flags, mtime 0, XFL 0, OS 255 (unknown)
    static const unsigned char head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255};
    pinned_reserve(Z.pinned, sizeof head, 0);
    std::memcpy(Z.pinned.p, head, sizeof head);
    used = sizeof head;
  }
  Z.open = true;
  gz_return(h, used, out, len);
}

void gzip_append_impl(msw_core *h, const char *bytes, size_t n, const char **out, size_t *len) {
  GzState &Z = h->gz;
  if (!out || !len) throw Fail("msw_core_gzip_append: null out or len");
  gz_require_open(h, "msw_core_gzip_append");
  if (n && !bytes) throw Fail("msw_core_gzip_append: null bytes");
  if (n > kGzMaxBytes) throw Fail("msw_core_gzip_append: at most 1 GiB fits one call");
  size_t used = 0;
  if (Z.host) {
    if (n) used = gz_host_deflate(h, bytes, n, Z_NO_FLUSH, 0);
  } else {
    used = gz_compress_host(h, bytes, n, 0);
  }
  gz_return(h, used, out, len);
}

void gzip_end_impl(msw_core *h, const char **out, size_t *len) {
  GzState &Z = h->gz;
  if (!out || !len) throw Fail("msw_core_gzip_end: null out or len");
  gz_require_open(h, "msw_core_gzip_end");
  size_t used = 0;
  if (Z.host) {
    used = gz_host_deflate(h, nullptr, 0, Z_FINISH, 0);
  } else {
    // the final empty fixed block, CRC-32 and ISIZE (mod 2^32), little-endian
    const uint32_t crc = ~Z.crc_reg, isize = (uint32_t)Z.isize;
    unsigned char tail[10] = {0x03, 0x00};
    for (int i = 0; i < 4; ++i) {
      tail[2 + i] = (unsigned char)(crc >> (8 * i));
      tail[6 + i] = (unsigned char)(isize >> (8 * i));
    }
    pinned_reserve(Z.pinned, sizeof tail, 0);
    std::memcpy(Z.pinned.p, tail, sizeof tail);
    used = sizeof tail;
  }
  gz_close(Z);
  gz_return(h, used, out, len);
}

// the gzip sink: the finished text of a block compressed where it lies; returns the bytes appended at `used`
size_t text_sink_gzip(msw_core *h, const TextDone &D, size_t used) {
  return D.dev ? gz_compress_device(h, D.dev, D.len, used) : gz_compress_host(h, D.host.data(), D.len, used);
}

void text_block_gzip_impl(msw_core *h, int what, size_t e0, size_t e1, const uint64_t *prefix, size_t n_zero, const char **out,
                          size_t *len, size_t *n_host_out, size_t *text_len_out) {
  GzState &Z = h->gz;
  if (!out || !len) throw Fail("msw_core_text_block_gzip: null out or len");
  gz_require_open(h, "msw_core_text_block_gzip");
  size_t used = 0, n_host = 0, text_len = 0;
  if (Z.host) {
    const char *text = nullptr;
    text_block_impl(h, what, e0, e1, prefix, n_zero, &text, &text_len, &n_host);
    if (text_len) used = gz_host_deflate(h, text, text_len, Z_NO_FLUSH, 0);
  } else {
    text_block_check(h, what, e0, e1, prefix, n_zero);
    text_block_each(h, what, e0, e1, prefix, [&](uint32_t G, size_t w, size_t j0, const uint64_t *pre) {
      const TextDone D = text_block_finish(h, what, G, w, j0, pre, n_zero, n_host);
      text_len += D.len;
      used += text_sink_gzip(h, D, used);
    });
  }
  gz_return(h, used, out, len);
  if (n_host_out) *n_host_out = n_host;
  if (text_len_out) *text_len_out = text_len;
}

}  // namespace
