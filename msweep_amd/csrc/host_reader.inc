// host_reader.inc -- the Themisto plaintext reader on the device (included by input.hip behind
// host_alignment.inc; kernels: reader_kernels.hpp).  Round 5: text -> equivalence classes was 1.5 of the 1.65 s from two
// strands of 10 M reads to abundances.txt, on 16 host threads; here the text goes to HBM as it is read (pinned staging,
// two chunks in flight) and every stage of host_alignment.inc -- parse, rows by read id, sorted sets, paired-end merge,
// hash, sort, classes -- is a streaming kernel or a rocPRIM scan / radix sort over it.  The outcome is the host reader's,
// array for array (tests/test_gpu_reader.py); the arrays stay on the device for msw_core_build_likelihood_aln.
//
// Text the host parser would not take silently (any byte besides digits, blanks, line ends; an id beyond 32 bits;
// a target id out of range) is NOT judged here: the kernels raise a flag and the file goes to the host reader, whose
// outcome -- a result or the reference's error message -- is final (ReaderFallback).
namespace {

struct ReaderFallback {};  // the text needs the host parser

// out[i] = in[0] + .. + in[i - 1] for i in [0, n): with in[n - 1] a spare zero, out[n - 1] is the total
struct ReaderCtx;
void scan_u32_u64(const uint32_t *in, uint64_t *out, size_t n, ReaderCtx &cx);
uint64_t fetch_u64(const uint64_t *d, hipStream_t st) {
  uint64_t v = 0;
  MSW_HIP(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  return v;
}
ReaderCtr fetch_ctr(const ReaderCtr *d, hipStream_t st) {
  ReaderCtr c = {};
  MSW_HIP(hipMemcpyAsync(&c, d, sizeof c, hipMemcpyDeviceToHost, st));
  MSW_HIP(hipStreamSynchronize(st));
  return c;
}
inline unsigned reader_grid(uint64_t n, int n_cu) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)n_cu * 32));
}

// Device buffers of the reader come from the handle's ReaderPool (reader_kernels.hpp) and go back to it: no hipMalloc
// on a repeated call, no hipFree while the handle lives.
struct ReaderCtx;
template <class T>
struct RBuf : DevBuf<T> {
  ReaderCtx *cx;
  explicit RBuf(ReaderCtx &c) : cx(&c) {}
  ~RBuf();
  void alloc(size_t count);
};
struct ReaderCtx {
  hipStream_t st;
  int n_cu;
  TextStager *stage;
  ReaderPool *pool;
  int device = 0;
  InflateState *inf = nullptr;      // the handle's gzip-input state (host_inflate.inc)
  RBuf<unsigned char> tmp{*this};   // rocPRIM's temporary storage
  RBuf<ReaderCtr> ctr{*this};
  bool timing = false;
  std::chrono::steady_clock::time_point t0;
  ReaderCtx(hipStream_t s, int cus, TextStager *sg, ReaderPool *pl, int dev) : st(s), n_cu(cus), stage(sg), pool(pl), device(dev) {}
  ReaderCtx(const ReaderCtx &) = delete;
  ReaderCtx &operator=(const ReaderCtx &) = delete;
  template <class T>
  void drop(DevBuf<T> &b) {
    if (b.p) pool->give(b.p);
    b.p = nullptr;
    b.n = 0;
  }
  unsigned char *scratch(size_t bytes) {  // grows, never shrinks
    tmp.alloc(bytes);
    return tmp.p;
  }
  void mark(const char *what) {
    if (!timing) return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[msweep reader/device] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};
template <class T>
RBuf<T>::~RBuf() { cx->drop(*this); }
template <class T>
void RBuf<T>::alloc(size_t count) {
  if (count <= this->n && this->p) return;
  cx->drop(*this);
  if (count == 0) count = 1;
  this->p = static_cast<T *>(cx->pool->take(count * sizeof(T)));
  this->n = count;
}

struct DevStrand {
  RBuf<uint64_t> ptr;   // [n_ids + 1]
  RBuf<uint32_t> tgt;
  uint64_t n_ids = 0, n_lines = 0, n_hits = 0;
  explicit DevStrand(ReaderCtx &c) : ptr(c), tgt(c) {}
};

void scan_u32_u64(const uint32_t *in, uint64_t *out, size_t n, ReaderCtx &cx) {
  if (!n) return;
  size_t bytes = 0;
  MSW_HIP(prim_scan(nullptr, bytes, in, out, n, cx.st));
  unsigned char *tmp = cx.scratch(bytes);
  MSW_HIP(prim_scan(tmp, bytes, in, out, n, cx.st));
}

// The text of one file in device memory, padded with line feeds to whole tiles (+ one: the parse kernel reads 16 bytes
// behind every segment).  Plain files are read with pread() on the reader's threads straight into pinned memory, one
// chunk on its way to the device while the next is read; gzip files travel compressed and are inflated by the kernels
// of inflate_kernels.hpp (host_inflate.inc), or, where that result cannot be vouched for, by the host reader's slurp_text.
// The copies run on the stager's own stream (`done` marks the last one): read_alignment_device sends the NEXT strand's
// text while this strand's kernels run.
struct DevText {
  RBuf<unsigned char> txt;
  uint64_t n = 0;
  unsigned char last = '\n';
  hipEvent_t done = nullptr;
  explicit DevText(ReaderCtx &cx) : txt(cx) {}
  DevText(const DevText &) = delete;
  DevText &operator=(const DevText &) = delete;
  ~DevText() {
    if (done) (void)hipEventDestroy(done);
  }
};
// n bytes -- of the open file fd, or of host memory `mem` when that is not null -- to dev through the stager, on its copy
// stream; last: the last of them
// bytes: when given, no more threads (pinned sub-buffers: ~0.4 ms per MB to pin) than that many bytes have blocks -- the
// likelihood-file reader's choice, whose small files would otherwise pay for 64 MB of staging; the Themisto reader, whose
// strands are sent while the previous one's kernels run, keeps the stager at its full size
void stager_ready(ReaderCtx &cx, uint64_t bytes = ~0ull) {
  // (reader threads: beyond ~8 the page-cache copies of these hosts stop scaling and only contend; MSWEEP_READER_THREADS
  // decides when set)
  size_t T0 = getenv("MSWEEP_READER_THREADS") ? reader_threads() : std::min<size_t>(reader_threads(), 8);
  if (bytes != ~0ull) {
    const uint64_t B = cx.stage->block_bytes();
    T0 = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(T0, (bytes + B - 1) / B));
  }
  cx.stage->ready(T0);
}
void stage_to_device(int fd, const char *path, const char *mem, uint64_t n, unsigned char *dev, ReaderCtx &cx, unsigned char &last_out,
                     const char *noun = "pseudoalignment file") {
  const size_t B = cx.stage->block;
  const size_t T = std::max<size_t>(1, std::min<size_t>(cx.stage->threads, (size_t)((n + B - 1) / B)));
  hipStream_t cs = cx.stage->copy;
  if (!n) return;
  unsigned char last = '\n';
  run_threads(T, [&](size_t k) {
    MSW_HIP(hipSetDevice(cx.device));
    int slot = 0;
    for (uint64_t blk = k; blk * B < n; blk += T, slot ^= 1) {
      const uint64_t off = blk * B;
      const size_t len = (size_t)std::min<uint64_t>(B, n - off);
      hipEvent_t e = cx.stage->ev[2 * k + slot];
      MSW_HIP(hipEventSynchronize(e));  // the copy that last read this sub-buffer is done (never recorded: returns at once)
      char *dst = cx.stage->sub(k, slot);
      if (!mem) {
        size_t got_all = 0;
        while (got_all < len) {
          const ssize_t got = pread(fd, dst + got_all, len - got_all, (off_t)(off + got_all));
          if (got <= 0) throw Fail(std::string("cannot read ") + noun + " " + path);
          got_all += (size_t)got;
        }
      } else {
        std::memcpy(dst, mem + off, len);
      }
      if (off + len == n) last = (unsigned char)dst[len - 1];
      MSW_HIP(hipMemcpyAsync(dev + off, dst, len, hipMemcpyHostToDevice, cs));
      MSW_HIP(hipEventRecord(e, cs));
    }
  });
  last_out = last;
}
bool upload_gzip_device(int fd, const char *path, uint64_t n, ReaderCtx &cx, DevText &t);  // host_inflate.inc
// noun: what the failure messages call the file (the likelihood-file reader is the other caller, host_likelihood_file.inc)
// fit_stager: the staging area sized by the file (stager_ready)
void upload_text(const char *path, ReaderCtx &cx, DevText &t, const char *noun = "pseudoalignment file", bool fit_stager = false) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) throw Fail(std::string("cannot open ") + noun + " " + path);
  struct FdGuard {
    int fd;
    ~FdGuard() { close(fd); }
  } guard{fd};
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) throw Fail(std::string("cannot open ") + noun + " " + path);
  unsigned char magic[6] = {0, 0, 0, 0, 0, 0};
  const ssize_t got_magic = pread(fd, magic, std::min<size_t>((size_t)sb.st_size, 6), 0);
  (void)got_magic;
  const bool plain = !(magic[0] == 0x1f && magic[1] == 0x8b) && !(magic[0] == 'B' && magic[1] == 'Z' && magic[2] == 'h') &&
                     !(magic[0] == 0xFD && magic[1] == '7' && magic[2] == 'z' && magic[3] == 'X' && magic[4] == 'Z');
  stager_ready(cx, fit_stager ? (uint64_t)sb.st_size : ~0ull);
  // a gzip file goes to the device compressed and is inflated there (host_inflate.inc); where that result cannot be
  // vouched for, the host path below stands
  if (magic[0] == 0x1f && magic[1] == 0x8b && cx.inf && upload_gzip_device(fd, path, (uint64_t)sb.st_size, cx, t)) return;
  if (plain && cx.inf) {
    msw_inflate_info info = {};
    info.text_bytes = (uint64_t)sb.st_size;
    cx.inf->last.push_back(info);
  }
  FileText ft;
  if (!plain) slurp_text(path, ft);  // (inflates gzip; names bzip2 / xz as unsupported)
  const uint64_t n = t.n = plain ? (uint64_t)sb.st_size : (uint64_t)ft.size;
  hipStream_t cs = cx.stage->copy;
  if (!t.done) MSW_HIP(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  const uint64_t padded = (n + kTileBytes - 1) / kTileBytes * kTileBytes + kTileBytes;
  t.txt.alloc(padded);
  MSW_HIP(hipMemsetAsync(t.txt.p + n, '\n', padded - n, cs));
  t.last = '\n';
  stage_to_device(fd, path, plain ? nullptr : ft.data, n, t.txt.p, cx, t.last, noun);
  MSW_HIP(hipEventRecord(t.done, cs));
}

// text -> rows by read id, every row an ascending set (read_strand of host_alignment.inc)
void device_strand(DevText &text, size_t n_targets, ReaderCtx &cx, DevStrand &s) {
  hipStream_t st = cx.st;
  RBuf<unsigned char> &txt = text.txt;
  const uint64_t n = text.n;
  const unsigned char last = text.last;
  MSW_HIP(hipStreamWaitEvent(st, text.done, 0));
  s.n_ids = s.n_lines = s.n_hits = 0;
  s.ptr.alloc(1);
  MSW_HIP(hipMemsetAsync(s.ptr.p, 0, sizeof(uint64_t), st));
  if (!n) return;
  if (n >= (1ull << 40)) throw ReaderFallback{};
  cx.ctr.alloc(1);
  cx.ctr.zero(st);
  // ---- tokens ----
  const uint64_t n_tiles = (n + kTileBytes - 1) / kTileBytes;
  RBuf<uint32_t> cnt_tok(cx), cnt_nl(cx);
  RBuf<uint64_t> base_tok(cx), base_nl(cx);
  cnt_tok.alloc(n_tiles + 1), cnt_nl.alloc(n_tiles + 1);
  base_tok.alloc(n_tiles + 1), base_nl.alloc(n_tiles + 1);
  MSW_HIP(hipMemsetAsync(cnt_tok.p + n_tiles, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemsetAsync(cnt_nl.p + n_tiles, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_text_count, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, txt.p, n, cnt_tok.p, cnt_nl.p, cx.ctr.p);
  MSW_HIP(hipGetLastError());
  scan_u32_u64(cnt_tok.p, base_tok.p, n_tiles + 1, cx);
  scan_u32_u64(cnt_nl.p, base_nl.p, n_tiles + 1, cx);
  const uint64_t n_tok = fetch_u64(base_tok.p + n_tiles, st), n_nl = fetch_u64(base_nl.p + n_tiles, st);
  if (fetch_ctr(cx.ctr.p, st).flags) throw ReaderFallback{};
  const uint64_t n_lines = n_nl + (last != '\n' ? 1 : 0);
  if (n_lines >= 0xffffffffull || n_tok < n_lines) throw ReaderFallback{};
  RBuf<uint32_t> tokens(cx);
  RBuf<uint64_t> line_first(cx);
  tokens.alloc(n_tok);
  line_first.alloc(n_lines + 1);
  const uint64_t ends[2] = {0, n_tok};
  MSW_HIP(hipMemcpyAsync(line_first.p, &ends[0], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MSW_HIP(hipMemcpyAsync(line_first.p + n_lines, &ends[1], sizeof(uint64_t), hipMemcpyHostToDevice, st));
  RBuf<uint32_t> tile_max(cx);
  tile_max.alloc(n_tiles);
  hipLaunchKernelGGL(k_text_parse, dim3((unsigned)n_tiles), dim3(kTileThreads), 0, st, txt.p, n, base_tok.p, base_nl.p,
                     (uint32_t)n_targets, tokens.p, line_first.p, tile_max.p, cx.ctr.p);
  hipLaunchKernelGGL(k_max_u32, dim3(1), dim3(1024), 0, st, tile_max.p, n_tiles, &cx.ctr.p->max_id);
  MSW_HIP(hipGetLastError());
  const ReaderCtr c1 = fetch_ctr(cx.ctr.p, st);  // (also: `ends` has been read)
  if (c1.flags) throw ReaderFallback{};
  cx.drop(txt);
  cx.mark("tokens");
  // ---- rows by read id ----
  const uint64_t n_ids = std::min<uint64_t>((uint64_t)c1.max_id + 1, n_lines);
  RBuf<uint32_t> cnt(cx), cur(cx);
  cnt.alloc(n_ids + 1), cur.alloc(n_ids + 1);
  cnt.zero(st), cur.zero(st);
  hipLaunchKernelGGL(k_row_count, dim3(reader_grid(n_lines, cx.n_cu)), dim3(256), 0, st, tokens.p, line_first.p, n_lines, n_ids,
                     cnt.p);
  s.ptr.alloc(n_ids + 1);
  scan_u32_u64(cnt.p, s.ptr.p, n_ids + 1, cx);
  uint64_t hits = fetch_u64(s.ptr.p + n_ids, st);
  RBuf<uint32_t> raw(cx);
  raw.alloc(hits);
  hipLaunchKernelGGL(k_row_fill, dim3(reader_grid(n_lines, cx.n_cu)), dim3(256), 0, st, tokens.p, line_first.p, n_lines, n_ids,
                     s.ptr.p, cur.p, raw.p);
  MSW_HIP(hipGetLastError());
  // ---- every row an ascending set ----
  RBuf<uint32_t> flen(cx);
  flen.alloc(n_ids + 1);
  MSW_HIP(hipMemsetAsync(flen.p + n_ids, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_row_check, dim3(reader_grid(n_ids, cx.n_cu)), dim3(256), 0, st, s.ptr.p, raw.p, n_ids, flen.p, cx.ctr.p);
  MSW_HIP(hipGetLastError());
  const ReaderCtr c2 = fetch_ctr(cx.ctr.p, st);
  cx.drop(tokens);
  cx.drop(line_first);
  cx.mark("rows by read id");
  if (c2.unsorted) {
    // short rows (nearly all): sorted by the wavefront that finds them; rows of more than 64 targets as (row, target)
    // keys through a radix sort
    hipLaunchKernelGGL(k_rows_sort_short, dim3(reader_grid(n_ids, cx.n_cu)), dim3(256), 0, st, s.ptr.p, raw.p, n_ids, flen.p,
                       cnt.p, cx.ctr.p);
    MSW_HIP(hipGetLastError());
    if (fetch_ctr(cx.ctr.p, st).long_rows) {
      RBuf<uint64_t> foff(cx), keys(cx), keys2(cx), kidx(cx);
      RBuf<uint32_t> keep(cx);
      foff.alloc(n_ids + 1);
      scan_u32_u64(flen.p, foff.p, n_ids + 1, cx);
      const uint64_t m = fetch_u64(foff.p + n_ids, st);
      keys.alloc(m), keys2.alloc(m), keep.alloc(m + 1), kidx.alloc(m + 1);
      hipLaunchKernelGGL(k_row_keys, dim3(reader_grid(n_ids, cx.n_cu)), dim3(256), 0, st, s.ptr.p, raw.p, n_ids, flen.p, foff.p,
                         keys.p);
      size_t bytes = 0;
      MSW_HIP(prim_sort_keys(nullptr, bytes, keys.p, keys2.p, (size_t)m, 64u, st));
      MSW_HIP(prim_sort_keys(cx.scratch(bytes), bytes, keys.p, keys2.p, (size_t)m, 64u, st));
      MSW_HIP(hipMemsetAsync(keep.p + m, 0, sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_keys_keep, dim3(reader_grid(m, cx.n_cu)), dim3(256), 0, st, keys2.p, m, keep.p);
      scan_u32_u64(keep.p, kidx.p, m + 1, cx);
      hipLaunchKernelGGL(k_rows_sorted_back, dim3(reader_grid(std::max(m, n_ids), cx.n_cu)), dim3(256), 0, st, keys2.p, keep.p,
                         kidx.p, s.ptr.p, flen.p, foff.p, n_ids, m, raw.p, cnt.p, cx.ctr.p);
      MSW_HIP(hipGetLastError());
    }
    if (fetch_ctr(cx.ctr.p, st).shrunk) {  // rows lost duplicates: laid end to end again
      RBuf<uint64_t> nptr(cx);
      RBuf<uint32_t> packed(cx);
      nptr.alloc(n_ids + 1);
      scan_u32_u64(cnt.p, nptr.p, n_ids + 1, cx);  // (cnt[n_ids] = 0 still)
      hits = fetch_u64(nptr.p + n_ids, st);
      packed.alloc(hits);
      hipLaunchKernelGGL(k_rows_compact, dim3(reader_grid(n_ids, cx.n_cu)), dim3(256), 0, st, s.ptr.p, raw.p, cnt.p, nptr.p, n_ids,
                         packed.p);
      MSW_HIP(hipGetLastError());
      MSW_HIP(hipStreamSynchronize(st));
      std::swap(s.ptr.p, nptr.p), std::swap(s.ptr.n, nptr.n);
      std::swap(raw.p, packed.p), std::swap(raw.n, packed.n);
    }
    cx.mark("rows sorted");
  }
  std::swap(s.tgt.p, raw.p), std::swap(s.tgt.n, raw.n);
  s.n_ids = n_ids;
  s.n_lines = n_lines;
  s.n_hits = hits;
}

inline unsigned merge_grid(uint64_t n, int n_cu) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kMergeThreads - 1) / kMergeThreads, (uint64_t)n_cu * 64));
}
// merge_strands of host_alignment.inc: a = a (intersection | union) b, read by read
void device_merge(DevStrand &a, const DevStrand &b, bool intersect, ReaderCtx &cx) {
  hipStream_t st = cx.st;
  const uint64_t n = intersect ? std::min(a.n_ids, b.n_ids) : std::max(a.n_ids, b.n_ids);
  RBuf<uint32_t> len(cx), out(cx);
  RBuf<uint64_t> optr(cx);
  len.alloc(n + 1), optr.alloc(n + 1);
  MSW_HIP(hipMemsetAsync(len.p + n, 0, sizeof(uint32_t), st));
  if (n)
    hipLaunchKernelGGL(k_merge_rows<false>, dim3(merge_grid(n, cx.n_cu)), dim3(kMergeThreads), 0, st, a.ptr.p, a.tgt.p, a.n_ids, b.ptr.p,
                       b.tgt.p, b.n_ids, n, intersect ? 1 : 0, len.p, (const uint64_t *)nullptr, (uint32_t *)nullptr);
  scan_u32_u64(len.p, optr.p, n + 1, cx);
  const uint64_t hits = fetch_u64(optr.p + n, st);
  out.alloc(hits);
  if (n)
    hipLaunchKernelGGL(k_merge_rows<true>, dim3(merge_grid(n, cx.n_cu)), dim3(kMergeThreads), 0, st, a.ptr.p, a.tgt.p, a.n_ids, b.ptr.p,
                       b.tgt.p, b.n_ids, n, intersect ? 1 : 0, (uint32_t *)nullptr, optr.p, out.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(st));
  std::swap(a.ptr.p, optr.p), std::swap(a.ptr.n, optr.n);
  std::swap(a.tgt.p, out.p), std::swap(a.tgt.n, out.n);
  a.n_ids = n;
  a.n_lines = b.n_lines;  // the last strand's line count (:119)
  a.n_hits = hits;
}

// collapse() of host_alignment.inc into the device arrays of `out`
void device_collapse(const DevStrand &s, size_t n_targets, ReaderCtx &cx, msw_alignment &out) {
  hipStream_t st = cx.st;
  out.n_targets = n_targets;
  out.n_queries = s.n_lines;
  const uint64_t n = std::min(s.n_ids, s.n_lines);
  RBuf<uint32_t> flag(cx), ids(cx), head(cx), tlen(cx);
  RBuf<uint64_t> idx(cx), keys(cx), keys2(cx), eidx(cx);
  flag.alloc(n + 1), idx.alloc(n + 1);
  MSW_HIP(hipMemsetAsync(flag.p + n, 0, sizeof(uint32_t), st));
  if (n) hipLaunchKernelGGL(k_flag_aligned, dim3(reader_grid(n, cx.n_cu)), dim3(256), 0, st, s.ptr.p, n, flag.p);
  scan_u32_u64(flag.p, idx.p, n + 1, cx);
  const uint64_t K = fetch_u64(idx.p + n, st);
  keys.alloc(K), keys2.alloc(K), ids.alloc(K), out.d_reads.alloc(K);
  if (n) hipLaunchKernelGGL(k_hash_reads, dim3(reader_grid(n, cx.n_cu)), dim3(256), 0, st, s.ptr.p, s.tgt.p, n, idx.p, keys.p, ids.p);
  MSW_HIP(hipGetLastError());
  if (K) {  // ascending hash; the sort is stable: read ids stay ascending inside a class
    size_t bytes = 0;
    MSW_HIP(prim_sort_pairs(nullptr, bytes, keys.p, keys2.p, ids.p, out.d_reads.p, (size_t)K, 64u, st));
    MSW_HIP(prim_sort_pairs(cx.scratch(bytes), bytes, keys.p, keys2.p, ids.p, out.d_reads.p, (size_t)K, 64u, st));
  }
  cx.mark("hash + sort");
  head.alloc(K + 1), eidx.alloc(K + 1);
  MSW_HIP(hipMemsetAsync(head.p + K, 0, sizeof(uint32_t), st));
  if (K) hipLaunchKernelGGL(k_ec_heads, dim3(reader_grid(K, cx.n_cu)), dim3(256), 0, st, keys2.p, K, head.p);
  scan_u32_u64(head.p, eidx.p, K + 1, cx);
  const uint64_t E = fetch_u64(eidx.p + K, st);
  out.d_rptr.alloc(E + 1), out.d_tptr.alloc(E + 1), out.d_counts.alloc(E), tlen.alloc(E + 1);
  MSW_HIP(hipMemsetAsync(tlen.p + E, 0, sizeof(uint32_t), st));
  MSW_HIP(hipMemcpyAsync(out.d_rptr.p + E, &K, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (K)
    hipLaunchKernelGGL(k_ec_meta, dim3(reader_grid(K, cx.n_cu)), dim3(256), 0, st, head.p, eidx.p, out.d_reads.p, s.ptr.p, K,
                       out.d_rptr.p, tlen.p);
  scan_u32_u64(tlen.p, out.d_tptr.p, E + 1, cx);
  const uint64_t H = fetch_u64(out.d_tptr.p + E, st);  // (also: K has been read)
  out.d_targets.alloc(H);
  if (E)
    hipLaunchKernelGGL(k_ec_rows, dim3(reader_grid(E, cx.n_cu)), dim3(256), 0, st, out.d_rptr.p, out.d_reads.p, s.ptr.p, s.tgt.p,
                       out.d_tptr.p, E, out.d_counts.p, out.d_targets.p);
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(st));
  out.E = E, out.H = H, out.K = K;
  out.on_device = true;
  out.host_have = 0u;
  cx.mark("classes");
}

bool path_is_gzip(const char *path) {
  unsigned char m[2] = {0, 0};
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return false;
  const ssize_t got = pread(fd, m, 2, 0);
  close(fd);
  return got == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

// the whole reader; throws ReaderFallback when the text needs the host parser
void read_alignment_device(const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode, ReaderCtx &cx,
                           msw_alignment &out) {
  cx.timing = getenv("MSWEEP_BUILD_TIMING") != nullptr;
  cx.t0 = std::chrono::steady_clock::now();
  // strand i + 1's text is read and sent (a host thread, the stager's copy stream) while strand i's kernels run
  DevStrand acc(cx);
  std::unique_ptr<DevText> cur(new DevText(cx)), nxt;
  upload_text(paths[0], cx, *cur);
  cx.mark("text to the device (first strand)");
  for (size_t i = 0; i < n_paths; ++i) {
    std::thread sender;
    std::exception_ptr send_err;
    if (i + 1 < n_paths) {
      nxt.reset(new DevText(cx));
      sender = std::thread([&, i] {
        try {
          MSW_HIP(hipSetDevice(cx.device));
          upload_text(paths[i + 1], cx, *nxt);
        } catch (...) {
          send_err = std::current_exception();
        }
      });
    }
    struct Join {
      std::thread &t;
      ~Join() {
        if (t.joinable()) t.join();
      }
    } join{sender};
    if (i == 0) {
      device_strand(*cur, n_targets, cx, acc);
    } else {
      DevStrand s(cx);
      device_strand(*cur, n_targets, cx, s);
      device_merge(acc, s, merge_mode == MSW_MERGE_INTERSECTION, cx);
      cx.mark("merge strands");
    }
    if (sender.joinable()) sender.join();
    if (send_err) std::rethrow_exception(send_err);
    cur.swap(nxt);
  }
  device_collapse(acc, n_targets, cx, out);
}

}  // namespace
