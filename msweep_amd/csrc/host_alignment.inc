// host_alignment.inc -- native reader of Themisto plaintext pseudoalignments and the collapse into
// equivalence classes (SURVEY.md 8f-1; reference: include/mSWEEP_alignment.hpp:54-94 line parser,
// :97-135 paired-end merge, :137-215 collapse).  Host code, no GPU: it produces the EC -> target
// lists msw_core_build_likelihood consumes, instead of the reference's E x T bit matrix.
// Kept semantics: a read is its SET of aligned targets over all lines that carry its id;
// n_reads = line count of the LAST strand and only read ids below it take part (:119, :148);
// strands are merged by intersection / union of the sets (:123-133); unaligned reads are dropped
// (:149); reads are keyed by  hash ^= j + 0x517cc1b727220a95 + (hash << 6) + (hash >> 2)  over
// the ascending target ids (:152-156) and reads with equal hash share an EC; ECs in ascending hash
// order (std::map, :186), read ids ascending inside an EC, the first one is the representative
// whose target set the EC keeps (:199-203).  Stricter than the reference: a target id >= n_targets
// is an error (the reference would set a bit of the next read).
#include <cerrno>
#include <cstring>
#include <thread>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

// (msw_alignment and its uninitialised vectors: handle.hpp)
namespace {

thread_local std::string g_aln_error;

// ---- host parallelism of the reader (round 4: every stage, not only the parse) ---------------------------------
// Threads: MSWEEP_READER_THREADS, else min(16, hardware threads, the cgroup's CPU quota) -- a GPU box shows all the
// host's hardware threads and grants a share of them.
size_t reader_threads() {
  if (const char *e = getenv("MSWEEP_READER_THREADS")) return (size_t)std::max(1, std::min(256, atoi(e)));
  size_t n = std::max<size_t>(1, std::min<size_t>(16, std::thread::hardware_concurrency()));
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64] = {0};
    unsigned long long period = 0;
    if (fscanf(f, "%63s %llu", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
      n = std::max<size_t>(1, std::min<size_t>(n, (size_t)(strtoull(q, nullptr, 10) / period)));
    fclose(f);
  }
  return n;
}
// fn(t) for t in [0, n) on n threads; the first exception is rethrown on the caller's thread
template <class F>
void run_threads(size_t n, F &&fn) {
  if (n <= 1) {
    fn((size_t)0);
    return;
  }
  std::vector<std::thread> pool;
  std::vector<std::exception_ptr> err(n);
  for (size_t t = 0; t < n; ++t)
    pool.emplace_back([&, t] {
      try {
        fn(t);
      } catch (...) {
        err[t] = std::current_exception();
      }
    });
  for (auto &th : pool) th.join();
  for (auto &e : err)
    if (e) std::rethrow_exception(e);
}
// [n * t / T, n * (t + 1) / T)
inline void share(size_t n, size_t T, size_t t, size_t &lo, size_t &hi) {
  lo = n / T * t + std::min(t, n % T);
  hi = lo + n / T + (t < n % T ? 1 : 0);
}
// boundaries of T contiguous ranges of rows with about equal numbers of entries (ptr = CSR row pointers)
std::vector<size_t> balanced_rows(const std::vector<uint64_t> &ptr, size_t T) {
  const size_t n = ptr.empty() ? 0 : ptr.size() - 1;
  std::vector<size_t> cut(T + 1, n);
  cut[0] = 0;
  const uint64_t tot = n ? ptr[n] : 0;
  for (size_t t = 1; t < T; ++t) {
    const uint64_t want = tot / T * t + n / T * t;  // entries + rows: rows of no entries cost time too
    size_t lo = cut[t - 1], hi = n;
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (ptr[mid] + mid < want) lo = mid + 1;
      else hi = mid;
    }
    cut[t] = lo;
  }
  return cut;
}

// one strand as CSR over read ids: sorted, de-duplicated target lists
struct Strand {
  std::vector<uint64_t> ptr;   // [n_ids + 1]
  uvec<uint32_t> tgt;
  size_t n_lines = 0;
  size_t n_ids() const { return ptr.empty() ? 0 : ptr.size() - 1; }
};

// Parses one file.  The text is split at line boundaries into one chunk per thread; every chunk is
// parsed on its own (lines, their targets, largest read id, first error) and the results are joined
// in file order, so line numbers in error messages and the outcome do not depend on the thread
// count.
struct ChunkOut {
  std::vector<uint32_t> rid, len;  // per line: read id, number of targets on the line
  std::vector<uint32_t> tgt;       // the lines' targets, in line order
  size_t n_lines = 0;
  uint64_t max_id = 0;
  bool any = false;
  size_t err_line = 0;          // 1-based line inside the chunk, 0 = none
  int err_kind = 0;             // 1 format, 2 target out of range, 3 compact format
  std::string err_text;
};

void parse_chunk(const char *p, const char *end, size_t n_targets, bool first_chunk, ChunkOut &o) {
  // (a line of a cfg3-like sample: ~8 bytes of read id + ~6 bytes per target)
  o.tgt.reserve((size_t)(end - p) / 5 + 16);
  o.rid.reserve((size_t)(end - p) / 48 + 16);
  o.len.reserve((size_t)(end - p) / 48 + 16);
  while (p < end) {
    const char *eol = static_cast<const char *>(memchr(p, '\n', (size_t)(end - p)));
    const char *le = eol ? eol : end;
    ++o.n_lines;
    const char *q = p;
    auto fail = [&](int kind) {
      if (!o.err_line) {
        o.err_line = o.n_lines;
        o.err_kind = kind;
        o.err_text.assign(p, le);
      }
    };
    if (first_chunk && o.n_lines == 1 && memchr(p, ',', (size_t)(le - p))) {
      fail(3);
      return;
    }
    bool ok = true;
    auto number = [&](uint64_t &v) {  // std::stoul semantics for what Themisto writes: digits only
      if (q == le || *q < '0' || *q > '9') { ok = false; return; }
      v = 0;
      while (q != le && *q >= '0' && *q <= '9') {
        v = v * 10 + (uint64_t)(*q - '0');
        if (v > 0xffffffffull) { ok = false; return; }
        ++q;
      }
    };
    uint64_t rid = 0, t = 0;
    number(rid);
    if (!ok) { fail(1); return; }
    o.any = true;
    o.max_id = std::max(o.max_id, rid);
    const size_t t0 = o.tgt.size();
    while (q != le) {
      if (*q == '\r' && q + 1 == le) break;  // CRLF
      if (*q != ' ') { ok = false; break; }
      ++q;
      if (q == le) break;        // trailing blank
      if (*q == ' ' || *q == '\r') continue;
      number(t);
      if (!ok) break;
      if (t >= n_targets) { fail(2); return; }
      o.tgt.push_back((uint32_t)t);
    }
    if (!ok) { fail(1); return; }
    o.rid.push_back((uint32_t)rid);
    o.len.push_back((uint32_t)(o.tgt.size() - t0));
    p = eol ? eol + 1 : end;
  }
}

// The text of one file: a read-only mapping of a plain file (no copy: the parser walks the page cache), or the
// inflated bytes of a gzip file.  gzip input (Themisto's --gzip-output, the `.aln.gz` files of docs/gpubenchmarks.md:3;
// the reference opens every input through bxzstr, which detects the compression by its magic bytes --
// CMakeLists.txt:156-158, include/mSWEEP_alignment.hpp:97-115) is inflated with zlib (one thread: a gzip stream is
// sequential); bzip2 / xz input is named as unsupported (their libraries are not part of this build).
struct FileText {
  const char *data = nullptr;
  size_t size = 0;
  void *map = nullptr;
  size_t map_size = 0;
  std::vector<char> own;
  FileText() = default;
  FileText(const FileText &) = delete;
  FileText &operator=(const FileText &) = delete;
  ~FileText() {
    if (map) munmap(map, map_size);
  }
};

void slurp_text(const char *path, FileText &ft) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) throw Fail(std::string("cannot open pseudoalignment file ") + path);
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    throw Fail(std::string("cannot open pseudoalignment file ") + path);
  }
  const size_t size = (size_t)st.st_size;
  unsigned char magic[6] = {0, 0, 0, 0, 0, 0};
  const ssize_t got_magic = pread(fd, magic, std::min<size_t>(size, 6), 0);
  (void)got_magic;
  if (magic[0] == 'B' && magic[1] == 'Z' && magic[2] == 'h') {
    close(fd);
    throw Fail(std::string("bzip2-compressed pseudoalignment files are not supported (decompress or use gzip): ") + path);
  }
  if (magic[0] == 0xFD && magic[1] == '7' && magic[2] == 'z' && magic[3] == 'X' && magic[4] == 'Z') {
    close(fd);
    throw Fail(std::string("xz-compressed pseudoalignment files are not supported (decompress or use gzip): ") + path);
  }
  if (magic[0] == 0x1f && magic[1] == 0x8b) {
    close(fd);
    gzFile gz = gzopen(path, "rb");
    if (!gz) throw Fail(std::string("cannot open pseudoalignment file ") + path);
    (void)gzbuffer(gz, 1u << 20);
    std::vector<char> &text = ft.own;
    // (the uncompressed size is not stored reliably: grow geometrically from 6 x the file size)
    size_t used = 0;
    text.resize(std::max<size_t>(size * 6, 1u << 20));
    for (;;) {
      if (used == text.size()) text.resize(text.size() * 2);
      const int want = (int)std::min<size_t>(text.size() - used, 1u << 30);
      const int got = gzread(gz, text.data() + used, (unsigned)want);
      if (got < 0) {
        int errnum = 0;
        const std::string msg = gzerror(gz, &errnum);
        gzclose(gz);
        throw Fail(std::string("cannot read gzip-compressed pseudoalignment file ") + path + ": " + msg);
      }
      if (got == 0) break;
      used += (size_t)got;
    }
    // a file that ends inside a gzip stream: gzread hands over what it could inflate and gzclose says so
    if (gzclose(gz) != Z_OK)
      throw Fail(std::string("cannot read gzip-compressed pseudoalignment file ") + path + ": unexpected end of file");
    text.resize(used);
    ft.data = text.data();
    ft.size = used;
    return;
  }
  if (size == 0) {
    close(fd);
    return;
  }
  void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
  if (m != MAP_FAILED) {
    (void)madvise(m, size, MADV_WILLNEED);
    ft.map = m;
    ft.map_size = size;
    ft.data = static_cast<const char *>(m);
    ft.size = size;
    close(fd);
    return;
  }
  // (a file system without mmap: read it)
  ft.own.resize(size);
  size_t used = 0;
  while (used < size) {
    const ssize_t got = pread(fd, ft.own.data() + used, size - used, (off_t)used);
    if (got <= 0) {
      close(fd);
      throw Fail(std::string("cannot read pseudoalignment file ") + path);
    }
    used += (size_t)got;
  }
  close(fd);
  ft.data = ft.own.data();
  ft.size = size;
}

Strand read_strand(const FileText &text, size_t n_targets) {
  const char *b0 = text.data, *e0 = b0 + text.size;
  const size_t nthr = std::max<size_t>(1, std::min<size_t>(reader_threads(), text.size / (1u << 20) + 1));
  std::vector<const char *> cut(nthr + 1, e0);
  cut[0] = b0;
  for (size_t t = 1; t < nthr; ++t) {
    const char *c = b0 + text.size / nthr * t;
    c = std::max(c, cut[t - 1]);
    const char *nl = c < e0 ? static_cast<const char *>(memchr(c, '\n', (size_t)(e0 - c))) : nullptr;
    cut[t] = nl ? nl + 1 : e0;
  }
  std::vector<ChunkOut> outs(nthr);
  run_threads(nthr, [&](size_t t) { parse_chunk(cut[t], cut[t + 1], n_targets, t == 0, outs[t]); });
  size_t n_lines = 0;
  uint64_t max_id = 0;
  bool any = false;
  for (auto &o : outs) {
    if (o.err_line) {  // the first error in file order, reported with the reference's wording
      const size_t line_no = n_lines + o.err_line;
      if (o.err_kind == 3)
        throw Fail("compact (alignment-writer) pseudoalignments are not supported: convert to Themisto plaintext");
      if (o.err_kind == 2) throw Fail("Pseudoalignment file has more target sequences than expected.");
      throw Fail("File format not supported on line " + std::to_string(line_no) + " with content: " + o.err_text);
    }
    n_lines += o.n_lines;
    max_id = std::max(max_id, o.max_id);
    any |= o.any;
  }
  Strand s;
  s.n_lines = n_lines;
  // a Themisto file numbers its reads 0 .. lines - 1; a malformed line with a huge read id must not size
  // the tables (2^32 ids would be 3 x 32 GB): ids at or beyond the line count never take part in the
  // equivalence classes anyway (collapse(), include/mSWEEP_alignment.hpp:148) and are dropped here
  const size_t n_ids = any ? std::min<size_t>((size_t)max_id + 1, n_lines) : 0;
  // CSR over read ids: a read is the SET of targets of all lines that carry its id -- lengths added up per id
  // (atomics: a Themisto file names every read once, so they never meet), prefix sums, every line's targets copied to
  // its id's row by the thread that parsed it
  std::vector<uint32_t> cnt(n_ids, 0), cur(n_ids, 0);
  run_threads(nthr, [&](size_t t) {
    const ChunkOut &o = outs[t];
    for (size_t i = 0; i < o.rid.size(); ++i)
      if (o.rid[i] < n_ids && o.len[i]) __atomic_fetch_add(&cnt[o.rid[i]], o.len[i], __ATOMIC_RELAXED);
  });
  s.ptr.assign(n_ids + 1, 0);
  for (size_t i = 0; i < n_ids; ++i) s.ptr[i + 1] = s.ptr[i] + cnt[i];
  uvec<uint32_t> raw(s.ptr[n_ids]);
  run_threads(nthr, [&](size_t t) {
    ChunkOut &o = outs[t];
    size_t at = 0;
    for (size_t i = 0; i < o.rid.size(); ++i) {
      const uint32_t n = o.len[i];
      if (o.rid[i] < n_ids && n) {
        const uint32_t off = __atomic_fetch_add(&cur[o.rid[i]], n, __ATOMIC_RELAXED);
        std::memcpy(raw.data() + s.ptr[o.rid[i]] + off, o.tgt.data() + at, (size_t)n * sizeof(uint32_t));
      }
      at += n;
    }
    std::vector<uint32_t>().swap(o.tgt);
    std::vector<uint32_t>().swap(o.rid);
    std::vector<uint32_t>().swap(o.len);
  });
  std::vector<uint32_t>().swap(cur);
  // every row sorted and de-duplicated (Themisto writes a read's targets once each, in no promised order): rows
  // that already ascend strictly -- nearly all -- are only looked at; the new lengths go to cnt
  const std::vector<size_t> rcut = balanced_rows(s.ptr, nthr);
  std::vector<char> shrunk(nthr, 0);
  run_threads(nthr, [&](size_t t) {
    for (size_t i = rcut[t]; i < rcut[t + 1]; ++i) {
      uint32_t *b = raw.data() + s.ptr[i], *e = raw.data() + s.ptr[i + 1];
      bool asc = true;
      for (uint32_t *q = b; asc && q + 1 < e; ++q) asc = q[0] < q[1];
      if (!asc) {
        std::sort(b, e);
        uint32_t *ne = std::unique(b, e);
        if (ne != e) shrunk[t] = 1;
        cnt[i] = (uint32_t)(ne - b);
      }
    }
  });
  if (std::any_of(shrunk.begin(), shrunk.end(), [](char c) { return c != 0; })) {  // compact the rows that lost entries
    std::vector<uint64_t> nptr(n_ids + 1, 0);
    for (size_t i = 0; i < n_ids; ++i) nptr[i + 1] = nptr[i] + cnt[i];
    uvec<uint32_t> packed(nptr[n_ids]);
    run_threads(nthr, [&](size_t t) {
      for (size_t i = rcut[t]; i < rcut[t + 1]; ++i)
        std::memcpy(packed.data() + nptr[i], raw.data() + s.ptr[i], (size_t)cnt[i] * sizeof(uint32_t));
    });
    s.ptr.swap(nptr);
    raw.swap(packed);
  }
  s.tgt.swap(raw);
  return s;
}

// set intersection / union of two strands, read by read (:123-133): every thread merges a contiguous range of reads
// into a buffer of its own; the buffers are then laid end to end
Strand merge_strands(const Strand &a, const Strand &b, bool intersect) {
  Strand m;
  m.n_lines = b.n_lines;  // the last strand's line count (:119)
  const size_t n = intersect ? std::min(a.n_ids(), b.n_ids()) : std::max(a.n_ids(), b.n_ids());
  m.ptr.assign(n + 1, 0);
  const size_t T = std::max<size_t>(1, std::min<size_t>(reader_threads(), n / 65536 + 1));
  std::vector<std::vector<uint32_t>> part(T);
  std::vector<size_t> cut(T + 1, n);
  {  // ranges balanced by the entries of both strands
    std::vector<uint64_t> both(n + 1);
    for (size_t i = 0; i <= n; ++i) both[i] = a.ptr[std::min(i, a.n_ids())] + b.ptr[std::min(i, b.n_ids())];
    cut = balanced_rows(both, T);
  }
  run_threads(T, [&](size_t t) {
    std::vector<uint32_t> &out = part[t];
    size_t est = 0;
    for (size_t i = cut[t]; i < cut[t + 1]; i += 64) est += 64;
    out.reserve((size_t)((a.ptr[std::min(cut[t + 1], a.n_ids())] - a.ptr[std::min(cut[t], a.n_ids())])) + 16);
    for (size_t i = cut[t]; i < cut[t + 1]; ++i) {
      const uint32_t *ab = i < a.n_ids() ? a.tgt.data() + a.ptr[i] : nullptr, *ae = i < a.n_ids() ? a.tgt.data() + a.ptr[i + 1] : nullptr;
      const uint32_t *bb = i < b.n_ids() ? b.tgt.data() + b.ptr[i] : nullptr, *be = i < b.n_ids() ? b.tgt.data() + b.ptr[i + 1] : nullptr;
      const size_t before = out.size();
      if (intersect) std::set_intersection(ab, ae, bb, be, std::back_inserter(out));
      else std::set_union(ab, ae, bb, be, std::back_inserter(out));
      m.ptr[i + 1] = out.size() - before;  // the row's length for now
    }
    (void)est;
  });
  for (size_t i = 0; i < n; ++i) m.ptr[i + 1] += m.ptr[i];
  m.tgt.resize(m.ptr[n]);
  run_threads(T, [&](size_t t) {
    if (!part[t].empty()) std::memcpy(m.tgt.data() + m.ptr[cut[t]], part[t].data(), part[t].size() * sizeof(uint32_t));
    std::vector<uint32_t>().swap(part[t]);
  });
  return m;
}

// (hash, read id) pairs sorted ascending: sorted runs per thread, then merged pairwise, round by round
struct Keyed {  // (hash, read id), ordered by both
  uint64_t first;
  uint32_t second;
  bool operator<(const Keyed &o) const { return first < o.first || (first == o.first && second < o.second); }
};
void sort_keyed(uvec<Keyed> &v, size_t T) {
  const size_t n = v.size();
  if (T <= 1 || n < (1u << 16)) {
    std::sort(v.begin(), v.end());
    return;
  }
  std::vector<size_t> cut(T + 1);
  for (size_t t = 0; t <= T; ++t) cut[t] = n / T * t + std::min(t, n % T);
  run_threads(T, [&](size_t t) { std::sort(v.begin() + cut[t], v.begin() + cut[t + 1]); });
  uvec<Keyed> tmp(n);
  auto *src = &v, *dst = &tmp;
  while (cut.size() > 2) {
    const size_t runs = cut.size() - 1, pairs = runs / 2;
    run_threads(pairs + (runs & 1), [&](size_t k) {
      if (k < pairs)
        std::merge(src->begin() + cut[2 * k], src->begin() + cut[2 * k + 1], src->begin() + cut[2 * k + 1],
                   src->begin() + cut[2 * k + 2], dst->begin() + cut[2 * k]);
      else  // the odd run out: carried over
        std::copy(src->begin() + cut[2 * k], src->begin() + cut[2 * k + 1], dst->begin() + cut[2 * k]);
    });
    std::vector<size_t> ncut;
    for (size_t k = 0; k < cut.size(); k += 2) ncut.push_back(cut[k]);
    if (ncut.back() != n) ncut.push_back(n);
    cut.swap(ncut);
    std::swap(src, dst);
  }
  if (src != &v) v.swap(tmp);
}

void collapse(const Strand &s, size_t n_targets, msw_alignment &out) {
  out.n_targets = n_targets;
  out.n_queries = s.n_lines;
  const size_t n = std::min(s.n_ids(), s.n_lines);  // read ids >= the line count never take part (:148)
  const size_t T = std::max<size_t>(1, std::min<size_t>(reader_threads(), n / 65536 + 1));
  // the aligned reads keyed by the reference's hash of their target set
  std::vector<size_t> rcut(T + 1), n_al(T + 1, 0);
  {
    std::vector<uint64_t> head(s.ptr.begin(), s.ptr.begin() + n + 1);
    rcut = balanced_rows(head, T);
  }
  run_threads(T, [&](size_t t) {
    size_t c = 0;
    for (size_t i = rcut[t]; i < rcut[t + 1]; ++i) c += s.ptr[i + 1] != s.ptr[i];
    n_al[t + 1] = c;
  });
  for (size_t t = 0; t < T; ++t) n_al[t + 1] += n_al[t];
  uvec<Keyed> keyed(n_al[T]);
  run_threads(T, [&](size_t t) {
    size_t w = n_al[t];
    for (size_t i = rcut[t]; i < rcut[t + 1]; ++i) {
      if (s.ptr[i + 1] == s.ptr[i]) continue;  // unaligned
      uint64_t h = 0;
      for (uint64_t k = s.ptr[i]; k < s.ptr[i + 1]; ++k) h ^= (uint64_t)s.tgt[k] + 0x517cc1b727220a95ull + (h << 6) + (h >> 2);
      keyed[w++] = Keyed{h, (uint32_t)i};
    }
  });
  sort_keyed(keyed, T);  // ascending hash, read ids ascending inside an EC
  // equivalence classes = runs of equal hash; the first read of a run keeps its target set
  const size_t K = keyed.size();
  std::vector<size_t> kcut(T + 1), n_ec(T + 1, 0);
  for (size_t t = 0; t <= T; ++t) kcut[t] = K / T * t + std::min(t, K % T);
  run_threads(T, [&](size_t t) {
    size_t c = 0;
    for (size_t k = kcut[t]; k < kcut[t + 1]; ++k) c += k == 0 || keyed[k].first != keyed[k - 1].first;
    n_ec[t + 1] = c;
  });
  for (size_t t = 0; t < T; ++t) n_ec[t + 1] += n_ec[t];
  const size_t E = n_ec[T];
  out.ec_tptr.assign(E + 1, 0);
  out.ec_rptr.assign(E + 1, 0);
  out.ec_counts.assign(E, 0);
  out.ec_reads.resize(K);
  run_threads(T, [&](size_t t) {
    size_t e = n_ec[t];
    for (size_t k = kcut[t]; k < kcut[t + 1]; ++k) {
      out.ec_reads[k] = keyed[k].second;
      if (k == 0 || keyed[k].first != keyed[k - 1].first) {
        const uint32_t rep = keyed[k].second;
        out.ec_rptr[e] = k;                                  // where the EC's reads start
        out.ec_tptr[e + 1] = s.ptr[rep + 1] - s.ptr[rep];    // its length for now
        ++e;
      }
    }
  });
  out.ec_rptr[E] = K;
  for (size_t e = 0; e < E; ++e) {
    out.ec_counts[e] = out.ec_rptr[e + 1] - out.ec_rptr[e];
    out.ec_tptr[e + 1] += out.ec_tptr[e];
  }
  out.ec_targets.resize(out.ec_tptr[E]);
  out.E = E, out.H = out.ec_tptr[E], out.K = K;
  run_threads(T, [&](size_t t) {
    size_t lo, hi;
    share(E, T, t, lo, hi);
    for (size_t e = lo; e < hi; ++e) {
      const uint32_t rep = out.ec_reads[out.ec_rptr[e]];
      std::memcpy(out.ec_targets.data() + out.ec_tptr[e], s.tgt.data() + s.ptr[rep],
                  (size_t)(s.ptr[rep + 1] - s.ptr[rep]) * sizeof(uint32_t));
    }
  });
}

}  // namespace

extern "C" {

const char *msw_alignment_last_error(void) { return g_aln_error.c_str(); }

}  // extern "C"
namespace {
void check_reader_args(const char *const *paths, const void *out, size_t n_paths, size_t n_targets, int merge_mode) {
  if (!paths || !out || n_paths == 0) throw Fail("msw_alignment_read: no pseudoalignment files given");
  if (n_targets == 0 || n_targets > 0xffffffffull) throw Fail("msw_alignment_read: bad number of target sequences");
  if (merge_mode != MSW_MERGE_INTERSECTION && merge_mode != MSW_MERGE_UNION)
    throw Fail("Unrecognized option for --themisto-mode");
}
}  // namespace
extern "C" {

int msw_alignment_read(const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode,
                       msw_alignment_t *out) {
  if (out) *out = nullptr;
  try {
    check_reader_args(paths, out, n_paths, n_targets, merge_mode);
    // MSWEEP_BUILD_TIMING=1 (developer switch): wall time of the reader's stages to stderr
    const bool timing = getenv("MSWEEP_BUILD_TIMING") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
      if (!timing) return;
      const auto t1 = std::chrono::steady_clock::now();
      fprintf(stderr, "[msweep reader] %-28s %8.2f ms (%zu threads)\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count(),
              reader_threads());
      t0 = t1;
    };
    // the files' text: mappings cost nothing; gzip files are inflated side by side, a thread per file (a gzip stream
    // is sequential: ~250 MB/s of text each)
    std::vector<std::unique_ptr<FileText>> texts(n_paths);
    for (auto &t : texts) t.reset(new FileText);
    run_threads(n_paths, [&](size_t i) { slurp_text(paths[i], *texts[i]); });
    mark("open / inflate");
    Strand acc = read_strand(*texts[0], n_targets);
    texts[0].reset();
    mark("strand 1: parse + rows");
    for (size_t i = 1; i < n_paths; ++i) {
      Strand nxt = read_strand(*texts[i], n_targets);
      texts[i].reset();
      mark("strand: parse + rows");
      acc = merge_strands(acc, nxt, merge_mode == MSW_MERGE_INTERSECTION);
      mark("merge strands");
    }
    std::unique_ptr<msw_alignment> a(new msw_alignment);
    collapse(acc, n_targets, *a);
    mark("collapse");
    *out = a.release();
    return 0;
  } catch (const std::exception &ex) {
    g_aln_error = ex.what();
    return 1;
  }
}

int msw_alignment_shape(msw_alignment_t a, size_t *n_ecs, size_t *n_reads, size_t *n_hits, size_t *n_aligned) {
  if (!a) return 1;
  if (n_ecs) *n_ecs = a->E;
  if (n_reads) *n_reads = a->n_queries;
  if (n_hits) *n_hits = a->H;
  if (n_aligned) *n_aligned = a->K;
  return 0;
}

int msw_alignment_export(msw_alignment_t a, uint64_t *ec_tptr, uint32_t *ec_targets, uint64_t *ec_counts,
                         uint64_t *ec_rptr, uint32_t *ec_reads) {
  if (!a) return 1;
  // (on the reader's threads: the destination is usually freshly mapped memory, and one thread faulting 0.9 GB in --
  // cfg3 -- took 0.35 s)
  const size_t T = reader_threads();
  auto copy = [&](auto *dst, const auto &src) {
    if (!dst || src.empty()) return;
    run_threads(std::min<size_t>(T, 1 + src.size() / (1u << 20)), [&](size_t t) {
      size_t lo, hi;
      share(src.size(), std::min<size_t>(T, 1 + src.size() / (1u << 20)), t, lo, hi);
      std::memcpy(dst + lo, src.data() + lo, (hi - lo) * sizeof(*dst));
    });
  };
  try {
    // (device-resident arrays the host does not hold yet go straight to the caller's memory)
    auto put = [&](unsigned bit, auto *dst, const auto &vec, const auto *dsrc, size_t n) {
      if (!dst) return;
      if (a->host_have & bit) {
        copy(dst, vec);
      } else if (n) {
        MSW_HIP(hipSetDevice(a->device));
        MSW_HIP(hipMemcpy(dst, dsrc, n * sizeof(*dst), hipMemcpyDeviceToHost));
      }
    };
    put(msw_alignment::kAlnTptr, ec_tptr, a->ec_tptr, a->d_tptr.p, a->E + 1);
    put(msw_alignment::kAlnTargets, ec_targets, a->ec_targets, a->d_targets.p, a->H);
    put(msw_alignment::kAlnCounts, ec_counts, a->ec_counts, a->d_counts.p, a->E);
    put(msw_alignment::kAlnRptr, ec_rptr, a->ec_rptr, a->d_rptr.p, a->E + 1);
    put(msw_alignment::kAlnReads, ec_reads, a->ec_reads, a->d_reads.p, a->K);
  } catch (...) {
    return 1;
  }
  return 0;
}

int msw_alignment_view(msw_alignment_t a, const uint64_t **ec_tptr, const uint32_t **ec_targets, const uint64_t **ec_counts,
                       const uint64_t **ec_rptr, const uint32_t **ec_reads) {
  if (!a) return 1;
  try {  // (only the arrays asked for leave the device)
    a->to_host((ec_tptr ? msw_alignment::kAlnTptr : 0u) | (ec_targets ? msw_alignment::kAlnTargets : 0u) |
               (ec_counts ? msw_alignment::kAlnCounts : 0u) | (ec_rptr ? msw_alignment::kAlnRptr : 0u) |
               (ec_reads ? msw_alignment::kAlnReads : 0u));
  } catch (...) {
    return 1;
  }
  if (ec_tptr) *ec_tptr = a->ec_tptr.data();
  if (ec_targets) *ec_targets = a->ec_targets.data();
  if (ec_counts) *ec_counts = a->ec_counts.data();
  if (ec_rptr) *ec_rptr = a->ec_rptr.data();
  if (ec_reads) *ec_reads = a->ec_reads.data();
  return 0;
}

int msw_alignment_on_device(msw_alignment_t a) { return a && a->on_device ? 1 : 0; }

void msw_alignment_destroy(msw_alignment_t a) {
  if (a && a->on_device) (void)hipSetDevice(a->device);
  delete a;
}

}  // extern "C"
