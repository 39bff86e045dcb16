// msweep_core.hip -- host side of libmsweep_core.so: the C ABI declared in
// include/msweep_core.h over the gfx950 kernels in kernels.hpp.
//
// No CPU fallback exists in this library: every numeric step of the hot path (likelihood
// expansion, RCG / EM sweeps, column reductions, ELBO, bootstrap resampling) is a HIP
// kernel; the host only validates shapes, lays out buffers and enqueues launches.
#include "../../include/msweep_core.h"

#include <algorithm>
#include <array>
#include <cerrno>
#include <cmath>
#include <chrono>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <zlib.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "kernels.hpp"
#include "pack_kernels.hpp"
#include "compress_kernels.hpp"
#include "comm.hpp"
#include "shm_comm.hpp"
#include "peer_comm.hpp"
#include "likelihood_kernels.hpp"
#include "bootstrap_kernels.hpp"
#include "em_kernels.hpp"
#include "em_f32_kernels.hpp"
#include "stream_kernels.hpp"
#include "reader_kernels.hpp"
#include "bin_kernels.hpp"
#include "text_kernels.hpp"
#include "deflate_kernels.hpp"
#include "inflate_kernels.hpp"
#include "inflate_member_kernels.hpp"
#include "likelihood_text_kernels.hpp"
#include "fastq_host.hpp"
#include "fastq_kernels.hpp"

using namespace msw;

namespace {
thread_local std::string g_create_error;
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kIterBatch = 16;
}  // namespace

// The handle's parts, by lifetime: the likelihood resident on the device (Resident: written by the
// build paths only), the state of one solve on it (Solver), the bootstrap's resampling state (Resampler), and what
// belongs to the handle as a whole (msw_core).  A bootstrap worker is a Solver and a Resampler of its own that
// solve on the handle's Resident through a const reference.

// shape and layout of the resident likelihood: plain values, so that a new build starts from one assignment
struct LikShape {
  int flavor = -1;  // -1 none, 0 CSR-of-ECs, 1 dense
  uint32_t G = 0, E = 0, n_lut = 0, nslices = 0, n_long = 0;
  uint64_t nnz = 0, nslots = 0;
  int enc = kEncNarrow;  // record encoding (sell.hpp): narrow byte offsets / wide / index records (hybrid area)
  bool glds = true, tlds = true;
  int gmodeB = 1;                // k_passB GMODE (sweep_kernels.hpp)
  RecDec dec = {};               // record encoding (sell.hpp); shiftH / maskH: index records, the rows of a hot segment
  uint32_t n_area = 0;           // 16-byte entries of the slot area
  uint32_t n_tab_lds = 0;        // ... of which the LDS images hold (all, the hot head, none)
  SliceClasses cls = {};         // slice classes: lanes per EC (sell.hpp)
  bool packed_scheduled = false;  // LDS-bank scheduling of the cells as the likelihood was packed (msw_core_set_pack_schedule)
  uint32_t long_row = kLongRow;  // ECs with more cells go one per wavefront (reset_likelihood)
  uint64_t rows_over8 = 0;       // rows of the slices of more than 8 rows (finish_sell)
  bool passB_rc8 = false;        // pass B runs its short-slice instantiation (sweep_kernels.hpp, RC = 8)
  double logzi = 0.0;
  int nblk = 0;  // persistent workgroups of the CSR sweeps
  int nblk_dense = 0;
  int nreg = 0;
  bool have_logc_res = false;  // logc_res holds the log counts msw_core_build_likelihood left
};

// ---- the likelihood resident on the device --------------------------------------------------------------------
struct Resident : LikShape {
  DevBuf<uint32_t> rec, slice_off, long_ptr, rec_long, perm;
  DevBuf<uint8_t> slice_hot;  // index records: rows of every slice's hot segment
  DevBuf<uint32_t> area_slot;
  DevBuf<double> lut_area;  // lut[area_slot[i]]: what the per-slot tables are built from, in their order
  DevBuf<double> lut, Lt;
  DevBuf<double> trange;    // {max, min} of the table values (bounds x_i = exp(a T_i) per pass: Scalars::xb)
  DevBuf<double> logc_res;  // log counts left on the device by msw_core_build_likelihood
  bool wide() const { return enc == kEncWide; }
  bool hybrid() const { return enc == kEncIndex; }
  int n_tab_inline() const { return flavor == 0 && n_area <= (uint32_t)kTabInline ? (int)n_area : 0; }
  // rows of per-workgroup (or per-wave) column-sum partials pass B leaves for k_redfin
  int npart_rows() const { return flavor == 0 ? nblk : (nreg >= 32 ? 4 * nblk_dense : nblk_dense); }
  // guarded ECs (sell.hpp), CSR flavour: room in a workgroup's list for every EC it can see (its wavefronts take
  // slices -- and long ECs -- round-robin, SliceStream's stride), and words of a wavefront's bitmap of groups
  uint32_t guard_cap() const {
    static_assert(kPassThreads / 64 <= 16 && kPassThreadsB / 64 <= 16, "guard_cap / guard_bits assume <= 16 wavefronts per workgroup");
    const uint32_t nb0 = (uint32_t)std::max(nblk, 1);
    return 64u * ((nslices + nb0 - 1) / nb0 + 16u) + (n_long + nb0 - 1) / nb0 + 16u;
  }
  uint32_t guard_words() const { return (G + 31u) / 32u; }
};

// ---- the state of one solve on a Resident ----------------------------------------------------------------------
struct Solver {
  hipStream_t stream = nullptr;
  int n_cu = 256;
  // EC-sharded solve: the handle's communicator and its in_collective flag (guarded()); none for a bootstrap worker
  msw_comm *const *commp;
  bool *collective;
  explicit Solver(msw_comm *const *c = nullptr, bool *coll = nullptr) : commp(c), collective(coll) {}
  msw_comm *comm() const { return commp ? *commp : nullptr; }
  // the settings a solve reads
  SolveOpts opts;  // msw_core_set_option
  bool profiling = false, fixed_iters = false;
  size_t trace_theta = 0;

  DevBuf<double> cvec, logc_d, alpha0, u, os_u, step_u, w, e, N, Nc, Acc;
  DevBuf<uint8_t> c8, c8s;  // byte image of cvec by EC position / by slice lane (sell.hpp)
  DevBuf<double2> ew, tabA, tabB;  // group table of pass A; per-slot tables of both sweeps (TabDev)
  TabDev tabs() const { return TabDev{tabA.p, tabB.p}; }
  DevBuf<int> tab_built;    // k_tables bookkeeping
  DevBuf<double> partA, partS, partAcc, partC, partR, totS;
  size_t lds_attr[3][80] = {};  // dynamic-LDS limit already granted per sweep instantiation ([2]: pass B's short-slice ones)
  DevBuf<double> commA, commB;  // 1 and G + 4 doubles
  // guarded ECs (sell.hpp): per-workgroup lists, per-wavefront bitmaps, error flag
  DevBuf<uint32_t> guard_list, guard_bits;
  DevBuf<unsigned long long> guard_tail;  // [2 G] the guarded ECs' shares per group, two fixed-point limbs
  DevBuf<int> guard_err;
  DevBuf<unsigned long long> guard_visits;
  DevBuf<Scalars> sc;
  Scalars *sc_host = nullptr;  // pinned
  DevBuf<double> tr_bound, tr_newnorm, tr_beta, tr_theta;
  DevBuf<int32_t> tr_reset;
  bool have_solution = false;
  bool prepared = false;
  int last_algo = MSW_ALGO_RCG;
  // EM state
  DevBuf<double> logth;
  DevBuf<float> e32, tab32;  // --emprecision float: e_g and the slot table {x_i - p0} as floats (em_f32_kernels.hpp)
  bool em_f32 = false;       // the EM run under way is served by the fp32 kernels (launch_passB)

  // ---- measurement ---------------------------------------------------------------------------
  msw_timing timing = {};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evA, evB, evC;  // pass A, pass B, collectives (sharded solve)
  size_t evA_used = 0, evB_used = 0, evC_used = 0;

  ~Solver() {
    if (sc_host) (void)hipHostFree(sc_host);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (auto &p : evA) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &p : evB) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto &p : evC) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  }
};

// ---- the bootstrap's resampling state of one stream of replicates (host_bootstrap.inc) --------------------------
struct Resampler {
  DevBuf<uint64_t> mtwords;
  DevBuf<uint32_t> bcounts, bcounts2;
  DevBuf<MtState> mt;
  hipStream_t stream2 = nullptr;  // resampling of the next replicate, under the current solve
  hipEvent_t ev_counts[2] = {nullptr, nullptr};
  uint32_t one_count = 0;
  bool mt_valid = false;
  int32_t mt_seed = 0;
  uint64_t mt_pos = 0;
  ~Resampler() {
    for (auto &e : ev_counts)
      if (e) (void)hipEventDestroy(e);
    if (stream2) (void)hipStreamDestroy(stream2);
  }
};

struct Worker {  // a bootstrap worker: replicates on a stream of their own, beside the handle's solver
  Solver s;
  Resampler r;
  explicit Worker(int n_cu) { MSW_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)); s.n_cu = n_cu; }
  ~Worker() { (void)hipStreamDestroy(s.stream); }
};

// pinned host bytes handed to the caller, valid until the next call of their family; grown by pinned_reserve
// (host_text.inc), which words its failure "<who>: cannot allocate ... for <what>"
struct PinnedBuf {
  const char *who, *what;
  char *p = nullptr;
  size_t cap = 0;
  PinnedBuf(const char *who_, const char *what_) : who(who_), what(what_) {}
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

// ---- what msw_core_text_block / msw_core_format_g6 keep between calls (host_text.inc) ----------------------------
struct TextState {
  PinnedBuf pinned{"msw_core_text_block", "the text"};
  DevBuf<double> val;      // the G x w block of values
  DevBuf<uint8_t> out, tmp, closed;  // the text as written; scan scratch; the text with its undecided cells closed
  DevBuf<uint32_t> len, n_list;
  DevBuf<uint64_t> off, prefix;
  DevBuf<TextHostCell> list;
  DevBuf<TextFilledCell> cells;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the length pass + scan, around the write pass
  double kernel_ms = 0.0;  // of the last call (msw_core_last_text_timing)
  uint64_t bytes = 0;
  void release_device() {
    val.release(); out.release(); tmp.release(); closed.release(); len.release(); n_list.release(); off.release();
    prefix.release(); list.release(); cells.release();
  }
  ~TextState() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// ---- the gzip stream open on the handle and what its calls keep between them (host_gzip.inc) ---------------------------
struct GzState {
  bool open = false, host = false;  // host: MSWEEP_HOST_GZIP=1, zlib on the plain text
  int level = 6;
  uint32_t crc_reg = 0;  // the CRC register over the text so far (deflate_format.hpp: R(~0, text))
  uint64_t isize = 0;    // ... and its length
  std::unique_ptr<z_stream> zs;
  PinnedBuf pinned{"msw_core_gzip", "the compressed bytes"};
  DevBuf<uint8_t> in, out, tmp;  // uploaded host bytes; the chunks; scan scratch
  DevBuf<uint32_t> tokens, tables, len, crc, pow8;
  DevBuf<GzChunk> meta;
  DevBuf<uint64_t> off;
  uint32_t pow8_host[40] = {};
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around parse + CRC + scan, around the emit pass
  double kernel_ms = 0.0;  // of the stream (msw_core_last_gzip_timing)
  uint64_t bytes_out = 0;
  void release_device() {
    in.release(); out.release(); tmp.release(); tokens.release(); tables.release(); len.release(); meta.release();
    off.release();
  }
  ~GzState() {
    if (zs) (void)deflateEnd(zs.get());
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// ---- gzip input inflated on the device: what its calls keep on the handle (host_inflate.inc) -------------------------------
struct InflateState {
  DevBuf<uint32_t> pow8;   // x^(8 2^j) mod P for k_gz_crc
  uint32_t pow8_host[40] = {};
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // pairs around the probe and around
                                                                                                 // pass (a) + scan; chain, pass (b), CRC in a row
  std::vector<msw_inflate_info> last;  // per file of the last msw_alignment_read_device
  PinnedBuf pinned{"msw_core_inflate_gzip", "the text"};
  std::vector<char> host_text;  // ... or the host path's
  ~InflateState() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// ---- --extract-reads: what the msw_fastq_* calls keep on the handle (host_fastq.inc); the text and the index of a read
// file live in its own msw_fastq ---------------------------------------------------------------------------------------
struct FastqState {
  PinnedBuf pinned{"msw_fastq_next", "the records"};
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the gather kernel
  double kernel_ms = 0.0;                 // of the pieces since the last msw_fastq_select (msw_fastq_last_timing)
  uint64_t bytes = 0;
  ~FastqState() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

struct msw_core {
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;
  std::string err;
  TextStager text_stage;  // pinned staging of msw_alignment_read_device (host_reader.inc)
  ReaderPool reader_pool;  // ... and its device memory, kept between calls (reader_kernels.hpp)
  // EC-sharded solve: this handle holds one rank's block of ECs (comm.hpp)
  msw_comm *comm = nullptr;
  bool in_collective = false;  // a solve / sharded build is under way: a failure now strands the peers (guarded())
  // build settings
  bool pack_schedule = true;  // LDS-bank scheduling of the cells at upload (msw_core_set_pack_schedule)
  bool no_hybrid = false;     // re-planning without the hybrid area (host_pack.inc: slice geometry beyond 2^27 rows)

  Resident lik;
  DevBuf<uint32_t> iperm;  // original EC index -> permuted position (gamma blocks; built on first use)
  TextState text;
  GzState gz;
  InflateState inf;
  FastqState fastq;
  std::vector<uint64_t> lik_counts;  // first column of the last served likelihood file (host_likelihood_file.inc)
  Solver solver{&comm, &in_collective};  // on the handle's stream

  // ---- bootstrap -------------------------------------------------------------------------
  DevBuf<double> cp;
  std::vector<uint32_t> cp_counts;  // the EC counts `cp` was made from (host_bootstrap.inc: kept across calls)
  bool cp_hit = false;              // ... and whether the last call found them again
  Resampler resampler;              // msw_core_resample_counts; its stream2 also carries the build's side upload
  std::vector<std::unique_ptr<Worker>> workers;  // the replicates run on these, several at a time
  msw_bootstrap_timing btiming = {};

  ~msw_core() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};
// a solve that failed NUMERICALLY (likelihood underflow, non-finite bound: where the reference returns NaN weights).
// The bootstrap driver turns exactly these into a row of NaN; every other failure fails the call.
struct NumericFail : Fail {
  using Fail::Fail;
};

// marks the stretch of a call in which this rank's peers wait for it in collectives
// (flag: the handle's in_collective; null for a bootstrap worker's solve, which has no peers)
struct CollectiveScope {
  bool *flag;
  explicit CollectiveScope(bool *f) : flag(f) { if (flag) *flag = true; }
  void leave() { if (flag) *flag = false; }  // on success only: guarded() reads the flag after a throw
};

template <class F>
int guarded(msw_handle h, F &&f) {
  if (!h) return 1;
  try {
    MSW_HIP(hipSetDevice(h->device));
    f();
    return 0;
  } catch (const std::exception &ex) {
    h->err = ex.what();
    (void)hipGetLastError();
    // peers of a sharded solve must not wait for this rank for ever -- but only a failure BETWEEN collectives
    // (a solve or a sharded build was under way) strands them: argument and state errors touch no collective
    if (h->comm && h->in_collective) h->comm->abort();
    h->in_collective = false;
    return 1;
  }
}

std::pair<hipEvent_t, hipEvent_t> &next_pair(std::vector<std::pair<hipEvent_t, hipEvent_t>> &v,
                                             size_t &used) {
  if (used == v.size()) {
    hipEvent_t a, b;
    MSW_HIP(hipEventCreate(&a));
    MSW_HIP(hipEventCreate(&b));
    v.emplace_back(a, b);
  }
  return v[used++];
}

SellDev sell_view(const Resident &L, const Solver &s) {
  SellDev S;
  S.rec = L.rec.p;
  S.slice_off = L.slice_off.p;
  S.long_ptr = L.long_ptr.p;
  S.rec_long = L.rec_long.p;
  S.perm = L.perm.p;
  S.cvec = s.cvec.p;
  S.c8 = s.c8.p;
  S.c8s = s.c8s.p;
  S.nslices = L.nslices;
  S.n_long = L.n_long;
  S.n_ecs = L.E;
  S.n_groups = L.G;
  S.n_lut = L.n_lut;
  S.n_area = L.n_area;
  S.area_slot = L.area_slot.p;
  S.shift = L.dec.shift;
  S.mask = L.dec.mask;
  S.bhi = L.dec.bhi;
  S.bhiA = L.dec.bhiA;
  S.shiftH = L.dec.shiftH;
  S.maskH = L.dec.maskH;
  S.n_tab_lds = L.n_tab_lds;
  S.slice_hot = L.slice_hot.p;
  S.lut_area = L.lut_area.p;
  S.cls = L.cls;
  return S;
}
GuardDev guard_view(const Resident &L, const Solver &s) {
  return GuardDev{s.guard_list.p, s.guard_bits.p, s.guard_tail.p, L.lut_area.p, s.guard_err.p, s.guard_visits.p, L.guard_cap(),
                  L.guard_words()};
}

// pass B's mode for a given placement of the group vectors (glds) and n_tab slot entries in LDS; -1 = no fit
int passB_mode(const Resident &L, bool glds, uint32_t n_tab, bool index) {
  const uint32_t G = L.G;
  if (glds) {
    if (pass_lds_bytes(1, n_tab, G, false, index) > kLdsMax) return -1;
    // column sums at the fixed immediate distance when e_g fits below it and the image still fits
    if (8ull * (G + kSentinels) <= kAccFixed && pass_lds_bytes(2, n_tab, G, false, index) <= kLdsMax) return 2;
    return 1;
  }
  if (pass_lds_bytes(0, n_tab, G, false, index) > kLdsMax) return -1;
  if (getenv("MSWEEP_GLOBAL_ATOMICS")) return 0;  // developer switch: mode 0 (column sums in HBM)
  // too many groups for {e, w} / e + sums in LDS: the column sums alone may still fit (mode 3) ...
  if (pass_lds_bytes(3, n_tab, G, false, index) <= kLdsMax) return 3;
  // ... and beyond that one range of groups at a time does (mode 4), whatever the group count
  if (pass_lds_bytes(4, n_tab, G, false, index) <= kLdsMax) return 4;
  return 0;
}

// MSWEEP_MULTILANE=0 (developer switch): every EC of up to 256 cells one lane (slices of up to 256 rows on the
// streaming path of the sweeps), the layout of rounds 1-2
bool multilane() {
  const char *e = getenv("MSWEEP_MULTILANE");
  return !(e && atoi(e) == 0);
}
// slice / position boundaries of the classes from the ECs per class (n[c]: class c = 64 >> c lanes per EC)
SliceClasses make_slice_classes(const uint32_t *n) {
  SliceClasses C = {};
  for (int c = 0; c < kSliceClasses; ++c) {
    const uint32_t per = 64u >> (kMaxLgm - c);
    C.p0[c + 1] = C.p0[c] + n[c];
    C.s0[c + 1] = C.s0[c] + (n[c] + per - 1) / per;
  }
  return C;
}

void choose_lds_mode(Resident &L) {
  const bool opts[4][2] = {{true, true}, {true, false}, {false, true}, {false, false}};
  const char *force = getenv("MSWEEP_FORCE_LDS");  // developer switch: "gt", e.g. "10" = groups in LDS, slots not
  for (auto &o : opts) {
    if (force && strlen(force) == 2 && (o[0] != (force[0] == '1') || o[1] != (force[1] == '1'))) continue;
    const uint32_t n_tab = o[1] ? L.n_area : 0u;
    const int gmB = passB_mode(L, o[0], n_tab, false);
    // (too many groups for the group vectors AND a slot table that leaves no room for the column sums: the table
    // goes to memory -- or into the hybrid area -- rather than the column sums into HBM atomics, 20 x the cost)
    if (!force && !o[0] && o[1] && gmB == 0 && !getenv("MSWEEP_GLOBAL_ATOMICS")) continue;
    if (gmB >= 0 && pass_lds_bytes(o[0] ? 1 : 0, n_tab, L.G, true, false) <= kLdsMax) {
      L.glds = o[0];
      L.tlds = o[1];
      L.gmodeB = gmB;
      L.n_tab_lds = n_tab;
      return;
    }
  }
  throw Fail("internal: no LDS configuration fits");
}

// LDS mode, then the record encoding that goes with it (sell.hpp): the narrowest split of a
// 32-bit record that holds both byte offsets, else 8-byte records.  Runs before the SELL packing.
void choose_layout(Resident &L) {
  choose_lds_mode(L);
  L.dec.bhi = sell_bhi(L.n_tab_lds);
  L.dec.bhiA = 2 * L.dec.bhi;
  const uint64_t lo_end = 16ull * std::max<uint32_t>(L.n_area, 1);              // lo < lo_end
  const uint64_t hi_end = (uint64_t)L.dec.bhi + 8ull * ((uint64_t)L.G + kSentinels);  // hi < hi_end
  L.enc = kEncWide;
  L.dec.shift = 0;
  L.dec.mask = 0xffffffffu;
  const char *force = getenv("MSWEEP_RECORD_BYTES");  // developer switch: 8 = skip the 4-byte formats
  for (uint32_t s = 5; s <= 31 && !(force && atoi(force) == 8); ++s) {
    if (lo_end <= (1ull << (s - 1)) && hi_end <= (1ull << (32 - s))) {
      L.enc = kEncNarrow;
      L.dec.shift = s;
      L.dec.mask = (1u << (s - 1)) - 1u;
      break;
    }
  }
  if (L.wide() && (hi_end > (1ull << 31) || lo_end > (1ull << 32)))
    throw Fail("likelihood too large: group / lookup-table offsets exceed the 8-byte record fields");
}

// The hybrid slot area (sell.hpp, index records) for likelihoods whose slot tables do not fit LDS beside the
// group vectors: 4-byte records of (group, entry) INDICES when both fit 32 bits, the group vectors where
// choose_lds_mode put them, and as many of the most-used entries in LDS as both sweeps' images leave room for.
// Returns false (layout untouched) when it does not apply.
bool choose_hybrid_layout(Resident &L, bool no_hybrid) {
  if (L.tlds || no_hybrid) return false;
  if (const char *e = getenv("MSWEEP_HYBRID"))  // developer switch: 0 = the all-memory tables (and wide records)
    if (atoi(e) == 0) return false;
  const char *force = getenv("MSWEEP_RECORD_BYTES");
  if (force && atoi(force) == 8) return false;
  uint32_t eb = 1, gb = 1;
  while ((1ull << eb) < std::max<uint32_t>(L.n_area, 2)) ++eb;
  while ((1ull << gb) < (uint64_t)L.G + kSentinels) ++gb;
  if (eb + gb > 32) return false;
  // room for the table: the largest multiple of 16 entries (256 bytes) that both images hold
  uint32_t n_hot = 0;
  {
    const int gmA = L.glds ? 1 : 0;
    uint32_t lo = 0, hi = std::min<uint32_t>(L.n_area, (uint32_t)(kLdsMax / 16)) / 16;  // in units of 16 entries
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) / 2, n = mid * 16;
      const bool ok = pass_lds_bytes(gmA, n, L.G, true, true) <= kLdsMax && passB_mode(L, L.glds, n, true) >= 0 &&
                      (L.glds || passB_mode(L, false, n, true) == passB_mode(L, false, 0, true));
      if (ok) lo = mid;
      else hi = mid - 1;
    }
    n_hot = lo * 16;
  }
  if (const char *e = getenv("MSWEEP_HYBRID_HOT")) n_hot = std::min<uint32_t>(n_hot, (uint32_t)atoi(e) & ~15u);  // developer switch
  L.enc = kEncIndex;
  L.dec.shift = eb;
  L.dec.mask = (1u << eb) - 1u;
  L.n_tab_lds = std::min(n_hot, L.n_area);
  // the rows of a hot segment carry 16 * entry (entry < n_tab_lds): as many bits as the table's LDS image takes
  uint32_t hb = 4;
  while ((1ull << hb) < 16ull * std::max<uint32_t>(L.n_tab_lds, 1)) ++hb;
  if (hb + gb > 32) return false;  // (cannot happen while the table's image and the group vectors share 160 KB of LDS)
  L.dec.shiftH = hb;
  L.dec.maskH = (1u << hb) - 1u;
  L.dec.bhi = L.dec.bhiA = sell_bhi(L.n_tab_lds);
  L.gmodeB = passB_mode(L, L.glds, L.n_tab_lds, true);
  return true;
}

// a solver's buffers for the likelihood resident in L (they only grow: a bootstrap worker gets ready by this call)
void alloc_solve_state(const Resident &L, Solver &s) {
  const uint32_t G = L.G, E = L.E;
  for (DevBuf<double> *b : {&s.alpha0, &s.u, &s.os_u, &s.step_u, &s.w, &s.e, &s.N, &s.Nc,
                            &s.Acc, &s.logth})
    b->alloc((size_t)G + kSentinels);
  s.ew.alloc((size_t)G + kSentinels);
  // entries G.. of e / ew are the sentinel groups of SELL padding records: zero, never rewritten
  s.e.zero(s.stream);
  s.ew.zero(s.stream);
  s.cvec.alloc(E);
  s.c8.alloc((size_t)E + 64);
  s.c8s.alloc((size_t)L.nslices * 64 + 64);  // lanes without an EC stay 0: no EC
  s.c8s.zero(s.stream);
  s.logc_d.alloc(E);
  s.tabA.alloc((size_t)std::max<uint32_t>(L.n_area, 1));
  s.tabB.alloc((size_t)std::max<uint32_t>(L.n_area, 1));
  s.tab_built.alloc(2);
  const int nb = std::max(L.nblk, std::max(L.nblk_dense, L.npart_rows()));
  s.partA.alloc(std::max(nb, 1024));
  s.partS.alloc(4 * (size_t)std::max(nb, 1024));
  s.partR.alloc(kRedfinParts * ((size_t)G / kRedfinGroups + 2));
  s.totS.alloc(4);
  s.commA.alloc(1);
  s.commB.alloc(3 * (size_t)G + 4);  // column sums, two limbs of the guarded ECs' shares, ELBO terms
  s.partAcc.alloc((size_t)std::max(nb, 1) * G);
  s.partC.alloc(1024);
  if (L.flavor == 0) {
    const uint32_t nb0 = (uint32_t)std::max(L.nblk, 1);
    s.guard_list.alloc((size_t)nb0 * L.guard_cap());
    s.guard_bits.alloc((size_t)nb0 * 16 * L.guard_words());
    s.guard_bits.zero(s.stream);
    s.guard_tail.alloc(2 * (size_t)G);
    s.guard_tail.zero(s.stream);
  }
  s.guard_err.alloc(1);
  s.guard_err.zero(s.stream);
  s.guard_visits.alloc(1);
  s.guard_visits.zero(s.stream);
  s.sc.alloc(1);
  s.tr_bound.alloc(kMaxTrace);
  s.tr_newnorm.alloc(kMaxTrace);
  s.tr_beta.alloc(kMaxTrace);
  s.tr_reset.alloc(kMaxTrace);
  if (!s.sc_host) MSW_HIP(hipHostMalloc((void **)&s.sc_host, sizeof(Scalars)));
  if (!s.ev0) {
    MSW_HIP(hipEventCreate(&s.ev0));
    MSW_HIP(hipEventCreate(&s.ev1));
  }
}

// ---- launch helpers for the templated sweeps ----------------------------------------------
// The sweeps address their LDS image by absolute ds addresses taken from the records: the image
// must start at LDS address 0, i.e. the kernels must not own static __shared__ memory.
template <class K>
void prepare_sweep(K k, size_t lds, size_t &lds_set) {
  if (lds > lds_set) {  // raise the dynamic-LDS limit of this instantiation only when it grows
    hipFuncAttributes fa;
    MSW_HIP(hipFuncGetAttributes(&fa, (const void *)k));
    if (fa.sharedSizeBytes != 0) throw Fail("internal: sweep kernel owns static LDS");
    MSW_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set = lds;
  }
}
template <int ENC, bool GL, bool TL>
void launch_passA_t(const Resident &L, Solver &s) {
  const size_t lds = pass_lds_bytes(GL ? 1 : 0, L.n_tab_lds, L.G, true, ENC == kEncIndex);
  // ML: some slices hold ECs over several lanes (sell.hpp slice classes) -- an instantiation of its own: the few
  // scalar operations and branches the classes cost per slice are 2-3 % of a sweep over short slices (cfg3, cfg5)
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  auto k = ml ? k_passA<ENC, GL, TL, true> : k_passA<ENC, GL, TL, false>;
  prepare_sweep(k, lds, s.lds_attr[0][(ml ? 40 : 0) + ENC * 4 + (GL ? 2 : 0) + (TL ? 1 : 0)]);
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_A<ENC>()), lds, s.stream, s.sc.p, sell_view(L, s),
                     s.ew.p, s.tabA.p, s.partA.p, s.partR.p, (int)((L.G + kRedfinGroups - 1) / kRedfinGroups),
                     guard_view(L, s));
}
template <int ENC, int GM, bool TL>
void launch_passB_t(const Resident &L, Solver &s) {
  const size_t lds = pass_lds_bytes(GM, L.n_tab_lds, L.G, false, ENC == kEncIndex);
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  if constexpr (ENC == kEncNarrow) {
    if (L.passB_rc8 && !ml) {  // (nearly) every slice at most 8 rows: 16 wavefronts per workgroup (finish_sell)
      auto k8 = k_passB<ENC, GM, TL, false, 8>;
      prepare_sweep(k8, lds, s.lds_attr[2][2 * GM + (TL ? 1 : 0)]);
      const auto rg_of = [&](uint32_t g0) {
        return GM == 4 ? RangeB{g0, std::min<uint32_t>(kRangeGroups, L.G - g0), g0 == 0 ? 1 : 0} : RangeB{0, 0, 1};
      };
      for (uint32_t g0 = 0; g0 < (GM == 4 ? L.G : 1u); g0 += kRangeGroups)
        hipLaunchKernelGGL(k8, dim3(L.nblk), dim3(pass_threads_B<ENC, 8>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                           s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p, rg_of(g0), guard_view(L, s));
      return;
    }
  }
  auto k = ml ? k_passB<ENC, GM, TL, true> : k_passB<ENC, GM, TL, false>;
  prepare_sweep(k, lds, s.lds_attr[1][(ml ? 40 : 0) + ENC * 10 + 2 * GM + (TL ? 1 : 0)]);
  if (GM == 4) {  // one run per range of groups; the first also delivers the ELBO terms
    for (uint32_t g0 = 0; g0 < L.G; g0 += kRangeGroups)
      hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_B<ENC>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                         s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p,
                         RangeB{g0, std::min<uint32_t>(kRangeGroups, L.G - g0), g0 == 0 ? 1 : 0}, guard_view(L, s));
    return;
  }
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(pass_threads_B<ENC>()), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p,
                     s.tabB.p, s.partAcc.p, s.partS.p, s.Acc.p, RangeB{0, 0, 1}, guard_view(L, s));
}

#define MSW_DISPATCH3(fn, ...)                                                       \
  do {                                                                               \
    const int key = L.enc * 4 + (L.glds ? 2 : 0) + (L.tlds ? 1 : 0);              \
    switch (key) {                                                                   \
      case 0: fn<kEncNarrow, false, false>(__VA_ARGS__); break;                      \
      case 1: fn<kEncNarrow, false, true>(__VA_ARGS__); break;                       \
      case 2: fn<kEncNarrow, true, false>(__VA_ARGS__); break;                       \
      case 3: fn<kEncNarrow, true, true>(__VA_ARGS__); break;                        \
      case 4: fn<kEncWide, false, false>(__VA_ARGS__); break;                        \
      case 5: fn<kEncWide, false, true>(__VA_ARGS__); break;                         \
      case 6: fn<kEncWide, true, false>(__VA_ARGS__); break;                         \
      case 7: fn<kEncWide, true, true>(__VA_ARGS__); break;                          \
      case 8: fn<kEncIndex, false, false>(__VA_ARGS__); break;                       \
      case 10: fn<kEncIndex, true, false>(__VA_ARGS__); break;                       \
      case 12: fn<kEncValue, false, false>(__VA_ARGS__); break;                      \
      case 14: fn<kEncValue, true, false>(__VA_ARGS__); break;                       \
      default: throw Fail("internal: no sweep for this layout");                     \
    }                                                                                \
  } while (0)
#define MSW_DISPATCH_B(fn, ...)                                                      \
  do {                                                                               \
    const int key = L.enc * 10 + 2 * L.gmodeB + (L.tlds ? 1 : 0);                 \
    switch (key) {                                                                   \
      case 0: fn<kEncNarrow, 0, false>(__VA_ARGS__); break;                          \
      case 1: fn<kEncNarrow, 0, true>(__VA_ARGS__); break;                           \
      case 2: fn<kEncNarrow, 1, false>(__VA_ARGS__); break;                          \
      case 3: fn<kEncNarrow, 1, true>(__VA_ARGS__); break;                           \
      case 4: fn<kEncNarrow, 2, false>(__VA_ARGS__); break;                          \
      case 5: fn<kEncNarrow, 2, true>(__VA_ARGS__); break;                           \
      case 6: fn<kEncNarrow, 3, false>(__VA_ARGS__); break;                          \
      case 7: fn<kEncNarrow, 3, true>(__VA_ARGS__); break;                           \
      case 8: fn<kEncNarrow, 4, false>(__VA_ARGS__); break;                          \
      case 9: fn<kEncNarrow, 4, true>(__VA_ARGS__); break;                           \
      case 10: fn<kEncWide, 0, false>(__VA_ARGS__); break;                           \
      case 11: fn<kEncWide, 0, true>(__VA_ARGS__); break;                            \
      case 12: fn<kEncWide, 1, false>(__VA_ARGS__); break;                           \
      case 13: fn<kEncWide, 1, true>(__VA_ARGS__); break;                            \
      case 14: fn<kEncWide, 2, false>(__VA_ARGS__); break;                           \
      case 15: fn<kEncWide, 2, true>(__VA_ARGS__); break;                            \
      case 16: fn<kEncWide, 3, false>(__VA_ARGS__); break;                           \
      case 17: fn<kEncWide, 3, true>(__VA_ARGS__); break;                            \
      case 18: fn<kEncWide, 4, false>(__VA_ARGS__); break;                           \
      case 19: fn<kEncWide, 4, true>(__VA_ARGS__); break;                            \
      case 20: fn<kEncIndex, 0, false>(__VA_ARGS__); break;                          \
      case 22: fn<kEncIndex, 1, false>(__VA_ARGS__); break;                          \
      case 24: fn<kEncIndex, 2, false>(__VA_ARGS__); break;                          \
      case 26: fn<kEncIndex, 3, false>(__VA_ARGS__); break;                          \
      case 28: fn<kEncIndex, 4, false>(__VA_ARGS__); break;                          \
      case 30: fn<kEncValue, 0, false>(__VA_ARGS__); break;                          \
      case 32: fn<kEncValue, 1, false>(__VA_ARGS__); break;                          \
      case 34: fn<kEncValue, 2, false>(__VA_ARGS__); break;                          \
      case 36: fn<kEncValue, 3, false>(__VA_ARGS__); break;                          \
      case 38: fn<kEncValue, 4, false>(__VA_ARGS__); break;                          \
      default: throw Fail("internal: no sweep for this layout");                     \
    }                                                                                \
  } while (0)

template <int NREG>
void launch_dense_A(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_passA<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.u.p, s.w.p, s.partA.p);
}
template <int NREG>
void launch_dense_B(const Resident &L, Solver &s) {
  const size_t lds = (32 + 4 * (size_t)L.G) * sizeof(double);
  hipLaunchKernelGGL(k_dense_passB<NREG>, dim3(L.nblk_dense), dim3(256), lds, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.cvec.p, s.u.p, s.partAcc.p, s.partS.p);
}
template <int NREG>
void launch_dense_big_A(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_big_passA<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.u.p, s.w.p, s.partA.p);
}
template <int NREG>
void launch_dense_big_B(const Resident &L, Solver &s) {
  hipLaunchKernelGGL(k_dense_big_passB<NREG>, dim3(L.nblk_dense), dim3(256), 0, s.stream, s.sc.p,
                     L.Lt.p, (int)L.G, L.E, s.cvec.p, s.u.p, s.partAcc.p, s.partS.p);
}
#define MSW_DISPATCH_NREG(fn, fnbig, ...)                \
  do {                                                   \
    switch (L.nreg) {                                   \
      case 1: fn<1>(__VA_ARGS__); break;                 \
      case 2: fn<2>(__VA_ARGS__); break;                 \
      case 4: fn<4>(__VA_ARGS__); break;                 \
      case 8: fn<8>(__VA_ARGS__); break;                 \
      case 16: fn<16>(__VA_ARGS__); break;               \
      case 32: fnbig<32>(__VA_ARGS__); break;            \
      case 64: fnbig<64>(__VA_ARGS__); break;            \
      default: fnbig<128>(__VA_ARGS__); break;           \
    }                                                    \
  } while (0)

void launch_passA(const Resident &L, Solver &s) {
  std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
  if (s.profiling) {
    ev = &next_pair(s.evA, s.evA_used);
    MSW_HIP(hipEventRecord(ev->first, s.stream));
  }
  if (L.flavor == 0) MSW_DISPATCH3(launch_passA_t, L, s);
  else MSW_DISPATCH_NREG(launch_dense_A, launch_dense_big_A, L, s);
  MSW_HIP(hipGetLastError());
  if (ev) MSW_HIP(hipEventRecord(ev->second, s.stream));
  s.timing.passA_launches++;
}

// --emprecision float: the fp32 sweeps of em_f32_kernels.hpp (run_em decides; one persistent workgroup per CU).
// Served: one GPU, the CSR flavour, the group vectors in LDS, at most kStepRegs * 1024 groups, and either offset records
// with the whole slot table in LDS or index records (the hybrid area, whatever part of it the fp64 images hold) whose
// FLOAT image -- 4 bytes per entry of the whole area, 12 per group -- fits LDS.
bool em_f32_layout_ok(const Resident &L, const Solver &s) {
  if (!kFx || L.flavor != 0 || !L.glds || s.comm() || L.G > (uint32_t)(kStepRegs * 1024)) return false;
  if (getenv("MSWEEP_EM_FLOAT_AS_DOUBLE")) return false;  // (developer switch: the fp64 kernels under MSW_PREC_FLOAT, as until round 4)
  if (L.enc == kEncNarrow)
    return L.tlds && L.n_tab_lds == L.n_area && em_f32_lds_bytes(L.n_tab_lds, L.G) <= kLdsMax;
  // (shift <= 30: the two shifts that leave 4 * entry of a record, em_f32_kernels.hpp F32Form)
  if (L.hybrid()) return L.dec.shift <= 30 && em_f32_idx_lds_bytes(L.n_area, L.G) <= kLdsMax;
  return false;
}
void launch_em_passB_f32(const Resident &L, Solver &s) {
  const bool idx = L.hybrid();
  const size_t lds = idx ? em_f32_idx_lds_bytes(L.n_area, L.G) : em_f32_lds_bytes(L.n_tab_lds, L.G);
  const bool ml = L.cls.s0[kSliceClasses - 1] > 0;
  auto k = idx ? (ml ? k_em_passB_f32_idx<true> : k_em_passB_f32_idx<false>)
               : (ml ? k_em_passB_f32<true> : k_em_passB_f32<false>);
  prepare_sweep(k, lds, s.lds_attr[2][30 + (idx ? 2 : 0) + (ml ? 1 : 0)]);
  hipLaunchKernelGGL(k, dim3(L.nblk), dim3(1024), lds, s.stream, s.sc.p, sell_view(L, s), s.e.p, s.e32.p, s.tab32.p,
                     s.partAcc.p, s.partS.p, guard_view(L, s));
}

void launch_passB(const Resident &L, Solver &s) {
  std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
  if (s.profiling) {
    ev = &next_pair(s.evB, s.evB_used);
    MSW_HIP(hipEventRecord(ev->first, s.stream));
  }
  if (L.flavor == 0 && s.em_f32) {
    launch_em_passB_f32(L, s);
  } else if (L.flavor == 0) {
    if (L.gmodeB == 0) MSW_HIP(hipMemsetAsync(s.Acc.p, 0, ((size_t)L.G + kSentinels) * sizeof(double), s.stream));
    MSW_DISPATCH_B(launch_passB_t, L, s);
  } else {
    MSW_DISPATCH_NREG(launch_dense_B, launch_dense_big_B, L, s);
  }
  MSW_HIP(hipGetLastError());
  if (ev) MSW_HIP(hipEventRecord(ev->second, s.stream));
  s.timing.passB_launches++;
  // column sums across workgroups + N_g / lgamma / digamma, spread over G/16 workgroups
  const bool partials = (L.flavor == 1) || L.gmodeB > 0 || s.em_f32;
  const int nb = L.npart_rows();
  // the CSR sweeps leave fixed-point integer rows (kFx); 2: the fp32 EM sweep's, without the per-group factor
  const int fxrows = L.flavor == 0 ? (s.em_f32 ? 2 : 1) : 0;
  if (s.comm()) {
    // EC-sharded: local column sums + ELBO terms -> one all-reduce -> k_redfin on the totals.  The
    // fixed-point column sums are all-reduced as INTEGERS: exact, so the totals -- and with them every
    // N_g -- are the same bits whatever the number of ranks the ECs are spread over.
    const size_t G3 = 3 * (size_t)L.G;
    std::pair<hipEvent_t, hipEvent_t> *evc = nullptr;
    if (s.profiling) {
      evc = &next_pair(s.evC, s.evC_used);
      MSW_HIP(hipEventRecord(evc->first, s.stream));
    }
    hipLaunchKernelGGL(k_colsum, dim3((L.G + 63) / 64), dim3(1024), 0, s.stream, s.sc.p, (int)L.G,
                       partials ? nb : 0, fxrows, nb, s.partAcc.p, s.Acc.p, s.partS.p,
                       fxrows ? s.guard_tail.p : nullptr, s.commB.p);
    if (kFx && fxrows) {
      s.comm()->allreduce_mixed(reinterpret_cast<uint64_t *>(s.commB.p), G3, s.commB.p + G3, 4, s.stream);
    } else {  // fp64 column sums (dense flavour, MSW_FX=0 builds): doubles, then the integer limbs
      s.comm()->allreduce(s.commB.p, (size_t)L.G, s.stream);
      s.comm()->allreduce_mixed(reinterpret_cast<uint64_t *>(s.commB.p) + L.G, 2 * (size_t)L.G, s.commB.p + G3, 4,
                               s.stream);
    }
    if (evc) MSW_HIP(hipEventRecord(evc->second, s.stream));
    hipLaunchKernelGGL(k_redfin, dim3((L.G + kRedfinGroups - 1) / kRedfinGroups), dim3(kRedfinThreads), 0, s.stream,
                       s.sc.p, (int)L.G, 0, fxrows, reinterpret_cast<unsigned long long *>(s.commB.p) + L.G, 0, 1,
                       s.partAcc.p, s.commB.p, s.commB.p + G3, s.e.p, s.u.p,
                       s.alpha0.p, s.Nc.p, s.N.p, s.w.p, s.ew.p, s.partR.p, s.totS.p);
    return;
  }
  hipLaunchKernelGGL(k_redfin, dim3((L.G + kRedfinGroups - 1) / kRedfinGroups), dim3(kRedfinThreads), 0, s.stream,
                     s.sc.p, (int)L.G, partials ? nb : 0, fxrows, fxrows ? s.guard_tail.p : nullptr, 1, nb,
                     s.partAcc.p, s.Acc.p, s.partS.p, s.e.p,
                     s.u.p, s.alpha0.p, s.Nc.p, s.N.p, s.w.p, s.ew.p, s.partR.p, s.totS.p);
}

// partS as seen by k_fin / k_em_fin: the all-reduced totals when sharded
const double *fin_partS(const Resident &L, Solver &s) { return s.comm() ? s.commB.p + 3 * (size_t)L.G : s.partS.p; }
int fin_npartS(const Resident &L, Solver &s) { return s.comm() ? 1 : L.npart_rows(); }

// slot areas beyond kTabInline entries: the tables are rebuilt by their own kernel after every
// kernel that may have moved a (it returns at once when they are current)
void launch_tables(const Resident &L, Solver &s) {
  if (L.flavor != 0 || L.n_area <= (uint32_t)kTabInline) return;
  const unsigned nb = std::min<unsigned>((L.n_area + 255) / 256, (unsigned)s.n_cu * 8);
  hipLaunchKernelGGL(k_tables, dim3(nb), dim3(256), 0, s.stream, s.sc.p, (int)L.n_area, L.lut_area.p, s.tabs(),
                     s.tab_built.p);
}

// the verdict on the pending evaluation + the next step (state_kernels.hpp k_finstep); mode 1: the verdict alone
void launch_finstep(const Resident &L, Solver &s, int mode) {
  TraceDev tr{s.tr_bound.p, s.tr_newnorm.p, s.tr_beta.p, s.tr_theta.p, s.tr_reset.p};
  const double *pA = s.partA.p;
  int npA = L.flavor == 0 ? L.nblk : L.nblk_dense;
  if (s.comm()) {  // |g|^2 summed over the EC shards (run_rcg)
    pA = s.commA.p;
    npA = 1;
  }
  hipLaunchKernelGGL(k_finstep, dim3(1), dim3(1024), 0, s.stream, s.sc.p, mode, (int)L.G, L.n_tab_inline(), npA, pA,
                     (int)((L.G + kRedfinGroups - 1) / kRedfinGroups), s.totS.p, s.partR.p, s.Nc.p, s.w.p, s.u.p,
                     s.os_u.p, s.step_u.p, L.lut_area.p, s.e.p, s.tabs(), tr);
  launch_tables(L, s);
}

void poll(Solver &s) {
  MSW_HIP(hipMemcpyAsync(s.sc_host, s.sc.p, sizeof(Scalars), hipMemcpyDeviceToHost, s.stream));
  MSW_HIP(hipStreamSynchronize(s.stream));
  if (s.comm()) s.comm()->check();
}

// Inputs of one solve: c_j (from log counts or from bootstrap counts already on the device) and
// the prior.  Leaves per-block partial sums of c in partC for k_init_state.
constexpr int kCvecBlocks = 512;
void prepare_inputs(const Resident &L, Solver &s, const double *logc_host, const uint32_t *counts_dev,
                    const double *alpha0_host) {
  if (L.flavor < 0) throw Fail("no likelihood resident: call msw_core_set_csr / set_dense_logl first");
  const uint32_t E = L.E, G = L.G;
  if (counts_dev) {
    hipLaunchKernelGGL(k_cvec_from_counts, dim3(kCvecBlocks), dim3(256), 0, s.stream, counts_dev,
                       L.flavor == 0 ? L.perm.p : nullptr, E, s.cvec.p, s.c8.p, s.partC.p, L.cls, L.n_long,
                       L.flavor == 0 ? s.c8s.p : nullptr);
  } else {
    const double *src = s.logc_d.p;
    if (logc_host) {
      MSW_HIP(hipMemcpyAsync(s.logc_d.p, logc_host, E * sizeof(double), hipMemcpyHostToDevice, s.stream));
    } else {  // the log counts msw_core_build_likelihood left on the device: no 8 * E byte upload
      if (!L.have_logc_res) throw Fail("null logc: only a likelihood built by msw_core_build_likelihood keeps its log counts");
      src = L.logc_res.p;
    }
    hipLaunchKernelGGL(k_cvec_from_logc, dim3(kCvecBlocks), dim3(256), 0, s.stream, src,
                       L.flavor == 0 ? L.perm.p : nullptr, E, s.cvec.p, s.c8.p, s.partC.p, L.cls, L.n_long,
                       L.flavor == 0 ? s.c8s.p : nullptr);
  }
  if (alpha0_host)
    MSW_HIP(hipMemcpyAsync(s.alpha0.p, alpha0_host, G * sizeof(double), hipMemcpyHostToDevice, s.stream));
  MSW_HIP(hipGetLastError());
  // logc_host / alpha0_host may be pageable caller memory: finish the copies before returning
  MSW_HIP(hipStreamSynchronize(s.stream));
  s.prepared = true;
}

// argument / state errors of a solve: thrown BEFORE anything that a peer of a sharded solve could wait for
void validate_solve(size_t max_iters, int algo, int prec) {
  if (algo != MSW_ALGO_RCG && algo != MSW_ALGO_EM) throw Fail("unknown algorithm id");
  if (prec != MSW_PREC_DOUBLE && prec != MSW_PREC_FLOAT) throw Fail("unknown precision id");
  if (max_iters == 0 || max_iters > (size_t)std::numeric_limits<int32_t>::max())
    throw Fail("max_iters out of range");
}

void begin_solve(const Resident &L, Solver &s, double tol, size_t max_iters) {
  const uint32_t G = L.G;
  if (s.trace_theta) s.tr_theta.alloc(s.trace_theta * G);
  const double *cpart = s.partC.p;
  int ncpart = kCvecBlocks;
  if (s.comm()) {  // global sum of the EC counts (bound constant, theta normalisation)
    s.comm()->rendezvous();  // the ranks' calls may be seconds apart on the host: meet before the device-side waits
    hipLaunchKernelGGL(k_sum_scalar, dim3(1), dim3(1024), 0, s.stream, s.sc.p, 0, kCvecBlocks, s.partC.p,
                       s.commA.p);
    s.comm()->allreduce(s.commA.p, 1, s.stream);
    cpart = s.commA.p;
    ncpart = 1;
  }
  hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1024), 0, s.stream, s.sc.p, (int)G, ncpart,
                     cpart, s.alpha0.p, s.u.p, s.os_u.p, s.step_u.p, tol, (int)max_iters,
                     s.fixed_iters ? 1 : 0, (int)s.trace_theta, L.flavor, L.logzi, s.opts, s.tab_built.p,
                     L.trange.p);
  MSW_HIP(hipGetLastError());
}

// iters_start > 0: the solve on the handle is continued (msw_core_continue) -- no initial evaluation
void run_rcg(const Resident &L, Solver &s, size_t max_iters, size_t iters_start = 0) {
  const int G = (int)L.G, n_lut = L.n_tab_inline();
  if (iters_start > 0 && s.comm()) s.comm()->rendezvous();  // msw_core_continue: as begin_solve
  if (iters_start == 0) {
    // initial update_N_k on gamma = log(1/G): the first slot's k_finstep finds it as Scalars::have_eval = 2
    hipLaunchKernelGGL(k_prepB, dim3(1), dim3(1024), 0, s.stream, s.sc.p, G, n_lut, s.u.p, L.lut_area.p,
                       s.e.p, s.tabs());
    launch_tables(L, s);
    launch_passB(L, s);
    s.timing.passB_launches--;  // the initial evaluation is not an iteration
    if (s.profiling && s.evB_used) s.evB_used--;
  }
  const int nbA = L.flavor == 0 ? L.nblk : L.nblk_dense;
  // Slots (state_kernels.hpp k_finstep): k_passA -> k_finstep -> k_passB (+ k_redfin); one per iteration plus one per
  // rejected step.  The verdict on a slot's evaluation is taken by the NEXT slot's k_finstep, so the iteration count
  // the host polls lags the evaluations by one: enqueue as many slots as iterations are still missing, poll, repeat;
  // slots enqueued past the end return at once (Scalars::done), and a verdict-only launch closes the run where the
  // count, not the tolerance, ends it.
  size_t iters_done = iters_start;
  for (;;) {
    // fixed-iteration runs know how many slots are missing; otherwise poll every kIterBatch
    const size_t missing = std::max<size_t>(1, max_iters - std::min(max_iters, iters_done));
    const size_t batch = s.fixed_iters ? std::min<size_t>(256, missing) : std::min<size_t>(kIterBatch, missing);
    for (size_t b = 0; b < batch; ++b) {
      launch_passA(L, s);
      if (s.comm()) {  // |g|^2 summed over the EC shards
        std::pair<hipEvent_t, hipEvent_t> *evc = nullptr;
        if (s.profiling) {
          evc = &next_pair(s.evC, s.evC_used);
          MSW_HIP(hipEventRecord(evc->first, s.stream));
        }
        hipLaunchKernelGGL(k_sum_scalar, dim3(1), dim3(1024), 0, s.stream, s.sc.p, 1, nbA, s.partA.p,
                           s.commA.p);
        s.comm()->allreduce(s.commA.p, 1, s.stream);
        if (evc) MSW_HIP(hipEventRecord(evc->second, s.stream));
      }
      launch_finstep(L, s, 0);
      launch_passB(L, s);
    }
    MSW_HIP(hipGetLastError());
    poll(s);
    if (s.sc_host->done) break;
    if (s.sc_host->have_eval && (size_t)s.sc_host->iter + 1 >= max_iters) {  // the last evaluation's verdict ends the run
      launch_finstep(L, s, 1);
      MSW_HIP(hipGetLastError());
      poll(s);
      if (s.sc_host->done) break;
    }
    iters_done = (size_t)s.sc_host->iter;
  }
}

void finish_solve(const Resident &L, Solver &s, double *theta_out, size_t *iters_out, double *bound_out) {
  poll(s);
  const uint32_t G = L.G;
  int gerr = 0;
  MSW_HIP(hipMemcpy(&gerr, s.guard_err.p, sizeof gerr, hipMemcpyDeviceToHost));
  if (gerr) {
    MSW_HIP(hipMemset(s.guard_err.p, 0, sizeof gerr));
    if (gerr == 2) throw Fail("internal: a workgroup's list of guarded equivalence classes overflowed");
    throw NumericFail("likelihood underflow: an equivalence class has zero probability under every group "
                      "(exp(a * log-likelihood) and the group weights underflow fp64 together)");
  }
  // (an EM run that was asked for no iteration leaves its initial bound, -inf: nothing is wrong)
  if (s.sc_host->iter > 0 && !std::isfinite(s.sc_host->bound))
    throw NumericFail("the evidence lower bound is not finite: the likelihood or the prior counts are out of range");
  if (theta_out) {
    if (s.last_algo == MSW_ALGO_EM) {
      MSW_HIP(hipMemcpy(theta_out, s.logth.p, G * sizeof(double), hipMemcpyDeviceToHost));  // theta of the last M-step
    } else {
      std::vector<double> nc(G);
      MSW_HIP(hipMemcpy(nc.data(), s.Nc.p, G * sizeof(double), hipMemcpyDeviceToHost));
      const double csum = s.sc_host->csum;
      for (uint32_t g = 0; g < G; ++g) theta_out[g] = nc[g] / csum;
    }
  }
  if (iters_out) *iters_out = (size_t)s.sc_host->iter;
  if (bound_out) *bound_out = s.sc_host->bound;
  s.have_solution = true;
}

void collect_timing(const Resident &L, Solver &s) {
  float ms = 0.f;
  MSW_HIP(hipEventElapsedTime(&ms, s.ev0, s.ev1));
  s.timing.solve_ms = ms;
  s.timing.passA_ms = s.timing.passB_ms = 0.0;
  if (s.profiling) {
    // launches enqueued after `done` was set return immediately; they are still counted
    for (size_t i = 0; i < s.evA_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evA[i].first, s.evA[i].second));
      s.timing.passA_ms += ms;
    }
    for (size_t i = 0; i < s.evB_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evB[i].first, s.evB[i].second));
      s.timing.passB_ms += ms;
    }
    s.timing.collective_ms = 0.0;
    for (size_t i = 0; i < s.evC_used; ++i) {
      MSW_HIP(hipEventElapsedTime(&ms, s.evC[i].first, s.evC[i].second));
      s.timing.collective_ms += ms;
    }
    s.timing.collectives = s.evC_used;
  }
  s.timing.iters = (uint64_t)s.sc_host->iter;
  const uint64_t recsz = L.enc == kEncValue ? 12 : (L.wide() ? 8 : 4);
  if (L.flavor == 0) {
    // algorithmic bytes: every real cell record once + the per-EC count vector in
    // pass B; SELL padding, slice offsets and the L2-served second read of pass B are not counted
    // (slot tables that do not fit LDS are read from memory: every used 16-byte entry at least once per sweep)
    // (a hybrid area: the entries beyond its LDS-resident head)
    const uint64_t tab = L.tlds ? 0ull : 16ull * (L.n_area - L.n_tab_lds);
    s.timing.bytes_passA = L.nnz * recsz + tab;
    s.timing.bytes_passB = L.nnz * recsz + 1ull * L.E + tab;  // + one byte per EC (its multiplicity)
  } else {
    s.timing.bytes_passA = 8ull * L.E * L.G;
    s.timing.bytes_passB = 8ull * L.E * L.G + 8ull * L.E;
  }
}

void run_em(const Resident &L, Solver &s, size_t max_iters, int prec);

// n more iterations of the fixed-iteration RCG solve that last ran on the handle: the state carries on
// where it stood (no re-initialisation, no initial evaluation) -- what a benchmark's "W warm-up steps,
// then exactly K timed steps" means for an iterative solver.
void continue_impl(const Resident &L, Solver &s, size_t n_iters, double *theta_out, size_t *iters_out, double *bound_out) {
  if (!s.have_solution || !s.fixed_iters || s.last_algo != MSW_ALGO_RCG)
    throw Fail("msw_core_continue: needs a fixed-iteration RCG solve on the handle (msw_core_set_fixed_iters, msw_core_run)");
  const size_t start = (size_t)s.sc_host->iter;
  if (n_iters == 0 || start + n_iters > (size_t)std::numeric_limits<int32_t>::max()) throw Fail("msw_core_continue: iteration count out of range");
  s.timing = {};
  s.evA_used = s.evB_used = s.evC_used = 0;
  CollectiveScope cs(s.collective);
  hipLaunchKernelGGL(k_extend, dim3(1), dim3(1), 0, s.stream, s.sc.p, (int)n_iters);
  MSW_HIP(hipEventRecord(s.ev0, s.stream));
  run_rcg(L, s, start + n_iters, start);
  MSW_HIP(hipEventRecord(s.ev1, s.stream));
  finish_solve(L, s, theta_out, iters_out, bound_out);
  collect_timing(L, s);
  s.timing.iters = (uint64_t)s.sc_host->iter - start;
  cs.leave();
}

void run_impl(const Resident &L, Solver &s, double tol, size_t max_iters, int algo, int prec, double *theta_out,
              size_t *iters_out, double *bound_out) {
  validate_solve(max_iters, algo, prec);
  if (!s.prepared) throw Fail("msw_core_run: inputs not prepared (call msw_core_prepare)");
  s.timing = {};
  s.evA_used = s.evB_used = s.evC_used = 0;
  CollectiveScope cs(s.collective);  // from here on a failure strands the peers of a sharded solve (guarded())
  begin_solve(L, s, tol, max_iters);
  MSW_HIP(hipEventRecord(s.ev0, s.stream));
  if (algo == MSW_ALGO_RCG) run_rcg(L, s, max_iters);
  else run_em(L, s, max_iters, prec);
  MSW_HIP(hipEventRecord(s.ev1, s.stream));
  s.last_algo = algo;
  finish_solve(L, s, theta_out, iters_out, bound_out);
  collect_timing(L, s);
  cs.leave();
}

}  // namespace

namespace {
// MSWEEP_BUILD_TIMING=1 (developer switch): wall time of every stage of the build / the packer to stderr (each
// mark drains the stream first, so the stages are what they say; off: no synchronisation, no output)
struct StageTimer {
  hipStream_t st;
  bool on;
  std::chrono::steady_clock::time_point t0;
  explicit StageTimer(hipStream_t s) : st(s), on(getenv("MSWEEP_BUILD_TIMING") != nullptr), t0(std::chrono::steady_clock::now()) {}
  void mark(const char *what) {
    if (!on) return;
    (void)hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[msweep build] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};
}  // namespace

#include "host_likelihood.inc"
#include "host_pack.inc"
#include "host_em.inc"
#include "host_mtjump.inc"
#include "host_bootstrap.inc"
#include "host_build.inc"
#include "host_compress.inc"
#include "host_alignment.inc"
#include "host_reader.inc"
#include "host_inflate.inc"
#include "host_inflate_members.inc"
#include "host_likelihood_file.inc"
#include "host_bin.inc"
#include "host_text.inc"
#include "host_gzip.inc"
#include "host_fastq.inc"

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

#ifndef MSW_SRC_HASH
#define MSW_SRC_HASH "unhashed"
#endif
// "... src <hash>": sha256 prefix of the sources this library was compiled from (__graft_entry__.source_hash)
const char *msw_core_version(void) { return "msweep_core 0.2 gfx950 (HIP, wave64) src " MSW_SRC_HASH; }

const char *msw_last_error(msw_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msw_core_create(int device, msw_handle *out) {
  if (!out) return 1;
  *out = nullptr;
  try {
    int n = 0;
    MSW_HIP(hipGetDeviceCount(&n));
    if (n <= 0) throw Fail("no HIP device visible: libmsweep_core has no CPU fallback");
    if (device < 0 || device >= n) throw Fail("device index out of range");
    MSW_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MSW_HIP(hipGetDeviceProperties(&prop, device));
    std::unique_ptr<msw_core> h(new msw_core);
    h->device = device;
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    MSW_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->solver.stream = h->stream;
    h->solver.n_cu = h->n_cu;
    hipLaunchKernelGGL(k_warm, dim3(1), dim3(1), 0, h->stream, (int *)nullptr);  // code object load: here, once per process
    MSW_HIP(hipGetLastError());
    MSW_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    return 1;
  }
}

void msw_core_destroy(msw_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

int msw_core_shape(msw_handle h, size_t *n_groups, size_t *n_ecs, size_t *nnz) {
  return guarded(h, [&] {
    if (h->lik.flavor < 0) throw Fail("no likelihood resident");
    if (n_groups) *n_groups = h->lik.G;
    if (n_ecs) *n_ecs = h->lik.E;
    if (nnz) *nnz = h->lik.flavor == 0 ? h->lik.nnz : (size_t)h->lik.G * h->lik.E;
  });
}

int msw_core_set_dense_logl(msw_handle h, const double *L, size_t n_groups, size_t n_ecs, size_t ld) {
  return guarded(h, [&] { set_dense_impl(h, L, n_groups, n_ecs, ld); });
}

int msw_core_set_dense_logl_file(msw_handle h, const char *path, size_t n_groups, msw_likfile_info *info) {
  return guarded(h, [&] {
    if (!path) throw Fail("msw_core_set_dense_logl_file: null path");
    set_dense_file_impl(h, path, nullptr, 0, n_groups, info);
  });
}

int msw_core_set_dense_logl_text(msw_handle h, const char *text, size_t n, size_t n_groups, msw_likfile_info *info) {
  return guarded(h, [&] { set_dense_file_impl(h, nullptr, text, n, n_groups, info); });
}

int msw_core_likfile_counts(msw_handle h, uint64_t *counts_out, size_t n_ecs) {
  return guarded(h, [&] { likfile_counts_impl(h, counts_out, n_ecs); });
}

int msw_core_set_csr(msw_handle h, const uint64_t *rowptr, const uint32_t *grp, const uint32_t *cnt,
                     const double *lut, size_t lut_ld, double logzi, size_t n_groups, size_t n_ecs) {
  return guarded(h, [&] { set_csr_impl(h, rowptr, grp, cnt, lut, lut_ld, logzi, n_groups, n_ecs); });
}

int msw_core_build_likelihood(msw_handle h, const uint64_t *ec_tptr, const uint32_t *ec_targets,
                              size_t n_ecs, const uint32_t *target_group, size_t n_targets,
                              const uint64_t *group_sizes, size_t n_groups, const uint64_t *ec_counts,
                              double q, double e, double zero_inflation, size_t min_hits,
                              size_t *n_groups_out, uint8_t *mask_out, double *logc_out) {
  return guarded(h, [&] {
    build_likelihood_impl(h, ec_tptr, ec_targets, n_ecs, target_group, n_targets, group_sizes,
                          n_groups, ec_counts, q, e, zero_inflation, min_hits, n_groups_out, mask_out,
                          logc_out, false, 0);
  });
}

int msw_core_build_likelihood_aln(msw_handle h, msw_alignment_t a, const uint32_t *target_group, size_t n_targets,
                                  const uint64_t *group_sizes, size_t n_groups, double q, double e,
                                  double zero_inflation, size_t min_hits, size_t *n_groups_out, uint8_t *mask_out,
                                  double *logc_out) {
  return guarded(h, [&] {
    if (!a) throw Fail("msw_core_build_likelihood_aln: null alignment");
    if (a->on_device && a->device == h->device) {
      // the reader's arrays are consumed where they lie (same device; the reader ran on this handle's stream or
      // has synchronised its own)
      build_likelihood_impl(h, a->d_tptr.p, a->d_targets.p, a->E, target_group, n_targets, group_sizes, n_groups,
                            a->d_counts.p, q, e, zero_inflation, min_hits, n_groups_out, mask_out, logc_out, true, a->H);
    } else {
      a->to_host(msw_alignment::kAlnTptr | msw_alignment::kAlnTargets | msw_alignment::kAlnCounts);
      build_likelihood_impl(h, a->ec_tptr.data(), a->ec_targets.data(), a->ec_counts.size(), target_group, n_targets,
                            group_sizes, n_groups, a->ec_counts.data(), q, e, zero_inflation, min_hits, n_groups_out,
                            mask_out, logc_out, false, 0);
    }
  });
}

int msw_core_trim(msw_handle h) {
  return guarded(h, [&] {
    MSW_HIP(hipStreamSynchronize(h->stream));
    h->reader_pool.trim();
    h->text.release_device();  // (the pinned text of the last msw_core_text_block stays valid)
    h->gz.release_device();
  });
}

int msw_alignment_read_device(msw_handle h, const char *const *paths, size_t n_paths, size_t n_targets, int merge_mode,
                              msw_alignment_t *out) {
  if (out) *out = nullptr;
  const int rc = guarded(h, [&] {
    check_reader_args(paths, out, n_paths, n_targets, merge_mode);
    std::unique_ptr<msw_alignment> a(new msw_alignment);
    a->device = h->device;
    MSW_HIP(hipStreamSynchronize(h->stream));
    h->reader_pool.recycle();  // (blocks the previous read handed back: nothing of it is in flight any more)
    ReaderCtx cx(h->stream, h->n_cu, &h->text_stage, &h->reader_pool, h->device);
    cx.inf = &h->inf;
    h->inf.last.clear();
    bool fits = true;
    {  // ~5 bytes of device memory per byte of text (measured: 10 GB at cfg3's 2.09 GB, 45 GB at 9.5 GB): a text that
       // would not fit beside what the device already holds goes to the host reader
      uint64_t text = 0;
      for (size_t i = 0; i < n_paths; ++i) {
        struct stat sb;
        if (paths[i] && stat(paths[i], &sb) == 0) text += (uint64_t)sb.st_size * (path_is_gzip(paths[i]) ? 8u : 1u);
      }
      size_t free_b = 0, total_b = 0;
      MSW_HIP(hipMemGetInfo(&free_b, &total_b));
      // (what earlier reads left idle on the handle counts as room; when it would be needed as FRESH memory -- a text of
      // another size class -- it goes back to the device first)
      const uint64_t need = 6 * text + (1ull << 30);
      if (need > (uint64_t)free_b && h->reader_pool.idle_bytes()) {
        h->reader_pool.trim();
        MSW_HIP(hipMemGetInfo(&free_b, &total_b));
      }
      fits = need <= (uint64_t)free_b + h->reader_pool.idle_bytes();
      if (getenv("MSWEEP_READER_FORCE_HOST")) fits = false;  // developer switch (tests): the host reader behind this entry
    }
    try {
      if (!fits) throw ReaderFallback{};
      try {
        read_alignment_device(paths, n_paths, n_targets, merge_mode, cx, *a);
      } catch (const HipError &ex) {
        if (!strstr(ex.what(), "out of memory")) throw;
        (void)hipGetLastError();
        throw ReaderFallback{};
      }
    } catch (const ReaderFallback &) {
      // text the kernels do not judge: the host reader's outcome -- a result or the reference's message -- stands
      msw_alignment_t host = nullptr;
      if (msw_alignment_read(paths, n_paths, n_targets, merge_mode, &host) != 0) throw Fail(msw_alignment_last_error());
      *out = host;
      return;
    }
    *out = a.release();
  });
  if (rc != 0 && h) g_aln_error = msw_last_error(h);
  return rc;
}

int msw_core_layout_info(msw_handle h, msw_layout_info *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    const Resident &L = h->lik;
    if (L.flavor != 0) throw Fail("msw_core_layout_info: no CSR-of-ECs likelihood resident");
    msw_layout_info li = {};
    li.record_bytes = L.enc == kEncValue ? 12 : (L.wide() ? 8 : 4);
    li.index_records = L.hybrid() ? 1 : 0;
    li.groups_in_lds = L.glds ? 1 : 0;
    li.table_in_lds = L.tlds ? 1 : 0;
    li.passB_mode = L.gmodeB;
    li.slot_entries = L.n_area;
    li.slot_entries_in_lds = L.n_tab_lds;
    li.n_slices = L.nslices;
    li.n_long_ecs = L.n_long;
    li.bank_scheduled = L.packed_scheduled ? 1 : 0;
    li.passB_reg_cells = L.passB_rc8 ? 8 : kRegCells;
    li.rows_over_8 = L.rows_over8;
    std::vector<uint32_t> off((size_t)L.nslices + 1);
    MSW_HIP(hipMemcpy(off.data(), L.slice_off.p, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    li.rows = off[L.nslices];
    for (int c = 0; c < kSliceClasses; ++c) li.slices_by_lanes[c] = L.cls.s0[c + 1] - L.cls.s0[c];
    for (uint32_t s2 = 0; s2 < L.nslices; ++s2) li.max_rows = std::max(li.max_rows, off[s2 + 1] - off[s2]);
    if (L.hybrid()) {
      std::vector<uint8_t> hot(std::max<uint32_t>(L.nslices, 1));
      MSW_HIP(hipMemcpy(hot.data(), L.slice_hot.p, hot.size(), hipMemcpyDeviceToHost));
      for (uint32_t s2 = 0; s2 < L.nslices; ++s2) li.rows_from_memory += (off[s2 + 1] - off[s2]) - hot[s2];
    } else if (!L.tlds && L.enc != kEncValue) {
      li.rows_from_memory = li.rows;
    }
    *out = li;
  });
}

int msw_core_layout_hash(msw_handle h, uint64_t *hash_out) {
  return guarded(h, [&] {
    if (!hash_out) throw Fail("null out");
    *hash_out = layout_hash(h->lik);
  });
}

int msw_core_get_dense_logl(msw_handle h, double *L_out, size_t ld) {
  return guarded(h, [&] { materialise_impl(h, L_out, ld, /*gamma=*/false, 0, h->lik.E); });
}

int msw_core_gamma(msw_handle h, double *gamma_out, size_t ld) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_gamma: no solve has run on this handle");
    materialise_impl(h, gamma_out, ld, /*gamma=*/true, 0, h->lik.E);
  });
}

int msw_core_gamma_block(msw_handle h, size_t ec_begin, size_t ec_end, double *gamma_out, size_t ld) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_gamma_block: no solve has run on this handle");
    materialise_impl(h, gamma_out, ld, /*gamma=*/true, ec_begin, ec_end);
  });
}

int msw_core_text_block(msw_handle h, int what, size_t ec_begin, size_t ec_end, const uint64_t *line_prefix,
                        size_t n_zero_cols, const char **text_out, size_t *len_out, size_t *n_host_cells_out) {
  return guarded(h, [&] { text_block_impl(h, what, ec_begin, ec_end, line_prefix, n_zero_cols, text_out, len_out, n_host_cells_out); });
}

int msw_core_format_g6(msw_handle h, const double *x, size_t n, const char **text_out, size_t *len_out, size_t *n_host_out) {
  return guarded(h, [&] { format_g6_impl(h, x, n, text_out, len_out, n_host_out); });
}

// ---- gzip input inflated on the device: the test and diagnostic entry, and the report of the last read --------------------
int msw_core_inflate_gzip(msw_handle h, const uint8_t *gz, size_t n, size_t chunk_bytes, const uint8_t **text_out, size_t *len_out,
                          msw_inflate_info *info) {
  return guarded(h, [&] { inflate_gzip_impl(h, gz, n, chunk_bytes, text_out, len_out, info); });
}

int msw_alignment_last_inflate(msw_handle h, msw_inflate_info *info, size_t max_files, size_t *n_files) {
  return guarded(h, [&] { last_inflate_impl(h, info, max_files, n_files); });
}

// ---- --compress z (src/OutfileDesignator.cpp:30-37) -----------------------------------------------------------------------
int msw_core_gzip_begin(msw_handle h, int level, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_begin_impl(h, level, out, len_out); });
}

int msw_core_text_block_gzip(msw_handle h, int what, size_t ec_begin, size_t ec_end, const uint64_t *line_prefix, size_t n_zero_cols,
                             const char **out, size_t *len_out, size_t *n_host_cells_out, size_t *text_len_out) {
  return guarded(h, [&] { text_block_gzip_impl(h, what, ec_begin, ec_end, line_prefix, n_zero_cols, out, len_out, n_host_cells_out, text_len_out); });
}

int msw_core_gzip_append(msw_handle h, const char *bytes, size_t n, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_append_impl(h, bytes, n, out, len_out); });
}

int msw_core_gzip_end(msw_handle h, const char **out, size_t *len_out) {
  return guarded(h, [&] { gzip_end_impl(h, out, len_out); });
}

int msw_core_last_gzip_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_in_out, uint64_t *bytes_out_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->gz.kernel_ms;
    if (bytes_in_out) *bytes_in_out = h->gz.isize;
    if (bytes_out_out) *bytes_out_out = h->gz.bytes_out;
  });
}

// ---- --extract-reads: the records of a FASTQ file by read id (host_fastq.inc) ------------------------------------------------
int msw_fastq_open(msw_handle h, const char *path, msw_fastq_t *out, msw_fastq_info *info) {
  return guarded(h, [&] { fastq_open_impl(h, path, out, info); });
}

int msw_fastq_select(msw_handle h, msw_fastq_t fq, const uint32_t *ids, size_t n, uint64_t *n_selected_out, uint64_t *bytes_out) {
  return guarded(h, [&] { fastq_select_impl(h, fq, ids, n, n_selected_out, bytes_out); });
}

int msw_fastq_next(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out) {
  return guarded(h, [&] { fastq_next_impl(h, fq, max_bytes, false, out, len_out, nullptr); });
}

int msw_fastq_next_gzip(msw_handle h, msw_fastq_t fq, size_t max_bytes, const char **out, size_t *len_out, size_t *text_len_out) {
  return guarded(h, [&] { fastq_next_impl(h, fq, max_bytes, true, out, len_out, text_len_out); });
}

int msw_fastq_last_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->fastq.kernel_ms;
    if (bytes_out) *bytes_out = h->fastq.bytes;
  });
}

void msw_fastq_close(msw_fastq_t fq) { fastq_close_impl(fq); }

int msw_core_last_text_timing(msw_handle h, double *kernel_ms_out, uint64_t *bytes_out) {
  return guarded(h, [&] {
    if (kernel_ms_out) *kernel_ms_out = h->text.kernel_ms;
    if (bytes_out) *bytes_out = h->text.bytes;
  });
}

int msw_core_bin_reads(msw_handle h, const uint64_t *ec_rptr, const uint32_t *ec_reads, size_t n_ecs,
                       const uint32_t *targets, const double *thresholds, size_t n_targets, uint64_t *bin_ptr,
                       uint32_t *reads_out, double *log_thr_out) {
  return guarded(h, [&] {
    bin_reads_impl(h, ec_rptr, ec_reads, n_ecs, false, targets, thresholds, n_targets, bin_ptr, reads_out, log_thr_out);
  });
}

int msw_core_bin_reads_aln(msw_handle h, msw_alignment_t a, const uint32_t *targets, const double *thresholds,
                           size_t n_targets, uint64_t *bin_ptr, uint32_t *reads_out, double *log_thr_out) {
  return guarded(h, [&] {
    if (!a) throw Fail("msw_core_bin_reads_aln: null alignment");
    if (a->on_device && a->device == h->device) {
      // the reader's classes are read where they lie
      bin_reads_impl(h, a->d_rptr.p, a->d_reads.p, a->E, true, targets, thresholds, n_targets, bin_ptr, reads_out,
                     log_thr_out);
    } else {
      a->to_host(msw_alignment::kAlnRptr | msw_alignment::kAlnReads);
      bin_reads_impl(h, a->ec_rptr.data(), a->ec_reads.data(), a->ec_rptr.empty() ? 0 : a->ec_rptr.size() - 1, false,
                     targets, thresholds, n_targets, bin_ptr, reads_out, log_thr_out);
    }
  });
}

int msw_core_solve(msw_handle h, const double *logc, const double *alpha0, double tol, size_t max_iters,
                   int algo, int prec, double *theta_out, size_t *iters_out, double *bound_out) {
  return guarded(h, [&] {
    if (!alpha0) throw Fail("msw_core_solve: null alpha0");
    prepare_inputs(h->lik, h->solver, logc, nullptr, alpha0);
    run_impl(h->lik, h->solver, tol, max_iters, algo, prec, theta_out, iters_out, bound_out);
  });
}

int msw_core_prepare(msw_handle h, const double *logc, const double *alpha0) {
  return guarded(h, [&] {
    if (!alpha0) throw Fail("msw_core_prepare: null alpha0");
    prepare_inputs(h->lik, h->solver, logc, nullptr, alpha0);
  });
}

int msw_core_run(msw_handle h, double tol, size_t max_iters, int algo, int prec, double *theta_out,
                 size_t *iters_out, double *bound_out) {
  return guarded(h, [&] { run_impl(h->lik, h->solver, tol, max_iters, algo, prec, theta_out, iters_out, bound_out); });
}

int msw_core_continue(msw_handle h, size_t n_iters, double *theta_out, size_t *iters_out, double *bound_out) {
  return guarded(h, [&] { continue_impl(h->lik, h->solver, n_iters, theta_out, iters_out, bound_out); });
}

int msw_core_set_trace_theta(msw_handle h, size_t n_iters) {
  return guarded(h, [&] {
    if (n_iters > (size_t)kMaxTrace) throw Fail("trace_theta: at most 4096 iterations");
    h->solver.trace_theta = n_iters;
  });
}

int msw_core_trace(msw_handle h, size_t n, double *bound, double *newnorm, double *beta,
                   int32_t *didreset, double *theta_trace, size_t *n_out) {
  return guarded(h, [&] {
    if (!h->solver.have_solution) throw Fail("msw_core_trace: no solve has run on this handle");
    size_t have = std::min<size_t>((size_t)h->solver.sc_host->iter, kMaxTrace);
    n = std::min(n, have);
    if (bound) MSW_HIP(hipMemcpy(bound, h->solver.tr_bound.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (newnorm) MSW_HIP(hipMemcpy(newnorm, h->solver.tr_newnorm.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (beta) MSW_HIP(hipMemcpy(beta, h->solver.tr_beta.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (didreset) MSW_HIP(hipMemcpy(didreset, h->solver.tr_reset.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (theta_trace) {
      const size_t nt = std::min(n, h->solver.trace_theta);
      if (nt) MSW_HIP(hipMemcpy(theta_trace, h->solver.tr_theta.p, nt * h->lik.G * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (n_out) *n_out = n;
  });
}

int msw_core_bootstrap(msw_handle h, const uint32_t *ec_counts, int32_t seed, size_t bootstrap_count,
                       size_t rep_begin, size_t rep_end, const double *alpha0, double tol,
                       size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out) {
  return guarded(h, [&] {
    bootstrap_impl(h, ec_counts, seed, bootstrap_count, rep_begin, rep_end, alpha0, tol, max_iters,
                   algo, prec, theta_out, iters_out);
  });
}

int msw_core_resample_counts(msw_handle h, const uint32_t *ec_counts, size_t n_ecs, int32_t seed,
                             size_t bootstrap_count, size_t rep_begin, size_t rep_end,
                             uint32_t *counts_out) {
  return guarded(h, [&] {
    resample_impl(h, ec_counts, n_ecs, seed, bootstrap_count, rep_begin, rep_end, counts_out);
  });
}

int msw_core_bootstrap_dist(msw_handle h, msw_comm_t comm, const uint32_t *ec_counts, int32_t seed,
                            size_t bootstrap_count, size_t n_replicates, const double *alpha0, double tol,
                            size_t max_iters, int algo, int prec, double *theta_out, size_t *iters_out) {
  // (a rank whose block fails still joins the all-gather and reports through its status word: every rank
  // returns non-zero, none is left waiting, and the communicator stays usable -- host_bootstrap.inc)
  return guarded(h, [&] {
    bootstrap_dist_impl(h, comm, ec_counts, seed, bootstrap_count, n_replicates, alpha0, tol, max_iters, algo,
                        prec, theta_out, iters_out);
  });
}

const char *msw_comm_last_error(void) { return g_create_error.c_str(); }

int msw_comm_size(msw_comm_t c, int *nranks, int *rank) {
  if (!c) {
    g_create_error = "msw_comm_size: null communicator";
    return 1;
  }
  if (nranks) *nranks = c->size();
  if (rank) *rank = c->rank();
  return 0;
}

int msw_comm_rccl_count(msw_comm_t c, int *count) {
  if (!c || !count) {
    g_create_error = "msw_comm_rccl_count: null argument";
    return 1;
  }
  if (const PeerComm *pc = dynamic_cast<const PeerComm *>(c)) c = pc->base.get();
  const RcclComm *rc = dynamic_cast<const RcclComm *>(c);
  *count = rc ? rc->count() : 0;
  return 0;
}

int msw_comm_allgather(msw_comm_t c, const double *send, size_t n, double *recv) {
  if (!c || (n && (!send || !recv))) {
    g_create_error = "msw_comm_allgather: null argument";
    return 1;
  }
  try {
    c->allgather_host(send, n, recv);
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    c->abort();
    return 1;
  }
}

int msw_comm_allreduce(msw_comm_t c, uint64_t *ints, size_t ni, double *reals, size_t nr, int repeats, double *ms_per_call) {
  if (!c || (ni && !ints) || (nr && !reals) || repeats < 1) {
    g_create_error = "msw_comm_allreduce: bad arguments";
    return 1;
  }
  hipStream_t st = nullptr;
  try {
    MSW_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf<double> buf, work;
    buf.alloc(ni + nr + 1);
    work.alloc(ni + nr + 1);
    if (ni) MSW_HIP(hipMemcpyAsync(buf.p, ints, ni * 8, hipMemcpyHostToDevice, st));
    if (nr) MSW_HIP(hipMemcpyAsync(buf.p + ni, reals, nr * 8, hipMemcpyHostToDevice, st));
    // repeats > 1: the same message again and again (timing; the sums of the last one are returned)
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < repeats; ++k) {
      MSW_HIP(hipMemcpyAsync(work.p, buf.p, (ni + nr) * 8, hipMemcpyDeviceToDevice, st));
      c->allreduce_mixed(reinterpret_cast<uint64_t *>(work.p), ni, work.p + ni, nr, st);
    }
    MSW_HIP(hipStreamSynchronize(st));
    c->check();
    if (ms_per_call)
      *ms_per_call = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
    if (ni) MSW_HIP(hipMemcpyAsync(ints, work.p, ni * 8, hipMemcpyDeviceToHost, st));
    if (nr) MSW_HIP(hipMemcpyAsync(reals, work.p + ni, nr * 8, hipMemcpyDeviceToHost, st));
    MSW_HIP(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st);
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    (void)hipGetLastError();
    if (st) (void)hipStreamDestroy(st);
    c->abort();
    return 1;
  }
}

int msw_comm_unique_id(unsigned char id_out[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  const ncclResult_t rc = ncclGetUniqueId(&id);
  if (rc != ncclSuccess) {
    g_create_error = std::string("ncclGetUniqueId: ") + ncclGetErrorString(rc);
    return 1;
  }
  std::memcpy(id_out, &id, 128);
  return 0;
}

int msw_comm_create_rccl(const unsigned char id[128], int rank, int nranks, int device, msw_comm_t *out) {
  if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) {
    g_create_error = "msw_comm_create_rccl: bad arguments";
    return 1;
  }
  try {
    MSW_HIP(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    std::unique_ptr<msw_comm> c(new RcclComm(uid, rank, nranks));
    if (peer_allreduce_requested() && nranks > 1) c.reset(new PeerComm(std::move(c), /*ipc=*/true));
    *out = c.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    return 1;
  }
}

int msw_comm_create_local(int nranks, msw_comm_t *out) {
  if (!out || nranks < 1) {
    g_create_error = "msw_comm_create_local: bad arguments";
    return 1;
  }
  try {
    const bool peer = peer_allreduce_requested() && nranks > 1;
    auto grp = std::make_shared<LocalGroup>(nranks);
    for (int r = 0; r < nranks; ++r) out[r] = nullptr;
    for (int r = 0; r < nranks; ++r) {
      std::unique_ptr<msw_comm> c(new LocalComm(grp, r));
      if (peer) c.reset(new PeerComm(std::move(c), /*ipc=*/false));
      out[r] = c.release();
    }
    return 0;
  } catch (const std::exception &ex) {
    for (int r = 0; r < nranks; ++r) delete out[r];
    g_create_error = ex.what();
    return 1;
  }
}

int msw_comm_create_shm(const char *name, int rank, int nranks, int device, msw_comm_t *out) {
  if (!out || !name || nranks < 1 || rank < 0 || rank >= nranks) {
    g_create_error = "msw_comm_create_shm: bad arguments";
    return 1;
  }
  try {
    MSW_HIP(hipSetDevice(device));
    std::unique_ptr<msw_comm> c(new ShmComm(name, rank, nranks));
    if (peer_allreduce_requested() && nranks > 1) c.reset(new PeerComm(std::move(c), /*ipc=*/true));
    *out = c.release();
    return 0;
  } catch (const std::exception &ex) {
    g_create_error = ex.what();
    return 1;
  }
}

void msw_comm_destroy(msw_comm_t c) { delete c; }

int msw_core_set_comm(msw_handle h, msw_comm_t comm) {
  return guarded(h, [&] { h->comm = comm; });
}

int msw_core_set_profiling(msw_handle h, int enabled) {
  return guarded(h, [&] { h->solver.profiling = enabled != 0; });
}
int msw_core_set_fixed_iters(msw_handle h, int enabled) {
  return guarded(h, [&] { h->solver.fixed_iters = enabled != 0; });
}
int msw_core_set_pack_schedule(msw_handle h, int enabled) {
  return guarded(h, [&] { h->pack_schedule = enabled != 0; });
}
int msw_core_set_option(msw_handle h, int option, double value) {
  return guarded(h, [&] {
    switch (option) {
      case MSW_OPT_CHECK_EVERY:
        if (!(value >= 1.0 && value <= 65536.0) || value != std::floor(value)) throw Fail("MSW_OPT_CHECK_EVERY: an integer in [1, 65536]");
        h->solver.opts.check_every = (int32_t)value;
        break;
      case MSW_OPT_INIT_BOUND:
        if (std::isnan(value) || value == INFINITY) throw Fail("MSW_OPT_INIT_BOUND: a number below +inf");
        h->solver.opts.init_bound = value;
        break;
      case MSW_OPT_EM_PRIOR:
        if (value != 0.0 && value != 1.0) throw Fail("MSW_OPT_EM_PRIOR: 0 (MAP) or 1 (ML)");
        h->solver.opts.em_prior = (int32_t)value;
        break;
      case MSW_OPT_EM_STOP:
        if (value != 0.0 && value != 1.0) throw Fail("MSW_OPT_EM_STOP: 0 (log-likelihood gain) or 1 (largest move of a weight)");
        h->solver.opts.em_stop = (int32_t)value;
        break;
      default: throw Fail("msw_core_set_option: unknown option id");
    }
  });
}
int msw_core_get_option(msw_handle h, int option, double *value) {
  return guarded(h, [&] {
    if (!value) throw Fail("null out");
    switch (option) {
      case MSW_OPT_CHECK_EVERY: *value = h->solver.opts.check_every; break;
      case MSW_OPT_INIT_BOUND: *value = h->solver.opts.init_bound; break;
      case MSW_OPT_EM_PRIOR: *value = h->solver.opts.em_prior; break;
      case MSW_OPT_EM_STOP: *value = h->solver.opts.em_stop; break;
      default: throw Fail("msw_core_get_option: unknown option id");
    }
  });
}
int msw_core_last_timing(msw_handle h, msw_timing *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    *out = h->solver.timing;
  });
}

#ifdef MSW_STAMPS
// diagnostic build only (tools/chain_timeline.py): the phase stamps of the last <= 64 iterations; clear = 1 zeroes them
int msw_debug_stamps(msw_handle h, uint64_t *out, int clear) {
  return guarded(h, [&] {
    MSW_HIP(hipStreamSynchronize(h->stream));
    if (out) MSW_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 64 * 40));
    if (clear) {
      std::vector<unsigned long long> z(64 * 40, 0);
      MSW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z.data(), z.size() * sizeof(unsigned long long)));
    }
  });
}
#endif

int msw_core_guarded_visits(msw_handle h, uint64_t *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    if (h->lik.flavor != 0) throw Fail("msw_core_guarded_visits: no CSR-of-ECs likelihood resident");
    unsigned long long v = 0;
    MSW_HIP(hipStreamSynchronize(h->stream));
    MSW_HIP(hipMemcpy(&v, h->solver.guard_visits.p, sizeof v, hipMemcpyDeviceToHost));
    *out = v;
  });
}

int msw_core_last_bootstrap_timing(msw_handle h, msw_bootstrap_timing *out) {
  return guarded(h, [&] {
    if (!out) throw Fail("null out");
    *out = h->btiming;
  });
}

int msw_core_hbm_stream_rates(msw_handle h, size_t n_bytes, int reps, double *read_gbs, double *triad_gbs) {
  return guarded(h, [&] {
    if (!read_gbs || !triad_gbs) throw Fail("null out");
    if (n_bytes < (1u << 20) || reps < 1) throw Fail("msw_core_hbm_stream_rates: at least 1 MiB and one repetition");
    const size_t n = n_bytes / sizeof(double2);
    DevBuf<double2> a, b, c;
    DevBuf<double> sink;
    a.alloc(n);
    b.alloc(n);
    c.alloc(n);
    sink.alloc(1);
    MSW_HIP(hipMemsetAsync(a.p, 0, n * sizeof(double2), h->stream));
    MSW_HIP(hipMemsetAsync(b.p, 0, n * sizeof(double2), h->stream));
    MSW_HIP(hipMemsetAsync(c.p, 0, n * sizeof(double2), h->stream));
    hipEvent_t e0, e1;
    MSW_HIP(hipEventCreate(&e0));
    MSW_HIP(hipEventCreate(&e1));
    // the rate depends on the launch shape by +-10 %: the best of a few shapes is the ceiling
    const int shapes[7][2] = {{256, 512}, {256, 1024}, {512, 256}, {512, 1024}, {1024, 512}, {2048, 1024}, {8192, 1024}};
    double best_r = 0.0, best_t = 0.0;
    for (int r = 0; r < reps + 2; ++r) {  // the first two rounds warm the clocks and the TLB
      for (const auto &sh : shapes) {
        float ms = 0.f;
        MSW_HIP(hipEventRecord(e0, h->stream));
        k_stream_read<<<sh[0], sh[1], 0, h->stream>>>(a.p, n, sink.p);
        MSW_HIP(hipEventRecord(e1, h->stream));
        MSW_HIP(hipEventSynchronize(e1));
        MSW_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) best_r = std::max(best_r, (double)(n * sizeof(double2)) / (ms * 1e-3) / 1e9);
        MSW_HIP(hipEventRecord(e0, h->stream));
        k_stream_triad<<<sh[0], sh[1], 0, h->stream>>>(a.p, b.p, c.p, n);
        MSW_HIP(hipEventRecord(e1, h->stream));
        MSW_HIP(hipEventSynchronize(e1));
        MSW_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 2) best_t = std::max(best_t, (double)(3 * n * sizeof(double2)) / (ms * 1e-3) / 1e9);
      }
    }
    MSW_HIP(hipGetLastError());
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *read_gbs = best_r;
    *triad_gbs = best_t;
  });
}

}  // extern "C"
