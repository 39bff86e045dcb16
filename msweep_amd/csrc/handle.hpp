// handle.hpp -- the handle of libmsweep_core.so and its parts, for every translation unit of the library:
// the structures below, the failure types, guarded() and the views of the handle the kernels take.  No kernel is
// defined here or in anything this header includes.
#pragma once
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

#include "common.hpp"
#include "device_util.hpp"
#include "guard.hpp"
#include "sell.hpp"
#include "comm.hpp"
#include "text_cells.hpp"
#include "reader_host.hpp"

namespace msw {
struct GzChunk;  // deflate_kernels.hpp
struct MtState;  // bootstrap_kernels.hpp
}  // namespace msw

using namespace msw;

namespace {
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
  // guarded ECs (guard.hpp), CSR flavour: room in a workgroup's list for every EC it can see (its wavefronts take
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
  // guarded ECs (guard.hpp): per-workgroup lists, per-wavefront bitmaps, error flag
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

// ---- what msw_core_assign_reads keeps for msw_core_assign_table_* (host_assign.inc): MSW_ASSIGN_KEEP_TABLE.  Dropped by
// a new likelihood, a solve, a bootstrap or an assign call without the flag ----------------------------------------------
struct AssignState {
  bool have = false;
  uint32_t n_targets = 0;
  size_t n_rows = 0;         // aligned reads: the table's rows
  DevBuf<uint64_t> off;      // [E + 1] the ECs' (target slot, EC) pairs as the write pass left them: a CSR by EC
  DevBuf<uint32_t> key;      // ... their target slots
  DevBuf<uint32_t> id, ec;   // [n_rows] read id and EC of every row, ascending id (stable)
  DevBuf<uint32_t> len;      // a block's text: row lengths, offsets, bytes, scan scratch
  DevBuf<uint64_t> toff;
  DevBuf<uint8_t> text, tmp;
  void drop() {
    have = false;
    off.release(); key.release(); id.release(); ec.release(); len.release(); toff.release(); text.release(); tmp.release();
  }
};

// ---- what msw_core_sparse_probs_begin keeps for msw_core_sparse_probs_next* (host_sparse_probs.inc).  Dropped by a new
// likelihood, a solve, a bootstrap and msw_core_trim ----------------------------------------------------------------------
struct SparseProbsState {
  bool have = false;
  uint64_t n_rows = 0, cur = 0;  // rows (ECs, or aligned reads); the next row to hand out
  double log_thr = 0.0, a = 1.0, tref = 0.0;
  const double *u = nullptr;     // the solver's u (a solve drops this state)
  DevBuf<uint32_t> order;        // [G] the groups by u descending ...
  DevBuf<double> us, lse_p;      // ... their u; [E] the normaliser at every permuted position
  DevBuf<uint32_t> id, ec;       // by read: [n_rows] read id and EC of every row, ascending id (stable); by EC: none
  DevBuf<uint64_t> coff, koff;   // [n_rows + 1] exclusive scans of the rows' candidates and kept cells
  // a piece: candidates as written and sorted, their gamma, line lengths and offsets, the text
  DevBuf<uint64_t> key, key2, eoff, pbits, span;
  DevBuf<uint32_t> idx, idx2, elen, n_list;
  DevBuf<double> gam;
  DevBuf<uint8_t> text, closed, tmp;
  DevBuf<TextHostCell> list;
  DevBuf<TextFilledCell> cells;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double kernel_ms = 0.0;  // since begin (msw_core_last_sparse_probs_timing)
  uint64_t bytes = 0, n_cells = 0;
  void drop() {
    have = false;
    u = nullptr;
    order.release(); us.release(); lse_p.release(); id.release(); ec.release(); coff.release(); koff.release();
    key.release(); key2.release(); eoff.release(); pbits.release(); span.release(); idx.release(); idx2.release();
    elen.release(); n_list.release(); gam.release(); text.release(); closed.release(); tmp.release(); list.release();
    cells.release();
  }
  ~SparseProbsState() {
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
  AssignState assign;
  SparseProbsState sparse;
  // what an earlier call kept of the solve before (host_assign.inc, host_sparse_probs.inc)
  void drop_kept() { assign.drop(); sparse.drop(); }
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

// vectors whose resize() leaves new elements uninitialised: the large arrays of the reader are written in full by the
// worker threads right after they are sized -- a zero fill by the sizing thread would be one more serial pass over
// (and first touch of) hundreds of megabytes
template <class T>
struct uninit_alloc : std::allocator<T> {
  template <class U> struct rebind { using other = uninit_alloc<U>; };
  uninit_alloc() = default;
  template <class U> uninit_alloc(const uninit_alloc<U> &) {}
  template <class U> void construct(U *p) noexcept { ::new (static_cast<void *>(p)) U; }
  template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
template <class T> using uvec = std::vector<T, uninit_alloc<T>>;

struct msw_alignment {
  size_t n_targets = 0, n_queries = 0;
  std::vector<uint64_t> ec_tptr, ec_counts, ec_rptr;
  uvec<uint32_t> ec_targets, ec_reads;
  // msw_alignment_read_device (host_reader.inc): the same five arrays in device memory; the host vectors above are
  // filled from them by the first accessor that needs them (to_host)
  bool on_device = false;
  unsigned host_have = 31u;    // which of the five host vectors are filled (bit k: kAln* below); the host reader: all
  int device = 0;
  size_t E = 0, H = 0, K = 0;  // classes, their target hits, aligned reads
  DevBuf<uint64_t> d_tptr, d_counts, d_rptr;
  DevBuf<uint32_t> d_targets, d_reads;
  enum : unsigned { kAlnTptr = 1u, kAlnTargets = 2u, kAlnCounts = 4u, kAlnRptr = 8u, kAlnReads = 16u };
  void to_host(unsigned want) {
    const unsigned need = want & ~host_have;
    if (!need) return;
    MSW_HIP(hipSetDevice(device));
    auto fetch = [&](unsigned bit, auto &vec, const auto *src, size_t n) {
      if (!(need & bit)) return;
      vec.resize(n);
      if (n) MSW_HIP(hipMemcpy(vec.data(), src, n * sizeof(*src), hipMemcpyDeviceToHost));
    };
    fetch(kAlnTptr, ec_tptr, d_tptr.p, E + 1);
    fetch(kAlnTargets, ec_targets, d_targets.p, H);
    fetch(kAlnCounts, ec_counts, d_counts.p, E);
    fetch(kAlnRptr, ec_rptr, d_rptr.p, E + 1);
    fetch(kAlnReads, ec_reads, d_reads.p, K);
    host_have |= need;
  }
};

// one type each for the whole library (not one per translation unit: a handler in one unit catches what a function of
// another throws), hidden like everything else that crosses units (host_api.hpp)
namespace msw {
namespace host __attribute__((visibility("hidden"))) {
struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};
// a solve that failed NUMERICALLY (likelihood underflow, non-finite bound: where the reference returns NaN weights).
// The bootstrap driver turns exactly these into a row of NaN; every other failure fails the call.
struct NumericFail : Fail {
  using Fail::Fail;
};
}  // namespace host
}  // namespace msw
using msw::host::Fail;
using msw::host::NumericFail;

namespace {

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

// (a, tref, u) of gamma after the last solve (host_likelihood.inc gamma_state): what k_gamma_block and the bin pass read
struct GammaState {
  double a, tref;
  const double *u;
};
// what a block of gamma (or of the likelihood itself: a = 1, u = 0) is computed from
struct MaterialiseArgs {
  double a = 1.0, tref = 0.0;
  const double *u = nullptr;
  DevBuf<double> zero_u;
};
