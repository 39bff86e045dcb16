// host_likelihood.inc -- likelihood upload / build / materialisation (included by
// build.hip).  Host code here only validates, lays out and launches.
namespace {

void sell_from_device(msw_core *h, const uint32_t *d_rowptr, const uint32_t *d_grp, const uint32_t *d_idx,
                      const double *cell_val = nullptr);
bool compress_dense(msw_core *h, const double *Lm, size_t ld, const double *stage, size_t G, size_t E, bool force);

}  // namespace

// a build starts from an empty shape and layout; the device buffers stay and only grow (DevBuf::alloc)
void msw::host::reset_likelihood(msw_core *h) {
  Resident &L = h->lik;
  static_cast<LikShape &>(L) = LikShape{};
  h->solver.have_solution = false;
  h->solver.prepared = false;
  h->iperm.release();
  h->drop_kept();
  L.long_row = multilane() ? kLongRow : kLongRowOneLane;
  if (const char *lr = getenv("MSWEEP_LONG_ROW"))  // developer switch
    L.long_row = (uint32_t)std::min(std::max(atoi(lr), 16), (int)L.long_row);
}

namespace {

// lane -> ds_read_b128 service group (MI355X_MICROARCH.md LDS table): {0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same pattern in the upper half
constexpr uint8_t kRGroup[64] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0,
                                 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3,
                                 2, 2, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3};

// lane -> its position (0..15) inside its ds_read_b128 service group
constexpr uint8_t kRPos[64] = {0, 1, 2,  3,  0,  1,  2,  3,  4,  5,  6,  7,  4,  5,  6,  7,  8,  9,  10, 11, 8, 9,
                               10, 11, 12, 13, 14, 15, 12, 13, 14, 15, 0,  1,  2,  3,  0,  1,  2,  3,  4,  5, 6, 7,
                               4,  5,  6,  7,  8,  9,  10, 11, 8,  9,  10, 11, 12, 13, 14, 15, 12, 13, 14, 15};

// ---- slot area (sell.hpp): the LUT slots some cell refers to, compacted in slot order, then --
// room in LDS and in the 32-bit records permitting -- 8 replicas of the H hottest slots.  Replica
// c keeps its entries in bank quads {2c, 2c+1} only and serves the two lanes at positions 2c,
// 2c+1 of each ds_read_b128 lane group, so the slot gathers of different lane pairs can never
// meet on a bank (un-replicated, the few dozen slots nearly every cell uses cost 3-4 LDS cycles
// per 16 lanes instead of 1).  Decides the LDS mode and the record encoding on the way
// (choose_layout) and uploads the entry -> slot map.
struct SlotPlan {
  std::vector<uint32_t> canon, hot_rank;  // [n_lut]: entry in the compact part / rank among the replicated
  uint32_t rep_base = 0, H = 0, sentinel_slot = 0;
};
SlotPlan plan_slot_area(msw_core *h, const std::vector<uint64_t> &freq) {
  Resident &L = h->lik;
  const uint32_t n_lut = L.n_lut;
  SlotPlan sp;
  std::vector<uint32_t> used;  // referenced slots, ascending
  for (uint32_t i = 0; i < n_lut; ++i) if (freq[i]) used.push_back(i);
  if (used.empty()) used.push_back(0);
  std::vector<uint32_t> by_freq(used);
  std::stable_sort(by_freq.begin(), by_freq.end(), [&](uint32_t a, uint32_t b) { return freq[a] > freq[b]; });
  sp.canon.assign(std::max<uint32_t>(n_lut, 1), 0);
  sp.hot_rank.assign(std::max<uint32_t>(n_lut, 1), UINT32_MAX);
  sp.sentinel_slot = used[0];
  for (uint32_t tryH : {64u, 32u, 16u, 8u, 0u}) {
    if (tryH > used.size()) continue;
    sp.H = tryH;
    sp.rep_base = sp.H ? (uint32_t)((used.size() + 15) & ~(size_t)15) : (uint32_t)used.size();
    L.n_area = sp.rep_base + 8 * sp.H;
    choose_layout(L);
    if (L.tlds && L.glds && !L.wide()) break;
  }
  bool hybrid = false;
  if (!L.tlds) {  // the per-slot tables stay in global memory: the used slots, no replicas
    sp.H = 0;
    sp.rep_base = (uint32_t)used.size();
    L.n_area = (uint32_t)used.size();
    choose_layout(L);
    // ... ordered by use, the head of them in LDS as well, 4-byte index records (sell.hpp) when that applies
    hybrid = choose_hybrid_layout(L, h->no_hybrid);
    if (hybrid) sp.sentinel_slot = by_freq[0];  // padding sits in hot segments too: an LDS-resident entry
  }
  const std::vector<uint32_t> &order = hybrid ? by_freq : used;
  std::vector<uint32_t> area_slot(L.n_area, used[0]);
  for (uint32_t e = 0; e < order.size(); ++e) area_slot[e] = order[e], sp.canon[order[e]] = e;
  for (uint32_t j = 0; j < sp.H; ++j) {
    sp.hot_rank[by_freq[j]] = j;
    for (uint32_t c = 0; c < 8; ++c) area_slot[sp.rep_base + (j >> 1) * 16 + 2 * c + (j & 1)] = by_freq[j];
  }
  L.area_slot.upload(area_slot.data(), area_slot.size(), h->stream);
  // the table values in area order: what k_step / k_tables rebuild the per-slot tables from
  L.lut_area.alloc(L.n_area);
  hipLaunchKernelGGL(k_gather_f64, dim3((L.n_area + 255) / 256), dim3(256), 0, h->stream, L.lut.p, L.area_slot.p,
                     L.n_area, L.lut_area.p);
  L.trange.alloc(2);
  minmax_launch(1, h->stream, L.lut_area.p, (uint64_t)L.n_area, 0, L.trange.p);  // (k_minmax: solve.hip)
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(h->stream));  // area_slot dies at return
  return sp;
}

// what both packers do once the records are in place
void finish_sell(msw_core *h) {
  Resident &L = h->lik;
  const uint32_t wg_for_slices = (L.nslices + (kPassThreads / 64) - 1) / (kPassThreads / 64);
  L.nblk = (int)std::max<uint32_t>(1, std::min<uint32_t>(std::max(wg_for_slices, L.n_long), (uint32_t)h->n_cu));
  L.nblk_dense = 0;
  L.flavor = 0;
  L.packed_scheduled = h->pack_schedule;
  // Which instantiation of pass B sweeps this layout (sweep_kernels.hpp, RC): the short-slice one -- 8 records per lane in
  // registers, 16 wavefronts per workgroup -- when the slices of more than 8 rows, which it walks in two chunks with a
  // second gather per cell, hold at most a twentieth of the rows (plain offset records, one lane per EC).
  // MSWEEP_PASSB_RC=8 | 16 (developer switch) forces either.
  L.rows_over8 = 0;
  L.passB_rc8 = false;
  if (L.nslices && L.enc == kEncNarrow && L.cls.s0[kSliceClasses - 1] == 0) {
    DevBuf<unsigned long long> d_over;
    d_over.alloc(1);
    d_over.zero(h->stream);
    hipLaunchKernelGGL(k_rows_over, dim3(std::min<uint32_t>((L.nslices + 255) / 256, (uint32_t)h->n_cu * 8)), dim3(256), 0,
                       h->stream, L.slice_off.p, L.nslices, 8u, d_over.p);
    unsigned long long over = 0;
    MSW_HIP(hipMemcpyAsync(&over, d_over.p, sizeof over, hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
    L.rows_over8 = over;
    L.passB_rc8 = 20 * over <= L.nslots / 64;
    if (const char *e = getenv("MSWEEP_PASSB_RC")) L.passB_rc8 = atoi(e) == 8;
  }
  alloc_solve_state(L, h->solver);
  MSW_HIP(hipStreamSynchronize(h->stream));
}

// Host packer (MSWEEP_HOST_PACK=1; the reference implementation of the device packer in
// pack_kernels.hpp, which produces the same bytes): CSR-of-ECs (rowptr + per-cell group / LUT
// slot) -> SELL-64 device layout: long ECs first (plain CSR), the rest stably sorted by descending
// cell count, cut into slices of 64 ECs stored column-major and padded with sentinel records.
template <class RP>
void upload_sell(msw_core *h, const RP *rowptr, const uint32_t *cell_grp, const uint32_t *cell_idx) {
  Resident &L = h->lik;
  const uint32_t E = L.E, G = L.G, n_lut = L.n_lut;
  const uint64_t nnz_all = rowptr[E];
  std::vector<uint64_t> freq(std::max<uint32_t>(n_lut, 1), 0);
  for (uint64_t k = 0; k < nnz_all; ++k) ++freq[cell_idx[k]];
  const SlotPlan sp = plan_slot_area(h, freq);
  const std::vector<uint32_t> &canon = sp.canon, &hot_rank = sp.hot_rank;
  const uint32_t rep_base = sp.rep_base;
  const std::vector<uint32_t> used = {sp.sentinel_slot};
  const bool wide = L.wide(), hybrid = L.hybrid();
  const int rw = wide ? 2 : 1;
  const RecDec dec = L.dec;
  const uint32_t n_hot = L.n_tab_lds;
  // entry of the slot area lane `lane` reads for LUT slot idx (lane < 0: any lane -> compact part)
  auto entry_of = [&](int lane, uint32_t idx) -> uint32_t {
    const uint32_t j = hot_rank[idx];
    if (lane < 0 || j == UINT32_MAX) return canon[idx];
    return rep_base + (j >> 1) * 16 + 2 * (kRPos[lane] >> 1) + (j & 1);
  };
  // record = the cell's two table positions as byte offsets (sell.hpp)
  // (hot: a row of an index-record slice's hot segment -- the record form with the entry pre-multiplied by 16, sell.hpp)
  auto put_entry = [&](std::vector<uint32_t> &dst, size_t slot, uint32_t g, uint32_t entry, bool hot = false) {
    if (wide) {
      const uint2 r = Rec<kEncWide>::make(g, entry, dec);
      dst[2 * slot] = r.x;
      dst[2 * slot + 1] = r.y;
    } else if (hybrid) {
      dst[slot] = hot ? Rec<kEncIndex>::make_h(g, entry, dec) : Rec<kEncIndex>::make(g, entry, dec);
    } else {
      dst[slot] = Rec<kEncNarrow>::make(g, entry, dec);
    }
  };
  auto put = [&](std::vector<uint32_t> &dst, size_t slot, uint32_t g, uint32_t idx, int lane, bool hot = false) {
    put_entry(dst, slot, g, entry_of(lane, idx), hot);
  };
  // permutation: long rows in original order, then counting sort by (length descending, cold class ascending:
  // pack_kernels.hpp cold_class -- 0 everywhere without a hybrid area), stable
  std::vector<uint32_t> perm(E);
  std::vector<uint32_t> cnt_len((kLongRow + 2) * 4, 0);
  std::vector<uint8_t> ccls(E, 0);
  uint32_t n_long = 0;
  uint32_t n_class[kSliceClasses] = {};  // ECs per slice class (sell.hpp)
  const bool ml = multilane();
  for (uint32_t j = 0; j < E; ++j) {
    const uint64_t len = rowptr[j + 1] - rowptr[j];
    if (hybrid && len <= 16) {
      uint32_t cc = 0;
      for (uint64_t k = rowptr[j]; k < rowptr[j + 1]; ++k) cc += canon[cell_idx[k]] >= n_hot;
      ccls[j] = (uint8_t)cold_class(cc);
    }
    if (len > (uint64_t)L.long_row) {
      ++n_long;
    } else {
      ++cnt_len[len * 4 + ccls[j]];
      ++n_class[slice_class_of((uint32_t)len, ml)];
    }
  }
  {
    std::vector<uint32_t> start((kLongRow + 2) * 4, 0);
    uint32_t pos = n_long;
    for (int len = kLongRow; len >= 0; --len)
      for (int cl = 0; cl < 4; ++cl) {
        start[len * 4 + cl] = pos;
        pos += cnt_len[len * 4 + cl];
      }
    uint32_t pl = 0;
    for (uint32_t j = 0; j < E; ++j) {
      const uint64_t len = rowptr[j + 1] - rowptr[j];
      if (len > (uint64_t)L.long_row) perm[pl++] = j;
      else perm[start[len * 4 + ccls[j]]++] = j;
    }
  }
  // long rows
  std::vector<uint32_t> long_ptr(n_long + 1, 0);
  for (uint32_t p = 0; p < n_long; ++p)
    long_ptr[p + 1] = long_ptr[p] + (uint32_t)(rowptr[perm[p] + 1] - rowptr[perm[p]]);
  std::vector<uint32_t> rec_long((size_t)long_ptr[n_long] * rw + 2);
  for (uint32_t p = 0; p < n_long; ++p) {  // cells sorted by (rank among the EC's cells of the same group mod 32,
    const uint64_t b = rowptr[perm[p]];    // group mod 32): pack_kernels.hpp k_pack_long
    const uint32_t n = long_ptr[p + 1] - long_ptr[p];
    uint32_t cnt[kLongResidues] = {}, run[kLongResidues] = {};
    for (uint32_t k = 0; k < n; ++k) ++cnt[cell_grp[b + k] & (kLongResidues - 1)];
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t r = cell_grp[b + k] & (kLongResidues - 1);
      put(rec_long, (size_t)long_ptr[p] + long_cell_pos(cnt, r, run[r]++), cell_grp[b + k], cell_idx[b + k], -1);
    }
  }
  // slices
  L.cls = make_slice_classes(n_class);
  const SliceClasses cls = L.cls;
  const bool schedule = h->pack_schedule;
  const uint32_t nslices = cls.s0[kSliceClasses];
  std::vector<uint32_t> slice_off(nslices + 1, 0);
  for (uint32_t s = 0; s < nslices; ++s) {
    const SliceGeo sg = slice_geo(cls, s);
    const uint32_t j0 = perm[n_long + (size_t)sg.ec0];
    const uint64_t len0 = rowptr[j0 + 1] - rowptr[j0];  // the first EC of a slice is its longest
    uint64_t maxlen = (len0 + (1u << sg.lgm) - 1) >> sg.lgm;  // its cells over its 2^lgm lanes
    if (!odd_slices(L.enc)) maxlen += maxlen & 1;   // sell.hpp odd_slices
    const uint64_t nxt = (uint64_t)slice_off[s] + maxlen;
    if (nxt > 0xffffffffull) throw Fail("msw_core_set_csr: likelihood too large for 32-bit slice offsets");
    slice_off[s + 1] = (uint32_t)nxt;
  }
  if (hybrid && slice_off[nslices] >= (1u << kGeoHotShift))
    throw Fail("msw_core_set_csr: likelihood too large for the hybrid slot area's slice geometry");
  const size_t nslots = (size_t)slice_off[nslices] * 64;
  // + one spare row behind the last slice
  std::vector<uint32_t> rec((nslots + 64) * rw + 2);
  std::vector<uint8_t> slice_hot(hybrid ? nslices : 0, 0);  // index records: rows of every slice's hot segment
  // Static LDS-bank scheduling.  The order of the cells inside an EC is free (row sums), and the
  // sweeps' LDS gathers and column-sum atomics -- not their arithmetic -- are what they spend on
  // top of the record stream.  An LDS wave instruction is served in fixed lane groups, one cycle
  // per distinct address on a busy bank within a group (MI355X_MICROARCH.md, LDS):
  //   ds_read_b128 (pass A {e,w}; both passes' slot entries): 4 groups of 16 lanes (kRGroup),
  //       16-byte entries -> bank quad = index mod 16, same address = broadcast;
  //   ds_add_u64 / ds_add_f64 (pass B column sums): 4 contiguous groups of 16 lanes, 32 banks -> bank pair =
  //       group id mod 16, same address does NOT combine;
  //   ds_read_b64 (pass B e_g): two 32-lane halves, 64 banks -> bank pair = group id mod 32.
  // Greedy per slice and step: every lane takes, among its unplaced cells, the one that is free in
  // most of these bank sets (weighted by what a conflict costs), lanes in rotating priority.
  {
    const int nthr = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (int t = 0; t < nthr; ++t) {
      pool.emplace_back([&, t] {
        std::vector<uint64_t> cells;  // (grp << 32 | idx) of the slice, lane-major
        std::vector<uint32_t> centry;  // slot-area entry the owning lane reads for the cell
        std::vector<uint32_t> cbeg(65);
        std::vector<uint8_t> ctaken;
        for (uint32_t s = t; s < nslices; s += nthr) {
          const uint32_t len = slice_off[s + 1] - slice_off[s];
          const size_t base = (size_t)slice_off[s] * 64;
          cells.clear();
          centry.clear();
          // a lane's cells: sub-lane t of the m lanes of its EC takes the EC's cells t, t + m, t + 2 m, ... (sell.hpp)
          const SliceGeo sg = slice_geo(cls, s);
          const uint32_t m = 1u << sg.lgm;
          for (int l = 0; l < 64; ++l) {
            cbeg[l] = (uint32_t)cells.size();
            if (((uint32_t)l >> sg.lgm) < sg.nec) {
              const uint32_t j = perm[n_long + sg.ec0 + ((uint32_t)l >> sg.lgm)];
              for (uint64_t k = rowptr[j] + ((uint32_t)l & (m - 1)); k < rowptr[j + 1]; k += m) {
                cells.push_back(((uint64_t)cell_grp[k] << 32) | cell_idx[k]);
                centry.push_back(entry_of(l, cell_idx[k]));
              }
            }
          }
          cbeg[64] = (uint32_t)cells.size();
          ctaken.assign(cells.size(), 0);
          // A slice of up to 16 rows is one window; a longer one (the streaming path of the sweeps) is scheduled
          // in windows of 16 rows: the cells [k0, k0 + 16) of every EC, in CSR order, go into the rows [k0, k0 + 16).
          const bool streaming = len > 16;
          for (uint32_t k0 = 0; k0 < len; k0 += 16) {
            const uint32_t nrows = std::min<uint32_t>(16, len - k0);
            // the lanes' cells of this window: [wb[l], we[l]) of the slice's cell list
            uint32_t wb[64], we[64];
            for (int l = 0; l < 64; ++l) {
              wb[l] = std::min(cbeg[l] + k0, cbeg[l + 1]);
              we[l] = std::min(wb[l] + 16, cbeg[l + 1]);
            }
            // index records: rows [0, nhot) hold cells of LDS-resident entries only, rows [nhot, len) what is left
            uint32_t nhot = nrows;
            if (hybrid && !streaming) {
              uint32_t mc = 0;
              for (int l = 0; l < 64; ++l) {
                uint32_t cc = 0;
                for (uint32_t c = wb[l]; c < we[l]; ++c) cc += centry[c] >= n_hot;
                mc = std::max(mc, cc);
              }
              nhot = mc > (uint32_t)kColdRows ? 0u : len - mc;
              slice_hot[s] = (uint8_t)nhot;
            }
            for (uint32_t k = 0; k < nhot; ++k) {
              // per lane group: address held by each bank (UINT32_MAX = free)
              uint32_t rg[4][16], rs[4][16], hg[2][32];
              uint16_t at[4] = {0, 0, 0, 0};
              std::memset(rg, 0xff, sizeof rg);
              std::memset(rs, 0xff, sizeof rs);
              std::memset(hg, 0xff, sizeof hg);
              for (int li = 0; li < 64; ++li) {
                const int l = (li + (int)(k0 + k) * 7) & 63;  // rotate the priority
                const int R = kRGroup[l], C = l >> 4, H = l >> 5;
                const size_t slot = base + (size_t)(k0 + k) * 64 + l;
                int best = -1, best_score = -1;
                for (uint32_t c = wb[l]; c < we[l]; ++c) {
                  if (ctaken[c]) continue;
                  const uint32_t g = (uint32_t)(cells[c] >> 32), i = centry[c];
                  if (hybrid && !streaming && i >= n_hot) continue;  // a cold cell: not in the hot segment
                  int score = 0;
                  if (!(at[C] >> (g & 15) & 1)) score += MSW_W_AT;                         // atomic: bank pair free
                  if (rg[R][g & 15] == UINT32_MAX || rg[R][g & 15] == g) score += MSW_W_EW;  // {e,w} b128
                  if (rs[R][i & 15] == UINT32_MAX || rs[R][i & 15] == i) score += MSW_W_XT;  // slot entry b128
                  if (hg[H][g & 31] == UINT32_MAX || hg[H][g & 31] == g) score += MSW_W_E;  // e_g b64
                  if (!schedule) score = MSW_W_AT + MSW_W_EW + MSW_W_XT + MSW_W_E;  // CSR order: the first unplaced cell
                  if (score > best_score) {
                    best_score = score;
                    best = (int)c;
                    if (score == MSW_W_AT + MSW_W_EW + MSW_W_XT + MSW_W_E) break;  // free everywhere
                  }
                }
                const bool hot_row = hybrid && !streaming;  // (rows [0, nhot) of a split slice: the hot record form)
                if (best < 0) {
                  put(rec, slot, G + (uint32_t)l, used[0], -1, hot_row);  // the lane's own sentinel group
                  continue;
                }
                ctaken[best] = 1;
                const uint32_t g = (uint32_t)(cells[best] >> 32), i = centry[best];
                at[C] |= (uint16_t)(1u << (g & 15));
                if (rg[R][g & 15] == UINT32_MAX) rg[R][g & 15] = g;
                if (rs[R][i & 15] == UINT32_MAX) rs[R][i & 15] = i;
                if (hg[H][g & 31] == UINT32_MAX) hg[H][g & 31] = g;
                put(rec, slot, g, (uint32_t)cells[best], l, hot_row);
              }
            }
            for (int l = 0; l < 64; ++l) {  // the cold segment: CSR order, then the lane's sentinel
              uint32_t c = wb[l];
              for (uint32_t k = nhot; k < nrows; ++k) {
                const size_t slot = base + (size_t)(k0 + k) * 64 + l;
                while (c < we[l] && ctaken[c]) ++c;
                if (c < we[l]) {
                  put_entry(rec, slot, (uint32_t)(cells[c] >> 32), centry[c]);
                  ++c;
                } else {
                  put(rec, slot, G + (uint32_t)l, used[0], -1);
                }
              }
            }
          }
        }
      });
    }
    for (auto &th : pool) th.join();
  }
  if (getenv("MSW_DEBUG_SCHED")) {
    // modelled LDS cycles per wave instruction = sum over its lane groups of the largest number of
    // DISTINCT addresses on one bank (atomics: of accesses)
    uint64_t steps = 0, cyc_ew = 0, cyc_xt = 0, cyc_at = 0, cyc_e = 0;
    for (uint32_t s = 0; s < nslices; ++s) {
      const uint32_t len = slice_off[s + 1] - slice_off[s];
      const size_t base = (size_t)slice_off[s] * 64;
      for (uint32_t k = 0; k < len; ++k) {
        uint32_t vg[64], vi[64];
        for (int l = 0; l < 64; ++l) {
          const size_t slot = base + (size_t)k * 64 + l;
          if (wide) {
            const uint2 r = make_uint2(rec[2 * slot], rec[2 * slot + 1]);
            vg[l] = Rec<kEncWide>::grp(r, dec), vi[l] = Rec<kEncWide>::t_off(r, dec) >> 4;
          } else if (hybrid) {
            const bool hot = k < slice_hot[s];
            vg[l] = hot ? Rec<kEncIndex>::grp_h(rec[slot], dec) : Rec<kEncIndex>::grp(rec[slot], dec);
            vi[l] = (hot ? Rec<kEncIndex>::t_off_h(rec[slot], dec) : Rec<kEncIndex>::t_off(rec[slot], dec)) >> 4;
          } else {
            vg[l] = Rec<kEncNarrow>::grp(rec[slot], dec), vi[l] = Rec<kEncNarrow>::t_off(rec[slot], dec) >> 4;
          }
        }
        auto cyc = [&](const uint32_t *v, int ngroups, auto group_of, uint32_t nbanks, bool combine) {
          int total = 0;
          for (int gr = 0; gr < ngroups; ++gr) {
            int mx = 0;
            for (uint32_t bnk = 0; bnk < nbanks; ++bnk) {
              uint32_t seen[64]; int ns = 0;
              for (int l = 0; l < 64; ++l) if (group_of(l) == gr && (v[l] % nbanks) == bnk) {
                bool dup = false;
                if (combine) for (int q = 0; q < ns; ++q) dup |= seen[q] == v[l];
                if (!dup) seen[ns++] = v[l];
              }
              mx = std::max(mx, ns);
            }
            total += mx;
          }
          return total;
        };
        ++steps;
        cyc_ew += cyc(vg, 4, [](int l) { return (int)kRGroup[l]; }, 16, true);
        cyc_xt += cyc(vi, 4, [](int l) { return (int)kRGroup[l]; }, 16, true);
        cyc_at += cyc(vg, 4, [](int l) { return l >> 4; }, 16, false);
        cyc_e += cyc(vg, 2, [](int l) { return l >> 5; }, 32, true);
      }
    }
    fprintf(stderr, "[msw sched] steps %llu  modelled LDS cycles / wave instruction: {e,w} b128 %.2f (ideal 4)  "
                    "slot b128 %.2f (4)  atomics %.2f (4)  e_g b64 %.2f (2)\n",
            (unsigned long long)steps, (double)cyc_ew / steps, (double)cyc_xt / steps, (double)cyc_at / steps,
            (double)cyc_e / steps);
  }
  L.n_long = n_long;
  L.nslices = nslices;
  L.nslots = nslots;
  L.perm.upload(perm.data(), perm.size(), h->stream);
  L.long_ptr.upload(long_ptr.data(), long_ptr.size(), h->stream);
  L.rec_long.upload(rec_long.data(), rec_long.size(), h->stream);
  L.slice_off.upload(slice_off.data(), slice_off.size(), h->stream);
  L.rec.upload(rec.data(), rec.size(), h->stream);
  if (hybrid) L.slice_hot.upload(slice_hot.data(), std::max<size_t>(slice_hot.size(), 1), h->stream);
  finish_sell(h);  // synchronises: host staging vectors die at return
}

void set_csr_impl(msw_core *h, const uint64_t *rowptr, const uint32_t *grp, const uint32_t *cnt,
                  const double *lut, size_t lut_ld, double logzi, size_t G, size_t E) {
  Resident &L = h->lik;
  if (!rowptr || !lut) throw Fail("msw_core_set_csr: null argument");
  if (G == 0 || E == 0) throw Fail("msw_core_set_csr: empty likelihood (n_groups and n_ecs must be > 0)");
  if (G > 0x7fffffffull || E >= 0xffffffffull) throw Fail("msw_core_set_csr: dimensions exceed 32 bits");
  if (lut_ld == 0) throw Fail("msw_core_set_csr: lut_ld must be >= 1");
  if (rowptr[0] != 0) throw Fail("msw_core_set_csr: rowptr[0] must be 0");
  const bool host_pack = getenv("MSWEEP_HOST_PACK") != nullptr;
  if (host_pack)  // (the device path checks the pointers in the kernel that narrows them to 32 bits)
    for (size_t j = 0; j < E; ++j)
      if (rowptr[j + 1] < rowptr[j]) throw Fail("msw_core_set_csr: rowptr not monotone");
  const uint64_t nnz = rowptr[E];
  if (nnz >= 0xffffffffull) throw Fail("msw_core_set_csr: more than 2^32-1 nonzero cells");
  if (nnz > 0 && (!grp || !cnt)) throw Fail("msw_core_set_csr: null grp / cnt");
  StageTimer tm(h->stream);
  reset_likelihood(h);

  // de-duplicate LUT rows (groups of equal size share a beta-binomial table)
  std::vector<uint32_t> cls(G);
  std::vector<double> lut_c;
  {
    std::unordered_map<std::string, uint32_t> seen;
    for (size_t g = 0; g < G; ++g) {
      std::string key(reinterpret_cast<const char *>(lut + g * lut_ld), lut_ld * sizeof(double));
      auto it = seen.find(key);
      if (it == seen.end()) {
        const uint32_t c = (uint32_t)seen.size();
        seen.emplace(std::move(key), c);
        cls[g] = c;
        lut_c.insert(lut_c.end(), lut + g * lut_ld, lut + (g + 1) * lut_ld);
      } else {
        cls[g] = it->second;
      }
    }
  }
  const uint64_t n_lut = lut_c.size();
  if (n_lut > 0x7fffffffull) throw Fail("msw_core_set_csr: lookup table too large");
  L.G = (uint32_t)G;
  L.E = (uint32_t)E;
  L.nnz = nnz;
  L.n_lut = (uint32_t)n_lut;
  L.logzi = logzi;
  L.lut.upload(lut_c.data(), lut_c.size(), h->stream);
  if (host_pack) {  // reference implementation of the device packer (and of the slot indices)
    std::vector<uint32_t> idx((size_t)nnz + 1);
    for (uint64_t k = 0; k < nnz; ++k) {
      const uint32_t g = grp[k], c = cnt[k];
      if (g >= G) throw Fail("msw_core_set_csr: group id out of range");
      if (c >= lut_ld) throw Fail("msw_core_set_csr: hit count exceeds the lookup table width");
      idx[k] = cls[g] * (uint32_t)lut_ld + c;
    }
    upload_sell(h, rowptr, grp, idx.data());
    return;
  }
  // the cells' table slots, the range checks of (group, count) and of the row pointers on the device: no O(nnz) or
  // O(E) host loop (a 32-bit copy of the pointers made on the host cost 10 ms of the 43 at cfg3: a zeroed vector of
  // 37 MB and two passes over the 75 MB)
  std::vector<uint32_t> lut_off(G);
  for (size_t g = 0; g < G; ++g) lut_off[g] = cls[g] * (uint32_t)lut_ld;
  DevBuf<uint64_t> d_rp64;
  DevBuf<uint32_t> d_rp, d_grp, d_cnt, d_idx, d_off;
  DevBuf<int> d_bad;
  d_bad.alloc(1);
  d_bad.zero(h->stream);
  d_rp64.upload(rowptr, (size_t)E + 1, h->stream);
  d_rp.alloc((size_t)E + 1);
  hipLaunchKernelGGL(k_rowptr_narrow, dim3((unsigned)std::min<size_t>((E + 256) / 256, (size_t)h->n_cu * 16)), dim3(256), 0,
                     h->stream, d_rp64.p, (uint64_t)E + 1, nnz, d_rp.p, d_bad.p);
  d_grp.upload(grp, (size_t)nnz, h->stream);
  d_cnt.upload(cnt, (size_t)nnz, h->stream);
  d_off.upload(lut_off.data(), G, h->stream);
  d_idx.alloc((size_t)nnz);
  tm.mark("set_csr: checks + uploads");
  if (nnz)
    hipLaunchKernelGGL(k_csr_lutidx, dim3((unsigned)std::min<uint64_t>((nnz + 255) / 256, (uint64_t)h->n_cu * 32)),
                       dim3(256), 0, h->stream, d_grp.p, d_cnt.p, nnz, (uint32_t)G, (uint32_t)lut_ld, d_off.p, d_idx.p,
                       d_bad.p);
  int bad = 0;
  MSW_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost, h->stream));
  MSW_HIP(hipStreamSynchronize(h->stream));
  if (bad & 4) {  // (nothing has walked the rows yet: every kernel so far is per cell)
    reset_likelihood(h);
    throw Fail("msw_core_set_csr: rowptr not monotone");
  }
  if (bad & 1) {
    reset_likelihood(h);
    throw Fail("msw_core_set_csr: group id out of range");
  }
  if (bad & 2) {
    reset_likelihood(h);
    throw Fail("msw_core_set_csr: hit count exceeds the lookup table width");
  }
  d_cnt.release();
  tm.mark("set_csr: slots");
  sell_from_device(h, d_rp.p, d_grp.p, d_idx.p);
  tm.mark("set_csr: pack (total)");
}

}  // namespace

// From the staged [G][E] device matrix on: what msw_core_set_dense_logl (a host matrix, staged below) and
// msw_core_set_dense_logl_file (a matrix parsed on the device, host_likelihood_file.inc: Lm = null) share.  The caller has
// called reset_likelihood.
void msw::host::dense_from_stage(msw_core *h, const double *Lm, size_t ld, const double *stage, size_t G, size_t E) {
  Resident &L = h->lik;
  // either re-expressed as CSR-of-ECs (host_compress.inc: the reference's matrices are a background value plus few
  // listed cells; more groups than the dense sweeps take, 8192: re-expressed whatever its shape) ...
  if (compress_dense(h, Lm, ld, stage, G, E, G > 8192)) return;
  // ... or kept dense, EC-major
  L.G = (uint32_t)G;
  L.E = (uint32_t)E;
  L.n_lut = 0;
  L.logzi = 0.0;
  int nreg = 1;
  while (nreg * 64 < (int)G) nreg *= 2;
  L.nreg = nreg;
  L.Lt.alloc(G * E);
  dim3 grid((unsigned)((E + 63) / 64), (unsigned)((G + 63) / 64));
  transpose_launch(grid, h->stream, stage, E, (int)G, (uint32_t)E, L.Lt.p);  // (k_transpose: sweep_dense.hip)
  MSW_HIP(hipGetLastError());
  MSW_HIP(hipStreamSynchronize(h->stream));
  L.lut.alloc(1);
  L.lut_area.alloc(1);
  L.trange.alloc(2);  // no tables: the sweeps do not read it
  L.trange.zero(h->stream);
  // register-resident kernels (G <= 1024): 8 workgroups per CU; two-sweep kernels: 2 per CU
  L.nblk_dense = (int)std::max<size_t>(1, std::min<size_t>((E + 3) / 4, (size_t)h->n_cu * (nreg >= 32 ? 2 : 8)));
  L.flavor = 1;
  alloc_solve_state(L, h->solver);
  MSW_HIP(hipStreamSynchronize(h->stream));
}

namespace {

void set_dense_impl(msw_core *h, const double *Lm, size_t G, size_t E, size_t ld) {
  if (!Lm) throw Fail("msw_core_set_dense_logl: null matrix");
  if (G == 0 || E == 0) throw Fail("msw_core_set_dense_logl: empty likelihood");
  if (ld < E) throw Fail("msw_core_set_dense_logl: ld < n_ecs");
  if (E >= 0xffffffffull) throw Fail("msw_core_set_dense_logl: n_ecs exceeds 32 bits");
  reset_likelihood(h);
  // rows = groups, staged as they come
  DevBuf<double> stage;
  stage.alloc(G * E);
  MSW_HIP(hipMemcpy2DAsync(stage.p, E * sizeof(double), Lm, ld * sizeof(double), E * sizeof(double), G,
                           hipMemcpyHostToDevice, h->stream));
  dense_from_stage(h, Lm, ld, stage.p, G, E);
}

// gamma (or the likelihood itself) of the ECs [e0, e1), rows = groups, columns in the caller's EC order:
// out[g * ld + (j - e0)].  Computed in column blocks of at most 2^27 / G ECs on the device.
// (a, tref, u) of gamma after the last solve: RCG's scaled state, or EM's u = log(theta) of the last M-step with a = 1;
// tref = the table value with the largest a T.  What k_gamma_block and the bin pass (host_bin.inc) both read.
// (GammaState, MaterialiseArgs: handle.hpp)
GammaState gamma_state(Solver &s) {
  poll(s);
  const double a = s.last_algo == MSW_ALGO_EM ? 1.0 : s.sc_host->a;
  return GammaState{a, a >= 0.0 ? s.sc_host->tmax : s.sc_host->tmin, s.u.p};
}

}  // namespace

void msw::host::materialise_args(msw_core *h, bool gamma, MaterialiseArgs &m) {
  const Resident &L = h->lik;
  if (gamma) {
    const GammaState gs = gamma_state(h->solver);
    m.a = gs.a;
    m.tref = gs.tref;
    m.u = gs.u;
  } else {
    m.zero_u.alloc(L.G);
    m.zero_u.zero(h->stream);
    m.u = m.zero_u.p;
  }
  if (L.flavor == 0 && !h->iperm.p) {
    h->iperm.alloc(L.E);
    hipLaunchKernelGGL(k_invert_perm, dim3((L.E + 255) / 256), dim3(256), 0, h->stream, L.perm.p, L.E, h->iperm.p);
  }
}

// the ECs [j0, j1) into device memory, buf[g * (j1 - j0) + (j - j0)]: enqueued on the handle's stream
void msw::host::materialise_block(msw_core *h, const MaterialiseArgs &m, bool gamma, size_t j0, size_t j1, double *buf) {
  const Resident &L = h->lik;
  const uint32_t G = L.G;
  const size_t w = j1 - j0;
  const unsigned nb = (unsigned)std::min<size_t>((w + 255) / 256, 4096);
  if (L.flavor == 0) {
    auto k = L.enc == kEncValue ? k_gamma_block<kEncValue>
                                 : (L.wide() ? k_gamma_block<kEncWide> : (L.hybrid() ? k_gamma_block<kEncIndex> : k_gamma_block<kEncNarrow>));
    hipLaunchKernelGGL(k, dim3(nb), dim3(256), 0, h->stream, sell_view(L, h->solver), h->iperm.p, (uint32_t)j0,
                       (uint32_t)j1, m.a, L.logzi, m.tref, m.u, L.lut.p, gamma ? 1 : 0, buf, w);
  } else {
    hipLaunchKernelGGL(k_gamma_dense, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, h->stream, L.Lt.p, (int)G,
                       (uint32_t)w, m.a, m.u, gamma ? 1 : 0, buf, w, 0, (int)G, (uint32_t)j0);
  }
  MSW_HIP(hipGetLastError());
}

namespace {

void materialise_impl(msw_core *h, double *out, size_t ld, bool gamma, size_t e0, size_t e1) {
  const Resident &L = h->lik;
  if (L.flavor < 0) throw Fail("no likelihood resident");
  if (!out) throw Fail("null output");
  const uint32_t G = L.G, E = L.E;
  if (e0 > e1 || e1 > E) throw Fail("EC range out of bounds");
  if (ld < e1 - e0) throw Fail("ld smaller than the number of ECs asked for");
  if (e0 == e1) return;
  MaterialiseArgs m;
  materialise_args(h, gamma, m);
  const size_t blk = std::max<size_t>(1, std::min<size_t>(e1 - e0, ((size_t)1 << 27) / std::max<uint32_t>(G, 1)));
  DevBuf<double> buf;
  buf.alloc((size_t)G * blk);
  for (size_t j0 = e0; j0 < e1; j0 += blk) {
    const size_t j1 = std::min(e1, j0 + blk), w = j1 - j0;
    materialise_block(h, m, gamma, j0, j1, buf.p);
    MSW_HIP(hipMemcpy2DAsync(out + (j0 - e0), ld * sizeof(double), buf.p, w * sizeof(double), w * sizeof(double), G,
                             hipMemcpyDeviceToHost, h->stream));
    MSW_HIP(hipStreamSynchronize(h->stream));
  }
}

void build_likelihood_impl(msw_core *h, const uint64_t *ec_tptr, const uint32_t *ec_targets, size_t E,
                           const uint32_t *target_group, size_t T, const uint64_t *group_sizes,
                           size_t G, const uint64_t *ec_counts, double q, double e, double zi,
                           size_t min_hits, size_t *n_groups_out, uint8_t *mask_out, double *logc_out);

}  // namespace
