// host_layout.inc -- layout planning of the resident likelihood: LDS placement, pass B's mode, the record encoding
// and the hybrid slot area (sell.hpp).  Runs before the SELL packing (host_likelihood.inc, host_pack.inc).
namespace {

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

}  // namespace
