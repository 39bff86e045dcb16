// sparse_probs_kernels.hpp -- the read-to-group probabilities as sparse text on the device (msw_core_sparse_probs_*,
// host_sparse_probs.inc): one line "id \t g \t g6(exp(gamma)) \n" per cell with gamma(g, j) >= log(tau),
// rows by EC or by aligned read, without a G x E block anywhere.
#pragma once
#include "gamma_cell.hpp"
#include "text_kernels.hpp"

namespace msw {

// ---------------------------------------------------------------------------------------
// Rule: cell (g, j) is kept <=> gamma(g, j) >= log(tau), gamma formed with gamma_cell.hpp's expressions (the bits
// msw_core_gamma_block returns), log(tau) formed once on the host.
//
// An EC's unlisted groups all have gamma_cell(a, logzi, u_g, lse_j): monotone in u_g (a floating-point add is monotone,
// with or without contraction of a * logzi + u_g).  With the groups ordered by u_g descending (once per begin: monotone
// integer keys, a stable radix sort) the unlisted groups that pass are a PREFIX of that order, found by a binary search
// that evaluates that very expression -- and, equal u_g giving equal values, the prefix never ends inside a run of ties,
// so "group g lies in the prefix" is that expression on u_g itself: no table of ranks is read.  Listed cells are tested
// one by one on their own value; a listed group inside the prefix is replaced by its listed value, which may fail.
//
// Passes (host_sparse_probs.inc):
//   count   a thread per permuted position: lse_j (kept), the prefix length K_j, and per EC its CANDIDATES (the K_j
//           prefix groups, and every listed cell that passes or lies in the prefix) and its kept cells
//   (rows: the candidate and kept counts of every row -- an EC, or the EC of an aligned read --, two exclusive scans)
//   per piece of rows:
//   write   a thread per row: its candidates as keys (row in piece, g, background?) with their gamma
//   (one stable radix sort of the keys: every row's candidates by g, a listed cell right in front of the background
//    candidate of the same group)
//   len     a thread per candidate: kept?  (listed: its value passes; background: no listed cell in front of it), the
//           bits of exp(gamma) and the length of its line
//   (exclusive scan; the piece is cut at the last row end within max_bytes: its rows were chosen by their kept cells at
//    16 bytes a line, and what a cut leaves over is formed again with the next piece)
//   text    a thread per kept cell: its line.  Undecided values (g6_format.hpp) as in text_kernels.hpp: 13 blanks and
//           an entry of the host's list; k_text_close puts them in.
// No atomic decides an order: the list of undecided cells is sorted by offset on the host.
// Work per EC: its listed cells, log G steps of the search, and its candidates; nothing runs over all groups except the
// guard path of gamma_lse.  (u_g is finite or -inf after a solve; a NaN would break the order and keep nothing it should not.)
// ---------------------------------------------------------------------------------------
struct SpRule {
  double a, logzi, logthr;
  const double *u;        // [G] by group
  const double *us;       // [G] u in descending order
  const uint32_t *order;  // [G] the group at every place of that order (ties: ascending g)
};

// keys whose ASCENDING order is u DESCENDING
__global__ __launch_bounds__(256) void k_sp_order_keys(const double *u, uint32_t G, uint64_t *key, uint32_t *grp) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const uint64_t b = (uint64_t)__double_as_longlong(u[g]);
  key[g] = ~(b ^ ((b >> 63) ? ~(uint64_t)0 : (uint64_t)1 << 63));
  grp[g] = g;
}
__global__ __launch_bounds__(256) void k_sp_gather(const double *u, const uint32_t *order, uint32_t G, double *us) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < G) us[k] = u[order[k]];
}

// the unlisted groups that pass: places [0, K) of the order
__device__ __forceinline__ uint32_t sp_prefix(const SpRule &R, uint32_t G, double lse) {
  uint32_t lo = 0, hi = G;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (gamma_cell(R.a, R.logzi, R.us[mid], lse) >= R.logthr) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// f(g, gamma, pass, in_prefix) for every listed cell of the EC at position p that passes or lies in the prefix.  Count
// and write pass both visit through here.
template <int ENC, class F>
__device__ __forceinline__ void sp_visit_listed(const SellDev &S, uint32_t p, const SpRule &R, double lse, F f) {
  for_each_cell<ENC>(S, p, [&](uint32_t g, double T) {
    const double v = gamma_cell(R.a, T, R.u[g], lse);
    const bool pass = v >= R.logthr, in = gamma_cell(R.a, R.logzi, R.u[g], lse) >= R.logthr;
    if (pass || in) f(g, v, pass, in);
  });
}

// count pass: lse_p[p]; cand[perm[p]] = the EC's candidates, kept[perm[p]] = its kept cells
template <int ENC>
__global__ __launch_bounds__(256) void k_sp_count(SellDev S, SpRule R, double tref, double *lse_p, uint32_t *cand, uint32_t *kept) {
  __shared__ double sh[32];
  double M, U;
  gamma_norm_consts(S.n_groups, R.u, sh, M, U);
  const double p0 = exp(R.a * (R.logzi - tref));
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_ecs; p += gridDim.x * blockDim.x) {
    const double lse = gamma_lse<ENC>(S, p, R.a, tref, R.u, M, U, p0);
    const uint32_t K = sp_prefix(R, S.n_groups, lse);
    uint32_t nl = 0, np = 0, nin = 0;
    sp_visit_listed<ENC>(S, p, R, lse, [&](uint32_t, double, bool pass, bool in) {
      ++nl;
      np += pass;
      nin += in;
    });
    const uint32_t j = S.perm[p];
    lse_p[p] = lse;
    cand[j] = nl + K;
    kept[j] = np + K - nin;
  }
}

// rc[r], rk[r] = candidates and kept cells of row r (ec == null: row r is EC r); the spare element r = n_rows: 0
__global__ __launch_bounds__(256) void k_sp_rows(const uint32_t *ec, const uint32_t *cand, const uint32_t *kept, uint64_t n_rows,
                                                uint32_t *rc, uint32_t *rk) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t j = r < n_rows ? (ec ? ec[r] : (uint32_t)r) : 0u;
    rc[r] = r < n_rows ? cand[j] : 0u;
    rk[r] = r < n_rows ? kept[j] : 0u;
  }
}

// one thread: out[0] = the largest r1 in [r0 + 1, hi] whose rows [r0, r1) have at most `kept` kept cells and `cand`
// candidates (r0 + 1 when none has: a piece holds a row at least), out[1] = their candidates
__global__ void k_sp_span(const uint64_t *koff, const uint64_t *coff, uint64_t r0, uint64_t hi, uint64_t kept, uint64_t cand,
                          uint64_t *out) {
  const uint64_t k0 = koff[r0], c0 = coff[r0];
  uint64_t lo = r0 + 1;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (koff[mid] - k0 <= kept && coff[mid] - c0 <= cand) lo = mid;
    else hi = mid - 1;
  }
  out[0] = lo;
  out[1] = coff[lo] - c0;
}

constexpr int kSpRowShift = 33;  // key = row in piece << 33 | g << 1 | background

// write pass: the candidates of the rows [r0, r0 + n) at [coff[r] - coff[r0], coff[r + 1] - coff[r0])
template <int ENC>
__global__ __launch_bounds__(256) void k_sp_write(SellDev S, SpRule R, const uint32_t *iperm, const double *lse_p, const uint32_t *ec,
                                                 const uint64_t *coff, uint64_t r0, uint32_t n, uint64_t *key, uint32_t *idx,
                                                 double *gam) {
  const uint64_t c0 = coff[r0];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t r = r0 + i;
    const uint32_t j = ec ? ec[r] : (uint32_t)r, p = iperm[j];
    const double lse = lse_p[p];
    uint64_t o = coff[r] - c0;
    const uint64_t end = coff[r + 1] - c0;
    auto put = [&](uint32_t g, uint32_t bg, double v) {
      if (o < end) {
        key[o] = (uint64_t)i << kSpRowShift | (uint64_t)g << 1 | bg;
        idx[o] = (uint32_t)o;
        gam[o] = v;
      }
      ++o;
    };
    sp_visit_listed<ENC>(S, p, R, lse, [&](uint32_t g, double v, bool, bool) { put(g, 0u, v); });
    const uint32_t K = sp_prefix(R, S.n_groups, lse);
    for (uint32_t k = 0; k < K; ++k) put(R.order[k], 1u, gamma_cell(R.a, R.logzi, R.us[k], lse));
  }
}

struct SpPiece {
  const uint64_t *key;   // the sorted candidates ...
  const uint32_t *idx;   // ... and where the write pass left each (its gamma)
  uint32_t n_cand, n_rows;
  uint64_t r0;           // the piece's first row
  const uint32_t *ids;   // by read: the id of every row; null: the row number is the id
};

__device__ __forceinline__ uint64_t sp_row_id(const SpPiece &P, uint64_t k) {
  const uint64_t r = P.r0 + (k >> kSpRowShift);
  return P.ids ? (uint64_t)P.ids[r] : r;
}
__device__ __forceinline__ uint32_t sp_group(uint64_t k) { return (uint32_t)(k >> 1); }

// length pass: elen[i] = the bytes of candidate i's line (0: not kept), pbits[i] = the bits of exp(gamma)
__global__ __launch_bounds__(256) void k_sp_len(SpPiece P, const double *gam, double logthr, uint32_t *elen, uint64_t *pbits) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < P.n_cand; i += gridDim.x * blockDim.x) {
    const uint64_t k = P.key[i];
    const uint32_t ix = P.idx[i];
    uint32_t len = 0;
    uint64_t bits = 0;
    if ((k >> kSpRowShift) < P.n_rows && ix < P.n_cand) {  // (a slot the write pass left out names no row of the piece)
      const double v = gam[ix];
      const bool keep = (k & 1) ? !(i > 0 && P.key[i - 1] + 1 == k) : v >= logthr;
      if (keep) {
        bits = text_cell_bits<kTextProbs>(v);
        g6::Text t;
        g6::format(bits, t);
        len = text_dec_len(sp_row_id(P, k)) + text_dec_len(sp_group(k)) + t.len + 3u;
      }
    }
    elen[i] = len;
    pbits[i] = bits;
  }
}

// one thread: the last row end within max_bytes.  out[0] = the largest r1 in [r0, r1p] whose rows [r0, r1) have at most
// max_bytes of text, out[1] = their candidates, out[2] = their bytes, out[3] = the bytes of row r0 alone, out[4] = their
// kept cells
__global__ void k_sp_cut(const uint64_t *coff, const uint64_t *koff, uint64_t r0, uint64_t r1p, const uint64_t *eoff,
                         uint64_t max_bytes, uint64_t *out) {
  const uint64_t c0 = coff[r0];
  uint64_t lo = r0, hi = r1p;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (eoff[coff[mid] - c0] <= max_bytes) lo = mid;
    else hi = mid - 1;
  }
  out[0] = lo;
  out[1] = coff[lo] - c0;
  out[2] = eoff[coff[lo] - c0];
  out[3] = eoff[coff[r0 + 1] - c0];
  out[4] = koff[lo] - koff[r0];
}

// write pass of the text: the line of every kept candidate i < n_use at eoff[i]
__global__ __launch_bounds__(256) void k_sp_text(SpPiece P, uint32_t n_use, const uint32_t *elen, const uint64_t *eoff,
                                                const uint64_t *pbits, uint8_t *__restrict__ out, TextHostCell *__restrict__ list,
                                                uint32_t *__restrict__ n_list, uint32_t list_cap) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_use; i += gridDim.x * blockDim.x) {
    if (elen[i] == 0) continue;
    const uint64_t k = P.key[i], o = eoff[i], id = sp_row_id(P, k), bits = pbits[i];
    const uint32_t g = sp_group(k);
    uint8_t *p = out + o;
    uint32_t nd = text_dec_len(id);
    text_put_dec(p, id, nd);
    p[nd] = '\t';
    p += nd + 1;
    nd = text_dec_len(g);
    text_put_dec(p, g, nd);
    p[nd] = '\t';
    p += nd + 1;
    g6::Text t;
    if (g6::format(bits, t) == g6::kUndecided) {
      const uint32_t q = atomicAdd(n_list, 1u);
      if (q < list_cap) list[q] = TextHostCell{o + (uint64_t)(p - (out + o)), bits};
      for (uint32_t b = 0; b < t.len; ++b) p[b] = ' ';
    } else {
      for (uint32_t b = 0; b < t.len; ++b) p[b] = (uint8_t)((b < 8 ? t.lo >> (8 * b) : t.hi >> (8 * (b - 8))) & 0xff);
    }
    p[t.len] = '\n';
  }
}

}  // namespace msw
