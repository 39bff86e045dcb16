// em_f32_kernels.hpp -- `--algorithm emgpu --emprecision float` (src/mSWEEP.cpp:129,200-203: rcgpar::em_torch with
// precision "float" [UPSTREAM-UNVERIFIED]; the reference's fastest GPU mode, docs/gpubenchmarks.md:22,25) as REAL
// fp32 arithmetic.  Until round 4 MSW_PREC_FLOAT ran the fp64 kernels.
//
// What "float" means here (the reading restated in oracle/rcg_oracle.cpp orc_em_dense_f32):
//   * the likelihood values, the weights theta, the responsibilities' numerators e_g exp(T - tref), the row sums
//     Z_j and the quotients r_j = c_j / Z_j are fp32;
//   * c_j log Z_j is formed in fp32 per EC; the sum over the ECs -- like every sum over millions of terms in this
//     library -- is accumulated in fp64, and the log-likelihood is ROUNDED TO FLOAT once per iteration: the stop rule
//     compares two floats (a float near 1e8 moves in steps of 8, which is why the reference's float mode stops after a
//     few hundred iterations where double runs into --max-iters: docs/gpubenchmarks.md:20-22);
//   * the column sums stay 64-bit fixed-point integers (exact, order-independent): a cell adds rint(2^K r_j e_g x)
//     with the product formed in fp32.  No per-group power-of-two factor (device_util.hpp fx_factor): 2^-K reads of
//     absolute resolution is far below fp32's relative 6e-8 of any weight a float run can resolve.
// An EM iteration with a = 1: x_i = exp(T_i - tref) never changes, so the slot table {x_i - p0} is built ONCE per solve
// and is 4 bytes per entry; e_g is 4 bytes per group: the sweep's LDS image holds the records' own byte offsets
// shifted down -- entry offset >> 2, group offset >> 1 -- so the 4-byte records of the fp64 sweeps serve unchanged.
// Per cell: 2 ds_read_b32 + 1 ds_add_u64 against ds_read_b64 + ds_read_b128 + ds_add_u64, ~7 instead of ~11 vector
// operations, no second table column (EM's objective has no entropy term).
//
// Served layouts (sweep_dense.hip em_f32_layout_ok), one GPU, at most kStepRegs * 1024 = 6144 groups, any EC length
// (slice classes, wavefront-per-EC), the group vectors in LDS:
//   * 4-byte offset records with the whole fp64 slot table in LDS (k_em_passB_f32);
//   * index records -- the layouts whose fp64 slot table does NOT fit LDS beside the group vectors and is kept as the
//     hybrid area (sell.hpp: groupings with sizes up to hundreds, thousands of used (size, count) pairs) -- whenever
//     the FLOAT image fits: 4 bytes per entry instead of 16, so the whole area goes to LDS and the sweep has neither a
//     cold segment nor a gather from memory (k_em_passB_f32_idx).  The records, slice_hot and the packer are those of
//     the fp64 sweeps: both record forms of a slice (hot rows carry 16 * entry, all others the entry index) address
//     the one float table.
// Everything else -- 8-byte and value records, index layouts whose float image does not fit, groups not in LDS, dense
// matrices without background structure, EC-sharded solves -- runs the fp64 kernels under MSW_PREC_FLOAT as before;
// msw_timing::em_float_kernels says which it was.
#pragma once
#include "sweep_kernels.hpp"

namespace msw {

// ---- fp32 lane reductions (DPP, as device_util.hpp's fp64 ones) ---------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move_f(float v, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_f(float v) {
  v += dpp_move_f<0x111, 0xf>(v, 0.0f);
  v += dpp_move_f<0x112, 0xf>(v, 0.0f);
  v += dpp_move_f<0x114, 0xf>(v, 0.0f);
  v += dpp_move_f<0x118, 0xf>(v, 0.0f);
  v += dpp_move_f<0x142, 0xa>(v, 0.0f);
  v += dpp_move_f<0x143, 0xc>(v, 0.0f);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float group_sum_f(float v, uint32_t lgm) {
  if (lgm >= 1) v += dpp_move_f<0xB1, 0xf>(v, 0.0f);
  if (lgm >= 2) v += dpp_move_f<0x4E, 0xf>(v, 0.0f);
  if (lgm >= 3) v += dpp_move_f<0x141, 0xf>(v, 0.0f);
  if (lgm >= 4) v += dpp_move_f<0x140, 0xf>(v, 0.0f);
  if (lgm >= 5) v += __shfl_xor(v, 16, 64);
  if (lgm >= 6) v += __shfl_xor(v, 32, 64);
  return v;
}

// LDS image of the fp32 sweep (byte offsets; bhi = sell_bhi(n_tab) as in the fp64 image, Gp = G + kSentinels):
//   [0, 4 n_tab)                       x_i - p0 as float, entry i at (16 i) >> 2
//   [bhi / 2, bhi / 2 + 4 Gp)          e_g as float, group g at (bhi + 8 g) >> 1
//   [bhi + C, bhi + C + 8 Gp)          column sums (64-bit fixed point), group g at (bhi + 8 g) + C
//   then 48 doubles of reduction scratch and the slice geometry of 16 wavefronts (as the fp64 image's tail)
__host__ __device__ inline uint32_t em_f32_acc_off(uint32_t G) { return ((4u * (G + kSentinels)) + 7u) & ~7u; }
__host__ __device__ inline size_t em_f32_scratch_off(uint32_t n_tab, uint32_t G) {
  return (size_t)sell_bhi(n_tab) + em_f32_acc_off(G) + 8 * ((size_t)G + kSentinels);
}
__host__ __device__ inline size_t em_f32_lds_bytes(uint32_t n_tab, uint32_t G) {
  return em_f32_scratch_off(n_tab, G) + 64 * sizeof(double) + 16 * kGeoStride;
}
// ... and of the index-record sweep: the WHOLE slot area (n_area entries, whatever part of it the fp64 images hold),
// the records carry indices, so nothing ties the three parts to the fp64 image's offsets:
//   [0, 4 n_area)                      x_i - p0 as float, entry i at 4 i
//   [eoff, eoff + 4 Gp)                e_g as float       (eoff = 4 n_area rounded up to 8)
//   [eoff + C, eoff + C + 8 Gp)        column sums        (C = em_f32_acc_off(G))
//   then the same tail
__host__ __device__ inline uint32_t em_f32_idx_e_off(uint32_t n_area) { return (4u * n_area + 7u) & ~7u; }
__host__ __device__ inline size_t em_f32_idx_scratch_off(uint32_t n_area, uint32_t G) {
  return (size_t)em_f32_idx_e_off(n_area) + em_f32_acc_off(G) + 8 * ((size_t)G + kSentinels);
}
__host__ __device__ inline size_t em_f32_idx_lds_bytes(uint32_t n_area, uint32_t G) {
  return em_f32_idx_scratch_off(n_area, G) + 64 * sizeof(double) + 16 * kGeoStride;
}

// Once per float solve, behind k_em_init (which left M, U, p0, tref and the fp64 e_g of the uniform start):
// the fp32 slot table from the FLOAT-rounded table values, e_g rounded to float (and written back as such: every
// consumer of e_g -- k_redfin's background share, the guarded ECs -- sees the values the sweep uses), U over them.
__global__ __launch_bounds__(1024) void k_em_f32_prep(Scalars *sc, int G, int n_tab, const double *lut_area, double *e,
                                                     float *e32, float *tab32) {
  __shared__ double sh[32];
  const int tid = threadIdx.x, nt = blockDim.x;
  const double tref = sc->tref, p0 = (double)(float)sc->p0;
  for (int i = tid; i < n_tab; i += nt)
    tab32[i] = (float)(exp((double)(float)lut_area[i] - tref) - p0);
  double su = 0.0;
  for (int g = tid; g < G + (int)kSentinels; g += nt) {
    const float ef = g < G ? (float)e[g] : 0.0f;
    e32[g] = ef;
    if (g < G) {
      e[g] = (double)ef;
      su += (double)ef;
    }
  }
  const double U = block_sum(su, sh);
  if (tid == 0) {
    sc->U = U;
    sc->p0 = p0;
  }
}

typedef __attribute__((address_space(3))) const float lds_cf_t;
typedef __attribute__((address_space(3))) unsigned long long lds_u64f_t;

// How a record is taken apart.  Offset records have one form and need nothing here.  Index records have two
// (sell.hpp): the rows of a slice's hot segment carry group << shiftH | 16 * entry, every other row -- cold segments,
// whole-memory and streaming slices, long ECs -- group << shift | entry.  Either way the group is one shift and
// 4 * entry, the float table's byte offset, two: (r << lsh) >> rsh.  Which form a row has is wave-uniform, so the three
// amounts sit in SGPRs and both forms run the same code.
struct F32Form {
  uint32_t gs, lsh, rsh;
};

// The sweep itself, for offset records (ENC = kEncNarrow) and index records (kEncIndex); smem = the workgroup's
// dynamic LDS, which starts at LDS address 0 (sweep_kernels.hpp: a record field IS the ds address).
template <int ENC, bool ML>
__device__ __forceinline__ void em_passB_f32_body(unsigned char *smem, const Scalars *sc, const SellDev &S, const double *e_g,
                                                  const float *e32_g, const float *tab32_g, double *partAcc, double *partS,
                                                  const GuardDev &GD) {
  static_assert(ENC == kEncNarrow || ENC == kEncIndex, "4-byte table records only");
  constexpr int NT = 1024;
  constexpr bool IDX = ENC == kEncIndex;
  using R = Rec<ENC>;
  const RecDec D = rec_dec(S);
  const uint32_t n_tab = IDX ? S.n_area : S.n_tab_lds;  // (index records: the whole area, not the fp64 images' hot head)
  const int skip = sc->done;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t G = S.n_groups, Gp = G + kSentinels, bhi = S.bhi;
  const uint32_t accC = em_f32_acc_off(G);
  // byte offsets of e_g[0] and of the first column sum (offset records: the fp64 image's, shifted -- above)
  const uint32_t eoff = IDX ? em_f32_idx_e_off(n_tab) : bhi / 2, accoff = IDX ? eoff + accC : bhi + accC;
  const uint32_t scratch_off = (uint32_t)(IDX ? em_f32_idx_scratch_off(n_tab, G) : em_f32_scratch_off(n_tab, G));
  // (index records: shift <= 30 and shiftH >= 4 -- em_f32_layout_ok, choose_hybrid_layout)
  const F32Form fcold = {D.shift, 32u - D.shift, 30u - D.shift}, fhot = {D.shiftH, 32u - D.shiftH, 34u - D.shiftH};
  double *sh = reinterpret_cast<double *>(smem + scratch_off);
  SliceStream<ENC, MSW_REVERSE_B> stream(S, uniform(blockIdx.x * (NT / 64) + (tid >> 6)), gridDim.x * (NT / 64),
                                         (uint32_t)lane, scratch_off + 64 * 8 + uniform(tid >> 6) * kGeoStride);
  // (the first slice's records in flight under the LDS fill: SliceStream::prime)
  const uint32_t n_lanes = S.nslices * 64u;
  const uint32_t null_rec = R::make(G + (uint32_t)lane, 0u, D);  // the lane's own sentinel group: e = 0
  uint32_t null_hot = null_rec;  // ... in the form of a hot segment's rows
  if constexpr (IDX) null_hot = R::make_h(G + (uint32_t)lane, 0u, D);
  stream.nullr = null_rec;
  stream.nullr_hot = null_hot;
  auto issue = [&](SliceBuf<ENC> &sb) {
    const uint32_t q = sb.sl * 64 + lane;
    const uint32_t cj = S.c8s[q < n_lanes ? q : 0u];
    sb.c8 = q < n_lanes ? cj : 0u;
  };
  // (offset records only, as in k_passB: the primed buffer of an index-record slice -- hot rows, cold rows, the two
  // null records -- is not kept in registers by the compiler: 104 bytes of scratch per lane)
  constexpr bool PRIME = !IDX;
  SliceBuf<ENC> first = {};
  if constexpr (PRIME) stream.prime(first, issue);
  {
    float *t = reinterpret_cast<float *>(smem);
    for (uint32_t i = tid; i < n_tab; i += NT) t[i] = tab32_g[i];
    float *el = reinterpret_cast<float *>(smem + eoff);
    unsigned long long *al = reinterpret_cast<unsigned long long *>(smem + accoff);
    for (uint32_t g = tid; g < Gp; g += NT) {
      el[g] = e32_g[g];
      al[g] = 0ull;
    }
  }
  // (f: the row's record form -- index records only)
  auto E_ = [&](uint32_t r, const F32Form &f) -> float {
    if constexpr (IDX) return *(lds_cf_t *)(size_t)(eoff + ((r >> f.gs) << 2));
    else return *(lds_cf_t *)(size_t)((r >> D.shift) >> 1);
  };
  auto X_ = [&](uint32_t r, const F32Form &f) -> float {
    if constexpr (IDX) return *(lds_cf_t *)(size_t)((r << f.lsh) >> f.rsh);
    else return *(lds_cf_t *)(size_t)((r & D.mask) >> 2);
  };
  // one column-sum update: rint(2^K q) as a 64-bit integer (sweep_kernels.hpp fx_bits; q = r_j e_g (x - p0) in fp32)
  const double fxs = uniform_d(sc->fx_scale);
  // (|q| <= 2^8 c_j: e_g x <= Z_j, and the guard keeps Z_j above 2^-8 of the background sum.  The one-fma conversion
  // needs |2^K q| < 2^51: an EC that holds more than ~2^-18 of all reads -- toy inputs -- splits its addends into two
  // parts of 32 and 51 bits like the fp64 sweep's wide adds; the sums are modulo 2^64, the parts need not meet)
  const float narrow_c = (float)(0x1p43 / fxs);
  auto add = [&](uint32_t r, float q, bool narrow, const F32Form &f) {
    lds_u64f_t *dst;
    if constexpr (IDX) dst = (lds_u64f_t *)(size_t)(accoff + ((r >> f.gs) << 3));
    else dst = (lds_u64f_t *)(size_t)((r >> D.shift) + accC);
    if (narrow) {
      __hip_atomic_fetch_add(dst, fx_bits((double)q, fxs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      const double qq = (double)q * fxs;                     // exact: fxs is a power of two
      const double vh = fma(qq, 0x1p-32, kFxMagic);
      const double qh = vh - kFxMagic;                       // rint(qq / 2^32)
      const double ql = fma(-qh, 0x1p32, qq);                // |ql| <= 2^31, exact
      __hip_atomic_fetch_add(dst, (unsigned long long)(uint32_t)__double2loint(vh) << 32, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(dst, fx_bits(1.0, ql), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  };
  const float p0 = (float)uniform_d(sc->p0), zbase = p0 * (float)uniform_d(sc->U);
  const GuardQueue<float> gq(GD, scratch_off, zbase);  // ECs whose Z falls below gthr are set aside (guard.hpp)
  const float gthr = gq.threshold();
  double s_clogZ = 0.0, s_W = 0.0;  // sums over millions of ECs: fp64 accumulators of fp32 terms (file header)
  if (skip) return;
  gq.reset(tid);
  __syncthreads();

  // Z, r, the EC's log-likelihood term and W for one EC whose row sum is zs; returns r (0: nothing to scatter)
  auto epilogue = [&](float zs, float c, bool spoke, uint32_t pos) -> float {
    const float Z = zbase + zs;
    if (c == 0.0f) return 0.0f;
    if (!(Z >= gthr)) {
      if (spoke) gq.defer(pos);
      return 0.0f;
    }
    const float rj = c / Z;
    if (spoke) {
      s_W += (double)rj;
      s_clogZ += (double)(c * logf(Z));
    }
    return rj;
  };
  auto process = [&](SliceBuf<ENC> &sb) {
    const uint32_t len = sb.len;
    const uint32_t lgm = ML ? sb.lgm : 0u;
    const uint32_t pos = S.n_long + (ML ? slice_geo(S.cls, sb.sl).ec0 + ((uint32_t)lane >> lgm) : sb.sl * 64 + lane);
    float c = (float)sb.c8;
    if (__builtin_amdgcn_ballot_w64(sb.c8 == kC8Escape)) {  // (wave-uniform; the wait inside: see k_passB)
      if (sb.c8 == kC8Escape) c = (float)S.cvec[pos];
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    const bool spoke = !ML || lgm == 0u || ((uint32_t)lane & ((1u << lgm) - 1u)) == 0u;
    if (len <= (uint32_t)kRegCells) {
      // index records: sb.r holds the rows of the slice's hot segment in their own form and sb.rc the (at most
      // kColdRows) others, or -- a slice the packer left uncut -- sb.r holds them all in the plain form
      // (load_slice_split).  All of them are served from the LDS table here: the cut only says how a row is decoded.
      uint32_t nr = len, ncold = 0, nullr = null_rec;  // rows in sb.r / in sb.rc; the null record of sb.r's form
      F32Form fr = fcold;
      if constexpr (IDX) {
        if (len - sb.nhot <= (uint32_t)kColdRows) {
          nr = sb.nhot, ncold = len - sb.nhot, nullr = null_hot;
          fr = fhot;
        }
      }
      float zs = 0.0f, pk[kRegCells];
      [[maybe_unused]] float pc[kColdRows];
      if constexpr (IDX) {
#pragma unroll
        for (int j = 0; j < kColdRows; ++j) {
          if ((uint32_t)j < ncold) {
            pc[j] = E_(sb.rc[j], fcold) * X_(sb.rc[j], fcold);
            zs += pc[j];
          }
        }
      }
#pragma unroll
      for (int k0 = 0; k0 < kRegCells; k0 += 4) {
        if ((uint32_t)k0 < nr) {  // (rows past an odd slice's end hold the lane's null record: load_slice)
          float ev[4], xv[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t r = (uint32_t)(k0 + k) < nr + (nr & 1u) ? sb.r[k0 + k] : nullr;
            ev[k] = E_(r, fr), xv[k] = X_(r, fr);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            pk[k0 + k] = ev[k] * xv[k];
            zs += pk[k0 + k];
          }
        }
      }
      if (ML && lgm != 0u) zs = group_sum_f(zs, lgm);
      const float rj = epilogue(zs, c, spoke, pos);
      if (rj != 0.0f) {
        const bool narrow = c < narrow_c;
#pragma unroll
        for (int k = 0; k < kRegCells; k += 2) {
          if ((uint32_t)k < nr) {
            add(sb.r[k], rj * pk[k], narrow, fr);
            add(sb.r[k + 1], rj * pk[k + 1], narrow, fr);  // (an odd slice's missing row: the null record, pk = 0)
          }
        }
        if constexpr (IDX) {
#pragma unroll
          for (int j = 0; j < kColdRows; ++j)
            if ((uint32_t)j < ncold) add(sb.rc[j], rj * pc[j], narrow, fcold);
        }
      }
    } else {
      // more rows than the registers hold (MSWEEP_MULTILANE=0 layouts only: one lane per EC): row by row, twice
      const size_t base = (size_t)sb.o * 64 + lane;
      float zs = 0.0f;
      for (uint32_t k = 0; k < len; ++k) {
        const uint32_t r = S.rec[base + (size_t)k * 64];
        zs += E_(r, fcold) * X_(r, fcold);
      }
      const float rj = epilogue(zs, c, true, pos);
      if (rj != 0.0f)
        for (uint32_t k = 0; k < len; ++k) {
          const uint32_t r = S.rec[base + (size_t)k * 64];
          add(r, rj * (E_(r, fcold) * X_(r, fcold)), c < narrow_c, fcold);
        }
    }
  };
  if constexpr (PRIME) stream.run(issue, process, [] {}, &first);
  else stream.run(issue, process, [] {});
  // long ECs (plain CSR): one wavefront per EC, a cell per lane and step
  for (uint32_t r = stream.s_first; r < S.n_long; r += stream.nw) {
    const uint32_t k0 = S.long_ptr[r], k1 = S.long_ptr[r + 1];
    float zs = 0.0f;
    for (uint32_t k = k0 + lane; k < k1; k += 64) {
      const uint32_t rc = S.rec_long[k];
      zs += E_(rc, fcold) * X_(rc, fcold);
    }
    zs = wave_sum_f(zs);
    const float c = (float)S.cvec[r];
    const float rj = epilogue(zs, c, lane == 0, r);
    if (rj != 0.0f)
      for (uint32_t k = k0 + lane; k < k1; k += 64) {
        const uint32_t rc = S.rec_long[k];
        add(rc, rj * (E_(rc, fcold) * X_(rc, fcold)), c < narrow_c, fcold);
      }
  }
  // guarded ECs (guard.hpp): pass B's evaluation in its fp32 form -- fp64 arithmetic (rare path) on float-rounded values
  __syncthreads();
  if (const uint32_t n_guard = gq.count()) {
    if (tid == 0) atomicAdd(GD.visits, (unsigned long long)n_guard);
    const double tref = uniform_d(sc->tref), p0d = uniform_d(sc->p0), tls = uniform_d(sc->fx_tscale);
    const uint32_t wv = uniform(tid >> 6);
    for (uint32_t i = wv; i < n_guard; i += NT / 64) {  // (the F32 form reads neither a nor logzi: 1.0, 0.0 stand in)
      guard_eval_B<ENC, true>(S, GD, gq.bits(wv), gq.entry(i), (uint32_t)lane, G, e_g, 1.0, tref, p0d, 0.0, tls,
                              [&](double c, double Z, double, double) { s_clogZ += c * log(Z); });
      __builtin_amdgcn_s_waitcnt(0);
    }
  }
  {
    double t3[3] = {s_clogZ, 0.0, s_W};
    block_sum_n<3>(t3, sh + 8);
    if (tid == 0) {
      partS[4 * blockIdx.x + 0] = t3[0];
      partS[4 * blockIdx.x + 1] = 0.0;
      partS[4 * blockIdx.x + 2] = t3[2];
      partS[4 * blockIdx.x + 3] = 0.0;
    }
  }
  __syncthreads();
  const double *al = reinterpret_cast<const double *>(smem + accoff);
  double *dst = partAcc + (size_t)blockIdx.x * G;
  for (uint32_t g = tid; g < G; g += NT) dst[g] = al[g];
}

template <bool ML>
__global__ __launch_bounds__(1024) void k_em_passB_f32(const Scalars *sc, SellDev S, const double *e_g, const float *e32_g,
                                                      const float *tab32_g, double *partAcc, double *partS, GuardDev GD) {
  extern __shared__ __align__(16) unsigned char smem[];
  em_passB_f32_body<kEncNarrow, ML>(smem, sc, S, e_g, e32_g, tab32_g, partAcc, partS, GD);
}
// index records (file header): tab32_g holds the whole slot area, S.n_area entries
template <bool ML>
__global__ __launch_bounds__(1024) void k_em_passB_f32_idx(const Scalars *sc, SellDev S, const double *e_g,
                                                          const float *e32_g, const float *tab32_g, double *partAcc,
                                                          double *partS, GuardDev GD) {
  extern __shared__ __align__(16) unsigned char smem[];
  em_passB_f32_body<kEncIndex, ML>(smem, sc, S, e_g, e32_g, tab32_g, partAcc, partS, GD);
}

}  // namespace msw
