// host_api.hpp -- what the translation units of libmsweep_core.so call in one another.  Everything a
// unit defines stays in its anonymous namespace except the functions declared here, once, in a namespace of hidden
// visibility: none of them is part of the library's exported surface.  The comment behind each block names the unit
// (and the file of text) that defines it.
#pragma once
#include "handle.hpp"
#include "lds_grants.hpp"
#include "prim_ops.hpp"

namespace msw {
namespace host __attribute__((visibility("hidden"))) {

// room for `count` elements in b (kept when it has them already): a failure is "<who>: cannot allocate <bytes> bytes of
// device memory for <what>", the wording of every entry whose device memory grows with its input
template <class T>
void named_alloc(DevBuf<T> &b, size_t count, const char *who, const char *what) {
  if (b.p && count <= b.n) return;
  b.release();
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc((void **)&b.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.p = nullptr;
    throw Fail(std::string(who) + ": cannot allocate " + std::to_string(bytes) + " bytes of device memory for " + what);
  }
  b.n = std::max<size_t>(count, 1);
}

extern thread_local std::string g_create_error;  // msweep_core.hip: msw_last_error(null), msw_comm_last_error
// msweep_core.hip: the dynamic-LDS limit of `kernel` on the current device becomes at least `bytes` (lds_grants.hpp: one
// table for all handles, limits only rise)
void grant_dynamic_lds(const void *kernel, size_t bytes);

// ---- the sweeps, each beside the instantiations it launches --------------------------------------------------------
// sweep_narrow.hip, sweep_wide.hip, sweep_index.hip (index and value records): k_passA and k_passB of an encoding
void passA_narrow(const Resident &L, Solver &s);
void passB_narrow(const Resident &L, Solver &s);
void passA_wide(const Resident &L, Solver &s);
void passB_wide(const Resident &L, Solver &s);
void passA_index(const Resident &L, Solver &s);
void passB_index(const Resident &L, Solver &s);
// sweep_dense.hip: dense_kernels.hpp and em_f32_kernels.hpp
void dense_passA(const Resident &L, Solver &s);
void dense_passB(const Resident &L, Solver &s);
bool em_f32_layout_ok(const Resident &L, const Solver &s);
void em_f32_prep(const Resident &L, Solver &s);   // k_em_f32_prep (host_em.inc)
void em_passB_f32(const Resident &L, Solver &s);
void transpose_launch(dim3 grid, hipStream_t st, const double *src, size_t ld, int G, uint32_t E, double *dst);  // k_transpose

// ---- solve.hip ---------------------------------------------------------------------------------------------------
void alloc_solve_state(const Resident &L, Solver &s);  // host_solve.inc
void poll(Solver &s);
void minmax_launch(unsigned nb, hipStream_t st, const double *v, uint64_t n, int pairs, double *out);  // k_minmax

// ---- build.hip ---------------------------------------------------------------------------------------------------
void reset_likelihood(msw_core *h);  // host_likelihood.inc
void dense_from_stage(msw_core *h, const double *Lm, size_t ld, const double *stage, size_t G, size_t E);
void materialise_args(msw_core *h, bool gamma, MaterialiseArgs &m);
void materialise_block(msw_core *h, const MaterialiseArgs &m, bool gamma, size_t j0, size_t j1, double *buf);
// host_assign.inc: the (read id, EC) pairs of device-resident classes in a stable sort by id (k_assign_expand, a radix sort)
void reads_by_id(msw_core *h, const uint64_t *d_rptr, const uint32_t *d_reads, uint32_t E, uint64_t n_rows,
                 DevBuf<uint32_t> &id, DevBuf<uint32_t> &ec, const char *who);

// ---- input.hip ---------------------------------------------------------------------------------------------------
void lik_gather_launch(hipStream_t st, const double *src, const uint64_t *idx, uint32_t n, double *out);  // k_lik_gather

// ---- output.hip --------------------------------------------------------------------------------------------------
void pinned_reserve(PinnedBuf &B, size_t need, size_t keep);                          // host_text.inc
// host_gzip.inc: the gzip stream open on the handle, as msw_fastq_next_gzip (host_fastq.inc) appends to it
void gz_require_open(msw_core *h, const char *who);
void gz_return(msw_core *h, size_t used, const char **out, size_t *len);
size_t gz_compress_device(msw_core *h, const uint8_t *d, size_t n, size_t used);
size_t gz_compress_host(msw_core *h, const char *bytes, size_t n, size_t used);
size_t gz_host_deflate(msw_core *h, const char *p, size_t n, int flush, size_t used);
void gz_crc_launch(int n_cu, hipStream_t st, const uint8_t *text, uint64_t n, const uint32_t *pow8, uint32_t *crc);  // k_gz_crc

// ---- prim.hip: every rocPRIM call of the library, with rocPRIM's convention (tmp == nullptr only sets `bytes`) -------
// exclusive scans into 64-bit offsets: of 32-bit lengths (text, reader; the bin pass), of owners' byte counts, of a functor
hipError_t prim_scan(void *tmp, size_t &bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t st);
hipError_t prim_scan(void *tmp, size_t &bytes, uint32_t *in, uint64_t *out, size_t n, hipStream_t st);
hipError_t prim_scan(void *tmp, size_t &bytes, InfOwner *in, uint64_t *out, size_t n, hipStream_t st);
hipError_t prim_scan(void *tmp, size_t &bytes, BinPairLen len, uint64_t *out, size_t n, hipStream_t st);
hipError_t prim_scan(void *tmp, size_t &bytes, FqLen len, uint64_t *out, size_t n, hipStream_t st);
// stable radix sorts by the low `bits` bits of the keys
hipError_t prim_sort_pairs(void *tmp, size_t &bytes, uint64_t *k, uint64_t *k2, uint32_t *v, uint32_t *v2, size_t n, unsigned bits, hipStream_t st);
hipError_t prim_sort_pairs(void *tmp, size_t &bytes, uint32_t *k, uint32_t *k2, uint32_t *v, uint32_t *v2, size_t n, unsigned bits, hipStream_t st);
hipError_t prim_sort_keys(void *tmp, size_t &bytes, uint64_t *k, uint64_t *k2, size_t n, unsigned bits, hipStream_t st);
hipError_t prim_sort_keys(void *tmp, size_t &bytes, uint32_t *k, uint32_t *k2, size_t n, unsigned bits, hipStream_t st);
// the first of every run of equal values; their number to *n_out
hipError_t prim_unique(void *tmp, size_t &bytes, uint32_t *in, uint32_t *out, uint64_t *n_out, size_t n, hipStream_t st);

// ---- the first launch out of a unit loads its code object: msw_core_create makes all of them ------------
void warm_solve(hipStream_t st);
void warm_build(hipStream_t st);
void warm_input(hipStream_t st);
void warm_output(hipStream_t st);
void warm_prim(hipStream_t st);
void warm_sweep_narrow(hipStream_t st);
void warm_sweep_wide(hipStream_t st);
void warm_sweep_index(hipStream_t st);
void warm_sweep_dense(hipStream_t st);

}  // namespace host
}  // namespace msw

using namespace msw::host;

// a unit's no-op kernel and the launch of it
#define MSW_UNIT_WARM(unit)                                                                         \
  namespace msw {                                                                                   \
  namespace host __attribute__((visibility("hidden"))) {                                            \
  __global__ void k_warm_##unit(int *p) {                                                           \
    if (p) *p = 0;                                                                                  \
  }                                                                                                 \
  void warm_##unit(hipStream_t st) { hipLaunchKernelGGL(k_warm_##unit, dim3(1), dim3(1), 0, st, (int *)nullptr); } \
  }                                                                                                 \
  }

// MSW_STAMPS (diagnostic build only, common.hpp): g_stamps is a __device__ variable of a header and no device link step
// joins the units, so every unit that holds stamped kernels has a copy of its own; its kernels write their slots of it and
// the rest stays zero.  msw_debug_stamps (solve.hip) takes the newest stamp of every slot over the copies, and clears all.
#ifdef MSW_STAMPS
namespace msw {
namespace host __attribute__((visibility("hidden"))) {
void stamps_solve(unsigned long long *newest, int clear);
void stamps_sweep_narrow(unsigned long long *newest, int clear);
void stamps_sweep_wide(unsigned long long *newest, int clear);
void stamps_sweep_index(unsigned long long *newest, int clear);
}  // namespace host
}  // namespace msw
#define MSW_UNIT_STAMPS(unit)                                                                          \
  void msw::host::stamps_##unit(unsigned long long *newest, int clear) {                               \
    std::vector<unsigned long long> v(64 * 40, 0);                                                     \
    if (newest) {                                                                                      \
      MSW_HIP(hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(g_stamps), v.size() * sizeof(unsigned long long))); \
      for (size_t i = 0; i < v.size(); ++i) newest[i] = std::max(newest[i], v[i]);                     \
      std::fill(v.begin(), v.end(), 0ull);                                                             \
    }                                                                                                  \
    if (clear) MSW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), v.data(), v.size() * sizeof(unsigned long long))); \
  }
#else
#define MSW_UNIT_STAMPS(unit)
#endif
