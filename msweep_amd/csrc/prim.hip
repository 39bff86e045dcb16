// prim.hip -- translation unit of every rocPRIM call of the library: the scans, radix sorts and the select that build.hip,
// input.hip and output.hip need (host_api.hpp: prim_scan, prim_sort_pairs, prim_sort_keys, prim_unique).  rocPRIM's
// kernels are templates that are instantiated where they are called, and calls of different units share many of them
// (the look-back state of every 64-bit scan, the sort of 64-bit keys with 32-bit values): with all calls here, each is
// held by one code object.  Every function keeps rocPRIM's convention: tmp == nullptr only sets `bytes`.
// The argument types are the callers' (pointers to const and to non-const are different instantiations).
#include "host_api.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

MSW_UNIT_WARM(prim)

namespace {

// widening functor of the scans over 32-bit lengths
struct U32ToU64 {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};
struct OwnerBytes {
  __host__ __device__ uint64_t operator()(const InfOwner &o) const { return o.bytes; }
};

template <class It>
hipError_t scan_u64(void *tmp, size_t &bytes, It in, uint64_t *out, size_t n, hipStream_t st) {
  return rocprim::exclusive_scan(tmp, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), st);
}

}  // namespace

hipError_t msw::host::prim_scan(void *tmp, size_t &bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t st) {
  return scan_u64(tmp, bytes, rocprim::make_transform_iterator(in, U32ToU64{}), out, n, st);
}
hipError_t msw::host::prim_scan(void *tmp, size_t &bytes, uint32_t *in, uint64_t *out, size_t n, hipStream_t st) {
  return scan_u64(tmp, bytes, rocprim::make_transform_iterator(in, U32ToU64{}), out, n, st);
}
hipError_t msw::host::prim_scan(void *tmp, size_t &bytes, InfOwner *in, uint64_t *out, size_t n, hipStream_t st) {
  return scan_u64(tmp, bytes, rocprim::make_transform_iterator(in, OwnerBytes{}), out, n, st);
}
hipError_t msw::host::prim_scan(void *tmp, size_t &bytes, BinPairLen len, uint64_t *out, size_t n, hipStream_t st) {
  return scan_u64(tmp, bytes, rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), len), out, n, st);
}
hipError_t msw::host::prim_scan(void *tmp, size_t &bytes, FqLen len, uint64_t *out, size_t n, hipStream_t st) {
  return scan_u64(tmp, bytes, rocprim::make_transform_iterator(rocprim::counting_iterator<size_t>(0), len), out, n, st);
}

hipError_t msw::host::prim_sort_pairs(void *tmp, size_t &bytes, uint64_t *k, uint64_t *k2, uint32_t *v, uint32_t *v2, size_t n,
                                      unsigned bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, k, k2, v, v2, n, 0u, bits, st);
}
hipError_t msw::host::prim_sort_pairs(void *tmp, size_t &bytes, uint32_t *k, uint32_t *k2, uint32_t *v, uint32_t *v2, size_t n,
                                      unsigned bits, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, k, k2, v, v2, n, 0u, bits, st);
}
hipError_t msw::host::prim_sort_keys(void *tmp, size_t &bytes, uint64_t *k, uint64_t *k2, size_t n, unsigned bits, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, bytes, k, k2, n, 0u, bits, st);
}
hipError_t msw::host::prim_sort_keys(void *tmp, size_t &bytes, uint32_t *k, uint32_t *k2, size_t n, unsigned bits, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, bytes, k, k2, n, 0u, bits, st);
}

hipError_t msw::host::prim_unique(void *tmp, size_t &bytes, uint32_t *in, uint32_t *out, uint64_t *n_out, size_t n, hipStream_t st) {
  return rocprim::unique(tmp, bytes, in, out, n_out, n, rocprim::equal_to<uint32_t>(), st);
}
