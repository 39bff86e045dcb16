"""CPU (hipcc cross-compiles without a GPU): the kernels of --write-read-probs (sparse_probs_kernels.hpp) run without
scratch -- every instantiation msw_core_sparse_probs_begin / _next can launch (the count and the write pass for the four
record encodings; the group order, the rows, the two one-thread searches, the length and the text kernels), compiled in a
translation unit of their own as tests/test_assign_kernel_resources.py does for the assign pass.  k_text_close, which puts
the host-printed cells in, is text_kernels.hpp's and is counted here because the header brings it along."""
from kernel_resources import compile_resources

TU = r'''
#include "sparse_probs_kernels.hpp"
using namespace msw;
#define P(ENC) \
  template __global__ void msw::k_sp_count<ENC>(SellDev, SpRule, double, double *, uint32_t *, uint32_t *); \
  template __global__ void msw::k_sp_write<ENC>(SellDev, SpRule, const uint32_t *, const double *, const uint32_t *, const uint64_t *, \
                                                uint64_t, uint32_t, uint64_t *, uint32_t *, double *);
P(kEncNarrow) P(kEncWide) P(kEncIndex) P(kEncValue)
'''


def test_sparse_probs_kernels_have_no_scratch(tmp_path):
    res = {k: v["ScratchSize"] for k, v in compile_resources(TU, tmp_path, "sparse_probs").items()}
    for frag, n in (("k_sp_count", 4), ("k_sp_write", 4), ("k_sp_order_keys", 1), ("k_sp_gather", 1), ("k_sp_rows", 1), ("k_sp_span", 1),
                    ("k_sp_len", 1), ("k_sp_cut", 1), ("k_sp_text", 1), ("k_text_close", 1)):
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == n, (frag, sorted(res))
        assert all(v == 0 for v in hit.values()), hit
