"""CPU (hipcc cross-compiles without a GPU): the bin pass of --bin-reads (bin_kernels.hpp) runs without scratch -- every
instantiation msw_core_bin_reads launches (four record encodings x slot map in LDS or global memory, count and write
pass; the offsets and the scatter), compiled in a translation unit of their own as tests/test_kernel_resources.py does
for the sweeps."""
import os

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "bin_kernels.hpp"
using namespace msw;
#define P(ENC, LDS) \
  template __global__ void msw::k_bin_count<ENC, LDS>(SellDev, double, double, double, const double *, BinTargets, double *, uint32_t *); \
  template __global__ void msw::k_bin_write<ENC, LDS>(SellDev, double, double, const double *, BinTargets, const double *, const uint64_t *, uint32_t *, uint32_t *);
P(kEncNarrow, true) P(kEncNarrow, false) P(kEncWide, true) P(kEncWide, false)
P(kEncIndex, true) P(kEncIndex, false) P(kEncValue, true) P(kEncValue, false)
'''


def test_bin_kernels_have_no_scratch(tmp_path):
    res = {k: v["ScratchSize"] for k, v in compile_resources(TU, tmp_path, "bin").items()}
    for frag, n in (("k_bin_count", 8), ("k_bin_write", 8), ("k_bin_ptr", 1), ("k_bin_scatter", 1)):
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == n, (frag, sorted(res))
        assert all(v == 0 for v in hit.values()), hit
