"""CPU (hipcc cross-compiles without a GPU): the kernels of --write-unassigned / --write-assignment-table
(assign_kernels.hpp) run without scratch -- every instantiation msw_core_assign_reads and msw_core_assign_table_block can
launch (the assign pass: four record encodings x slot map in LDS or global memory, count and write; the class sums, the
position expansion, the table's length and write kernels), compiled in a translation unit of their own as
tests/test_bin_kernel_resources.py does for the bin pass."""
from kernel_resources import compile_resources

TU = r'''
#include "assign_kernels.hpp"
using namespace msw;
#define P(ENC, LDS) \
  template __global__ void msw::k_assign_count<ENC, LDS>(SellDev, double, double, double, const double *, AssignGroups, double *, uint32_t *, uint32_t *); \
  template __global__ void msw::k_assign_write<ENC, LDS>(SellDev, double, double, const double *, AssignGroups, const double *, const uint64_t *, uint32_t *, uint32_t *);
P(kEncNarrow, true) P(kEncNarrow, false) P(kEncWide, true) P(kEncWide, false)
P(kEncIndex, true) P(kEncIndex, false) P(kEncValue, true) P(kEncValue, false)
'''


def test_assign_kernels_have_no_scratch(tmp_path):
    res = {k: v["ScratchSize"] for k, v in compile_resources(TU, tmp_path, "assign").items()}
    for frag, n in (("k_assign_count", 8), ("k_assign_write", 8), ("k_assign_class_reads", 1), ("k_assign_expand", 1),
                    ("k_assign_table_len", 1), ("k_assign_table_write", 1)):
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == n, (frag, sorted(res))
        assert all(v == 0 for v in hit.values()), hit
    # the kernels the assign pass borrows from the bin pass, and no name of its own that would count as one of theirs
    for frag, n in (("k_bin_count", 0), ("k_bin_write", 0), ("k_bin_ptr", 1), ("k_bin_scatter", 1)):
        assert sum(frag in k for k in res) == n, (frag, sorted(res))
