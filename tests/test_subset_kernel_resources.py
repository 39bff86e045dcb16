"""CPU (hipcc cross-compiles without a GPU): the kernels of msw_alignment_subset (subset_kernels.hpp) run without scratch --
every instantiation host_subset.inc launches (the filter's two passes; the flags, hash, bitmap, mark, keys, meta and
rows kernels), compiled in a translation unit of their own as tests/test_assign_kernel_resources.py does for the assign
pass."""
from kernel_resources import compile_resources

TU = r'''
#include "subset_kernels.hpp"
using namespace msw;
template __global__ void msw::k_subset_filter<false>(const uint64_t *, const uint32_t *, uint64_t, const uint32_t *, const uint64_t *, uint32_t *, const uint64_t *, uint32_t *);
template __global__ void msw::k_subset_filter<true>(const uint64_t *, const uint32_t *, uint64_t, const uint32_t *, const uint64_t *, uint32_t *, const uint64_t *, uint32_t *);
'''


def test_subset_kernels_have_no_scratch(tmp_path):
    res = {k: v["ScratchSize"] for k, v in compile_resources(TU, tmp_path, "subset").items()}
    for frag, n in (("k_subset_filter", 2), ("k_subset_keep_flags", 1), ("k_subset_hash", 1), ("k_subset_bitmap", 1),
                    ("k_subset_mark", 1), ("k_subset_keys", 1), ("k_subset_meta", 1), ("k_subset_rows", 1)):
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == n, (frag, sorted(res))
        assert all(v == 0 for v in hit.values()), hit
    # every kernel the header defines is named above, and the one it borrows from the reader is there too
    assert sum("k_subset_" in k for k in res) == 9, sorted(res)
    assert sum("k_ec_heads" in k for k in res) == 1, sorted(res)
