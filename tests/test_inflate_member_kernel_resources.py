"""CPU (hipcc cross-compiles without a GPU): the member decode host_inflate_members.inc launches
(inflate_member_kernels.hpp: a wavefront per BGZF member, the trailer check fused into it) runs without scratch memory and
holds so little LDS -- the decode tables, the code lengths and the 8-bit 32 KiB ring -- that four workgroups share a CU's
160 KiB.  Compiled in a translation unit of its own, parsed as tests/test_inflate_kernel_resources.py parses."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "inflate_member_kernels.hpp"
'''

KERNELS = ("k_infm_decode",)


def test_member_kernels_have_no_scratch_and_four_fit_a_cu(tmp_path):
    res = compile_resources(TU, tmp_path, "infm")
    # every kernel host_inflate_members.inc launches is one of these, and it launches them with one wavefront a workgroup
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_inflate_members.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS), launched
    assert re.search(r"hipLaunchKernelGGL\(k_infm_decode, dim3\(n_members\), dim3\(kWave\)", inc)
    for frag in KERNELS:
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == 1, (frag, sorted(res))
        for v in hit.values():
            print(frag, v)
            assert v["ScratchSize"] == 0, hit
            assert 32768 < v["LDS Size"] and 4 * v["LDS Size"] <= 160 * 1024, hit
