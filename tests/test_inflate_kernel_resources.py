"""CPU (hipcc cross-compiles without a GPU): the inflate kernels host_inflate.inc launches (inflate_kernels.hpp) -- the
probe, pass (a), the window chain, pass (b) -- and the CRC it borrows from the gzip kernels run without scratch memory and
hold at most 80 KiB of LDS per workgroup: the decode tables, the code lengths and the 32 Ki-entry rings live in LDS, the
probe keeps the code-length code in registers, and an indexed local array would show up here as scratch.  Compiled in a
translation unit of their own, as tests/test_deflate_kernel_resources.py does for the gzip kernels."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "deflate_kernels.hpp"
#include "inflate_kernels.hpp"
'''

KERNELS = ("k_inf_probe", "k_inf_window", "k_inf_chain", "k_inf_write", "k_gz_crc")


def test_inflate_kernels_have_no_scratch_and_fit_lds(tmp_path):
    res = compile_resources(TU, tmp_path, "inf")
    # every kernel host_inflate.inc launches is one of these; the CRC it reaches through gz_crc_launch of the output
    # unit, whose launch of k_gz_crc tests/test_deflate_kernel_resources.py pins over host_gzip.inc
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_inflate.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS) - {"k_gz_crc"}, launched
    assert re.search(r"^\s*gz_crc_launch\(", inc, re.M), "host_inflate.inc no longer checks its text's CRC on the device"
    gz = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_gzip.inc")).read()
    body = gz[gz.index("void msw::host::gz_crc_launch("):]
    assert re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", body[:body.index("\n}\n")]) == ["k_gz_crc"]
    for frag in KERNELS:
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == 1, (frag, sorted(res))
        for v in hit.values():
            assert v["ScratchSize"] == 0, hit
            assert v["LDS Size"] <= 80 * 1024, hit
    # two owners of pass (a) and four of pass (b) share a CU's 160 KiB
    window = next(v for k, v in res.items() if "k_inf_window" in k)
    write = next(v for k, v in res.items() if "k_inf_write" in k)
    assert 2 * window["LDS Size"] <= 160 * 1024 and 4 * write["LDS Size"] <= 160 * 1024
