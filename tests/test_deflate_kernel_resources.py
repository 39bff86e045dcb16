"""CPU (hipcc cross-compiles without a GPU): the gzip kernels host_gzip.inc launches (deflate_kernels.hpp) -- the parse,
the emit pass and the CRC -- run without scratch memory and hold at most 80 KiB of LDS per workgroup, so that two
workgroups fit a CU's 160 KiB (the closing of a text block's undecided cells, k_text_close, is a text kernel now and
held to the same bounds by tests/test_text_kernel_resources.py).  Compiled in a translation unit of their own, as
tests/test_text_kernel_resources.py does for the text kernels: the code-length builder and the canonical codes work in
areas that are passed in, and an indexed local array would show up here as scratch."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "deflate_kernels.hpp"
'''

KERNELS = ("k_gz_parse", "k_gz_emit", "k_gz_crc")


def test_gzip_kernels_have_no_scratch_and_fit_lds(tmp_path):
    res = compile_resources(TU, tmp_path, "gz")
    # every kernel host_gzip.inc launches is one of these
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_gzip.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS), launched
    for frag in KERNELS:
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == 1, (frag, sorted(res))
        for v in hit.values():
            assert v["ScratchSize"] == 0, hit
            assert v["LDS Size"] <= 80 * 1024, hit
    parse = next(v for k, v in res.items() if "k_gz_parse" in k)
    assert 3 * parse["LDS Size"] <= 160 * 1024          # three parses share a CU
