"""CPU (hipcc cross-compiles without a GPU): the kernels host_fastq.inc launches (fastq_kernels.hpp: the record index, the
validation and the gather of --extract-reads) run without scratch memory -- the gather assembles the 16 bytes of a vector
that crosses a record end in four registers, and an indexed local array would show up here as scratch -- and hold a few
words of LDS at most.  Compiled in a translation unit of their own, as tests/test_deflate_kernel_resources.py does."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "fastq_kernels.hpp"
'''

KERNELS = ("k_fq_count", "k_fq_index", "k_fq_validate", "k_fq_gather")


def test_fastq_kernels_have_no_scratch(tmp_path):
    res = compile_resources(TU, tmp_path, "fq")
    # every kernel host_fastq.inc launches is one of these
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_fastq.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS), launched
    for frag in KERNELS:
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == 1, (frag, sorted(res))
        for v in hit.values():
            assert v["ScratchSize"] == 0, hit
            assert v["LDS Size"] <= 64, hit
