"""CPU (hipcc cross-compiles without a GPU): the kernels host_likelihood_file.inc launches (likelihood_text_kernels.hpp: the
two passes over the text of a --read-likelihood file, the scatter of the host-converted cells, the transpose) run without
scratch memory -- the 40 bytes a thread holds and the token's 24 stay in registers, extracted by shifts -- and hold at most
16 KiB of LDS.  Compiled in a translation unit of its own, parsed as tests/test_inflate_member_kernel_resources.py parses."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "likelihood_text_kernels.hpp"
'''

KERNELS = ("k_lik_count", "k_lik_parse", "k_lik_scatter", "k_lik_transpose")


def test_likelihood_text_kernels_have_no_scratch_and_little_lds(tmp_path):
    res = compile_resources(TU, tmp_path, "liktext")
    # every kernel host_likelihood_file.inc launches is among those compiled here
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_likelihood_file.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS), launched
    for frag in launched | {"k_lik_gather"}:       # (k_lik_gather: compress_dense's background sample, host_compress.inc)
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == 1, (frag, sorted(res))
        for v in hit.values():
            print(frag, v)
            assert v["ScratchSize"] == 0, hit
            assert v["LDS Size"] <= 16 * 1024, hit
