"""CPU (hipcc cross-compiles without a GPU): the text kernels of msw_core_text_block / msw_core_format_g6
(text_kernels.hpp) run without scratch -- every instantiation host_text.inc launches (the three flavours and the plain
one, length and write pass; the exp of the whole-block host path; k_text_close, which puts the cells the host printed
into a block, also within 80 KiB of LDS), compiled in a translation unit of their own as
tests/test_bin_kernel_resources.py does for the bin pass.  The "%g" routine keeps a cell's text in registers; an
indexed array of characters or digits would show up here as scratch."""
import os
import re

from kernel_resources import compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "text_kernels.hpp"
using namespace msw;
#define P(WHAT) \
  template __global__ void msw::k_text_len<WHAT>(TextJob, uint32_t *); \
  template __global__ void msw::k_text_write<WHAT>(TextJob, const uint64_t *, uint8_t *, TextHostCell *, uint32_t *, uint32_t);
P(kTextProbs) P(kTextLogl) P(kTextBitseq) P(kTextPlain)
'''


def test_text_kernels_have_no_scratch(tmp_path):
    full = compile_resources(TU, tmp_path, "text")
    res = {k: v["ScratchSize"] for k, v in full.items()}
    lds = {k: v["LDS Size"] for k, v in full.items()}
    # every kernel host_text.inc launches is one of these
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_text.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == {"k_text_len", "k_text_write", "k_text_exp", "k_text_close"}, launched
    for frag, n in (("k_text_len", 4), ("k_text_write", 4), ("k_text_exp", 1), ("k_text_close", 1)):
        hit = {k: v for k, v in res.items() if frag in k}
        assert len(hit) == n, (frag, sorted(res))
        assert all(v == 0 for v in hit.values()), hit
    close = [v for k, v in lds.items() if "k_text_close" in k]
    assert len(close) == 1 and close[0] <= 80 * 1024, close
