"""CPU (hipcc cross-compiles without a GPU): the text kernels of msw_core_text_block / msw_core_format_g6
(text_kernels.hpp) run without scratch -- every instantiation host_text.inc launches (the three flavours and the plain
one, length and write pass; the exp of the whole-block host path; k_text_close, which puts the cells the host printed
into a block, also within 80 KiB of LDS), compiled in a translation unit of their own as
tests/test_bin_kernel_resources.py does for the bin pass.  The "%g" routine keeps a cell's text in registers; an
indexed array of characters or digits would show up here as scratch."""
import os
import re
import subprocess

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
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "text.hip"
    src.write_text(TU)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", os.path.join(ROOT, "msweep_amd", "csrc"),
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "text.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res, lds, cur = {}, {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and cur:
            res[cur] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", ln)
        if m and cur:
            lds[cur] = int(m.group(1))
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
