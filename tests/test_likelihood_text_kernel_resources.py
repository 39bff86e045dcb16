"""CPU (hipcc cross-compiles without a GPU): the kernels host_likelihood_file.inc launches (likelihood_text_kernels.hpp: the
two passes over the text of a --read-likelihood file, the scatter of the host-converted cells, the transpose) run without
scratch memory -- the 40 bytes a thread holds and the token's 24 stay in registers, extracted by shifts -- and hold at most
16 KiB of LDS.  Compiled in a translation unit of its own, parsed as tests/test_inflate_member_kernel_resources.py parses."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "likelihood_text_kernels.hpp"
'''

KERNELS = ("k_lik_count", "k_lik_parse", "k_lik_scatter", "k_lik_transpose")


def test_likelihood_text_kernels_have_no_scratch_and_little_lds(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "liktext.hip"
    src.write_text(TU)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", os.path.join(ROOT, "msweep_amd", "csrc"),
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "liktext.o")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
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
