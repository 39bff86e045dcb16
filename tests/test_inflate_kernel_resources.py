"""CPU (hipcc cross-compiles without a GPU): the inflate kernels host_inflate.inc launches (inflate_kernels.hpp) -- the
probe, pass (a), the window chain, pass (b) -- and the CRC it borrows from the gzip kernels run without scratch memory and
hold at most 80 KiB of LDS per workgroup: the decode tables, the code lengths and the 32 Ki-entry rings live in LDS, the
probe keeps the code-length code in registers, and an indexed local array would show up here as scratch.  Compiled in a
translation unit of their own, as tests/test_deflate_kernel_resources.py does for the gzip kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "deflate_kernels.hpp"
#include "inflate_kernels.hpp"
'''

KERNELS = ("k_inf_probe", "k_inf_window", "k_inf_chain", "k_inf_write", "k_gz_crc")


def test_inflate_kernels_have_no_scratch_and_fit_lds(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "inf.hip"
    src.write_text(TU)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", os.path.join(ROOT, "msweep_amd", "csrc"),
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / "inf.o")],
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
    # every kernel host_inflate.inc launches is one of these
    inc = open(os.path.join(ROOT, "msweep_amd", "csrc", "host_inflate.inc")).read()
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", inc))
    assert launched == set(KERNELS), launched
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
