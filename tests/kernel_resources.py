"""Shared by the tests/test_*kernel_resources*.py files: compile a translation unit of kernels for gfx950 (hipcc
cross-compiles without a GPU) and read what `-Rpass-analysis=kernel-resource-usage` reports for every kernel in it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_resources(tu, tmp_path, stem):
    """{mangled kernel name: {"VGPRs" | "SGPRs" | "ScratchSize" | "LDS Size" | "Occupancy" | ...: value}} of the kernels the
    text `tu` defines or instantiates; the keys are the remark's field names without their unit."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / (stem + ".hip")
    src.write_text(tu)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I", os.path.join(ROOT, "msweep_amd", "csrc"),
                        "-Rpass-analysis=kernel-resource-usage", str(src), "-o", str(tmp_path / (stem + ".o"))],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur:
            res[cur][m.group(1)] = int(m.group(2))
    return res
