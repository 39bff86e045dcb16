"""No GPU: what pass_threads_B_of (sweep_kernels.hpp) promises, read off the built library.  Every k_passB instantiation
compiled for 1024 threads -- 16 wavefronts per workgroup, four per SIMD -- must fit the 128 registers that leaves a lane
(AGPRs included) WITHOUT scratch: a spill inside the slice loop drains the record prefetch at every reload,
and the compiler adds one silently when an edit costs a few registers.

The figures are the code objects' own metadata (.max_flat_workgroup_size: the launch bound the host launches with;
.vgpr_count, .agpr_count, .private_segment_fixed_size), the ones tools/kernel_resources.py prints at compile time."""
import os
import re
import struct
import subprocess
import tempfile

from msweep_amd import buildlib

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """the gfx950 code objects of every translation unit's fat binary in the library"""
    data = open(lib, "rb").read()
    for m in re.finditer(MAGIC, data):
        b = m.start()
        (n,) = struct.unpack_from("<Q", data, b + len(MAGIC))
        p = b + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield data[b + off:b + off + size]


def kernel_metadata(elf):
    readelf = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(buildlib.hipcc()))), "llvm", "bin", "llvm-readelf")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        text = subprocess.run([readelf, "--notes", f.name], check=True, capture_output=True, text=True).stdout
    for block in re.split(r"\n  - (?=\.agpr_count:)", text)[1:]:
        def field(key, block=block):
            m = re.search(r"\n    \." + key + r":\s+(\S+)", "\n    " + block)
            assert m, (key, block[:200])
            return m.group(1)
        yield {"name": field("name"), "threads": int(field("max_flat_workgroup_size")), "vgpr": int(field("vgpr_count")),
               "agpr": int(field("agpr_count")), "scratch": int(field("private_segment_fixed_size"))}


def test_passB_at_16_wavefronts_fits_128_registers_without_scratch():
    assert os.path.exists(buildlib.LIB), "build the library first (__graft_entry__.build)"
    kernels = [k for elf in code_objects(buildlib.LIB) for k in kernel_metadata(elf)]
    passB = [k for k in kernels if re.match(r"_ZN3msw7k_passBI", k["name"])]
    # offset records: 5 GMODEs x table placement x (16 rows with and without multi-lane slices, 8 rows) and the rest
    assert len(passB) >= 30, f"{len(passB)} k_passB instantiations found among {len(kernels)} kernels"
    wave16 = [k for k in passB if k["threads"] == 1024]
    names = {k["name"] for k in wave16}
    for inst in ("Li0ELi1ELb1ELb0ELi16E", "Li0ELi1ELb1ELb1ELi16E", "Li0ELi2ELb1ELb0ELi16E", "Li0ELi2ELb1ELb1ELi16E",
                 "Li0ELi2ELb1ELb0ELi8E"):
        assert any(("k_passBI" + inst) in n for n in names), f"k_passB<{inst}> is not built for 1024 threads"
    for k in wave16:
        print(k)
        assert max(k["vgpr"], k["vgpr"] + k["agpr"] if k["agpr"] else 0) <= 128 and k["scratch"] == 0, k
