"""How libmsweep_core.so is built: its translation units, the flags, the hash of its sources and one build function.
Pure Python, no ctypes: __graft_entry__.build(), core.source_hash and tools/ab_build.py all come here.

The units are compiled in parallel with `-c -MD` into objects under build/ and then linked.  Staleness is judged by
CONTENT, never by mtime: an object is stale when the hash over its flags and the contents of the files its depfile names
differs from the hash stored beside it.  The whole-library rule stands above that: the .so carries the hash of all
sources (msw_core_version()), and a library that does not is rebuilt, never used."""
import hashlib
import os
import re
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msweep_amd", "csrc")
LIB = os.path.join(ROOT, "msweep_amd", "libmsweep_core.so")
ABI_UNIT = "msweep_core"    # the only unit that sees MSW_SRC_HASH
# longest first: the pool starts them in this order
UNITS = ["sweep_index", "sweep_narrow", "sweep_wide", "input", "build", "prim", "output", "sweep_dense", "solve", ABI_UNIT]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# Pass B's 16-row kernel over offset records at 16 wavefronts per workgroup (common.hpp MSW_PASS_THREADS_B16: kernels, launches
# and layout_info follow the one constant, so every unit sees it) goes with its unit compiled without machine-level
# loop-invariant hoisting: hoisted constants cost the kernel 20 registers (143 -> 123) and, under the 128 of 16 wavefronts, scratch
# (tests/test_passB_wave16_resources.py holds the built code objects to 128 registers and no scratch).
WAVE16_FLAGS = ["-DMSW_PASS_THREADS_B16=1024"]
UNIT_FLAGS = {"sweep_narrow": ["-mllvm", "-disable-machine-licm"]}
LINK = ["-L/opt/rocm/lib", "-lrccl", "-lz", "-Wl,-rpath,/opt/rocm/lib"]
MAX_JOBS = 16


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def source_hash():
    """sha256 over every source the library is compiled from (file names and contents): what msw_core_version() of an
    up-to-date build reports."""
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".inc", ".h")))
    for f in files + [os.path.join(ROOT, "include", "msweep_core.h")]:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def built_hash(lib):
    """The source hash a built library carries (None: missing, unreadable or built before hashes)."""
    try:
        data = open(lib, "rb").read()
    except OSError:
        return None
    m = re.search(rb"msweep_core [0-9.]+ gfx950 \(HIP, wave64\) src ([0-9a-f]{16})", data)
    return m.group(1).decode() if m else None


def cpu_share():
    """CPUs this process may really use: the cgroup quota when there is one, else the affinity mask (never the
    machine's CPU count: a GPU box shows all of its CPUs and grants a share)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def job_count(n_units, jobs=None):
    """min(units, CPU share, MAX_JOBS of the environment when set, `jobs` when given), and never more than 16."""
    n = min(n_units, cpu_share(), MAX_JOBS)
    env = os.environ.get("MAX_JOBS")
    if env and env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    if jobs:
        n = min(n, int(jobs))
    return max(1, n)


def depfile_names(path):
    """The prerequisites a make-style depfile names (None: no readable depfile)."""
    try:
        text = open(path).read()
    except OSError:
        return None
    text = text.replace("\\\n", " ")
    names = []
    for rule in text.splitlines():
        if ":" in rule:
            names += [n.replace("\\ ", " ") for n in re.split(r"(?<!\\)\s+", rule.split(":", 1)[1].strip()) if n]
    return names


def unit_hash(flags, names, cwd):
    """Hash over a unit's flags and the contents of the files it was compiled from (None: one of them is gone)."""
    h = hashlib.sha256("\0".join(flags).encode() + b"\0\0")
    for n in sorted(set(names)):
        try:
            h.update(n.encode() + b"\0" + hashlib.sha256(open(os.path.join(cwd, n), "rb").read()).digest())
        except OSError:
            return None
    return h.hexdigest()


def is_stale(obj, flags, cwd=CSRC):
    """obj + '.d' is the depfile, obj + '.hash' the hash stored by record()."""
    names = depfile_names(obj + ".d")
    if names is None or not os.path.exists(obj):
        return True
    try:
        stored = open(obj + ".hash").read().strip()
    except OSError:
        return True
    return unit_hash(flags, names, cwd) != stored


def record(obj, flags, cwd=CSRC):
    h = unit_hash(flags, depfile_names(obj + ".d") or [], cwd)
    with open(obj + ".hash", "w") as f:
        f.write(h or "")


def unit_flags(unit, extra_flags, src_hash):
    return (FLAGS + WAVE16_FLAGS + UNIT_FLAGS.get(unit, []) + list(extra_flags)
            + ([f'-DMSW_SRC_HASH="{src_hash}"'] if unit == ABI_UNIT else []))


def build_library(out=LIB, extra_flags=(), jobs=None, build_dir=None, log=None):
    """Compile the stale units (in parallel) and link `out`.  Returns {unit compiled: seconds it took}."""
    build_dir = build_dir or os.path.join(ROOT, "build")
    os.makedirs(build_dir, exist_ok=True)
    want = source_hash()
    obj = {u: os.path.join(build_dir, u + ".o") for u in UNITS}
    flags = {u: unit_flags(u, extra_flags, want) for u in UNITS}
    todo = [u for u in UNITS if is_stale(obj[u], flags[u])]

    def compile_unit(u):
        t0 = time.time()
        cmd = [hipcc(), *flags[u], "-c", "-MD", "-MF", obj[u] + ".d", "-o", obj[u], u + ".hip"]
        r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if log:
            log(u, r.stdout)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-4000:]}")
        if source_hash() == want:   # (a source edited during the compile: no hash is stored, the object stays stale)
            record(obj[u], flags[u])
        return time.time() - t0

    took = {}
    if todo:
        with ThreadPoolExecutor(job_count(len(todo), jobs)) as pool:
            took = dict(zip(todo, pool.map(compile_unit, todo)))
    if source_hash() != want:
        raise RuntimeError("the sources changed during the build: build again")
    if todo or built_hash(out) != want:
        subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *[obj[u] for u in UNITS], *LINK],
                              cwd=ROOT)
    if built_hash(out) != want:
        raise RuntimeError(f"{out} does not carry the hash of its sources after the build")
    return took
