"""Developer timing of the matrix outputs with the text formatted on the device (msw_core_text_block, text_kernels.hpp)
against the host formatting of the same build (MSWEEP_HOST_TEXT=1): Themisto strands of `reads` reads x `groups` groups
(synth.write_themisto), output to a tmpfs path.
  - wall time of `--write-probs` and of `--write-likelihood --no-fit-model`, whole process, for msweep_mini and for
    `python -m msweep_amd`, device text and host text alternated in the same call, `reps` repeats each (min / median /
    max: the spread the comparison is read against);
  - the text calls alone, in process: per flavour the time of the msw_core_text_block calls over all classes
    (materialising the block, kernels, scan and the copy of the bytes to pinned host memory), the text kernels' own
    time from device events (msw_core_last_text_timing) and the bytes per second of both -- to be read against the D2H
    rate profiles/bin_timing.txt records, the floor of this path;
  - `big` (optional 4th argument, "reads,groups"): `msweep_mini --write-likelihood --no-fit-model` once at a shape whose
    dense G x E matrix is larger than the host memory this process may use, the file going to /dev/null through a
    symlink: what the flag could not do while it asked for the dense matrix.
usage: python tools/text_timing.py [reads] [groups] [reps] [big_reads,big_groups] [drivers: mini (default), py]
       (every child process is ended after MSWEEP_TEXT_CHILD_LIMIT seconds, 600 by default)
       (MSWEEP_PROBE_DIR keeps the generated strands; MSWEEP_TEXT_TMPFS: where strands and outputs go, /dev/shm by
       default; the native driver is built in the ordinary temporary directory)"""
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth
from msweep_amd.core import TEXT_BITSEQ, TEXT_LOGL, TEXT_PROBS, Core
from msweep_amd.reference import read_reference

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
BIG = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 and sys.argv[4] not in ("", "-") else None
# (the Python CLI's host side formats every cell in Python -- 10^9 of them at the default shape: ask for it by name, at a
# smaller shape)
DRIVERS = sys.argv[5].split(",") if len(sys.argv) > 5 else ["mini"]
CHILD_LIMIT = float(os.environ.get("MSWEEP_TEXT_CHILD_LIMIT", "600"))   # seconds a child process may take


def strands(tmp, reads, groups):
    f = [os.path.join(tmp, f"r1_{reads}_{groups}.txt"), os.path.join(tmp, f"r2_{reads}_{groups}.txt")]
    clus = os.path.join(tmp, f"clustering_{reads}_{groups}.txt")
    if not (os.path.exists(clus) and all(os.path.exists(x) for x in f)):
        t = time.perf_counter()
        prob = synth.make_csr_problem(reads, groups, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(f):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
        with open(clus, "w") as c:
            c.write("\n".join(f"g{int(g)}" for g in aln["target_group"]) + "\n")
        print(f"text of {reads} reads x {groups} groups generated in {time.perf_counter() - t:.1f} s", flush=True)
    return f, clus


def memory_limit():
    """bytes of host memory this process may use: the cgroup limit when there is one, else MemTotal"""
    total = os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES")
    try:
        v = open("/sys/fs/cgroup/memory.max").read().strip()
        if v != "max":
            total = min(total, int(v))
    except (OSError, ValueError):
        pass
    return total


def stats(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.3f} s, median {ts[len(ts) // 2]:.3f} s, max {ts[-1]:.3f} s"


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_text_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
os.makedirs(tmp, exist_ok=True)
try:
    f, clus = strands(tmp, R, G)
    lib = os.path.join(ROOT, "msweep_amd")
    bin_dir = tempfile.mkdtemp(prefix="msweep_text_bin_")     # (a tmpfs such as /dev/shm is usually mounted noexec)
    mini = os.path.join(bin_dir, "msweep_mini")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", mini, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    common = ["--themisto-1", f[0], "--themisto-2", f[1], "-i", clus]
    drivers = {"mini": [mini], "py": [sys.executable, "-m", "msweep_amd"]}
    out = os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)
    env0 = {**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")}
    env0.pop("MSWEEP_HOST_TEXT", None)

    # ---- whole processes: device text against host text, alternated
    for name in DRIVERS:
        for flags, produced in ((["--write-probs"], "probs.tsv"), (["--write-likelihood", "--no-fit-model"], "likelihoods.tsv")):
            walls = {"device": [], "host": []}
            size = {}
            for rep in range(REPS):
                for side in ("device", "host"):
                    env = dict(env0, **({"MSWEEP_HOST_TEXT": "1"} if side == "host" else {}))
                    t = time.perf_counter()
                    p = subprocess.run(drivers[name] + common + ["-o", os.path.join(out, side)] + flags, capture_output=True,
                                       text=True, env=env, cwd=ROOT, timeout=CHILD_LIMIT)
                    walls[side].append(time.perf_counter() - t)
                    assert p.returncode == 0, p.stderr[-1000:]
                    size[side] = os.path.getsize(os.path.join(out, f"{side}_{produced}"))
            print(f"{name} {' '.join(flags)} (R={R} G={G}, {size['device'] / 1e6:.1f} MB of text, {REPS} repeats alternated): "
                  f"device text {stats(walls['device'])}; host text {stats(walls['host'])}; "
                  f"files of equal size: {size['device'] == size['host']}", flush=True)

    # ---- the text calls alone
    grouping = read_reference(open(clus))
    with Core(0) as core:
        a = core.read_alignment(f, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        core.solve(None, np.ones(kept))
        E = a.n_ecs
        counts = a.ec_counts()
        block = max(1, min(8192, (256 << 20) // (20 + 14 * kept + 12)))
        import ctypes as C
        L = core._L
        p, n, nh = C.c_void_p(), C.c_size_t(), C.c_size_t()
        for label, what in (("PROBS", TEXT_PROBS), ("LOGL", TEXT_LOGL), ("BITSEQ", TEXT_BITSEQ)):
            best = None
            for rep in range(3):
                nbytes, host_cells, kernel_ms = 0, 0, 0.0
                t = time.perf_counter()
                for e0 in range(0, E, block):
                    e1 = min(E, e0 + block)
                    pre = counts[e0:e1].ctypes.data_as(C.c_void_p) if what == TEXT_LOGL else None
                    core._check(L.msw_core_text_block(core._h, what, e0, e1, pre, 0, C.byref(p), C.byref(n), C.byref(nh)))
                    nbytes += n.value
                    host_cells += nh.value
                    kernel_ms += core.last_text_timing()[0]
                dt = time.perf_counter() - t
                best = (dt, kernel_ms) if best is None else min(best, (dt, kernel_ms))
            dt, kernel_ms = best
            print(f"msw_core_text_block {label}: E={E} G={kept} in blocks of {block} classes: {nbytes / 1e6:.1f} MB in "
                  f"{dt * 1e3:.1f} ms = {nbytes / dt / 1e9:.2f} GB/s of text in pinned host memory "
                  f"({kept * E / dt / 1e9:.2f} G cells/s); the text kernels alone (length pass, scan, write pass; device "
                  f"events) {kernel_ms:.1f} ms = {nbytes / (kernel_ms * 1e-3) / 1e9:.1f} GB/s; "
                  f"{host_cells} cells formatted by the host", flush=True)

    # ---- --write-likelihood where the dense matrix does not fit the host
    if BIG:
        fb, clusb = strands(tmp, BIG[0], BIG[1])
        os.symlink("/dev/null", os.path.join(out, "big_likelihoods.tsv"))
        t = time.perf_counter()
        p = subprocess.run([mini, "--themisto-1", fb[0], "--themisto-2", fb[1], "-i", clusb, "-o", os.path.join(out, "big"),
                            "--write-likelihood", "--no-fit-model", "--verbose"], capture_output=True, text=True, env=env0,
                           timeout=CHILD_LIMIT)
        dt = time.perf_counter() - t
        assert p.returncode == 0, p.stderr[-1000:]
        with Core(0) as core:
            a = core.read_alignment(fb, len(read_reference(open(clusb)).group_indicators))
            Eb = a.n_ecs
        dense = 8 * Eb * BIG[1]
        print(f"msweep_mini --write-likelihood --no-fit-model at R={BIG[0]} G={BIG[1]}: E={Eb}, the dense matrix would be "
              f"{dense / 1e9:.1f} GB, this process may use {memory_limit() / 1e9:.1f} GB of host memory "
              f"(exceeded: {dense > memory_limit()}); file to /dev/null, {dt:.1f} s wall (whole process)", flush=True)
finally:
    if "bin_dir" in globals():
        shutil.rmtree(bin_dir, ignore_errors=True)
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
