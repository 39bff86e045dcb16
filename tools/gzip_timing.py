"""Developer timing of --compress z: the gzip stream of the text outputs compressed on the device (msw_core_gzip_*,
deflate_kernels.hpp) against zlib on the host behind the same calls (MSWEEP_HOST_GZIP=1, the reference's method) and
against the plain file: Themisto strands of `reads` reads x `groups` groups (synth.write_themisto), output to a tmpfs path.
  - wall time of `msweep_mini --write-probs`, whole process: plain, `--compress z` on the device, and zlib on the host at
    the `levels` asked for, alternated in the same call, `reps` repeats each (min / median / max); the size of every
    file, so the device's ratio stands beside zlib's at those levels on the same text; every `.gz` is read back with
    Python's gzip and compared with the plain file once;
  - the gzip calls alone, in process: msw_core_text_block_gzip over all classes, the time of the calls, the gzip
    kernels' own time from device events (msw_core_last_gzip_timing: parse, CRC, scan, emit) and the bytes per second of
    text of both.
usage: python tools/gzip_timing.py [reads] [groups] [reps] [levels, e.g. 1,6] [reps of the zlib levels above 1]
       (zlib level 6 takes minutes per run at the default shape: its repeats can be fewer, and the output says how many)
       (every child process is ended after MSWEEP_GZIP_CHILD_LIMIT seconds, 600 by default)
       (MSWEEP_PROBE_DIR keeps the generated strands; MSWEEP_TEXT_TMPFS: where strands and outputs go, /dev/shm by
       default; the native driver is built in the ordinary temporary directory)"""
import gzip, hashlib, os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth
from msweep_amd.core import TEXT_PROBS, Core
from msweep_amd.reference import read_reference

R = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
LEVELS = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 6]
REPS_SLOW = int(sys.argv[5]) if len(sys.argv) > 5 else REPS
CHILD_LIMIT = float(os.environ.get("MSWEEP_GZIP_CHILD_LIMIT", "600"))   # seconds a child process may take


def strands(tmp, reads, groups):
    f = [os.path.join(tmp, f"r1_{reads}_{groups}.txt"), os.path.join(tmp, f"r2_{reads}_{groups}.txt")]
    clus = os.path.join(tmp, f"clustering_{reads}_{groups}.txt")
    if not (os.path.exists(clus) and all(os.path.exists(x) for x in f)):
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
    return f, clus


def stats(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.3f} s, median {ts[len(ts) // 2]:.3f} s, max {ts[-1]:.3f} s"


def digest(stream):
    h, n = hashlib.sha256(), 0
    while True:
        b = stream.read(1 << 24)
        if not b:
            return h.hexdigest(), n
        h.update(b)
        n += len(b)


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_gzip_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
os.makedirs(tmp, exist_ok=True)
try:
    f, clus = strands(tmp, R, G)
    lib = os.path.join(ROOT, "msweep_amd")
    bin_dir = tempfile.mkdtemp(prefix="msweep_gzip_bin_")     # (a tmpfs such as /dev/shm is usually mounted noexec)
    mini = os.path.join(bin_dir, "msweep_mini")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", mini, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    common = ["--themisto-1", f[0], "--themisto-2", f[1], "-i", clus, "--write-probs"]
    out = os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)
    env0 = dict(os.environ)
    for k in ("MSWEEP_HOST_TEXT", "MSWEEP_HOST_GZIP", "MSWEEP_TEXT_BLOCK"):
        env0.pop(k, None)

    # ---- whole processes, alternated
    sides = {"plain": ([], {}), "device": (["--compress", "z"], {})}
    for lv in LEVELS:
        sides[f"zlib-{lv}"] = (["--compress", "z", "--compression-level", str(lv)], {"MSWEEP_HOST_GZIP": "1"})
    walls = {s: [] for s in sides}
    size = {}
    for rep in range(REPS):
        for side, (flags, env) in sides.items():
            if side.startswith("zlib-") and side != "zlib-1" and rep >= REPS_SLOW:
                continue
            t = time.perf_counter()
            p = subprocess.run([mini] + common + ["-o", os.path.join(out, side)] + flags, capture_output=True, text=True,
                               env=dict(env0, **env), cwd=ROOT, timeout=CHILD_LIMIT)
            walls[side].append(time.perf_counter() - t)
            assert p.returncode == 0, p.stderr[-1000:]
            size[side] = os.path.getsize(os.path.join(out, f"{side}_probs.tsv" + ("" if side == "plain" else ".gz")))
    with open(os.path.join(out, "plain_probs.tsv"), "rb") as fh:
        want = digest(fh)
    same = {}
    for side in sides:
        if side != "plain":
            with gzip.open(os.path.join(out, f"{side}_probs.tsv.gz"), "rb") as fh:
                same[side] = digest(fh) == want
    print(f"msweep_mini --write-probs (R={R} G={G}, {size['plain'] / 1e6:.1f} MB of text, {REPS} repeats alternated; zlib above level 1: {REPS_SLOW}):", flush=True)
    for side in sides:
        note = "" if side == "plain" else f", ratio {size[side] / size['plain']:.4f}, gzip reads it back to the plain file: {same[side]}"
        print(f"  {side:8s} {stats(walls[side])}; {size[side] / 1e6:.1f} MB{note}", flush=True)
    med = {s: sorted(w)[len(w) // 2] for s, w in walls.items()}
    if "zlib-1" in med:
        print(f"  device against zlib level 1, median wall: {med['zlib-1'] / med['device']:.2f} x "
              f"({'faster' if med['device'] < med['zlib-1'] else 'NOT faster'})", flush=True)

    # ---- the gzip calls alone
    grouping = read_reference(open(clus))
    with Core(0) as core:
        a = core.read_alignment(f, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        core.solve(None, np.ones(kept))
        E = a.n_ecs
        block = max(1, min(8192, (256 << 20) // (20 + 14 * kept + 12)))
        best = None
        for rep in range(3):
            t = time.perf_counter()
            n_out = len(core.gzip_begin(6))
            for e0 in range(0, E, block):
                n_out += len(core.text_block_gzip(TEXT_PROBS, e0, min(E, e0 + block)))
            n_out += len(core.gzip_end())
            dt = time.perf_counter() - t
            ms, n_in, n_o = core.last_gzip_timing()
            assert n_o == n_out
            best = (dt, ms, n_in, n_out) if best is None else min(best, (dt, ms, n_in, n_out))
        dt, ms, n_in, n_out = best
        print(f"msw_core_text_block_gzip PROBS: E={E} G={kept} in blocks of {block} classes: {n_in / 1e6:.1f} MB of text -> "
              f"{n_out / 1e6:.1f} MB (ratio {n_out / n_in:.4f}) in {dt * 1e3:.1f} ms = {n_in / dt / 1e9:.2f} GB/s of text, "
              f"text kernels and copy included; the gzip kernels alone (parse, CRC, scan, emit; device events) {ms:.1f} ms = "
              f"{n_in / (ms * 1e-3) / 1e9:.2f} GB/s of text", flush=True)
finally:
    if "bin_dir" in globals():
        shutil.rmtree(bin_dir, ignore_errors=True)
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
