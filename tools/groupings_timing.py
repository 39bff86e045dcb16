"""Developer timing of the grouping loop: ONE `msweep_mini` process over a three-column -i file (one read of the
pseudoalignment, three builds / solves on the one handle) against THREE `msweep_mini` processes over the three
single-column files -- the only way to get the three results before the loop existed, and the baseline.  Same box,
sides alternated inside every repeat, after one unmeasured pass.
Workload: cfg3's synthetic reads (synth.make_csr_problem(reads, groups, seed=2) written as two Themisto strands, as
tools/bin_timing.py writes them) with the columns
  0  the `groups` groups the reads were drawn from,
  1  a coarser grouping: ten consecutive groups of column 0 each,
  2  every reference sequence a group of its own (--fine N: N consecutive sequences each instead).
Every run writes abundances only (`-o`); the files of the two sides are compared byte for byte in every repeat.
min / median / max of `reps` repeats; the verdict compares medians beside the larger spread.
usage: python tools/groupings_timing.py [reads] [groups] [reps] [--mini PATH] [--fine N]
       (MSWEEP_PROBE_DIR keeps the generated strands; MSWEEP_TEXT_TMPFS: where they go otherwise, /dev/shm by default)"""
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth

ARGS = list(sys.argv[1:])
opt = lambda name: ARGS[ARGS.index(name) + 1] if name in ARGS else None
MINI, FINE = opt("--mini"), int(opt("--fine") or 1)
NUMS = [a for k, a in enumerate(ARGS) if a.isdigit() and (k == 0 or ARGS[k - 1] not in ("--fine", "--mini"))]
R = int(NUMS[0]) if len(NUMS) > 0 else 10_000_000
G = int(NUMS[1]) if len(NUMS) > 1 else 5000
REPS = int(NUMS[2]) if len(NUMS) > 2 else 5


def stats(ts):
    ts = sorted(ts)
    return f"min {ts[0]:.3f} s, median {ts[len(ts) // 2]:.3f} s, max {ts[-1]:.3f} s"


def median(ts):
    return sorted(ts)[len(ts) // 2]


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_groupings_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
os.makedirs(tmp, exist_ok=True)
bin_dir = None
try:
    strands = [os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt")]
    multi = os.path.join(tmp, "groupings.tsv")
    single = [os.path.join(tmp, f"column{k}.txt") for k in range(3)]
    if not all(os.path.exists(x) for x in strands + [multi] + single):
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(strands):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
        tg = aln["target_group"].astype(np.int64)
        cols = [[f"g{g}" for g in tg], [f"c{g // 10}" for g in tg], [f"s{i // FINE}" for i in range(len(tg))]]
        with open(multi, "w") as f:
            f.write("".join(f"{a}\t{b}\t{c}\n" for a, b, c in zip(*cols)))
        for path, col in zip(single, cols):
            with open(path, "w") as f:
                f.write("\n".join(col) + "\n")
        del prob, aln, ec_of, cols
        print(f"text generated in {time.perf_counter() - t:.1f} s", flush=True)
    n_seq = sum(1 for _ in open(multi))
    n_groups = [len(set(open(p).read().split("\n")[:-1])) for p in single]
    print(f"cfg3 text: R={R}: strands of {os.path.getsize(strands[0]) / 1e9:.2f} + {os.path.getsize(strands[1]) / 1e9:.2f} GB, "
          f"{n_seq} reference sequences; groups per column: {n_groups[0]} / {n_groups[1]} / {n_groups[2]}; "
          f"{REPS} repeats, sides alternated", flush=True)
    if not MINI:
        lib = os.path.join(ROOT, "msweep_amd")
        bin_dir = tempfile.mkdtemp(prefix="msweep_groupings_bin_")      # (not beside the text: /dev/shm may be mounted noexec)
        MINI = os.path.join(bin_dir, "msweep_mini")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", MINI, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                               "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = os.path.join(tmp, "out")
    os.makedirs(out, exist_ok=True)

    def run(indicators, prefix):
        t1 = time.perf_counter()
        p = subprocess.run([MINI, "--themisto-1", strands[0], "--themisto-2", strands[1], "-i", indicators, "-o", os.path.join(out, prefix)],
                           capture_output=True, text=True)
        dt = time.perf_counter() - t1
        assert p.returncode == 0, p.stderr[-2000:]
        return dt

    times = {"one process, three columns": [], "three processes, one column each": []}
    per_column = [[], [], []]
    for rep in range(-1, REPS):      # (-1: unmeasured; page cache, allocator and clocks warm for both sides)
        order = ("multi", "single") if rep % 2 else ("single", "multi")
        for side in order:
            if side == "multi":
                dt = run(multi, "M")
                if rep >= 0:
                    times["one process, three columns"].append(dt)
            else:
                dts = [run(single[k], f"S{k}") for k in range(3)]
                if rep >= 0:
                    times["three processes, one column each"].append(sum(dts))
                    for k in range(3):
                        per_column[k].append(dts[k])
        for k in range(3):
            a, b = open(os.path.join(out, f"M_{k}_abundances.txt"), "rb").read(), open(os.path.join(out, f"S{k}_abundances.txt"), "rb").read()
            assert len(a) > 100 and a == b, f"column {k}: the two sides wrote different abundances"
    for s, ts in times.items():
        print(f"  {s:34s} {stats(ts)}")
    for k in range(3):
        print(f"    the process of column {k} alone ({n_groups[k]} groups)  {stats(per_column[k])}")
    m, s = median(times["one process, three columns"]), median(times["three processes, one column each"])
    spread = max(max(ts) - min(ts) for ts in times.values())
    word = "faster by more than the spread" if s - m > spread else ("SLOWER by more than the spread" if m - s > spread else "no difference beyond the spread")
    print(f"three groupings: one process median {m:.3f} s, three processes median {s:.3f} s, largest spread {spread:.3f} s: "
          f"{s / m:.2f} x, {s - m:+.3f} s ({word}); abundances of every column byte-identical on both sides in every repeat")
finally:
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
    if bin_dir:
        shutil.rmtree(bin_dir, ignore_errors=True)
