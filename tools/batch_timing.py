"""Developer timing of --samples: a study's samples in ONE `msweep_mini` process on resident handles against one process
per sample, whole processes on both sides.  Same box, the sides in another order inside every repeat, after one
unmeasured pass; median and min-max of `reps` repeats.
Shapes (msweep_amd.synth, written as two Themisto strands as tools/groupings_timing.py writes them):
  small  16 samples of 300 k reads x 1 k groups
  cfg3    8 samples of 10 M reads x 5 k groups
The samples of a shape share the reference and the -i file, as those of a study do.  A shape has `--texts N` distinct
texts (the same classes, the reads in another order and with other strand disagreements; default 4 for small, 1 for cfg3:
8 x 4 GB would not fit the memory file system) and the samples take them in turn.
Sides:
  a  one process per sample, one after the other: this tree's msweep_mini WITHOUT --samples (--parent-mini PATH: the binary
     of the parent commit linked to its own library instead) -- the only way to these results before the flag, the baseline
  b  --samples with one worker   (--devices 0)
  c  --samples with two workers  (--devices 0,0)
Every run writes abundances only; before any time is reported the abundances of every sample are byte-identical on all
sides, in every repeat.
usage: python tools/batch_timing.py [small|cfg3|both] [reps] [--mini PATH] [--parent-mini PATH] [--texts N]
       (MSWEEP_TEXT_TMPFS: where the text goes, /dev/shm by default)"""
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth

ARGS = list(sys.argv[1:])
opt = lambda name: ARGS[ARGS.index(name) + 1] if name in ARGS else None
MINI, PARENT, TEXTS = opt("--mini"), opt("--parent-mini"), opt("--texts")
POS = [a for k, a in enumerate(ARGS) if not a.startswith("--") and (k == 0 or ARGS[k - 1] not in ("--mini", "--parent-mini", "--texts"))]
WHICH = POS[0] if POS else "both"
REPS = int(POS[1]) if len(POS) > 1 else 5
SHAPES = {"small": (16, 300_000, 1000, 4), "cfg3": (8, 10_000_000, 5000, 1)}     # samples, reads, groups, distinct texts


def stats(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2]:.3f} s (min {ts[0]:.3f}, max {ts[-1]:.3f})"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def spread(ts):
    return max(ts) - min(ts)


def timing(shape, mini, bin_dir):
    N, R, G, n_texts = SHAPES[shape]
    n_texts = min(N, int(TEXTS) if TEXTS else n_texts)
    tmp = tempfile.mkdtemp(prefix="msweep_batch_", dir=os.environ.get("MSWEEP_TEXT_TMPFS", "/dev/shm"))
    try:
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        indicators = os.path.join(tmp, "groups.txt")
        with open(indicators, "w") as f:
            f.write("\n".join(f"g{g}" for g in aln["target_group"].astype(np.int64)) + "\n")
        texts = []
        for k in range(n_texts):
            rng = np.random.default_rng(11 + k)
            ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
            texts.append([os.path.join(tmp, f"t{k}_r1.txt"), os.path.join(tmp, f"t{k}_r2.txt")])
            for s, path in enumerate(texts[-1]):
                synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                     extra=(rng, 0.1, aln["n_targets"]) if s else None)
        del prob, aln, ec_of
        size = sum(os.path.getsize(p) for p in texts[0]) / 1e9
        print(f"{shape}: {N} samples of R={R} G={G} ({size:.2f} GB of text each, {n_texts} distinct text(s) taken in turn; generated in "
              f"{time.perf_counter() - t:.1f} s); {REPS} repeats after one unmeasured pass, the sides in another order in every repeat",
              flush=True)
        sample_files = [texts[k % n_texts] for k in range(N)]

        def prefix(side, k):
            d = os.path.join(tmp, "out", side, f"s{k:02d}")
            os.makedirs(d, exist_ok=True)
            return os.path.join(d, "P")

        manifests = {}
        for side in ("b", "c"):
            manifests[side] = os.path.join(tmp, f"samples_{side}.tsv")
            with open(manifests[side], "w") as f:
                f.write("".join(f"{prefix(side, k)}\t{','.join(sample_files[k])}\n" for k in range(N)))

        def process(cmd):
            t1 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True)
            dt = time.perf_counter() - t1
            assert p.returncode == 0, p.stderr[-2000:]
            return dt

        def side_a():
            exe = PARENT or mini
            return sum(process([exe, "--themisto", ",".join(sample_files[k]), "-i", indicators, "-o", prefix("a", k)]) for k in range(N))

        run = {"a": side_a,
               "b": lambda: process([mini, "--samples", manifests["b"], "-i", indicators, "--devices", "0"]),
               "c": lambda: process([mini, "--samples", manifests["c"], "-i", indicators, "--devices", "0,0"])}
        label = {"a": f"a  {N} processes, one per sample" + (" (parent commit's binary)" if PARENT else " (this tree's binary, no --samples)"),
                 "b": "b  one process, --samples, one worker", "c": "c  one process, --samples, --devices 0,0"}
        times = {s: [] for s in run}
        for rep in range(-1, REPS):      # (-1: unmeasured; page cache, allocator and clocks warm for every side)
            order = "abc"[rep % 3:] + "abc"[:rep % 3]
            for side in order:
                dt = run[side]()
                if rep >= 0:
                    times[side].append(dt)
            for k in range(N):
                want = open(prefix("a", k) + "_abundances.txt", "rb").read()
                assert len(want) > 100, k
                for side in "bc":
                    assert open(prefix(side, k) + "_abundances.txt", "rb").read() == want, f"sample {k}: side {side} wrote other abundances"
        for s in "abc":
            print(f"  {label[s]:62s} {stats(times[s])}")
        a, b, c = (median(times[s]) for s in "abc")
        sp_ab, sp_bc = max(spread(times["a"]), spread(times["b"])), max(spread(times["b"]), spread(times["c"]))
        word = lambda gain, sp: "faster by more than the spread" if gain > sp else ("SLOWER by more than the spread" if -gain > sp else "no difference beyond the spread")
        print(f"  b against a: {a / b:.2f} x, {a - b:+.3f} s, {(a - b) / (N - 1):.3f} s per process saved; largest spread {sp_ab:.3f} s: {word(a - b, sp_ab)}")
        print(f"  c against b: {b / c:.2f} x, {b - c:+.3f} s; largest spread {sp_bc:.3f} s: {word(b - c, sp_bc)}")
        print(f"  per sample: a {a / N:.3f} s, b {b / N:.3f} s, c {c / N:.3f} s; abundances of all {N} samples byte-identical on the three sides in every repeat",
              flush=True)
        return b - c > sp_bc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


bin_dir = None
try:
    if not MINI:
        lib = os.path.join(ROOT, "msweep_amd")
        bin_dir = tempfile.mkdtemp(prefix="msweep_batch_bin_")      # (not beside the text: /dev/shm may be mounted noexec)
        MINI = os.path.join(bin_dir, "msweep_mini")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", MINI, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                               "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    shapes = ["small", "cfg3"] if WHICH == "both" else [WHICH]
    two_pays = [timing(s, MINI, bin_dir) for s in shapes]
    if len(shapes) == 2:
        print("default number of workers without --devices: " +
              ("two (c beats b by more than the spread at both shapes)" if all(two_pays) else
               "one (c does not beat b by more than the spread at both shapes)"))
finally:
    if bin_dir:
        shutil.rmtree(bin_dir, ignore_errors=True)
