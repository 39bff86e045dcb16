"""Developer timing of --bin-reads (msw_core_bin_reads_aln, bin_kernels.hpp) on cfg3-sized text: Themisto strands of
`reads` reads x `groups` groups (synth.write_themisto), read on the device, likelihood built there, one RCG solve; then
  - the bin pass with every group a target, and with the targets --min-abundance 0.01 leaves: a sizes-only call (count,
    scan, write, sort, offsets) and a fill call (the same + scatter + the D2H copy of the ids);
  - a load case that is not mGEMS's threshold: t = 0.5 for every group (each EC's majority group, if any), millions of
    pairs through the sort and the scatter;
  - the D2H copy alone (the same number of bytes from a device buffer, hipMemcpy through the runtime the library
    already loaded: this process must not import torch, whose wheel bundles a second ROCm runtime);
  - the writers: binning.write_bin (Python) and the native driver's whole run with and without --bin-reads;
  - on a smaller shape (`alt_reads` x 1000 groups, t = 0.5): the existing alternative, msw_core_gamma_block streamed to
    the host and thresholded there, against the bin pass on the same solve.
usage: python tools/bin_timing.py [reads] [groups] [alt_reads]   (MSWEEP_PROBE_DIR keeps the generated strands)"""
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import binning, synth
from msweep_amd.core import Core
from msweep_amd.likelihood import from_grouped_counts

R = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
R_ALT = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000


def best(fn, reps=3):
    out, ts = None, []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3, out


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_bin_", dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(tmp, exist_ok=True)
try:
    f = [os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt")]
    clus = os.path.join(tmp, "clustering.txt")
    if not (os.path.exists(clus) and all(os.path.exists(x) for x in f)):
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(f):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
        with open(clus, "w") as c:
            c.write("\n".join(f"g{int(g)}" for g in aln["target_group"]) + "\n")
        del prob, aln, ec_of
        print(f"text generated in {time.perf_counter() - t:.1f} s", flush=True)
    from msweep_amd.reference import read_reference
    grouping = read_reference(open(clus))
    with Core(0) as core:
        a = core.read_alignment(f, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        theta = core.solve(None, np.ones(kept))["theta"]
        print(f"cfg3 text: R={R} G={G}: E={a.n_ecs} aligned reads={a.n_aligned} (reader on the device: {a.on_device})")
        names = [n for n, m in zip(grouping.get_names(), mask) if m]
        for label, targets in (("all groups", names),
                               ("--min-abundance 0.01", binning.filter_min_abundance(names, names, theta, 0.01)),
                               ("load case t = 0.5, all groups", names)):
            rows = np.array([names.index(t) for t in targets], np.uint32) if label.startswith("--min") else np.arange(kept)
            thr = binning.thresholds(rows, theta) if not label.startswith("load") else np.full(len(rows), 0.5)
            core.bin_reads_aln(a, rows, thr)                         # warm-up
            t_sz, (bp, _, _) = best(lambda: core.bin_reads_aln(a, rows, thr, want_reads=False))
            t_fill, (bp, reads, _) = best(lambda: core.bin_reads_aln(a, rows, thr))
            print(f"{label}: {len(rows)} targets, {int(bp[-1])} read ids binned: sizes-only call {t_sz:.2f} ms, "
                  f"fill call {t_fill:.2f} ms (the fill call is a sizes pass + scatter + D2H)", flush=True)
        import ctypes as C
        hip = C.CDLL("libamdhip64.so.7")
        nbytes = 4 * int(bp[-1])
        dptr = C.c_void_p()
        pageable = np.empty(max(nbytes // 4, 1), np.uint32)
        if nbytes and hip.hipMalloc(C.byref(dptr), C.c_size_t(nbytes)) == 0:
            t_d2h, _ = best(lambda: hip.hipMemcpy(pageable.ctypes.data_as(C.c_void_p), dptr, C.c_size_t(nbytes), 2))
            hip.hipFree(dptr)
            print(f"D2H of {nbytes / 1e6:.1f} MB into pageable host memory (as the fill call does): {t_d2h:.2f} ms")
        out_dir = os.path.join(tmp, "bins")
        os.makedirs(out_dir, exist_ok=True)
        t_w, _ = best(lambda: [binning.write_bin(os.path.join(out_dir, f"{names[int(r)]}.bin"),
                                                 reads[int(bp[k]):int(bp[k + 1])]) for k, r in enumerate(rows)], reps=1)
        print(f"binning.write_bin (Python): {len(rows)} files, {int(bp[-1])} ids: {t_w:.1f} ms", flush=True)
    lib = os.path.join(ROOT, "msweep_amd")
    mini = os.path.join(tmp, "msweep_mini")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", mini, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    args = [mini, "--themisto-1", f[0], "--themisto-2", f[1], "-i", clus]
    for extra in ([], ["--bin-reads"], ["--bin-reads", "--min-abundance", "0.01"]):
        o = os.path.join(tmp, "mini", "run")
        shutil.rmtree(os.path.dirname(o), ignore_errors=True)
        os.makedirs(os.path.dirname(o))
        walls = []
        for rep in range(2):
            t = time.perf_counter()
            p = subprocess.run(args + ["-o", o] + extra, capture_output=True, text=True)
            walls.append(time.perf_counter() - t)
            assert p.returncode == 0, p.stderr[-1000:]
        print(f"msweep_mini {' '.join(extra) or '(no binning)'}: {min(walls):.3f} s wall (whole process)", flush=True)

    # the existing alternative on a shape it can serve: gamma_block to the host, thresholded there
    p = synth.make_csr_problem(R_ALT, 1000, seed=2)
    rptr = np.zeros(len(p["ec_counts"]) + 1, np.uint64)
    rptr[1:] = np.cumsum(p["ec_counts"])
    ids = np.arange(int(rptr[-1]), dtype=np.uint32)
    with Core(0) as core:
        from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
        th = core.solve(np.log(p["ec_counts"].astype(float)), np.ones(1000))["theta"]
        rows = np.arange(1000)
        thr = np.full(1000, 0.5)          # the load case (1 - theta bins nothing on this synthetic shape either)
        E = len(p["ec_counts"])

        def streamed(block=16384):
            logt = np.log(thr)[:, None]
            n = 0
            for e0 in range(0, E, block):
                n += int(np.count_nonzero(core.gamma_block(e0, min(E, e0 + block)) >= logt))
            return n
        core.bin_reads(rptr, ids, rows, thr)
        t_dev, (bp, _, _) = best(lambda: core.bin_reads(rptr, ids, rows, thr))
        t_str, n_pairs = best(streamed, reps=1)
        print(f"alternative at R={R_ALT} G=1000 (E={E}): gamma_block streamed + host threshold {t_str:.0f} ms "
              f"({8 * 1000 * E / 1e9:.1f} GB over the link, {n_pairs} passing (EC, target) pairs); "
              f"bin pass incl. upload of the read ids {t_dev:.2f} ms", flush=True)
finally:
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
