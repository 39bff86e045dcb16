"""Developer timing of --write-unassigned / --write-assignment-table (msw_core_assign_reads_aln and
msw_core_assign_table_block, assign_kernels.hpp): Themisto strands of `reads` reads x `groups` groups
(synth.write_themisto), read on the device, likelihood built there, one RCG solve; then, in ONE process with the sides
alternated and the median of `reps` repeats,
  (a) the assign call with the unassigned bin against msw_core_bin_reads_aln for the same targets and thresholds 1 - theta
      (each a sizes call and a fill call, as the drivers make them): the cost the flag adds.  A library of another commit
      named by MSWEEP_ASSIGN_BASE_LIB runs the unchanged bin call in a child process (through MSWEEP_CORE_LIB): its base;
  (b) the table for `table_targets` targets through assign_table_block, plain and inside a gzip stream, against the same
      rows rendered on the host from gamma_block -- the only way to the table without the kernels; the two are compared byte for byte.
usage: python tools/assign_timing.py [reads groups reps table_targets]   (MSWEEP_PROBE_DIR keeps the generated strands)"""
import os, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import binning, synth
from msweep_amd.core import Core
from msweep_amd.reference import read_reference

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
NT = int(sys.argv[4]) if len(sys.argv) > 4 else 16
BASE_ONLY = os.environ.get("MSWEEP_ASSIGN_BASE_CHILD") == "1"


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def alternate(sides, reps=REPS):
    """{name: median ms} of the callables in `sides`, run in turn `reps` times (after one warm-up each)"""
    ts = {k: [] for k in sides}
    for k, fn in sides.items():
        fn()
    for _ in range(reps):
        for k, fn in sides.items():
            ts[k].append(timed(fn)[0])
    return {k: float(np.median(v)) for k, v in ts.items()}


def render_host(core, rptr, reads, order, ec_of, rows, log_thr, r0, r1):
    """rows [r0, r1) of the table on the host: gamma_block of the ECs the rows touch, thresholded, printed"""
    idx = order[r0:r1]
    ecs = ec_of[idx]
    lo, hi = int(ecs.min()), int(ecs.max()) + 1
    out = []
    blk = 8192
    cells = np.zeros((len(idx), len(rows)), bool)
    for e0 in range(lo, hi, blk):
        e1 = min(hi, e0 + blk)
        m = (ecs >= e0) & (ecs < e1)
        if not m.any():
            continue
        g = core.gamma_block(e0, e1)[rows]
        cells[m] = (g[:, ecs[m] - e0] >= log_thr[:, None]).T
    tab = np.where(cells, "\t1", "\t0")
    for i, rid in enumerate(reads[idx]):
        out.append(str(int(rid)) + "".join(tab[i]) + "\n")
    return "".join(out).encode()


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_assign_", dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(tmp, exist_ok=True)
try:
    f = [os.path.join(tmp, "r1.txt")]
    clus = os.path.join(tmp, "clustering.txt")
    if not (os.path.exists(clus) and os.path.exists(f[0])):
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        ec_of = np.random.default_rng(11).permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        synth.write_themisto(f[0], ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000)
        with open(clus, "w") as c:
            c.write("\n".join(f"g{int(g)}" for g in aln["target_group"]) + "\n")
        del prob, aln, ec_of
        if not BASE_ONLY:
            print(f"text generated in {time.perf_counter() - t:.1f} s", flush=True)
    grouping = read_reference(open(clus))
    with Core(0) as core:
        a = core.read_alignment(f, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        theta = core.solve(None, np.ones(kept))["theta"]
        rows_all = np.arange(kept, dtype=np.uint32)
        thr_all = binning.all_thresholds(theta)
        bin_call = lambda: core.bin_reads_aln(a, rows_all, thr_all)
        if BASE_ONLY:
            print(f"base library, msw_core_bin_reads_aln, {kept} targets (sizes + fill): {alternate({'bin': bin_call})['bin']:.2f} ms")
            sys.exit(0)
        print(f"R={R} G={G}: E={a.n_ecs} aligned reads={a.n_aligned} (reader on the device: {a.on_device}); "
              f"medians of {REPS}, sides alternated")
        # (a) what the flag adds: every group a target, thresholds 1 - theta
        res = core.assign_reads_aln(a, thr_all, rows_all)
        c0, c1, c2 = (int(x) for x in res["class_reads"])
        m = alternate({"bin": bin_call, "assign": lambda: core.assign_reads_aln(a, thr_all, rows_all),
                       "assign+table state": lambda: core.assign_reads_aln(a, thr_all, rows_all, keep_table=True)})
        print(f"(a) {kept} targets, 1 - theta: reads in ECs claimed by 0 / 1 / >= 2 groups: {c0} / {c1} / {c2}; "
              f"{int(res['bin_ptr'][-1])} ids out (sizes + fill call each)")
        print(f"    msw_core_bin_reads_aln {m['bin']:.2f} ms | msw_core_assign_reads_aln with the unassigned bin {m['assign']:.2f} ms "
              f"| ... with MSW_ASSIGN_KEEP_TABLE {m['assign+table state']:.2f} ms")
        # load case: t = 0.5 for every group
        half = np.full(kept, 0.5)
        res = core.assign_reads_aln(a, half, rows_all)
        m = alternate({"bin": lambda: core.bin_reads_aln(a, rows_all, half), "assign": lambda: core.assign_reads_aln(a, half, rows_all)})
        print(f"    load case t = 0.5: {int(res['bin_ptr'][-1])} ids out: bin {m['bin']:.2f} ms | assign {m['assign']:.2f} ms")
        base = os.environ.get("MSWEEP_ASSIGN_BASE_LIB")
        if base:
            env = dict(os.environ, MSWEEP_CORE_LIB=base, MSWEEP_ASSIGN_BASE_CHILD="1", MSWEEP_PROBE_DIR=tmp)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, capture_output=True, text=True,
                               timeout=600)
            print("    " + (p.stdout.strip() or "base child failed: " + p.stderr[-300:]))
        # (b) the table for NT targets
        targets = np.argsort(-theta)[:NT].astype(np.uint32)
        core.assign_reads_aln(a, thr_all, targets, keep_table=True)
        n = core.assign_table_rows()
        block = binning.table_block_rows(NT)
        arr = a.arrays()
        rptr, reads = np.asarray(arr["ec_rptr"], np.int64), np.asarray(arr["ec_reads"])
        order = np.argsort(reads, kind="stable")
        ec_of = np.repeat(np.arange(len(rptr) - 1), np.diff(rptr))
        log_thr = np.log(thr_all[targets])

        def dev_plain():
            return sum(len(core.assign_table_block(r0, min(n, r0 + block))) for r0 in range(0, n, block))

        def dev_gzip():
            z = len(core.gzip_begin(6))
            for r0 in range(0, n, block):
                z += len(core.assign_table_block_gzip(r0, min(n, r0 + block)))
            return z + len(core.gzip_end())

        t_host, host_text = timed(lambda: render_host(core, rptr, reads, order, ec_of, targets, log_thr, 0, n))
        assert host_text == b"".join(core.assign_table_block(r0, min(n, r0 + block)) for r0 in range(0, n, block))
        nbytes = len(host_text)
        m = alternate({"plain": dev_plain, "gzip": dev_gzip})
        print(f"(b) table, {NT} targets, {n} rows, {nbytes / 1e6:.1f} MB of text, blocks of {block} rows:")
        print(f"    assign_table_block {m['plain']:.2f} ms ({nbytes / m['plain'] / 1e6:.2f} GB/s, kernels + D2H + the copy into Python) | "
              f"assign_table_block_gzip {m['gzip']:.2f} ms ({dev_gzip() / 1e6:.1f} MB out) | "
              f"host rendering from gamma_block {t_host:.0f} ms (once)")
finally:
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
