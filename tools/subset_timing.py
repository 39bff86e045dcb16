"""Developer timing of msw_alignment_subset (subset_kernels.hpp, host_subset.inc) on cfg3-sized text: Themisto strands of
`reads` reads x `groups` groups (synth.write_themisto) read on the device; a COARSE grouping joins every `per` consecutive
groups (500 coarse groups over cfg3's 5 000); likelihood built and solved for it, the bins of the `children` most abundant
coarse groups taken with thresholds 1 - theta (t = 0.5 where that rule bins nothing on this synthetic shape, said so);
then, per bin, the subset of the resident alignment with that bin's reads and that coarse group's sequences:
  - the device path against the host loops behind the same call (MSWEEP_HOST_SUBSET=1), alternated inside every repeat,
    median (min-max) of `reps`; the host side's FIRST call also copies the source's five arrays out of device memory and
    is reported on its own;
  - the five arrays of both paths compared before a time is reported;
  - the device path's stage split (MSWEEP_BUILD_TIMING=1: filter + hash, select + sort, classes) for the largest bin.
usage: python tools/subset_timing.py [reads] [groups] [per] [children] [reps]   (MSWEEP_PROBE_DIR keeps the strands)"""
import os, shutil, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import binning, synth
from msweep_amd.core import Core

R = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
PER = int(sys.argv[3]) if len(sys.argv) > 3 else 10
CHILDREN = int(sys.argv[4]) if len(sys.argv) > 4 else 24
REPS = int(sys.argv[5]) if len(sys.argv) > 5 else 5
ARRAYS = ("ec_tptr", "ec_targets", "ec_counts", "ec_rptr", "ec_reads")


def stats(ts):
    return f"{np.median(ts) * 1e3:9.2f} ms ({min(ts) * 1e3:.2f}-{max(ts) * 1e3:.2f})"


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def host_loops(core, a, ids, keep):
    os.environ["MSWEEP_HOST_SUBSET"] = "1"
    try:
        return core.subset_alignment(a, ids, keep)
    finally:
        del os.environ["MSWEEP_HOST_SUBSET"]


keep_dir = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep_dir or tempfile.mkdtemp(prefix="msweep_subset_", dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(tmp, exist_ok=True)
try:
    f = [os.path.join(tmp, "r1.txt"), os.path.join(tmp, "r2.txt")]
    tg_path = os.path.join(tmp, "target_group.npy")
    if not (os.path.exists(tg_path) and all(os.path.exists(x) for x in f)):
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        rng = np.random.default_rng(11)
        ec_of = rng.permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        for k, path in enumerate(f):
            synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000,
                                 extra=(rng, 0.1, aln["n_targets"]) if k else None)
        np.save(tg_path, np.asarray(aln["target_group"], np.uint32))
        del prob, aln, ec_of
        print(f"text generated in {time.perf_counter() - t:.1f} s", flush=True)
    fine = np.load(tg_path)
    coarse = (fine // PER).astype(np.uint32)
    n_coarse = int(coarse.max()) + 1
    sizes = np.bincount(coarse, minlength=n_coarse).astype(np.uint64)
    with Core(0) as core:
        t_read, a = timed(lambda: core.read_alignment(f, len(coarse)))
        kept, mask, _ = core.build_likelihood_aln(a, coarse, sizes, want_logc=False)
        theta = core.solve(None, np.ones(kept))["theta"]
        print(f"cfg3 text: R={R} G={G}, {n_coarse} coarse groups of {PER}: E={a.n_ecs} hits={a.n_hits} aligned reads={a.n_aligned} "
              f"(read on the device: {a.on_device}, {t_read:.2f} s)", flush=True)
        est = np.flatnonzero(mask)
        rows = np.argsort(-theta, kind="stable")[:CHILDREN].astype(np.uint32)
        thr = binning.thresholds(rows, theta)
        bp, reads, _ = core.bin_reads_aln(a, rows, thr)
        rule = "1 - theta"
        if int(bp[-1]) == 0:
            thr = np.full(len(rows), 0.5)
            bp, reads, _ = core.bin_reads_aln(a, rows, thr)
            rule = "t = 0.5 (1 - theta bins nothing on this synthetic shape)"
        print(f"{len(rows)} bins by {rule}: {int(bp[-1])} read ids, theta of the targets {theta[rows[0]]:.4f} ... {theta[rows[-1]]:.4f}",
              flush=True)
        first_host = None
        total_dev, total_host = [0.0] * REPS, [0.0] * REPS
        biggest = None
        for k, r in enumerate(rows):
            ids = reads[int(bp[k]):int(bp[k + 1])]
            keep = (coarse == est[r]).astype(np.uint8)
            if biggest is None or len(ids) > len(biggest[0]):
                biggest = (ids, keep)
            core.subset_alignment(a, ids, keep).close()          # warm-up: the pool's blocks
            dev, host = [], []
            for rep in range(REPS):
                for side in ((0, 1) if rep % 2 == 0 else (1, 0)):
                    if side == 0:
                        t, sub = timed(lambda: core.subset_alignment(a, ids, keep))
                        dev.append(t)
                    else:
                        t, hsub = timed(lambda: host_loops(core, a, ids, keep))
                        if first_host is None:      # (it also copied the source's arrays out of device memory: timed again)
                            first_host = t
                            hsub.close()
                            t, hsub = timed(lambda: host_loops(core, a, ids, keep))
                        host.append(t)
                    if rep == REPS - 1:
                        continue
                    (sub if side == 0 else hsub).close()
                total_dev[rep] += dev[-1]
                total_host[rep] += host[-1]
            da, ha = sub.arrays(), hsub.arrays()
            assert sub.on_device and not hsub.on_device
            assert all(np.array_equal(da[x], ha[x]) for x in ARRAYS) and da["n_reads"] == ha["n_reads"] == len(ids)
            print(f"  child {k:2d}: {len(ids):8d} reads, {int(keep.sum()):3d} sequences -> {sub.n_ecs:7d} classes, {sub.n_hits:8d} hits: "
                  f"device {stats(dev)}   host loops {stats(host)}", flush=True)
            sub.close(), hsub.close()
        print(f"all {len(rows)} children: device {stats(total_dev)}   host loops {stats(total_host)}   "
              f"(the host side's first call, with the copy of the source's arrays: {first_host * 1e3:.1f} ms)", flush=True)
        os.environ["MSWEEP_BUILD_TIMING"] = "1"
        print(f"stage split of the largest child ({len(biggest[0])} reads), to stderr:", flush=True)
        core.subset_alignment(a, *biggest).close()
        del os.environ["MSWEEP_BUILD_TIMING"]
finally:
    if not keep_dir:
        shutil.rmtree(tmp, ignore_errors=True)
