"""Developer timing of --write-read-probs (msw_core_sparse_probs_*, sparse_probs_kernels.hpp): Themisto strands of `reads`
reads x `groups` groups (synth.write_themisto), read on the device, likelihood built there, one RCG solve; then, in ONE
process with the sides alternated and the median of `reps` repeats, the whole selection at tau -- begin and every piece,
kernels + D2H + the copy into Python -- by EC and by read, plain and inside a gzip stream, with the device time of its
kernels (msw_core_last_sparse_probs_timing) beside the wall time.
  extra   that many more groups of one sequence each that no read hits: the same reads and the same listed cells under
          groups + extra groups -- whether the pass is output-sensitive shows in the two runs' times
  dense   also the dense --write-probs text of the same ECs from the same build (Core.text_block, the driver's blocks)
usage: python tools/sparse_probs_timing.py [reads groups extra reps tau dense]   (MSWEEP_PROBE_DIR keeps the generated strands)"""
import os, shutil, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd import synth
from msweep_amd.__main__ import text_block_ecs
from msweep_amd.core import TEXT_PROBS, Core
from msweep_amd.reference import read_reference

R = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
EXTRA = int(sys.argv[3]) if len(sys.argv) > 3 else 0
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
TAU = float(sys.argv[5]) if len(sys.argv) > 5 else 0.001
DENSE = len(sys.argv) > 6 and sys.argv[6] == "dense"
PIECE = 256 << 20


def alternate(sides, reps=REPS):
    """{name: (median ms, last result)} of the callables in `sides`, run in turn `reps` times (after one warm-up each)"""
    ts, out = {k: [] for k in sides}, {}
    for k, fn in sides.items():
        fn()
    for _ in range(reps):
        for k, fn in sides.items():
            t = time.perf_counter()
            out[k] = fn()
            ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: (float(np.median(v)), out[k]) for k, v in ts.items()}


keep = os.environ.get("MSWEEP_PROBE_DIR")
tmp = keep or tempfile.mkdtemp(prefix="msweep_sparse_", dir=os.environ.get("TMPDIR", "/tmp"))
os.makedirs(tmp, exist_ok=True)
try:
    f = [os.path.join(tmp, "r1.txt")]
    base, clus = os.path.join(tmp, "clustering_0.txt"), os.path.join(tmp, f"clustering_{EXTRA}.txt")
    if not (os.path.exists(base) and os.path.exists(f[0])):
        t = time.perf_counter()
        prob = synth.make_csr_problem(R, G, seed=2)
        aln = synth.csr_to_targets(prob, shuffle=False)
        E = len(prob["ec_counts"])
        ec_of = np.random.default_rng(11).permutation(np.repeat(np.arange(E, dtype=np.int64), prob["ec_counts"].astype(np.int64)))
        synth.write_themisto(f[0], ec_of, aln["ec_tptr"], aln["ec_targets"], chunk=1_000_000)
        with open(base, "w") as c:
            c.write("\n".join(f"g{int(g)}" for g in aln["target_group"]) + "\n")
        del prob, aln, ec_of
        print(f"text generated in {time.perf_counter() - t:.1f} s", flush=True)
    if EXTRA:      # (kept strands serve every `extra`: the new groups' sequences stand behind the old ones)
        with open(clus, "w") as c:
            c.write(open(base).read() + "".join(f"x{k}\n" for k in range(EXTRA)))
    grouping = read_reference(open(clus))
    with Core(0) as core:
        a = core.read_alignment(f, len(grouping.group_indicators))
        kept, mask, _ = core.build_likelihood_aln(a, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        res = core.solve(None, np.ones(kept))
        E = a.n_ecs
        print(f"R={R} G={G}+{EXTRA}: estimated groups={kept} E={E} aligned reads={a.n_aligned} target hits={a.n_hits} "
              f"(reader on the device: {a.on_device}); {res['iters']} iterations; tau={TAU:g}; medians of {REPS}, sides alternated")

        def sparse(aln, gz=False):
            def run():
                sp = core.sparse_probs(aln, TAU)
                if gz:
                    n = len(core.gzip_begin(6)) + sum(len(z) for z in sp.pieces_gzip(PIECE)) + len(core.gzip_end())
                else:
                    n = sum(len(p) for p in sp.pieces(PIECE))
                return (n,) + sp.last_timing()
            return run

        def dense():
            block = text_block_ecs(kept)
            return (sum(len(core.text_block(TEXT_PROBS, e0, min(E, e0 + block))) for e0 in range(0, E, block)), core.last_text_timing()[0], 0, 0)

        sides = {"by EC": sparse(None), "by read": sparse(a), "by read, gzip": sparse(a, True)}
        if DENSE:
            sides["dense --write-probs text"] = dense
        for name, (ms, (n, kms, nbytes, cells)) in alternate(sides).items():
            what = f"{cells} cells, {nbytes / 1e6:.2f} MB of text" if cells else f"{E} x {kept} cells (kernel time of the last block only)"
            print(f"    {name:26s} {ms:10.2f} ms wall | kernels {kms:9.2f} ms | {n / 1e6:10.2f} MB out | {what}")
finally:
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)
