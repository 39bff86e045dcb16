"""GPU: --bin-reads -- the mGEMS binning step of src/mSWEEP.cpp:437-469 with the bin pass on the device
(msw_core_bin_reads / _aln, msweep_amd/csrc/bin_kernels.hpp) against the restated rule applied to
msw_core_gamma_block's output, bit for bit and order included; the refusals; both drivers against the oracle pipeline
and against each other, byte for byte.

The rule is restated here (mGEMS is fetched by the reference's build, not vendored; DESIGN.md [UPSTREAM-UNVERIFIED]):
the reads of EC j go to the bin of target k when gamma(g_k, j) >= log t_k, t_k = 1 - theta_k; within a bin the ECs in
EC order and the reads of each EC in the order the alignment holds them."""
import os
import subprocess

import numpy as np
import pytest

from msweep_amd import core as core_mod
from msweep_amd import synth
from msweep_amd.__main__ import main
from msweep_amd.alignment import Alignment
from msweep_amd.core import ALGO_EM, Core, MswError
from msweep_amd.likelihood import from_alignment, from_dense, from_grouped_counts
from msweep_amd.reference import read_reference

pytestmark = pytest.mark.gpu


# ---- the restatement --------------------------------------------------------------------------------------------
def expected_bins(gamma_cols, rptr, reads, targets, log_thr, e0=0):
    """bins of the ECs [e0, e0 + gamma_cols.shape[1]): list of per-target lists of EC indices (EC order)."""
    passed = gamma_cols[np.asarray(targets, np.int64)] >= np.asarray(log_thr)[:, None]
    return [np.nonzero(row)[0] + e0 for row in passed]


def reads_of(ecs, rptr, reads):
    if len(ecs) == 0:
        return np.zeros(0, np.uint32)
    rptr = np.asarray(rptr, np.int64)
    lens = rptr[ecs + 1] - rptr[ecs]
    start = np.repeat(rptr[ecs], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    return np.asarray(reads)[start]


def restated(core, rptr, reads, targets, log_thr, block=None):
    """(bin_ptr, reads_out) of the rule on gamma_block, in column blocks"""
    E = len(rptr) - 1
    block = block or E
    ecs = [[] for _ in targets]
    for e0 in range(0, E, block):
        blk = core.gamma_block(e0, min(E, e0 + block))
        for k, b in enumerate(expected_bins(blk, rptr, reads, targets, log_thr, e0)):
            ecs[k].append(b)
    out = [reads_of(np.concatenate(b).astype(np.int64) if b else np.zeros(0, np.int64), rptr, reads) for b in ecs]
    bin_ptr = np.zeros(len(targets) + 1, np.uint64)
    bin_ptr[1:] = np.cumsum([len(x) for x in out])
    return bin_ptr, (np.concatenate(out) if out else np.zeros(0, np.uint32)).astype(np.uint32)


def read_ids(ec_counts, seed):
    """ec_rptr / ec_reads of a seeded permutation of read ids, ascending within each EC (what the reader exports)"""
    c = np.asarray(ec_counts, np.int64)
    rptr = np.zeros(len(c) + 1, np.uint64)
    rptr[1:] = np.cumsum(c)
    ids = np.random.default_rng(seed).permutation(int(c.sum())).astype(np.uint32)
    ec = np.repeat(np.arange(len(c)), c)
    return rptr, ids[np.lexsort((ids, ec))]


def mixed_thresholds(n, theta_rows, seed):
    """1 - theta (listed passes), small t (background passes), t = 0 (every read) and t = 1"""
    rng = np.random.default_rng(seed)
    t = 1.0 - np.asarray(theta_rows, np.float64)
    pick = rng.integers(0, 4, n)
    t = np.where(pick == 1, np.exp(rng.uniform(-40, -2, n)), t)
    t = np.where(pick == 2, 0.0, t)
    t = np.where(pick == 3, 1.0, t)
    if n >= 4:
        t[:4] = [0.0, 1.0, 1e-30, 1.0 - theta_rows[3]]
    return t


def check_bins(core, rptr, reads, targets, thr, block=None):
    bp, got, log_thr = core.bin_reads(rptr, reads, targets, thr)
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(log_thr, np.log(thr), rtol=1e-15, atol=0)   # (the library's log; the rule uses log_thr)
    want_bp, want = restated(core, rptr, reads, targets, log_thr, block)
    np.testing.assert_array_equal(bp, want_bp)
    np.testing.assert_array_equal(got, want)
    return bp, got


def solve(core, p, algo=0):
    lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    G = len(p["group_sizes"])
    return core.solve(lik.log_counts(), np.ones(G), algo=algo, max_iters=300 if algo == ALGO_EM else 5000)["theta"]


# ---- 1. exact against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, ALGO_EM])
@pytest.mark.parametrize("slots", ["lds", "global"])
def test_bins_equal_the_rule_narrow(monkeypatch, algo, slots):
    if slots == "global":
        monkeypatch.setenv("MSWEEP_BIN_LDS", "0")
    p = synth.make_csr_problem(20000, 60, seed=41, max_other=6)
    rptr, reads = read_ids(p["ec_counts"], 3)
    with Core(0) as core:
        theta = solve(core, p, algo)
        assert core.layout_info()["record_bytes"] == 4 and core.layout_info()["index_records"] == 0
        G = len(theta)
        targets = np.arange(G)
        thr = mixed_thresholds(G, theta, 5)
        bp, got = check_bins(core, rptr, reads, targets, thr)
        assert bp[1] - bp[0] == len(reads) and np.array_equal(got[:len(reads)], reads)   # t = 0: every read, EC order
        # the natural thresholds 1 - theta, targets in another order, a subset
        order = np.random.default_rng(1).permutation(G)[:25]
        check_bins(core, rptr, reads, order, 1.0 - theta[order])


def test_bins_equal_the_rule_wide_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    p = synth.make_csr_problem(15000, 50, seed=43, max_other=8)
    rptr, reads = read_ids(p["ec_counts"], 4)
    with Core(0) as core:
        theta = solve(core, p)
        assert core.layout_info()["record_bytes"] == 8
        check_bins(core, rptr, reads, np.arange(50), mixed_thresholds(50, theta, 6))


@pytest.mark.parametrize("slots", ["lds", "global"])
def test_bins_equal_the_rule_index_records(monkeypatch, slots):
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")        # as tests/test_gpu_hybrid.py: the hybrid slot area
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "48")
    if slots == "global":
        monkeypatch.setenv("MSWEEP_BIN_LDS", "0")
    p = synth.make_csr_problem(30000, 300, seed=21, max_other=12, group_sizes=synth.diverse_group_sizes)
    rptr, reads = read_ids(p["ec_counts"], 5)
    with Core(0) as core:
        theta = solve(core, p)
        assert core.layout_info()["index_records"] == 1
        check_bins(core, rptr, reads, np.arange(300), mixed_thresholds(300, theta, 7))


def test_bins_equal_the_rule_value_records():
    d = synth.make_dense_problem(20000, 40, seed=31, max_support=12)     # as tests/test_gpu_value_records.py
    counts = np.random.default_rng(2).integers(1, 5, 20000)
    rptr, reads = read_ids(counts, 6)
    with Core(0) as core:
        from_dense(core, d["logl"], d["logc"])
        assert core.layout_info()["record_bytes"] == 12
        theta = core.solve(d["logc"], np.ones(40))["theta"]
        check_bins(core, rptr, reads, np.arange(40), mixed_thresholds(40, theta, 8))


def test_bins_with_min_hits_index_kept_rows():
    p = synth.make_csr_problem(20000, 80, seed=7, max_other=4, theta_support=30)
    t = synth.csr_to_targets(p)
    rptr, reads = read_ids(p["ec_counts"], 9)
    with Core(0) as core:
        lik = from_alignment(core, t["ec_tptr"], t["ec_targets"], t["target_group"], p["group_sizes"], p["ec_counts"],
                             min_hits=1)
        assert lik.n_groups < 80
        theta = core.solve(lik.log_counts(), np.ones(lik.n_groups))["theta"]
        check_bins(core, rptr, reads, np.arange(lik.n_groups), mixed_thresholds(lik.n_groups, theta, 10))
        with pytest.raises(MswError, match="out of range"):
            core.bin_reads(rptr, reads, [lik.n_groups], [0.5])


def test_bins_mid_size():
    """a few hundred thousand ECs, 1 200 groups, compared on the target rows in column blocks"""
    p = synth.make_csr_problem(300_000, 1200, seed=17, max_other=8)
    rptr, reads = read_ids(p["ec_counts"], 11)
    E = len(p["ec_counts"])
    assert E > 200_000
    with Core(0) as core:
        theta = solve(core, p)
        targets = np.arange(1200)
        bp, got = check_bins(core, rptr, reads, targets, 1.0 - theta, block=20000)
        assert 0 < bp[-1] <= len(reads) * 2
        sub = np.random.default_rng(3).permutation(1200)[:40]
        check_bins(core, rptr, reads, sub, mixed_thresholds(40, theta[sub], 12), block=20000)


# ---- 2. the alignment entry ---------------------------------------------------------------------------------------
def test_aln_entry_device_and_host_alignments(tmp_path):
    p = synth.make_csr_problem(8000, 30, seed=19, max_other=5)
    t = synth.csr_to_targets(p)
    ec_of = np.repeat(np.arange(len(p["ec_counts"])), p["ec_counts"].astype(np.int64))
    ec_of = ec_of[np.random.default_rng(4).permutation(len(ec_of))]
    path = str(tmp_path / "aln.txt")
    synth.write_themisto(path, ec_of, t["ec_tptr"], t["ec_targets"])
    with Core(0) as core:
        dev = core.read_alignment([path], t["n_targets"])
        assert dev.on_device
        host = core_mod.read_alignment([path], t["n_targets"])
        kept, _, logc = core.build_likelihood_aln(dev, t["target_group"], p["group_sizes"])
        theta = core.solve(logc, np.ones(kept))["theta"]
        targets = np.arange(kept)
        thr = mixed_thresholds(kept, theta, 13)
        arr = dev.arrays()
        np.testing.assert_array_equal(arr["ec_rptr"], host["ec_rptr"])
        bp, got = check_bins(core, arr["ec_rptr"], arr["ec_reads"], targets, thr)
        # a host-read alignment handle (msw_alignment_read): its host arrays are uploaded
        import ctypes as C
        L = core_mod.load_library()
        arrp = (C.c_char_p * 1)(os.fsencode(path))
        hh = C.c_void_p()
        assert L.msw_alignment_read(arrp, 1, int(t["n_targets"]), 0, C.byref(hh)) == 0
        ha = core_mod.DeviceAlignment(L, hh)
        assert not ha.on_device
        b3, r3, _ = core.bin_reads_aln(ha, targets, thr)
        np.testing.assert_array_equal(b3, bp)
        np.testing.assert_array_equal(r3, got)


# ---- 3. refusals and repeatability --------------------------------------------------------------------------------
def test_refusals_and_repeatability(monkeypatch):
    p = synth.make_csr_problem(6000, 20, seed=23, max_other=4)
    rptr, reads = read_ids(p["ec_counts"], 14)
    with Core(0) as core:
        from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
        with pytest.raises(MswError, match="no solve"):
            core.bin_reads(rptr, reads, [0], [0.5])
        theta = core.solve(np.log(p["ec_counts"].astype(float)), np.ones(20))["theta"]
        thr = mixed_thresholds(20, theta, 15)
        a = core.bin_reads(rptr, reads, np.arange(20), thr)
        b = core.bin_reads(rptr, reads, np.arange(20), thr)
        sizes, none, _ = core.bin_reads(rptr, reads, np.arange(20), thr, want_reads=False)
        assert none is None
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(sizes, a[0])
        with pytest.raises(MswError, match="equivalence classes"):
            core.bin_reads(rptr[:-1], reads, [0], [0.5])
        with pytest.raises(MswError, match="out of range"):
            core.bin_reads(rptr, reads, [20], [0.5])
        for bad in (np.nan, -0.1, 1.5):
            with pytest.raises(MswError, match=r"\[0, 1\]"):
                core.bin_reads(rptr, reads, [0], [bad])
        with pytest.raises(MswError, match="twice"):
            core.bin_reads(rptr, reads, [3, 3], [0.5, 0.5])
        # after the refusals the handle still bins as before
        c = core.bin_reads(rptr, reads, np.arange(20), thr)
        np.testing.assert_array_equal(c[1], a[1])
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    d = synth.make_dense_problem(2000, 10, seed=53)
    r2, i2 = read_ids(np.ones(2000, np.int64), 1)
    with Core(0) as core:
        from_dense(core, d["logl"], d["logc"])
        core.solve(d["logc"], np.ones(10))
        with pytest.raises(MswError, match="dense"):
            core.bin_reads(r2, i2, [0], [0.5])
    monkeypatch.delenv("MSWEEP_DENSE_COMPRESS")
    comm = core_mod.Comm.local(1)[0]
    try:
        with Core(0) as core:
            from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
            core.solve(np.log(p["ec_counts"].astype(float)), np.ones(20))
            core.set_comm(comm)            # an EC-sharded handle: this rank holds one block of the ECs
            try:
                with pytest.raises(MswError, match="communicator"):
                    core.bin_reads(rptr, reads, [0], [0.5])
            finally:
                core.set_comm(None)
    finally:
        comm.close()


# ---- 4. the Python CLI against the oracle pipeline ----------------------------------------------------------------
def _toy(tmp_path, n_reads=1500, seed=3):
    """4 clusters x ~10 reference sequences, paired-end reads drawn from theta = (.5,.3,.15,.05) (as in
    tests/test_gpu_cli_toy.py)."""
    rng = np.random.default_rng(seed)
    sizes = [12, 9, 10, 8]
    names = [f"clust{k + 1}" for k in range(4)]
    indicators = [names[k] for k in range(4) for _ in range(sizes[k])]
    order = rng.permutation(len(indicators))
    indicators = [indicators[i] for i in order]
    members = {n: [i for i, x in enumerate(indicators) if x == n] for n in names}
    theta = [0.5, 0.3, 0.15, 0.05]
    l1, l2 = [], []
    for r in range(n_reads):
        g = rng.choice(4, p=theta)
        hit = set(rng.choice(members[names[g]], max(1, rng.binomial(sizes[g], 0.65)), replace=False).tolist())
        for o in range(4):
            if o != g and rng.random() < 0.3:
                hit |= set(rng.choice(members[names[o]], max(1, rng.binomial(sizes[o], 0.15)), replace=False).tolist())
        h1 = sorted(hit | ({int(rng.integers(0, len(indicators)))} if rng.random() < 0.1 else set()))
        h2 = sorted(hit) if rng.random() > 0.05 else []
        l1.append(" ".join(map(str, [r] + h1)))
        l2.append(" ".join(map(str, [r] + h2)))
    (tmp_path / "toy_1.txt").write_text("\n".join(l1) + "\n")
    (tmp_path / "toy_2.txt").write_text("\n".join(l2) + "\n")
    (tmp_path / "clustering.txt").write_text("\n".join(indicators) + "\n")
    return names


def _first_group(tmp_path):
    return open(tmp_path / "clustering.txt").readline().strip()


def _toy_args(tmp_path):
    return ["--themisto-1", str(tmp_path / "toy_1.txt"), "--themisto-2", str(tmp_path / "toy_2.txt"),
            "-i", str(tmp_path / "clustering.txt")]


def _oracle_bins(oracle, tmp_path, targets=None, min_abundance=None, min_hits=0):
    """the restated rule on the oracle's gamma and theta: {name: (read ids of the bin, read ids of ECs within 1e-9 of
    the threshold -- reported and left out of the comparison)}, the target names"""
    grouping = read_reference(open(tmp_path / "clustering.txt"))
    aln = Alignment(len(grouping.group_indicators))
    aln.read("intersection", [open(tmp_path / "toy_1.txt"), open(tmp_path / "toy_2.txt")])
    aln.collapse()
    counts = oracle.group_counts(aln.ec_tptr, aln.ec_targets, grouping.group_indicators, grouping.get_n_groups())
    L, mask = oracle.fill_ll_mat(counts, aln.ec_counts, grouping.get_sizes(), min_hits=min_hits)
    logc = oracle.fill_ec_counts(aln.ec_counts)
    gamma = oracle.rcg_optl_dense(L, logc, np.ones(L.shape[0]))["gamma"]
    theta = oracle.mixture_components(gamma, logc)
    names = [n for n, m in zip(grouping.get_names(), mask) if m]
    targets = list(names) if targets is None else targets
    if min_abundance is not None:
        targets = [t for t in targets if not theta[names.index(t)] < min_abundance]
    rptr = np.zeros(len(aln.ec_counts) + 1, np.int64)
    rptr[1:] = np.cumsum(aln.ec_counts)
    reads = _aligned_reads(tmp_path, aln)
    out = {}
    for name in targets:
        k = names.index(name)
        logt = np.log(1.0 - theta[k])
        near = np.nonzero(np.abs(gamma[k] - logt) < 1e-9)[0]
        if len(near):
            print(f"{name}: ECs within 1e-9 of the threshold, left out: {near.tolist()}")
        ecs = np.setdiff1d(np.nonzero(gamma[k] >= logt)[0], near)
        out[name] = (reads_of(ecs, rptr, reads), set(reads_of(near, rptr, reads).tolist()))
    return out, targets


def _bin_file(path, skip):
    ids = [int(x) for x in open(path).read().splitlines()]
    return np.array([x for x in ids if x not in skip], np.int64)


def _aligned_reads(tmp_path, aln):
    """Alignment::get_aligned_reads: the read ids of every EC, ascending (the native reader's ec_reads; checked against
    the classes' read counts of the mirror)"""
    h = core_mod.read_alignment([str(tmp_path / "toy_1.txt"), str(tmp_path / "toy_2.txt")], aln.n_targets, copy=True)
    assert np.array_equal(h["ec_counts"], aln.ec_counts) and np.array_equal(h["ec_tptr"], aln.ec_tptr)
    return h["ec_reads"]


@pytest.mark.parametrize("extra,targets,min_ab", [
    ([], None, None),
    (["--target-groups", "clust3,clust1"], ["clust3", "clust1"], None),
    (["--min-abundance", "0.1"], None, 0.1),
    (["--target-groups", "clust4,clust2,clust1", "--min-abundance", "0.1"], ["clust4", "clust2", "clust1"], 0.1),
])
def test_cli_bins_against_the_oracle(tmp_path, oracle, extra, targets, min_ab):
    _toy(tmp_path)
    os.makedirs(tmp_path / "sub")
    assert main(_toy_args(tmp_path) + ["-o", str(tmp_path / "sub" / "run"), "--bin-reads"] + extra) == 0
    want, names = _oracle_bins(oracle, tmp_path, targets, min_ab)
    got = sorted(f for f in os.listdir(tmp_path / "sub") if f.endswith(".bin"))
    assert got == sorted(n + ".bin" for n in names)
    for n in names:
        ids, skip = want[n]
        np.testing.assert_array_equal(_bin_file(tmp_path / "sub" / (n + ".bin"), skip), ids)
    if not extra:
        assert len(names) == 4 and sum(len(want[n][0]) > 0 for n in names) >= 3
        # the abundances are those of a run without --bin-reads, byte for byte
        assert main(_toy_args(tmp_path) + ["-o", str(tmp_path / "plain")]) == 0
        assert (tmp_path / "sub" / "run_abundances.txt").read_bytes() == (tmp_path / "plain_abundances.txt").read_bytes()


def _min_hits_split(oracle, tmp_path):
    """(min_hits, pruned, kept): the smallest --min-hits (in steps of 50) that prunes a group of the toy and keeps two"""
    grouping = read_reference(open(tmp_path / "clustering.txt"))
    aln = Alignment(len(grouping.group_indicators))
    aln.read("intersection", [open(tmp_path / "toy_1.txt"), open(tmp_path / "toy_2.txt")])
    aln.collapse()
    counts = oracle.group_counts(aln.ec_tptr, aln.ec_targets, grouping.group_indicators, grouping.get_n_groups())
    names = grouping.get_names()
    for min_hits in range(50, 20000, 50):
        _, mask = oracle.fill_ll_mat(counts, aln.ec_counts, grouping.get_sizes(), min_hits=min_hits)
        pruned = [n for n, m in zip(names, mask) if not m]
        kept = [n for n, m in zip(names, mask) if m]
        if pruned:
            assert len(kept) >= 2, (min_hits, pruned, kept)
            return min_hits, pruned, kept
    raise AssertionError("no --min-hits prunes a group of the toy")


def test_cli_bin_refusals(tmp_path, oracle, capsys):
    _toy(tmp_path)
    rc = main(_toy_args(tmp_path) + ["-o", str(tmp_path / "r"), "--bin-reads", "--target-groups", "clust1,nope"])
    assert rc == 1 and "Binning the reads failed:\n  " in capsys.readouterr().err
    # a group pruned by --min-hits is not an estimated group: refused as a target; the kept ones bin as the rule says
    min_hits, pruned, kept = _min_hits_split(oracle, tmp_path)
    rc = main(_toy_args(tmp_path) + ["-o", str(tmp_path / "m"), "--bin-reads", "--min-hits", str(min_hits),
                                     "--target-groups", pruned[0]])
    err = capsys.readouterr().err
    assert rc == 1 and "Binning the reads failed:" in err and pruned[0] in err
    os.makedirs(tmp_path / "mh")
    assert main(_toy_args(tmp_path) + ["-o", str(tmp_path / "mh" / "r"), "--bin-reads", "--min-hits", str(min_hits)]) == 0
    want, names = _oracle_bins(oracle, tmp_path, min_hits=min_hits)
    assert names == kept and sorted(f for f in os.listdir(tmp_path / "mh") if f.endswith(".bin")) == sorted(
        n + ".bin" for n in kept)
    for n in kept:
        np.testing.assert_array_equal(_bin_file(tmp_path / "mh" / (n + ".bin"), want[n][1]), want[n][0])
    assert main(["--themisto-1", str(tmp_path / "toy_1.txt"), "-i", str(tmp_path / "clustering.txt"), "-o",
                 str(tmp_path / "w"), "--write-likelihood", "--no-fit-model"]) == 0
    rc = main(["-i", str(tmp_path / "clustering.txt"), "--read-likelihood", str(tmp_path / "w_likelihoods.tsv"),
               "--bin-reads", "-o", str(tmp_path / "x")])
    err = capsys.readouterr().err
    assert rc == 1 and "Binning the reads failed:" in err and "--read-likelihood" in err
    assert not (tmp_path / "x_abundances.txt").exists()
    rc = main(_toy_args(tmp_path) + ["-o", str(tmp_path / "nodir" / "r"), "--bin-reads"])
    assert rc == 1 and "Writing the bin for target group %s failed:" % _first_group(tmp_path) in capsys.readouterr().err


def test_cli_bins_with_bootstrap_count(tmp_path):
    """--bootstrap-count with --bin-reads is the number of draws (src/Sample.cpp:30-50); the bins are those of the
    point estimate"""
    _toy(tmp_path)
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    assert main(_toy_args(tmp_path) + ["-o", str(tmp_path / "a" / "r"), "--bin-reads", "--iters", "3", "--seed", "42",
                                       "--bootstrap-count", "500"]) == 0
    assert main(_toy_args(tmp_path) + ["-o", str(tmp_path / "b" / "r"), "--bin-reads"]) == 0
    for n in ("clust1", "clust2", "clust3", "clust4"):
        assert (tmp_path / "a" / (n + ".bin")).read_bytes() == (tmp_path / "b" / (n + ".bin")).read_bytes()
    rows = [ln.split("\t") for ln in open(tmp_path / "a" / "r_abundances.txt") if not ln.startswith("#")]
    got = np.array([[float(x) for x in r[2:]] for r in rows])
    with Core(0) as core:
        aln = core.read_alignment([str(tmp_path / "toy_1.txt"), str(tmp_path / "toy_2.txt")], 39)
        grouping = read_reference(open(tmp_path / "clustering.txt"))
        kept, _, logc = core.build_likelihood_aln(aln, grouping.group_indicators, grouping.get_sizes())
        w = aln.ec_counts().astype(np.uint32)
        thetas, _ = core.bootstrap(w, 42, 500, 0, 3, np.ones(kept))
    np.testing.assert_allclose(got, thetas.T, rtol=6e-6, atol=1e-12)        # the file holds 6 significant digits


# ---- 5. the native driver, byte for byte --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bin_mini_binary(tmp_path_factory):
    """msweep_amd/cpp/msweep_mini.cpp, built for this module"""
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("binmini") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("extra", [[], ["--target-groups", "clust3,clust1"], ["--min-abundance", "0.1"],
                                   ["--target-groups", "clust4,clust2,clust1", "--min-abundance", "0.1"],
                                   ["--iters", "3", "--seed", "42", "--bootstrap-count", "500"]])
def test_native_driver_bins_match_python_cli(tmp_path, bin_mini_binary, extra):
    _toy(tmp_path)
    for d in ("py", "cc"):
        os.makedirs(tmp_path / d)
    args = _toy_args(tmp_path) + ["--bin-reads"] + extra
    assert main(args + ["-o", str(tmp_path / "py" / "r")]) == 0
    p = subprocess.run([bin_mini_binary] + args + ["-o", str(tmp_path / "cc" / "r")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    py = sorted(os.listdir(tmp_path / "py"))
    assert py == sorted(os.listdir(tmp_path / "cc")) and "r_abundances.txt" in py and len(py) >= 2
    for name in py:
        assert (tmp_path / "cc" / name).read_bytes() == (tmp_path / "py" / name).read_bytes(), name


def test_native_driver_bin_refusals(tmp_path, bin_mini_binary):
    _toy(tmp_path)
    p = subprocess.run([bin_mini_binary] + _toy_args(tmp_path) + ["-o", str(tmp_path / "r"), "--bin-reads",
                                                                  "--target-groups", "clust1,nope"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Binning the reads failed:\n  " in p.stderr
    p = subprocess.run([bin_mini_binary, "-i", str(tmp_path / "clustering.txt"), "--read-likelihood",
                        str(tmp_path / "toy_1.txt"), "--bin-reads"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Binning the reads failed:" in p.stderr
    p = subprocess.run([bin_mini_binary] + _toy_args(tmp_path) + ["-o", str(tmp_path / "nodir" / "r"), "--bin-reads"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Writing the bin for target group %s failed:" % _first_group(tmp_path) in p.stderr
