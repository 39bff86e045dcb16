"""GPU: msw_core_assign_reads / _aln and msw_core_assign_table_* (msweep_amd/csrc/assign_kernels.hpp) against
the rule restated in numpy on msw_core_gamma_block's output, bit for bit and order included.

The rule ([UPSTREAM-UNVERIFIED], as DESIGN.md 7b's): pass(g, j) <=> gamma(g, j) >= log t_g for every estimated group g;
n_assigned[j] counts the passing groups of ALL G; target bins as msw_core_bin_reads; the unassigned bin holds the reads of
the ECs with n_assigned == 0, ECs in EC order; the table has one row per aligned read in ascending id (stable),
dec(id), "\\t1" / "\\t0" per target in target order, "\\n"."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from msweep_amd import core as core_mod
from msweep_amd import synth
from msweep_amd.core import ALGO_EM, Core, MswError
from msweep_amd.likelihood import from_dense, from_grouped_counts

pytestmark = pytest.mark.gpu


# ---- the restatement --------------------------------------------------------------------------------------------------
def reads_of(ecs, rptr, reads):
    ecs = np.asarray(ecs, np.int64)
    if len(ecs) == 0:
        return np.zeros(0, np.uint32)
    rptr = np.asarray(rptr, np.int64)
    lens = rptr[ecs + 1] - rptr[ecs]
    start = np.repeat(rptr[ecs], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    return np.asarray(reads)[start]


def read_ids(ec_counts, seed, ids=None):
    """ec_rptr / ec_reads of a seeded permutation of the read ids (0 .. n - 1, or `ids`), ascending within each EC"""
    c = np.asarray(ec_counts, np.int64)
    rptr = np.zeros(len(c) + 1, np.uint64)
    rptr[1:] = np.cumsum(c)
    n = int(c.sum())
    ids = np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
    ids = ids[np.random.default_rng(seed).permutation(n)]
    ec = np.repeat(np.arange(len(c)), c)
    return rptr, ids[np.lexsort((ids, ec))]


def mixed_thresholds(theta, seed):
    """a threshold for every group: 1 - theta_g, exp(U(-6, -0.2)) or 1.0 -- none 0 or tiny, or every EC would be assigned"""
    rng = np.random.default_rng(seed)
    G = len(theta)
    t = 1.0 - np.asarray(theta, np.float64)
    pick = rng.integers(0, 3, G)
    t = np.where(pick == 1, np.exp(rng.uniform(-6.0, -0.2, G)), t)
    return np.where(pick == 2, 1.0, t)


def passes(core, rptr, reads, thr):
    """G x E: pass(g, j) on gamma_block's output; log t_g is the library's own (msw_core_bin_reads reports it)"""
    G, E = core.shape()[:2]
    log_thr = core.bin_reads(rptr, reads, np.arange(G), thr, want_reads=False)[2]
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(log_thr, np.log(thr), rtol=1e-15, atol=0)
    return core.gamma_block(0, E) >= log_thr[:, None]


def restated(passed, rptr, reads, targets, unassigned=True):
    n_assigned = passed.sum(0).astype(np.uint32)
    bins = [reads_of(np.nonzero(passed[g])[0], rptr, reads) for g in targets]
    if unassigned:
        bins.append(reads_of(np.nonzero(n_assigned == 0)[0], rptr, reads))
    bin_ptr = np.zeros(len(bins) + 1, np.uint64)
    bin_ptr[1:] = np.cumsum([len(b) for b in bins])
    lens = np.diff(np.asarray(rptr, np.int64))
    cls = np.array([lens[n_assigned == 0].sum(), lens[n_assigned == 1].sum(), lens[n_assigned >= 2].sum()], np.uint64)
    out = np.concatenate(bins).astype(np.uint32) if bins else np.zeros(0, np.uint32)
    return dict(bin_ptr=bin_ptr, reads=out, n_assigned=n_assigned, class_reads=cls)


def same(a, b):
    for k in ("bin_ptr", "reads", "n_assigned", "class_reads"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def check_assign(core, rptr, reads, thr, targets):
    """assign_reads against the restatement and against bin_reads; sizes-only and repeated calls.  Returns (result, passed)"""
    passed = passes(core, rptr, reads, thr)
    want = restated(passed, rptr, reads, targets)
    got = core.assign_reads(rptr, reads, thr, targets)
    same(got, want)
    nt = len(targets)
    bp, br, _ = core.bin_reads(rptr, reads, targets, np.asarray(thr)[np.asarray(targets, np.int64)])
    np.testing.assert_array_equal(got["bin_ptr"][:nt + 1], bp)
    np.testing.assert_array_equal(got["reads"][:int(bp[-1])], br)
    sizes = core.assign_reads(rptr, reads, thr, targets, want_reads=False)
    assert sizes["reads"] is None
    np.testing.assert_array_equal(sizes["bin_ptr"], got["bin_ptr"])
    np.testing.assert_array_equal(sizes["n_assigned"], got["n_assigned"])
    same(core.assign_reads(rptr, reads, thr, targets), got)
    # without the unassigned bin: the target bins alone
    plain = core.assign_reads(rptr, reads, thr, targets, unassigned=False)
    same(plain, restated(passed, rptr, reads, targets, unassigned=False))
    return got, passed


def solve(core, p, algo=0):
    lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    G = len(p["group_sizes"])
    return core.solve(lik.log_counts(), np.ones(G), algo=algo, max_iters=300 if algo == ALGO_EM else 5000)["theta"]


@pytest.fixture(scope="module")
def narrow_problem():
    p = synth.make_csr_problem(20000, 60, seed=41, max_other=6)
    return p, read_ids(p["ec_counts"], 3)


# ---- 1. narrow records ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, ALGO_EM])
@pytest.mark.parametrize("slots", ["lds", "global"])
def test_assign_equals_the_rule_narrow(monkeypatch, narrow_problem, algo, slots):
    if slots == "global":
        monkeypatch.setenv("MSWEEP_BIN_LDS", "0")
    p, (rptr, reads) = narrow_problem
    with Core(0) as core:
        theta = solve(core, p, algo)
        assert core.layout_info()["record_bytes"] == 4 and core.layout_info()["index_records"] == 0
        thr = mixed_thresholds(theta, 2)
        assert thr.min() > 1e-3
        targets = np.random.default_rng(1).permutation(60)[:25]
        got, passed = check_assign(core, rptr, reads, thr, targets)
        # the conditions on the input, on the restated side
        n = passed.sum(0)
        E = len(n)
        for cls in (n == 0, n == 1, n >= 2):
            assert cls.sum() >= 0.01 * E, (int((n == 0).sum()), int((n == 1).sum()), int((n >= 2).sum()), E)
        non_target = np.setdiff1d(np.arange(60), targets)
        assert ((n == 1) & (passed[non_target].sum(0) == 1)).any()     # an EC whose only passing group is no target
        assert 0 < got["bin_ptr"][-1] - got["bin_ptr"][-2] < len(reads)


def test_prefilter_is_taken_over_all_groups(narrow_problem):
    """one NON-target group at t = 1e-30, every other group at 1.0: every EC is claimed (by that group at least), the
    unassigned bin is empty -- a prefilter bound over the targets alone would skip the background loop and fail here"""
    p, (rptr, reads) = narrow_problem
    with Core(0) as core:
        solve(core, p)
        targets = np.random.default_rng(1).permutation(60)[:25]
        lone = int(np.setdiff1d(np.arange(60), targets)[7])
        thr = np.ones(60)
        thr[lone] = 1e-30
        got, passed = check_assign(core, rptr, reads, thr, targets)
        assert passed[lone].all()
        assert (got["n_assigned"] >= 1).all()
        assert got["bin_ptr"][-1] == got["bin_ptr"][-2]
        assert got["class_reads"][0] == 0


# ---- 2. the other encodings ---------------------------------------------------------------------------------------------
def test_assign_wide_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    p = synth.make_csr_problem(15000, 50, seed=43, max_other=8)
    rptr, reads = read_ids(p["ec_counts"], 4)
    with Core(0) as core:
        theta = solve(core, p)
        assert core.layout_info()["record_bytes"] == 8
        check_assign(core, rptr, reads, mixed_thresholds(theta, 5), np.random.default_rng(2).permutation(50)[:20])


def test_assign_index_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")        # as tests/test_gpu_hybrid.py: the hybrid slot area
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "48")
    p = synth.make_csr_problem(30000, 300, seed=21, max_other=12, group_sizes=synth.diverse_group_sizes)
    rptr, reads = read_ids(p["ec_counts"], 5)
    with Core(0) as core:
        theta = solve(core, p)
        assert core.layout_info()["index_records"] == 1
        check_assign(core, rptr, reads, mixed_thresholds(theta, 5), np.random.default_rng(3).permutation(300)[:120])


def test_assign_value_records():
    d = synth.make_dense_problem(20000, 40, seed=31, max_support=12)     # as tests/test_gpu_value_records.py
    counts = np.random.default_rng(2).integers(1, 5, 20000)
    rptr, reads = read_ids(counts, 6)
    with Core(0) as core:
        from_dense(core, d["logl"], d["logc"])
        assert core.layout_info()["record_bytes"] == 12
        theta = core.solve(d["logc"], np.ones(40))["theta"]
        check_assign(core, rptr, reads, mixed_thresholds(theta, 2), np.random.default_rng(4).permutation(40)[:15])


# ---- 3. the table -------------------------------------------------------------------------------------------------------
def digit_ids(n, seed):
    """n distinct read ids that cross every digit count: 0, 9, 10, 99, 100, ... 999 999 999, 1 000 000 000 and
    4 294 967 295, the rest spread over all lengths -- with gaps, so that some ids are unaligned"""
    rng = np.random.default_rng(seed)
    special = {0, 4294967295}
    for d in range(1, 10):
        special |= {10 ** d - 1, 10 ** d}
    ids = set(special)
    while len(ids) < n:
        d = int(rng.integers(1, 11))
        lo, hi = (0 if d == 1 else 10 ** (d - 1)), min(10 ** d, 2 ** 32)
        ids.add(int(rng.integers(lo, hi)))
    assert len(ids) == n and special <= ids
    return np.array(sorted(ids), np.uint64).astype(np.uint32)


def render_table(passed, rptr, reads, targets, r0=0, r1=None):
    ec = np.repeat(np.arange(len(rptr) - 1), np.diff(np.asarray(rptr, np.int64)))
    order = np.argsort(np.asarray(reads, np.uint32), kind="stable")
    r1 = len(order) if r1 is None else r1
    cols = passed[np.asarray(targets, np.int64)] if len(targets) else np.zeros((0, passed.shape[1]), bool)
    out = []
    for i in order[r0:r1]:
        out.append(str(int(reads[i])) + "".join("\t1" if c else "\t0" for c in cols[:, ec[i]]) + "\n")
    return "".join(out).encode()


@pytest.mark.parametrize("G,n_targets", [(20, (0, 1, 2)), (100, (31, 32, 33, 64, 65))])
def test_table_bytes(G, n_targets):
    p = synth.make_csr_problem(6000, G, seed=23, max_other=4)
    n = int(p["ec_counts"].sum())
    rptr, reads = read_ids(p["ec_counts"], 14, digit_ids(n, 9))
    with Core(0) as core:
        theta = solve(core, p)
        thr = mixed_thresholds(theta, 1 if G == 20 else 2)
        passed = passes(core, rptr, reads, thr)
        for nt in n_targets:
            targets = np.random.default_rng(nt).permutation(G)[:nt]
            got = core.assign_reads(rptr, reads, thr, targets, keep_table=True)
            same(got, restated(passed, rptr, reads, targets))
            assert core.assign_table_rows() == n
            want = render_table(passed, rptr, reads, targets)
            whole = core.assign_table_block(0, n)
            assert whole == want, nt
            if nt:
                assert b"\t1" in whole and b"\t0" in whole
            # the same bytes from blocks of 1, 7 and 1000 rows, in turn
            parts, r0, k = [], 0, 0
            while r0 < n:
                r1 = min(n, r0 + (1, 7, 1000)[k % 3])
                parts.append(core.assign_table_block(r0, r1))
                r0, k = r1, k + 1
            assert b"".join(parts) == want, nt
            assert core.assign_table_block(5, 5) == b""


def test_table_rows_of_an_id_in_two_classes():
    """host-supplied arrays may list a read id in two ECs: two rows, in EC order (the sort by id is stable)"""
    p = synth.make_csr_problem(6000, 20, seed=23, max_other=4)
    n = int(p["ec_counts"].sum())
    rptr, reads = read_ids(p["ec_counts"], 14)
    reads = reads.copy()
    reads[-1] = reads[0]
    with Core(0) as core:
        theta = solve(core, p)
        thr = mixed_thresholds(theta, 1)
        passed = passes(core, rptr, reads, thr)
        targets = np.arange(20)
        core.assign_reads(rptr, reads, thr, targets, keep_table=True)
        assert core.assign_table_block(0, n) == render_table(passed, rptr, reads, targets)


def test_table_through_gzip():
    p = synth.make_csr_problem(6000, 20, seed=23, max_other=4)
    n = int(p["ec_counts"].sum())
    rptr, reads = read_ids(p["ec_counts"], 14, digit_ids(n, 9))
    with Core(0) as core:
        theta = solve(core, p)
        thr = mixed_thresholds(theta, 1)
        targets = np.random.default_rng(0).permutation(20)[:7]
        core.assign_reads(rptr, reads, thr, targets, keep_table=True)
        plain = core.assign_table_block(0, n)
        z, text_len = [core.gzip_begin(6)], 0
        for r0, r1 in ((0, 1), (1, 4321), (4321, n)):
            piece, nt = core.assign_table_block_gzip(r0, r1, with_info=True)
            z.append(piece)
            text_len += nt
        z.append(core.gzip_end())
        assert zlib.decompress(b"".join(z), 31) == plain
        assert text_len == len(plain)
        assert len(b"".join(z)) < len(plain)


# ---- 4. the alignment entry ---------------------------------------------------------------------------------------------
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
        kept, _, logc = core.build_likelihood_aln(dev, t["target_group"], p["group_sizes"])
        theta = core.solve(logc, np.ones(kept))["theta"]
        thr = mixed_thresholds(theta, 5)
        targets = np.random.default_rng(5).permutation(kept)[:12]
        arr = dev.arrays()
        want, passed = check_assign(core, arr["ec_rptr"], arr["ec_reads"], thr, targets)
        n = len(arr["ec_reads"])
        got = core.assign_reads_aln(dev, thr, targets, keep_table=True)
        same(got, want)
        assert core.assign_table_rows() == n
        table = core.assign_table_block(0, n)
        assert table == render_table(passed, arr["ec_rptr"], arr["ec_reads"], targets)
        # a host-read alignment handle (msw_alignment_read): its host arrays are uploaded
        L = core_mod.load_library()
        arrp = (C.c_char_p * 1)(os.fsencode(path))
        hh = C.c_void_p()
        assert L.msw_alignment_read(arrp, 1, int(t["n_targets"]), 0, C.byref(hh)) == 0
        ha = core_mod.DeviceAlignment(L, hh)
        assert not ha.on_device
        same(core.assign_reads_aln(ha, thr, targets, keep_table=True), want)
        assert core.assign_table_block(0, n) == table


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    p = synth.make_csr_problem(6000, 20, seed=23, max_other=4)
    rptr, reads = read_ids(p["ec_counts"], 14)
    n = len(reads)
    half = np.full(20, 0.5)
    with Core(0) as core:
        lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
        with pytest.raises(MswError, match="no solve"):
            core.assign_reads(rptr, reads, half, [0])
        theta = core.solve(lik.log_counts(), np.ones(20))["theta"]
        thr = mixed_thresholds(theta, 1)
        targets = np.arange(0, 20, 2)
        first = core.assign_reads(rptr, reads, thr, targets, keep_table=True)
        table = core.assign_table_block(0, n)

        def still_fine():
            same(core.assign_reads(rptr, reads, thr, targets, keep_table=True), first)
            assert core.assign_table_block(0, n) == table

        with pytest.raises(MswError, match="equivalence classes"):
            core.assign_reads(rptr[:-1], reads, thr, targets)
        still_fine()
        for bad in (np.nan, -0.1, 1.5):
            t2 = thr.copy()
            t2[1] = bad                                  # group 1 is no target
            with pytest.raises(MswError, match=r"\[0, 1\]"):
                core.assign_reads(rptr, reads, t2, targets)
            still_fine()
        with pytest.raises(MswError, match="out of range"):
            core.assign_reads(rptr, reads, thr, [20])
        with pytest.raises(MswError, match="twice"):
            core.assign_reads(rptr, reads, thr, [3, 3])
        still_fine()
        # the table: a row range out of bounds, the gzip variant without a stream, no kept state
        with pytest.raises(MswError, match="out of bounds"):
            core.assign_table_block(0, n + 1)
        with pytest.raises(MswError, match="out of bounds"):
            core.assign_table_block(7, 6)
        with pytest.raises(MswError, match="no gzip stream"):
            core.assign_table_block_gzip(0, n)
        still_fine()
        core.assign_reads(rptr, reads, thr, targets)                    # a call without the flag drops the state
        with pytest.raises(MswError, match="no assignment table"):
            core.assign_table_block(0, 1)
        with pytest.raises(MswError, match="no assignment table"):
            core.assign_table_rows()
        still_fine()
        core.solve(lik.log_counts(), np.ones(20))                       # ... and so does a new solve
        with pytest.raises(MswError, match="no assignment table"):
            core.assign_table_block(0, 1)
        still_fine()
    # a block whose worst-case text exceeds 1 GiB: many targets, many reads per class
    big = synth.make_csr_problem(3000, 4000, seed=29, max_other=4)
    E = len(big["ec_counts"])
    per_row = 11 + 2 * 4000
    fit = (1 << 30) // per_row
    counts = np.full(E, (fit + 1000) // E + 1, np.int64)
    r2, i2 = read_ids(counts, 1)
    assert len(i2) > fit
    with Core(0) as core:
        solve(core, big)
        core.assign_reads(r2, i2, np.ones(4000), np.arange(4000), keep_table=True, want_reads=False)
        with pytest.raises(MswError, match=f"at most {fit} rows"):
            core.assign_table_block(0, len(i2))
        assert len(core.assign_table_block(0, 3).split(b"\n")) == 4
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    d = synth.make_dense_problem(2000, 10, seed=53)
    r3, i3 = read_ids(np.ones(2000, np.int64), 1)
    with Core(0) as core:
        from_dense(core, d["logl"], d["logc"])
        core.solve(d["logc"], np.ones(10))
        with pytest.raises(MswError, match="dense"):
            core.assign_reads(r3, i3, np.full(10, 0.5), [0])
    monkeypatch.delenv("MSWEEP_DENSE_COMPRESS")
    comm = core_mod.Comm.local(1)[0]
    try:
        with Core(0) as core:
            lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
            core.solve(lik.log_counts(), np.ones(20))
            core.set_comm(comm)            # an EC-sharded handle: this rank holds one block of the ECs
            try:
                with pytest.raises(MswError, match="communicator"):
                    core.assign_reads(rptr, reads, half, [0])
            finally:
                core.set_comm(None)
    finally:
        comm.close()
