"""GPU: msw_core_sparse_probs_* (msweep_amd/csrc/sparse_probs_kernels.hpp) against the rule restated in numpy on
msw_core_gamma_block's output, byte for byte.  No tolerance is involved:

  1. core.gamma_block(0, E) gives the doubles; the kept set is `gamma >= sp.log_threshold` on those same doubles;
  2. the tokens come from core.text_block(TEXT_PROBS, 0, E), split on tabs;
  3. the expected file -- "id\\tg\\ttoken\\n" per kept cell, rows in order, ascending g within a row -- is assembled here and
     compared with b"".join(sp.pieces()) for equality.

The conditions a case has to meet are asserted on the restated side (a case that does not meet them fails, it does not skip):
  (a) a kept cell is the background cell of an unlisted group,
  (b) a listed cell is rejected although its group lies inside the passing prefix (its background value would pass),
  (c) a row has no kept cell,
  (d) by read: an EC holds >= 2 reads and the read ids are not contiguous from 0.
(b) needs a listed value BELOW log(zi), which precalc_lls never gives: the CSR cases set the table value of a single hit of
every group of two or more sequences to -9 (a weak hit).  (a)-(c) together need a threshold between the largest background
probability and the smallest row maximum: each main case runs at such a tau (found on the CPU oracle's dense gamma) and at
1e-3.  The boundary cases (E = 1, G = 1, tau = 1 ...) cannot meet all of them by construction and assert what they are about."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import ec_length_cases as elc
from msweep_amd import core as core_mod
from msweep_amd import synth
from msweep_amd.core import ALGO_EM, PREC_DOUBLE, PREC_FLOAT, TEXT_PROBS, Core, MswError
from msweep_amd.likelihood import precalc_lls
from test_gpu_guard import isolate_problem

pytestmark = pytest.mark.gpu

LOGZI = np.log(0.01)


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate(core, sp):
    """(keep G x E bool, tokens E x G of bytes) from gamma_block and the dense text of the same solve"""
    G, E = core.shape()[:2]
    gamma = core.gamma_block(0, E)
    keep = gamma >= sp.log_threshold
    tok = np.array(core.text_block(TEXT_PROBS, 0, E).replace(b"\n", b"\t").split(b"\t")[:-1], dtype=object).reshape(E, G + 1)
    assert [int(x) for x in tok[:3, 0]] == list(range(min(E, 3)))
    return keep, tok[:, 1:], gamma


def ec_chunks(keep, tok):
    """per EC the list of b"\\tg\\ttoken\\n" of its kept cells, ascending g"""
    out = [[] for _ in range(keep.shape[1])]
    for j, g in zip(*np.nonzero(keep.T)):
        out[j].append(b"\t%d\t%s\n" % (g, tok[j, g]))
    return out


def by_ec_bytes(keep, tok):
    return b"".join(b"%d" % j + c for j, cs in enumerate(ec_chunks(keep, tok)) for c in cs)


def by_read_bytes(keep, tok, rptr, reads):
    ec = np.repeat(np.arange(len(rptr) - 1), np.diff(np.asarray(rptr, np.int64)))
    chunks = ec_chunks(keep, tok)
    order = np.argsort(np.asarray(reads, np.uint32), kind="stable")
    return b"".join(b"%d" % int(reads[i]) + c for i in order for c in chunks[ec[i]])


def listed_of(rowptr, grp, G):
    rp = np.asarray(rowptr, np.int64)
    m = np.zeros((G, len(rp) - 1), bool)
    m[np.asarray(grp, np.int64), np.repeat(np.arange(len(rp) - 1), np.diff(rp))] = True
    return m


def conditions(core, sp, keep, gamma, listed):
    """(a), (b), (c) on the restated side.  The background value of a listed cell is a * log(zi) + u_g - lse_j = gamma -
    a * (L - log(zi)); a is 1 up to the tolerance of the solve (exactly 1 under EM), and a margin of 1e-3 covers that: a cell
    counted here lies inside the passing prefix by far more than the rule's rounding."""
    L = core.get_dense_logl()
    assert (keep & ~listed).any(), "(a) no kept background cell"
    bg = gamma - L + LOGZI
    assert (listed & ~keep & (bg >= sp.log_threshold + 1e-3)).any(), "(b) no listed cell rejected inside the prefix"
    assert (keep.sum(0) == 0).any(), "(c) no row without a kept cell"


def check_by_ec(core, tau, listed=None, all_conditions=False, max_bytes=None):
    sp = core.sparse_probs(None, tau)
    G, E = core.shape()[:2]
    assert sp.rows == E
    assert sp.log_threshold == np.log(tau)
    keep, tok, gamma = restate(core, sp)
    got = b"".join(sp.pieces(**({} if max_bytes is None else dict(max_bytes=max_bytes))))
    want = by_ec_bytes(keep, tok)
    assert got == want, (len(got), len(want))
    assert sp.cells == int(keep.sum())
    ms, nbytes, ncells = sp.last_timing()
    assert ncells == sp.cells and nbytes == len(want) and ms > 0.0
    if all_conditions:
        conditions(core, sp, keep, gamma, listed)
    return want, keep


def weak_hit_lut(sizes):
    """precalc_lls with the table value of a single hit of every group of >= 2 sequences at -9 < log(zi): condition (b)"""
    lut = precalc_lls(sizes)
    lut[:, 1] = np.where(np.asarray(sizes) >= 2, -9.0, lut[:, 1])
    return lut


def set_weak(core, p):
    G = len(p["group_sizes"])
    core.set_csr(p["rowptr"], p["grp"], p["cnt"], weak_hit_lut(p["group_sizes"]), LOGZI, G)
    return np.log(p["ec_counts"].astype(np.float64)), listed_of(p["rowptr"], p["grp"], G)


# ---- 1. the four encodings --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow_problem():
    return synth.make_csr_problem(6000, 60, seed=41, max_other=6)


@pytest.mark.parametrize("force", [None, "00"])
def test_narrow_records_and_tables_in_memory(monkeypatch, narrow_problem, force):
    if force:
        monkeypatch.setenv("MSWEEP_FORCE_LDS", force)        # the sweeps' tables in global memory
    with Core(0) as core:
        logc, listed = set_weak(core, narrow_problem)
        info = core.layout_info()
        if force:       # (without LDS for the tables the layout turns to index records: the cold part of the slot area is read from memory)
            assert info["groups_in_lds"] == 0 and info["table_in_lds"] == 0 and info["index_records"] == 1
        else:
            assert info["record_bytes"] == 4 and info["index_records"] == 0 and info["table_in_lds"] == 1
        core.solve(logc, np.ones(60))
        check_by_ec(core, 0.3, listed, all_conditions=True)
        check_by_ec(core, 1e-3)


def test_wide_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    p = synth.make_csr_problem(5000, 50, seed=43, max_other=8)
    with Core(0) as core:
        logc, listed = set_weak(core, p)
        assert core.layout_info()["record_bytes"] == 8
        core.solve(logc, np.ones(50))
        check_by_ec(core, 0.4, listed, all_conditions=True)
        check_by_ec(core, 1e-3)


def test_index_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")        # as tests/test_gpu_hybrid.py: the hybrid slot area
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "48")
    p = synth.make_csr_problem(8000, 300, seed=21, max_other=12, group_sizes=synth.diverse_group_sizes)
    assert 100 < p["group_sizes"].max() <= 400
    with Core(0) as core:
        logc, listed = set_weak(core, p)
        assert core.layout_info()["index_records"] == 1
        core.solve(logc, np.ones(300))
        check_by_ec(core, 0.15, listed, all_conditions=True)
        check_by_ec(core, 1e-3)


def test_value_records():
    d = synth.make_dense_problem(20000, 40, seed=31, max_support=12)     # as tests/test_gpu_assign.py: > 65536 distinct values
    with Core(0) as core:
        core.set_dense_logl(d["logl"])
        assert core.layout_info()["record_bytes"] == 12
        core.solve(d["logc"], np.ones(40))
        check_by_ec(core, 0.3, d["logl"] != LOGZI, all_conditions=True)
        check_by_ec(core, 1e-3)


# ---- 2. EC lengths, E and G boundaries ----------------------------------------------------------------------------------
def test_ec_lengths_in_one_likelihood():
    """ECs of 1, 16, 17, 64, 65, 256, 257, 1024 and 1025 cells in one likelihood, G just above the longest"""
    lens = np.repeat([1, 16, 17, 64, 65, 256, 257, 1024, 1025], 3)
    rng = np.random.default_rng(5)
    rng.shuffle(lens)
    G = 1030
    sizes = (1 + rng.poisson(4, G)).astype(np.uint64)
    grp = np.concatenate([elc.distinct_groups(rng, 1, G, int(n))[0] for n in lens]).astype(np.uint32)
    cnt = rng.integers(1, sizes[grp].astype(np.int64) + 1).astype(np.uint32)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, weak_hit_lut(sizes), LOGZI, G)
        info = core.layout_info()
        assert info["n_long_ecs"] >= 3 and sum(info["slices_by_lanes"]) >= 2
        core.solve(np.log(rng.integers(1, 16, len(lens)).astype(np.float64)), rng.uniform(0.5, 2.0, G))
        for tau in (1e-3, 1e-4, 0.2):
            want, keep = check_by_ec(core, tau)
            assert keep.any()


@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_ec_count_boundaries(E):
    c = elc.uniform_case(3, E, seed=1000 + E, G=40, small_only=True)
    with Core(0) as core:
        elc.set_csr(core, c)
        core.solve(c["logc"], c["alpha0"])
        want, keep = check_by_ec(core, 1e-3)
        assert keep.shape == (40, E) and keep.any(0).all()       # (every EC keeps a cell: a maximum is >= 1 / G)
        check_by_ec(core, 0.9)


@pytest.mark.parametrize("G", [1, 2])
def test_group_count_boundaries(G):
    rng = np.random.default_rng(G)
    E = 300
    sizes = np.full(G, 5, np.uint64)
    lens = rng.integers(1, G + 1, E)
    grp = np.concatenate([np.sort(rng.permutation(G)[:n]) for n in lens]).astype(np.uint32)
    cnt = rng.integers(1, 6, len(grp)).astype(np.uint32)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, weak_hit_lut(sizes), LOGZI, G)
        core.solve(np.zeros(E), np.ones(G))
        want, keep = check_by_ec(core, 1e-3)
        if G == 1:
            assert want == b"".join(b"%d\t0\t1\n" % j for j in range(E))
        check_by_ec(core, 0.5)


# ---- 3. thresholds --------------------------------------------------------------------------------------------------------
def test_thresholds(narrow_problem):
    with Core(0) as core:
        logc, listed = set_weak(core, narrow_problem)
        core.solve(logc, np.ones(60))
        want1, keep1 = check_by_ec(core, 1.0)           # only a probability that prints as the double 1.0 is kept
        assert keep1.sum(0).max() <= 1
        want5, keep5 = check_by_ec(core, 0.5)
        assert keep5.sum(0).max() <= 2 and keep5.any() and not keep5.any(0).all()
        check_by_ec(core, 1e-3)


def test_tiny_threshold_is_the_dense_file_relaid():
    """tau = 1e-300 on 300 x 40: every printable cell is kept -- the dense file's non-zero content as triplets"""
    p = synth.make_csr_problem(600, 40, seed=8, max_other=5)
    keep_ecs = 300
    assert len(p["ec_counts"]) >= keep_ecs
    rp = p["rowptr"][:keep_ecs + 1]
    with Core(0) as core:
        core.set_csr(rp, p["grp"][:int(rp[-1])], p["cnt"][:int(rp[-1])], weak_hit_lut(p["group_sizes"]), LOGZI, 40)
        assert core.shape()[:2] == (40, 300)
        core.solve(np.log(p["ec_counts"][:300].astype(np.float64)), np.ones(40))
        want, keep = check_by_ec(core, 1e-300)
        dense = core.text_block(TEXT_PROBS, 0, 300)
        relaid = b"".join(b"%d\t%d\t%s\n" % (j, g, t) for j, line in enumerate(dense.split(b"\n")[:-1])
                          for g, t in enumerate(line.split(b"\t")[1:]) if t != b"0")
        assert want == relaid
        assert keep.sum() > 0.9 * keep.size


def test_prefix_ends_at_a_run_of_equal_weights():
    """many groups nobody lists share one theta, hence one u_g: the passing prefix takes the whole run or none of it"""
    G, E = 200, 1500
    rng = np.random.default_rng(12)
    sizes = np.full(G, 4, np.uint64)
    lens = rng.integers(1, 4, E)
    grp = np.concatenate([np.sort(rng.choice(20, n, replace=False)) for n in lens]).astype(np.uint32)   # groups 20 ... 199: unlisted
    cnt = rng.integers(1, 5, len(grp)).astype(np.uint32)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, weak_hit_lut(sizes), LOGZI, G)
        theta = core.solve(np.zeros(E), np.ones(G))["theta"]
        assert len(np.unique(theta[20:])) == 1
        gamma = core.gamma_block(0, E)
        # a threshold that the run's background value passes in some ECs and misses in others
        run = np.sort(gamma[20])
        tau = float(np.exp(run[len(run) // 2]))
        want, keep = check_by_ec(core, tau)
        n_run = keep[20:].sum(0)
        assert set(np.unique(n_run)) == {0, 180}


# ---- 4. a guarded EC; the EM state ------------------------------------------------------------------------------------------
def test_guarded_ecs():
    p = isolate_problem(seed=121, deep=-120.0)
    G = p["G"]
    with Core(0) as core:
        core.set_csr(p["rowptr"], p["grp"], p["cnt"], p["lut"], LOGZI, G)
        core.solve(np.log(p["ec_counts"].astype(np.float64)), np.full(G, 1e-3))
        assert core.guarded_visits() > 0
        listed = listed_of(p["rowptr"], p["grp"], G)
        check_by_ec(core, 1e-3)
        check_by_ec(core, 0.3)
        sp = core.sparse_probs(None, 1e-3)
        keep, tok, gamma = restate(core, sp)
        assert (listed & ~keep).any() and (keep & ~listed).any()


@pytest.mark.parametrize("prec", [PREC_DOUBLE, PREC_FLOAT])
def test_em_state(narrow_problem, prec):
    with Core(0) as core:
        logc, listed = set_weak(core, narrow_problem)
        core.solve(logc, np.ones(60), algo=ALGO_EM, prec=prec, max_iters=300)
        check_by_ec(core, 0.3, listed, all_conditions=True)
        check_by_ec(core, 1e-3)


# ---- 5. by read -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aligned(tmp_path_factory):
    """a CSR problem, its pseudoalignment as a Themisto file (read ids from 3, shuffled over the ECs)"""
    p = synth.make_csr_problem(8000, 30, seed=19, max_other=5)
    t = synth.csr_to_targets(p)
    ec_of = np.repeat(np.arange(len(p["ec_counts"])), p["ec_counts"].astype(np.int64))
    ec_of = ec_of[np.random.default_rng(4).permutation(len(ec_of))]
    path = str(tmp_path_factory.mktemp("sparse") / "aln.txt")
    synth.write_themisto(path, ec_of, t["ec_tptr"], t["ec_targets"], first_read_id=3)
    return p, t, path


def solved_on_alignment(core, aligned):
    p, t, path = aligned
    dev = core.read_alignment([path], t["n_targets"])
    kept, _, logc = core.build_likelihood_aln(dev, t["target_group"], p["group_sizes"])
    core.solve(logc, np.ones(kept))
    return dev


def test_by_read_device_and_host_alignments(aligned):
    p, t, path = aligned
    with Core(0) as core:
        dev = solved_on_alignment(core, aligned)
        assert dev.on_device
        arr = dev.arrays()
        rptr, reads = arr["ec_rptr"], arr["ec_reads"]
        assert np.diff(rptr.astype(np.int64)).max() >= 2 and reads.min() == 3        # (d)
        for tau in (0.5, 1e-3):
            sp = core.sparse_probs(dev, tau)
            assert sp.rows == len(reads)
            keep, tok, gamma = restate(core, sp)
            want = by_read_bytes(keep, tok, rptr, reads)
            assert b"".join(sp.pieces()) == want
            assert sp.cells == int((keep.sum(0) * np.diff(rptr.astype(np.int64))).sum())
            if tau == 0.5:
                assert (keep.sum(0) == 0).any() and keep.any()      # (c)
            # a host-read alignment handle (msw_alignment_read): its host arrays are uploaded
            ha = core_mod.read_alignment_handle([path], t["n_targets"])
            assert not ha.on_device
            hp = core.sparse_probs(ha, tau)
            assert hp.rows == sp.rows and b"".join(hp.pieces()) == want
            # and by EC on the same solve
            assert b"".join(core.sparse_probs(None, tau).pieces()) == by_ec_bytes(keep, tok)


def test_by_read_an_id_in_two_classes(aligned):
    """host-supplied arrays may list a read id in two ECs: two rows, in EC order (the sort by id is stable)"""
    p, t, path = aligned
    with Core(0) as core:
        solved_on_alignment(core, aligned)
        ha = core_mod.read_alignment_handle([path], t["n_targets"])
        ptrs = [C.c_void_p() for _ in range(5)]
        assert core_mod.load_library().msw_alignment_view(ha._h, *[C.byref(x) for x in ptrs]) == 0
        n = ha.n_aligned
        raw = (C.c_uint32 * n).from_address(ptrs[4].value)      # the handle's own ec_reads
        raw[n - 1] = raw[0]
        arr = ha.arrays()
        rptr, reads = np.array(arr["ec_rptr"]), np.array(arr["ec_reads"])
        assert reads[-1] == reads[0] and len(np.unique(reads)) == n - 1
        sp = core.sparse_probs(ha, 1e-3)
        keep, tok, _ = restate(core, sp)
        got = b"".join(sp.pieces())
        assert got == by_read_bytes(keep, tok, rptr, reads)
        dup = b"%d\t" % int(reads[0])
        assert sum(line.startswith(dup) for line in got.split(b"\n")) == keep[:, 0].sum() + keep[:, -1].sum()


# ---- 6. pieces, gzip, determinism ---------------------------------------------------------------------------------------------
def test_pieces_end_at_row_ends(aligned):
    with Core(0) as core:
        dev = solved_on_alignment(core, aligned)
        whole = b"".join(core.sparse_probs(dev, 1e-3).pieces())
        assert len(whole) > 100000
        sp = core.sparse_probs(dev, 1e-3)
        longest = max(len(b"".join(g)) for g in _rows(whole))
        # (by read a row of this case is longer than 64 bytes, which is the documented error below: the rows by read are cut
        # at their own longest row and at 4096; max_bytes = 64 itself is exercised by EC, at the end of this test)
        for mb in (max(64, longest), 4096):
            sp = core.sparse_probs(dev, 1e-3)
            parts = list(sp.pieces(max_bytes=mb))
            assert b"".join(parts) == whole
            assert len(parts) > 1 and all(0 < len(x) <= mb and x.endswith(b"\n") for x in parts)
            for x, y in zip(parts, parts[1:]):      # a row is never split over two pieces
                assert x.rsplit(b"\n", 2)[-2].split(b"\t")[0] != y.split(b"\t", 1)[0]
        # a row larger than max_bytes: the documented error, and the handle stays usable
        sp = core.sparse_probs(dev, 1e-3)
        with pytest.raises(MswError, match=r"bytes of text, more than max_bytes = 8"):
            list(sp.pieces(max_bytes=8))
        assert b"".join(sp.pieces()) == whole
        if longest > 64:
            sp = core.sparse_probs(dev, 1e-3)
            with pytest.raises(MswError, match="more than max_bytes = 64"):
                list(sp.pieces(max_bytes=64))
        # by EC, 64 bytes at a time, at a threshold that keeps at most two short lines per row
        keep_whole = b"".join(core.sparse_probs(None, 0.4).pieces())
        parts = list(core.sparse_probs(None, 0.4).pieces(max_bytes=64))
        assert b"".join(parts) == keep_whole and len(parts) > 10 and all(len(x) <= 64 for x in parts)


def _rows(text):
    """the lines of a file grouped by their id, in order"""
    out, last = [], None
    for line in text.split(b"\n")[:-1]:
        i = line.split(b"\t", 1)[0]
        if i != last:
            out.append([])
            last = i
        out[-1].append(line + b"\n")
    return out


def test_gzip_variant_and_determinism(aligned):
    with Core(0) as core:
        dev = solved_on_alignment(core, aligned)
        plain = b"".join(core.sparse_probs(dev, 1e-3).pieces())
        assert b"".join(core.sparse_probs(dev, 1e-3).pieces()) == plain
        streams = []
        for _ in range(2):
            z = [core.gzip_begin(6)]
            z += list(core.sparse_probs(dev, 1e-3).pieces_gzip(max_bytes=1 << 16))
            z.append(core.gzip_end())
            streams.append(b"".join(z))
        assert gzip.decompress(streams[0]) == plain
        assert streams[0] == streams[1] and len(streams[0]) < len(plain)


def test_undecided_cells_go_through_the_host(monkeypatch, narrow_problem):
    """MSWEEP_TEXT_HOST_CAP=0: every piece that holds an undecided cell is rendered on the host -- the same bytes"""
    with Core(0) as core:
        logc, _ = set_weak(core, narrow_problem)
        core.solve(logc, np.ones(60))
        want, _ = check_by_ec(core, 1e-3)
        sp = core.sparse_probs(None, 1e-3)
        assert b"".join(sp.pieces()) == want
        on_device = sp.host_cells
        monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", "0")
        sp = core.sparse_probs(None, 1e-3)
        assert b"".join(sp.pieces(max_bytes=1 << 16)) == want
        assert sp.host_cells >= on_device


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch, aligned, narrow_problem):
    p, t, path = aligned
    L = core_mod.load_library()

    def next_plain(core):
        ptr, n, done, nc, nh = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_size_t()
        core._check(L.msw_core_sparse_probs_next(core._h, 1 << 20, C.byref(ptr), C.byref(n), C.byref(done), C.byref(nc), C.byref(nh)))

    with Core(0) as core:
        dev = core.read_alignment([path], t["n_targets"])
        kept, _, logc = core.build_likelihood_aln(dev, t["target_group"], p["group_sizes"])
        with pytest.raises(MswError, match="no solve"):
            core.sparse_probs(None, 0.5)
        with pytest.raises(MswError, match="no selection"):
            next_plain(core)
        core.solve(logc, np.ones(kept))
        whole = b"".join(core.sparse_probs(dev, 0.01).pieces())

        def still_fine():
            assert b"".join(core.sparse_probs(dev, 0.01).pieces()) == whole

        for bad in (np.nan, 0.0, -0.5, 1.0000001, np.inf):
            with pytest.raises(MswError, match=r"\(0, 1\]"):
                core.sparse_probs(None, bad)
            still_fine()
        other = synth.make_csr_problem(500, 30, seed=3, max_other=5)
        to = synth.csr_to_targets(other)
        path2 = os.path.join(os.path.dirname(path), "other.txt")
        synth.write_themisto(path2, np.repeat(np.arange(len(other["ec_counts"])), other["ec_counts"].astype(np.int64)),
                             to["ec_tptr"], to["ec_targets"])
        with pytest.raises(MswError, match="equivalence classes"):
            core.sparse_probs(core_mod.read_alignment_handle([path2], to["n_targets"]), 0.01)
        still_fine()
        sp = core.sparse_probs(dev, 0.01)
        with pytest.raises(MswError, match="no gzip stream"):
            list(sp.pieces_gzip())
        with pytest.raises(MswError, match="max_bytes"):
            list(sp.pieces(max_bytes=0))
        assert b"".join(sp.pieces()) == whole
        # the state is dropped by a solve, a bootstrap, a trim and a new likelihood
        for drop in (lambda: core.solve(logc, np.ones(kept)),
                     lambda: core.bootstrap(dev.ec_counts().astype(np.uint32), 7, int(dev.ec_counts().sum()), 0, 1, np.ones(kept)),
                     lambda: core.trim()):
            core.sparse_probs(dev, 0.01)
            drop()
            with pytest.raises(MswError, match="no selection"):
                next_plain(core)
            still_fine()
        core.sparse_probs(None, 0.01)
        set_weak(core, narrow_problem)
        with pytest.raises(MswError, match="no selection"):
            next_plain(core)
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    d = synth.make_dense_problem(2000, 10, seed=53)
    with Core(0) as core:
        core.set_dense_logl(d["logl"])
        core.solve(d["logc"], np.ones(10))
        with pytest.raises(MswError, match="dense"):
            core.sparse_probs(None, 0.5)
    monkeypatch.delenv("MSWEEP_DENSE_COMPRESS")
    comm = core_mod.Comm.local(1)[0]
    try:
        with Core(0) as core:
            logc, _ = set_weak(core, narrow_problem)
            core.solve(logc, np.ones(60))
            core.set_comm(comm)            # an EC-sharded handle: this rank holds one block of the ECs
            try:
                with pytest.raises(MswError, match="communicator"):
                    core.sparse_probs(None, 0.5)
            finally:
                core.set_comm(None)
    finally:
        comm.close()
