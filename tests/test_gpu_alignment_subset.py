"""GPU: msw_alignment_subset on a device-resident alignment (subset_kernels.hpp, host_subset.inc) -- the cases of
tests/test_alignment_subset_cpu.py on an alignment from msw_alignment_read_device.  The five arrays and the shape are held
against the host path (MSWEEP_HOST_SUBSET=1), element for element, and against the existing readers on the restricted text
(tests/subset_cases.py); further: target lists on both sides of every length at which the filter kernel changes strategy,
a paired-end intersection input, the source's arrays after the call, a build + solve + bins on the subset handle against
the same on a fresh read of the restricted text, and two calls giving the same bytes."""
import numpy as np
import pytest

import subset_cases as sc
from msweep_amd.core import Core, MswError

pytestmark = pytest.mark.gpu

# subset_kernels.hpp: a class's target list is filtered by one lane up to kSubsetLaneMax targets, by its wavefront beyond,
# kSubsetWaveChunk targets per step -- one step, or a loop
K_SUBSET_LANE_MAX = 32
K_SUBSET_WAVE_CHUNK = 64
LONG_TARGETS = 3000
LONG_LENGTHS = (1, 2, K_SUBSET_LANE_MAX - 1, K_SUBSET_LANE_MAX, K_SUBSET_LANE_MAX + 1, K_SUBSET_WAVE_CHUNK - 1,
                K_SUBSET_WAVE_CHUNK, K_SUBSET_WAVE_CHUNK + 1, 2 * K_SUBSET_WAVE_CHUNK - 1, 2 * K_SUBSET_WAVE_CHUNK,
                2 * K_SUBSET_WAVE_CHUNK + 1, 900, LONG_TARGETS - 1, LONG_TARGETS)


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


@pytest.fixture(scope="module")
def source(core, tmp_path_factory):
    p = tmp_path_factory.mktemp("subset_gpu") / "source.txt"
    sc.write_rows(p, sc.source_rows(), sc.N_LINES)
    aln = core.read_alignment([str(p)], sc.N_TARGETS)
    assert aln.on_device
    return aln, sc.copy_arrays(core.read_alignment([str(p)], sc.N_TARGETS))


def _host_path(core, monkeypatch, aln, ids, keep):
    monkeypatch.setenv("MSWEEP_HOST_SUBSET", "1")
    sub = core.subset_alignment(aln, ids, keep)
    monkeypatch.delenv("MSWEEP_HOST_SUBSET")
    assert not sub.on_device
    return sc.copy_arrays(sub)


def _both_paths(core, monkeypatch, aln, src, ids, keep, tmp_path, what):
    sub = core.subset_alignment(aln, ids, keep)
    assert sub.on_device and sub.n_targets == int(np.count_nonzero(keep))
    got = sc.copy_arrays(sub)
    assert (sub.n_ecs, sub.n_reads, sub.n_hits, sub.n_aligned) == (len(got["ec_counts"]), len(ids), len(got["ec_targets"]),
                                                                  len(got["ec_reads"]))
    sc.assert_same(got, _host_path(core, monkeypatch, aln, ids, keep), what + ": host path")
    sc.check_against_readers(got, src, ids, keep, tmp_path, what)
    return sub, got


def test_constructed_cases_are_in_the_input(source):
    sc.assert_constructed(source[1])


@pytest.mark.parametrize("case", range(len(sc.selections())), ids=[s[0] for s in sc.selections()])
def test_device_subset_is_the_restricted_text_and_the_host_path(core, source, tmp_path, monkeypatch, case):
    aln, src = source
    name, ids, keep = sc.selections()[case]
    _both_paths(core, monkeypatch, aln, src, ids, keep, tmp_path, name)


def test_source_unchanged_everything_kept_no_ids_and_twice_the_same_bytes(core, source, tmp_path):
    src = source[1]
    sc.write_rows(tmp_path / "source.txt", sc.source_rows(), sc.N_LINES)
    aln = core.read_alignment([str(tmp_path / "source.txt")], sc.N_TARGETS)   # (no host copy of its arrays exists yet)
    assert aln.on_device
    name, ids, keep = sc.selections()[0]
    one = sc.copy_arrays(core.subset_alignment(aln, ids, keep))
    two = sc.copy_arrays(core.subset_alignment(aln, ids, keep))
    for k in sc.ARRAYS:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert len(one["ec_counts"]) > 5
    sub = core.subset_alignment(aln, np.arange(sc.N_LINES)[::-1], np.ones(sc.N_TARGETS, np.uint8))
    sc.assert_same(sc.copy_arrays(sub), src, "keep all, select all")
    none = sc.copy_arrays(core.subset_alignment(aln, [], keep))
    assert none["n_reads"] == 0 and len(none["ec_counts"]) == 0 and none["ec_tptr"].tolist() == [0] and none["ec_rptr"].tolist() == [0]
    # the source's arrays, copied out of device memory only now
    sc.assert_same(sc.copy_arrays(aln), src, "the source after the calls")


def test_subset_of_a_resident_subset(core, source):
    aln, src = source
    keep1 = sc.keep_default()
    ids1 = sorted(set(list(range(0, sc.N_LINES, 2)) + [3, 11, 31, 63, 41, 43, 777]))
    one = core.subset_alignment(aln, ids1, keep1)
    kept = np.flatnonzero(keep1)
    keep2 = np.ones(len(kept), np.uint8)
    keep2[[1, 4, 9, 20]] = 0
    ids2 = [i for i in ids1 if i % 3 != 1] + [9999]
    two = core.subset_alignment(one, ids2, keep2)
    keep12 = np.zeros(sc.N_TARGETS, np.uint8)
    keep12[kept[keep2 != 0]] = 1
    direct = core.subset_alignment(aln, ids2, keep12)
    assert two.on_device and direct.on_device and two.n_targets == direct.n_targets
    assert direct.n_ecs > 5
    sc.assert_same(sc.copy_arrays(two), sc.copy_arrays(direct), "subset of a subset")


def test_refusals(core, source):
    aln, src = source
    kd = sc.keep_default()
    many = list(range(250)) + [200, 17, 64, 17, 249]       # the SMALLEST id listed twice, whichever thread meets it first
    with pytest.raises(MswError, match=r"msw_alignment_subset: read id 17 is listed twice"):
        core.subset_alignment(aln, many, kd)
    with pytest.raises(MswError, match=r"msw_alignment_subset: keep_target keeps no target sequence"):
        core.subset_alignment(aln, [1, 2, 3], np.zeros(sc.N_TARGETS, np.uint8))
    # the handle stays usable, the source as it was
    sub = core.subset_alignment(aln, np.arange(sc.N_LINES), np.ones(sc.N_TARGETS, np.uint8))
    sc.assert_same(sc.copy_arrays(sub), src, "after the refusals")


def _long_rows():
    """400 reads over 3 000 targets: runs of consecutive targets of every length of LONG_LENGTHS, three reads each (one
    class per length and start), among short random lists -- a wavefront's 64 classes hold lists of every kind"""
    rng = np.random.default_rng(7)
    rows, r = {}, 0
    for ln in LONG_LENGTHS:
        for start in (0, 17):
            s = min(start, LONG_TARGETS - ln)
            for _ in range(3):
                rows[r] = tuple(range(s, s + ln))
                r += 1
    while r < 400:
        rows[r] = tuple(sorted(rng.choice(LONG_TARGETS, size=int(rng.integers(1, 9)), replace=False).tolist()))
        r += 1
    order = rng.permutation(400)
    return {int(order[i]): rows[i] for i in range(400)}


def test_lists_on_both_sides_of_every_strategy_boundary(core, tmp_path, monkeypatch):
    rows = _long_rows()
    p = tmp_path / "long.txt"
    sc.write_rows(p, rows, 400)
    aln = core.read_alignment([str(p)], LONG_TARGETS)
    assert aln.on_device
    src = sc.copy_arrays(aln)
    lens = set(np.diff(src["ec_tptr"].astype(np.int64)).tolist())
    assert set(LONG_LENGTHS) <= lens                          # every length is a class of the source
    rng = np.random.default_rng(8)
    ids = sorted(rng.choice(400, 300, replace=False).tolist())
    keeps = {"half": (rng.random(LONG_TARGETS) < 0.5).astype(np.uint8),
             "all": np.ones(LONG_TARGETS, np.uint8),
             "a few": (np.arange(LONG_TARGETS) % 41 == 3).astype(np.uint8),
             "the last one": (np.arange(LONG_TARGETS) == LONG_TARGETS - 1).astype(np.uint8),
             "none of the runs' first 100": (np.arange(LONG_TARGETS) >= 100).astype(np.uint8)}
    for name, keep in keeps.items():
        sub, got = _both_paths(core, monkeypatch, aln, src, ids, keep, tmp_path, name)
        assert sub.n_ecs > 0


def test_paired_end_intersection_input(core, tmp_path, monkeypatch):
    rng = np.random.default_rng(9)
    rows1 = sc.source_rows()
    rows2 = {i: tuple(t for t in tg if rng.random() < 0.8) for i, tg in rows1.items()}
    sc.write_rows(tmp_path / "s1.txt", rows1, sc.N_LINES)
    sc.write_rows(tmp_path / "s2.txt", rows2, sc.N_LINES)
    paths = [str(tmp_path / "s1.txt"), str(tmp_path / "s2.txt")]
    aln = core.read_alignment(paths, sc.N_TARGETS, "intersection")
    assert aln.on_device
    src = sc.copy_arrays(aln)
    assert len(src["ec_counts"]) > 20
    for name, ids, keep in sc.selections()[:2]:
        _both_paths(core, monkeypatch, aln, src, ids, keep, tmp_path, "paired-end, " + name)


def _build_solve_bins(core, aln, n_targets):
    group = (np.arange(n_targets) % 5).astype(np.uint32)
    sizes = np.bincount(group, minlength=5).astype(np.uint64)
    n_kept, mask, logc = core.build_likelihood_aln(aln, group, sizes)
    res = core.solve(None, np.ones(n_kept))
    bin_ptr, reads, _ = core.bin_reads_aln(aln, np.arange(n_kept, dtype=np.uint32), 1.0 - res["theta"])
    return dict(n_kept=np.array(n_kept), mask=mask, logc=logc, theta=res["theta"], iters=np.array(res["iters"]),
                bound=np.array(res["bound"]), gamma=core.gamma(), bin_ptr=bin_ptr, reads=reads)


@pytest.mark.parametrize("case", [0, 4], ids=["padded text", "exact text"])
def test_build_solve_and_bins_on_the_subset_handle(core, source, tmp_path, case):
    """the subset handle serves a build, a solve and the bin pass as a fresh device read of the restricted text does (the
    text padded with bare ids where a selected id is not below the number of selected ids: tests/subset_cases.py)"""
    aln, src = source
    name, ids, keep = sc.selections()[case]
    sub = core.subset_alignment(aln, ids, keep)
    got = _build_solve_bins(core, sub, sub.n_targets)
    text, n_keep = sc.restricted_text(src, ids, keep, pad=max(ids) >= len(ids))
    (tmp_path / "restricted.txt").write_text(text)
    with Core(0) as other:
        fresh = other.read_alignment([str(tmp_path / "restricted.txt")], n_keep)
        assert fresh.on_device
        want = _build_solve_bins(other, fresh, n_keep)
    assert int(want["bin_ptr"][-1]) > 0 and len(want["theta"]) == 5
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
