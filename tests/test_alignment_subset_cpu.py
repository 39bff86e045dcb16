"""CPU: msw_alignment_subset on a host-resident alignment, without a handle (no GPU is touched): the alignment restricted
to a set of reads and a set of target sequences, collapsed into classes again.  The oracle is the contract itself
(include/msweep_core.h): the restricted text read by the existing readers (tests/subset_cases.py says which reader reads
which text, and why the host reader needs the padding where a selected id is not below the number of selected ids)."""
import numpy as np
import pytest

import subset_cases as sc
from msweep_amd import core


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    p = tmp_path_factory.mktemp("subset") / "source.txt"
    sc.write_rows(p, sc.source_rows(), sc.N_LINES)
    aln = core.read_alignment_handle([str(p)], sc.N_TARGETS)
    assert not aln.on_device
    return aln, sc.copy_arrays(aln)


def test_constructed_cases_are_in_the_input(source):
    sc.assert_constructed(source[1])


@pytest.mark.parametrize("case", range(len(sc.selections())), ids=[s[0] for s in sc.selections()])
def test_subset_is_the_restricted_text(source, tmp_path, case):
    aln, src = source
    name, ids, keep = sc.selections()[case]
    sub = core.subset_alignment(aln, ids, keep)
    assert not sub.on_device and sub.n_targets == int(np.count_nonzero(keep))
    got = sc.copy_arrays(sub)
    sc.check_against_readers(got, src, ids, keep, tmp_path, name)
    sc.assert_same(sc.copy_arrays(aln), src, "the source is not modified")


def test_merge_takes_the_smallest_read_id_from_the_later_class(source):
    aln, src = source
    name, ids, keep = sc.selections()[0]
    got = sc.copy_arrays(core.subset_alignment(aln, ids, keep))
    cls = sc.class_of_read(got)
    assert cls[3] == cls[10] == cls[11] == cls[12]                      # X and Y fell together
    rp = got["ec_rptr"].astype(np.int64)
    assert got["ec_reads"][rp[cls[3]]] == 3                              # the representative: from the later class
    assert sc.class_targets(got, cls[3]) == (1, 6)                       # targets 2 and 7, renumbered without 0
    assert len(got["ec_counts"]) < len({e for r, e in sc.class_of_read(src).items() if r in set(ids)})
    assert 20 not in cls and 70 not in cls and 1000 not in cls and 42 not in cls and 41 in cls


def test_everything_kept_reproduces_the_alignment(source):
    aln, src = source
    sub = core.subset_alignment(aln, np.arange(sc.N_LINES)[::-1], np.ones(sc.N_TARGETS, np.uint8))
    sc.assert_same(sc.copy_arrays(sub), src, "keep all, select all")


def test_no_ids(source):
    aln, src = source
    got = sc.copy_arrays(core.subset_alignment(aln, [], sc.keep_default()))
    assert got["n_reads"] == 0 and len(got["ec_counts"]) == 0 and len(got["ec_reads"]) == 0 and len(got["ec_targets"]) == 0
    assert got["ec_tptr"].tolist() == [0] and got["ec_rptr"].tolist() == [0]


def test_subset_of_a_subset_is_the_one_step_subset(source):
    aln, src = source
    keep1 = sc.keep_default()
    ids1 = list(range(0, sc.N_LINES, 2)) + [3, 11, 31, 63, 41, 43, 777]
    ids1 = sorted(set(ids1))
    one = core.subset_alignment(aln, ids1, keep1)
    kept = np.flatnonzero(keep1)
    keep2 = np.ones(len(kept), np.uint8)
    keep2[[1, 4, 9, 20]] = 0
    ids2 = [i for i in ids1 if i % 3 != 1] + [9999]
    two = core.subset_alignment(one, ids2, keep2)
    keep12 = np.zeros(sc.N_TARGETS, np.uint8)
    keep12[kept[keep2 != 0]] = 1
    direct = core.subset_alignment(aln, ids2, keep12)
    assert two.n_targets == direct.n_targets == int(keep12.sum())
    assert len(sc.copy_arrays(direct)["ec_counts"]) > 5
    sc.assert_same(sc.copy_arrays(two), sc.copy_arrays(direct), "subset of a subset")


def test_refusals(source):
    aln, src = source
    kd = sc.keep_default()
    # the SMALLEST id listed twice, wherever it stands
    with pytest.raises(core.MswError, match=r"msw_alignment_subset: read id 17 is listed twice"):
        core.subset_alignment(aln, [200, 5, 17, 200, 9, 17, 64, 64], kd)
    with pytest.raises(core.MswError, match=r"msw_alignment_subset: keep_target keeps no target sequence"):
        core.subset_alignment(aln, [1, 2, 3], np.zeros(sc.N_TARGETS, np.uint8))
    with pytest.raises(core.MswError, match=r"keep has 39 entries, the alignment 40 target sequences"):
        core.subset_alignment(aln, [1, 2, 3], np.ones(sc.N_TARGETS - 1, np.uint8))
    # (the third refusal, an alignment resident on another device than the handle's, needs two GPUs: not tested)
    sc.assert_same(sc.copy_arrays(aln), src, "the source after the refusals")
