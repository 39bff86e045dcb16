"""CPU: the driver side of --bin-reads (msweep_amd/binning.py): targets, the --min-abundance filter, thresholds, the
bin paths of OutfileDesignator::bin (src/OutfileDesignator.cpp:80-93) and the bin file format."""
import numpy as np
import pytest

from msweep_amd import binning

NAMES = ["a", "b", "c", "d"]
THETA = [0.5, 0.2, 0.2, 0.1]


def test_default_targets_are_the_estimated_groups_in_order():
    assert binning.resolve_targets(NAMES) == NAMES
    assert binning.resolve_targets(["b", "d"]) == ["b", "d"]      # --min-hits kept b and d


def test_target_groups_keep_their_order_and_unknown_or_pruned_names_are_refused():
    assert binning.resolve_targets(NAMES, ["d", "a", "c"]) == ["d", "a", "c"]
    assert binning.resolve_targets(NAMES, ["c", "c", "a"]) == ["c", "a"]
    with pytest.raises(binning.BinningError, match="zz"):
        binning.resolve_targets(NAMES, ["a", "zz"])
    with pytest.raises(binning.BinningError, match="a"):           # pruned by --min-hits: not estimated
        binning.resolve_targets(["b", "c"], ["a"])


def test_min_abundance_drops_below_and_keeps_ties():
    assert binning.filter_min_abundance(NAMES, NAMES, THETA, 0.2) == ["a", "b", "c"]
    assert binning.filter_min_abundance(["d", "b"], NAMES, THETA, 0.2) == ["b"]
    assert binning.filter_min_abundance(NAMES, NAMES, THETA, 0.0) == NAMES
    assert binning.filter_min_abundance(NAMES, NAMES, THETA, 0.6) == []


def test_thresholds_are_one_minus_theta_of_the_target_rows():
    np.testing.assert_array_equal(binning.thresholds([3, 0], THETA), [1.0 - 0.1, 1.0 - 0.5])
    assert binning.thresholds([], THETA).shape == (0,)


def test_bin_paths():
    assert binning.bin_path("dir/sub/p", "g1") == "dir/sub/g1.bin"
    assert binning.bin_path("/abs/p", "g1") == "/abs/g1.bin"
    assert binning.bin_path("p", "g1") == "./g1.bin"
    assert binning.bin_path("", "g1") == "./g1.bin"                # no -o
    assert binning.bin_path("dir/", "g1") == "dir/g1.bin"


def test_writer_format(tmp_path):
    ids = np.array([0, 7, 10, 99, 100, 123456, 4294967295, 1000000000, 9], np.uint32)
    p = tmp_path / "x.bin"
    binning.write_bin(str(p), ids)
    assert p.read_bytes() == b"".join(b"%d\n" % int(x) for x in ids)
    binning.write_bin(str(tmp_path / "empty.bin"), np.zeros(0, np.uint32))
    assert (tmp_path / "empty.bin").read_bytes() == b""


def test_writer_matches_plain_formatting_on_random_ids():
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(0, 2**32, 20000, dtype=np.uint64),
                          10 ** rng.integers(0, 10, 2000, dtype=np.uint64) - rng.integers(0, 2, 2000, dtype=np.uint64)])
    ids = ids.astype(np.uint32)
    assert binning.format_ids(ids) == "".join(f"{int(x)}\n" for x in ids).encode()
