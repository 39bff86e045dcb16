"""CPU: --write-unassigned / --write-assignment-table of `python -m msweep_amd` are judged before a device is touched --
without --bin-reads they are refused with status 1 in the words of the binning error -- and what binning.py decides around
them: where the unassigned bin lies, the table's header, the rows per block, the group name that would collide."""
import argparse

import numpy as np
import pytest

from msweep_amd import __main__ as cli
from msweep_amd import binning


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


def _args(tmp_path):
    return ["-i", str(tmp_path / "none.txt"), "--themisto-1", "a", "-o", str(tmp_path / "o")]


@pytest.mark.parametrize("flag", ["--write-unassigned", "--write-assignment-table"])
def test_the_flags_need_bin_reads(no_device, capsys, tmp_path, flag):
    rc = cli.main(_args(tmp_path) + [flag])
    err = capsys.readouterr().err
    assert rc == 1
    assert err == f"Binning the reads failed:\n  {flag} needs --bin-reads\nexiting\n"


def test_read_likelihood_stays_refused_first(no_device, capsys, tmp_path):
    rc = cli.main(["-i", str(tmp_path / "none.txt"), "--read-likelihood", "x.tsv", "--bin-reads", "--write-unassigned",
                   "--write-assignment-table"])
    assert rc == 1
    assert capsys.readouterr().err == "Binning the reads failed:\n  --read-likelihood can't be used with --bin-reads\nexiting\n"


def test_valid_flags_pass_the_check(monkeypatch, tmp_path):
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "Core", reached)
    with pytest.raises(Reached):
        cli.main(_args(tmp_path) + ["--bin-reads", "--write-unassigned", "--write-assignment-table"])


def test_unassigned_path_lies_beside_the_bins():
    assert binning.unassigned_path("out/p") == "out/unassigned_reads.bin"
    assert binning.unassigned_path("p") == "./unassigned_reads.bin"
    assert binning.unassigned_path("/a/b/c") == "/a/b/unassigned_reads.bin"
    assert binning.extract_path("out/p", binning.UNASSIGNED, 2) == "out/unassigned_reads_2.fastq"


def test_table_header_bytes():
    assert binning.table_header([]) == b"#read_id\n"
    assert binning.table_header(["clust3"]) == b"#read_id\tclust3\n"
    assert binning.table_header(["b", "a", ""]) == b"#read_id\tb\ta\t\n"
    names = [f"g{i}" for i in range(10 ** 6)]
    head = binning.table_header(names)
    assert head.startswith(b"#read_id\tg0\tg1\t") and head.endswith(b"\tg999999\n") and head.count(b"\t") == 10 ** 6


def test_table_block_rows():
    assert binning.table_block_rows(0) == 1 << 20                      # 11 bytes per row: the cap of 2^20 rows holds
    assert binning.table_block_rows(1) == 1 << 20
    assert binning.table_block_rows(122) == 1 << 20                    # 255 bytes per row: still 2^20 rows in 256 MiB
    assert binning.table_block_rows(123) == (256 << 20) // 257
    assert binning.table_block_rows(10 ** 6) == (256 << 20) // (11 + 2 * 10 ** 6) == 134
    assert binning.table_block_rows(1 << 40) == 1
    for n in (0, 1, 123, 10 ** 6):                                     # the worst case of a block stays within 256 MiB
        assert binning.table_block_rows(n) * (11 + 2 * n) <= 256 << 20


def test_all_thresholds():
    np.testing.assert_array_equal(binning.all_thresholds([0.25, 0.5, 0.0]), [0.75, 0.5, 1.0])
    theta = np.array([0.1, 0.2, 0.7])
    np.testing.assert_array_equal(binning.all_thresholds(theta)[[2, 0]], binning.thresholds([2, 0], theta))


def test_a_group_named_like_the_unassigned_bin_is_refused(capsys):
    with pytest.raises(binning.BinningError, match="unassigned_reads"):
        binning.check_unassigned_name(["a", "unassigned_reads"])
    binning.check_unassigned_name(["a", "unassigned_reads2"])

    class NoCore:
        def __getattr__(self, name):
            raise AssertionError("the refusal must come before the device is asked: " + name)

    a = argparse.Namespace(target_groups=None, min_abundance=None, write_unassigned=True, write_assignment_table=False,
                           verbose=False, compress="plaintext", prefix="p", extract_reads=None)
    rc = cli.bin_reads(NoCore(), None, ["a", "unassigned_reads"], np.array([0.5, 0.5]), a, "p_reads_to_groups.tsv")
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("Binning the reads failed:\n  ") and "unassigned_reads" in err
