"""CPU: every tab-separated column of the -i file is a grouping of its own (include/Reference.hpp:67-94) -- the
reader of all columns, the names of the per-grouping outputs (src/OutfileDesignator.cpp:64-74,116-123) and the
refusal of --read-likelihood with more than one grouping (src/mSWEEP.cpp:360-362), which comes before a device is
touched."""
import io

import numpy as np
import pytest

from msweep_amd import __main__ as cli
from msweep_amd.reference import output_path, read_reference, read_references

# three columns; an empty middle field (line 3: the group named "") and a trailing tab (line 4: adds no field)
TEXT = "a\tx\tp\nb\tx\tq\na\t\tp\nc\ty\tq\t\nb\tx\tp\n"


def test_every_column_is_the_grouping_read_reference_gives_for_it():
    gs = read_references(io.StringIO(TEXT))
    assert len(gs) == 3
    for i, g in enumerate(gs):
        want = read_reference(io.StringIO(TEXT), "\t", column=i)
        assert g.get_names() == want.get_names()
        np.testing.assert_array_equal(g.get_sizes(), want.get_sizes())
        np.testing.assert_array_equal(g.group_indicators, want.group_indicators)
        assert g.group_indicators.dtype == np.uint32 and g.get_sizes().dtype == np.uint64
    assert gs[0].get_names() == ["a", "b", "c"] and gs[0].get_sizes().tolist() == [2, 2, 1]
    assert gs[1].get_names() == ["x", "", "y"] and gs[1].get_sizes().tolist() == [3, 1, 1]      # the empty field is a group
    assert gs[2].get_names() == ["p", "q"] and gs[2].group_indicators.tolist() == [0, 1, 0, 1, 0]


def test_a_single_column_is_what_it_was():
    text = "g1\ng2\n\ng1\n"         # (an empty line: the group named "", as read_reference has always read it)
    (g,) = read_references(io.StringIO(text))
    want = read_reference(io.StringIO(text))
    assert g.get_names() == want.get_names() == ["g1", "g2", ""]
    np.testing.assert_array_equal(g.group_indicators, want.group_indicators)
    # another delimiter; the last line without its line end
    gs = read_references(io.StringIO("a,b\nc,b"), ",")
    assert [g.get_names() for g in gs] == [["a", "c"], ["b"]]


@pytest.mark.parametrize("text, message", [
    ("a\tx\nb\n", "The grouping has 1 columns on line 2, 2 on line 1"),
    ("a\tx\nb\ty\tz\n", "The grouping has 3 columns on line 2, 2 on line 1"),
    ("a\nb\nc\tx\n", "The grouping has 2 columns on line 3, 1 on line 1"),
    ("a\tx\n\nb\ty\n", "The grouping has 1 columns on line 2, 2 on line 1"),
    ("", "The grouping contains 0 reference sequences"),
])
def test_jagged_and_empty_files_are_refused(text, message):
    with pytest.raises(RuntimeError) as ex:
        read_references(io.StringIO(text))
    assert str(ex.value) == message


def test_output_names():
    """today's names for one grouping, the index after the prefix for several; no prefix: the bare name"""
    for name in ("abundances.txt", "probs.tsv", "likelihoods.tsv", "bitseq_likelihoods.tsv"):
        assert output_path("out/P", 0, 1, name) == "out/P_" + name
        assert output_path("out/P", 0, 3, name) == "out/P_0_" + name
        assert output_path("out/P", 2, 3, name) == "out/P_2_" + name
        assert output_path("", 1, 3, name) == name and output_path("", 0, 1, name) == name


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


def test_read_likelihood_with_two_groupings_is_refused_before_the_device(no_device, capsys, tmp_path):
    ind = tmp_path / "two.tsv"
    ind.write_text("a\tx\nb\tx\na\ty\n")
    rc = cli.main(["-i", str(ind), "--read-likelihood", str(tmp_path / "none.tsv"), "-o", str(tmp_path / "o")])
    assert rc == 1
    assert capsys.readouterr().err == ("Reading the likelihoods failed:\n  Using more than one grouping with --read-likelihood "
                                       "is not yet implemented.\nexiting\n")
    assert [p.name for p in tmp_path.iterdir()] == ["two.tsv"]


def test_read_likelihood_with_a_jagged_indicator_file(no_device, capsys, tmp_path):
    """with --read-likelihood the indicators are read in front of the device: a file the reader refuses ends the run there"""
    ind = tmp_path / "jagged.tsv"
    ind.write_text("a\tx\nb\n")
    rc = cli.main(["-i", str(ind), "--read-likelihood", str(tmp_path / "none.tsv")])
    assert rc == 1
    assert capsys.readouterr().err == ("Reading the pseudoalignments failed:\n  The grouping has 1 columns on line 2, 2 on line 1\n"
                                       "exiting\n")
