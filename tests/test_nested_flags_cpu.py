"""CPU: --nested is judged before a device is touched, in both drivers and in the same words -- one column, the flags it
refuses, a group name with '/', two label paths whose stems are one name -- and the naming rules as pure functions
(msweep_amd/nested.py; msweep_amd/cpp/nested_tree.hpp is the same for msweep_mini, which is run here as a whole program:
every refusal ends it before it asks for a device)."""
import os
import subprocess

import pytest

from msweep_amd import __main__ as cli
from msweep_amd import nested

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _both(capsys, mini_binary, argv, message):
    """the Python driver and msweep_mini refuse `argv` with the same three lines and status 1"""
    want = f"Parsing arguments failed:\n  {message}\nexiting\n"
    rc = cli.main(argv)
    assert rc == 1 and capsys.readouterr().err == want
    p = subprocess.run([mini_binary] + argv, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr == want and p.stdout == ""


def _indicators(tmp_path, text, name="groups.tsv"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


TWO = "a\tx\na\ty\nb\tz\nb\tw\n"


def test_one_column(no_device, capsys, mini_binary, tmp_path):
    i = _indicators(tmp_path, "a\nb\na\n")
    _both(capsys, mini_binary, ["-i", i, "--themisto-1", "x.txt", "--nested"], f"--nested needs at least two columns in -i ({i} has 1)")


@pytest.mark.parametrize("flag, extra", [("--read-likelihood", ["--read-likelihood", "l.tsv"]), ("--no-fit-model", ["--no-fit-model"]),
                                         ("--alphas", ["--alphas", "1,1"]),
                                         ("--write-unassigned", ["--bin-reads", "--write-unassigned"]),
                                         ("--write-assignment-table", ["--bin-reads", "--write-assignment-table"]),
                                         ("--print-probs", ["--print-probs"])])
def test_flags_nested_refuses(no_device, capsys, mini_binary, tmp_path, flag, extra):
    i = _indicators(tmp_path, TWO)
    _both(capsys, mini_binary, ["-i", i, "--themisto-1", "x.txt", "--nested"] + extra, f"--nested can't be used with {flag}")


def test_the_first_refused_flag_is_named(no_device, capsys, mini_binary, tmp_path):
    i = _indicators(tmp_path, TWO)
    _both(capsys, mini_binary, ["-i", i, "--themisto-1", "x.txt", "--print-probs", "--alphas", "1,1", "--nested", "--no-fit-model"],
          "--nested can't be used with --no-fit-model")


TREES = [
    ("a\tx\nb/c\ty\n", "the group name b/c contains '/' (--nested names files by group)"),
    ("a\tx\na\tu/v\n", "the group name u/v contains '/' (--nested names files by group)"),
    # stem equal to stem: two nodes of a three-column file would write the same files
    ("a_b\tc\tp\na\tb_c\tq\n", "the label paths a_b > c and a > b_c give the same name `a_b_c`"),
    # a bin below the root named like a bin of the root
    ("a\tb\na_b\tc\n", "the label paths a > b and a_b give the same name `a_b`"),
    ("a_b\tc\na\tb\n", "the label paths a_b and a > b give the same name `a_b`"),
    # a group without a name at level 0 is the root's own stem
    ("\tx\na\ty\n", "the label paths (root) and  give the same name ``"),
]


@pytest.mark.parametrize("text, message", TREES)
def test_trees_nested_refuses(no_device, capsys, mini_binary, tmp_path, text, message):
    i = _indicators(tmp_path, text)
    _both(capsys, mini_binary, ["-i", i, "--themisto-1", "x.txt", "--nested"], f"{i}: {message}")


def test_with_samples_the_tree_is_judged_before_the_device_too(no_device, capsys, mini_binary, tmp_path):
    i = _indicators(tmp_path, "a\tb\na_b\tc\n")
    m = tmp_path / "samples.tsv"
    m.write_text("s1/p\tx.txt\ns2/p\ty.txt\n")
    _both(capsys, mini_binary, ["-i", i, "--samples", str(m), "--nested"],
          f"{i}: the label paths a > b and a_b give the same name `a_b`")


def test_an_unreadable_indicator_file(no_device, capsys, mini_binary, tmp_path):
    i = _indicators(tmp_path, "a\tx\nb\n")
    want = "Reading the pseudoalignments failed:\n  The grouping has 1 columns on line 2, 2 on line 1\nexiting\n"
    assert cli.main(["-i", i, "--themisto-1", "x.txt", "--nested"]) == 1 and capsys.readouterr().err == want
    p = subprocess.run([mini_binary, "-i", i, "--themisto-1", "x.txt", "--nested"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr == want


def test_a_good_tree_reaches_the_device(monkeypatch, tmp_path):
    class Reached(Exception):
        pass

    def core(device):
        raise Reached()
    monkeypatch.setattr(cli, "Core", core)
    i = _indicators(tmp_path, TWO)
    with pytest.raises(Reached):
        cli.main(["-i", i, "--themisto-1", "x.txt", "--nested", "--bin-reads", "--write-probs", "--min-abundance", "0.1"])


def test_stems_paths_and_bin_names():
    assert nested.stem([]) == "" and nested.stem(["sp1"]) == "sp1" and nested.stem(["sp1", "lin_a"]) == "sp1_lin_a"
    assert nested.show([]) == "(root)" and nested.show(["a", "b"]) == "a > b"
    # the root's names are the single-column names
    assert nested.node_path("out/P", "", "abundances.txt") == "out/P_abundances.txt" == cli.output_path("out/P", 0, 1, "abundances.txt")
    assert nested.node_path("out/P", "sp1", "probs.tsv") == "out/P_sp1_probs.tsv"
    assert nested.node_path("out/P", "sp1_lin_a", "abundances.txt") == "out/P_sp1_lin_a_abundances.txt"
    assert nested.node_path("", "", "likelihoods.tsv") == "likelihoods.tsv" and nested.node_path("", "sp1", "likelihoods.tsv") == "sp1_likelihoods.tsv"
    assert nested.bin_name("", "sp1") == "sp1" and nested.bin_name("sp1", "lin_a") == "sp1_lin_a"
    assert nested.bin_name("sp1_lin_a", "st9") == "sp1_lin_a_st9"


def test_check_tree_takes_what_does_not_collide():
    rows = [["a", "x", "p"], ["a", "x", "q"], ["a", "y", "p"], ["b", "x", "p"], ["b", "z", "a"]]
    nested.check_tree("f", rows)                   # the same name below two parents is two stems
    nested.check_tree("f", [["a", "a"], ["b", "a"]])
    nested.check_flags(["--bin-reads", "--write-probs"])
    with pytest.raises(nested.NestedError, match="give the same name `a_a`"):
        nested.check_tree("f", [["a", "a"], ["a_a", "b"]])
