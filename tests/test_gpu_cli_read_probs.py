"""GPU: --write-read-probs / --probs-threshold through both drivers, on the four-cluster toy of tests/test_gpu_cli_assign.py:
`python -m msweep_amd` and msweep_mini write the same bytes -- one grouping column, two (`_0_`, `_1_`), under --compress z
(compared after gunzip), with --min-hits dropping a group (the header's indices are the estimated rows) and with a bootstrap
behind it --; the bootstrap leaves the file as it is; the rows are what Core.sparse_probs gives when called directly; and
every other output file of the run is byte-identical to the run without the flag."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from msweep_amd import read_probs
from msweep_amd.__main__ import main
from msweep_amd.alignment import Alignment
from msweep_amd.core import Core
from msweep_amd.reference import read_reference
from test_gpu_cli_assign import _toy

pytestmark = pytest.mark.gpu

FILE = "r_read_probs.tsv"


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("read_probs_toy")
    _toy(d)
    return {"dir": d}


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    """msweep_amd/cpp/msweep_mini.cpp, built for this module"""
    out = str(tmp_path_factory.mktemp("readprobsmini") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _args(toy, clustering="clustering.txt"):
    d = toy["dir"]
    return ["--themisto-1", str(d / "toy_1.txt"), "--themisto-2", str(d / "toy_2.txt"), "-i", str(d / clustering)]


def _run_py(toy, name, extra, clustering="clustering.txt"):
    out = toy["dir"] / name
    os.makedirs(out)
    assert main(_args(toy, clustering) + ["-o", str(out / "r")] + extra) == 0
    return out


def _run_cc(toy, mini_binary, name, extra, clustering="clustering.txt"):
    out = toy["dir"] / name
    os.makedirs(out)
    p = subprocess.run([mini_binary] + _args(toy, clustering) + ["-o", str(out / "r")] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return out, p.stderr


def _files(d):
    return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


def _split(text):
    """(header lines, rows) of a read_probs file"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    head = [ln for ln in lines[:-1] if ln.startswith(b"#")]
    assert lines[:len(head)] == head
    return head, lines[len(head):-1]


@pytest.fixture(scope="module")
def plain_run(toy):
    return _run_py(toy, "py_plain", ["--write-read-probs"])


def test_the_file_and_the_rows_of_the_core(toy, plain_run):
    text = open(plain_run / FILE, "rb").read()
    head, rows = _split(text)
    assert b"\n".join(head) + b"\n" == read_probs.header(0.001, NAMES_IN_ORDER(toy))
    assert head[0] == b"#threshold\t0.001" and head[-1] == b"#read_id\tgroup\tprob" and len(head) == 6
    # every row: a read id, a group of the header, a probability in [0.001, 1]; ascending ids, ascending groups within an id
    keys = [(int(a), int(b)) for a, b, _ in (r.split(b"\t") for r in rows)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert {g for _, g in keys} == {0, 1, 2, 3}
    assert all(0.0009995 <= float(r.split(b"\t")[2]) <= 1.0 for r in rows)
    # the rows are Core.sparse_probs by read on the same alignment, grouping and solve
    d = toy["dir"]
    grouping = read_reference(open(d / "clustering.txt"))
    with Core(0) as core:
        core.set_pack_schedule(False)       # as the driver sets it without a bootstrap
        dev = core.read_alignment([str(d / "toy_1.txt"), str(d / "toy_2.txt")], len(grouping.group_indicators))
        kept, _, _ = core.build_likelihood_aln(dev, grouping.group_indicators, grouping.get_sizes(), want_logc=False)
        core.solve(None, np.ones(kept))
        sp = core.sparse_probs(dev, 0.001)
        direct = b"".join(sp.pieces())
        assert sp.rows == dev.n_aligned
    assert b"\n".join(rows) + b"\n" == direct
    # reads that did not pseudoalign give no line
    aln = Alignment(len(grouping.group_indicators))
    aln.read("intersection", [open(d / "toy_1.txt"), open(d / "toy_2.txt")])
    aln.collapse()
    assert int(np.sum(aln.ec_counts)) == dev.n_aligned < dev.n_reads
    assert len({i for i, _ in keys}) == dev.n_aligned      # (at 0.001 with four groups every aligned read keeps a cell)


def NAMES_IN_ORDER(toy):
    return read_reference(open(toy["dir"] / "clustering.txt")).get_names()


def test_both_drivers_one_column(toy, mini_binary, plain_run):
    cc, _ = _run_cc(toy, mini_binary, "cc_plain", ["--write-read-probs"])
    assert _files(cc) == _files(plain_run) and FILE in _files(cc)


def test_both_drivers_threshold_and_verbose(toy, mini_binary):
    py = _run_py(toy, "py_half", ["--write-read-probs", "--probs-threshold", "0.5"])
    cc, err = _run_cc(toy, mini_binary, "cc_half", ["--write-read-probs", "--probs-threshold", "0.5", "--verbose"])
    assert _files(cc) == _files(py)
    head, rows = _split(_files(py)[FILE])
    assert head[0] == b"#threshold\t0.5" and rows and all(float(r.split(b"\t")[2]) >= 0.4999995 for r in rows)
    assert "read probabilities: " in err and f"{len(rows)} cells at or above 0.5" in err


def test_both_drivers_two_columns(toy, mini_binary):
    py = _run_py(toy, "py_two", ["--write-read-probs"], "two_columns.txt")
    cc, _ = _run_cc(toy, mini_binary, "cc_two", ["--write-read-probs"], "two_columns.txt")
    f = _files(py)
    assert _files(cc) == f
    assert "r_0_read_probs.tsv" in f and "r_1_read_probs.tsv" in f and FILE not in f
    assert _split(f["r_0_read_probs.tsv"])[0][1:5] == [b"#group\t%d\t%s" % (g, n.encode()) for g, n in enumerate(NAMES_IN_ORDER(toy))]
    assert len(_split(f["r_1_read_probs.tsv"])[0]) == 4       # two groups in the second column


def test_both_drivers_compressed(toy, mini_binary, plain_run):
    py = _run_py(toy, "py_z", ["--write-read-probs", "--compress", "z"])
    cc, _ = _run_cc(toy, mini_binary, "cc_z", ["--write-read-probs", "--compress", "z"])
    assert _files(cc) == _files(py)
    assert FILE + ".gz" in _files(py) and FILE not in _files(py)
    assert gzip.decompress(_files(py)[FILE + ".gz"]) == _files(plain_run)[FILE]


def test_both_drivers_min_hits_drops_a_group(toy, mini_binary, oracle):
    d = toy["dir"]
    grouping = read_reference(open(d / "clustering.txt"))
    aln = Alignment(len(grouping.group_indicators))
    aln.read("intersection", [open(d / "toy_1.txt"), open(d / "toy_2.txt")])
    aln.collapse()
    counts = oracle.group_counts(aln.ec_tptr, aln.ec_targets, grouping.group_indicators, grouping.get_n_groups())
    for min_hits in range(50, 20000, 50):
        _, mask = oracle.fill_ll_mat(counts, aln.ec_counts, grouping.get_sizes(), min_hits=min_hits)
        if not all(mask):
            break
    est = [n for n, m in zip(grouping.get_names(), mask) if m]
    assert 2 <= len(est) < 4
    py = _run_py(toy, "py_min_hits", ["--write-read-probs", "--min-hits", str(min_hits)])
    cc, _ = _run_cc(toy, mini_binary, "cc_min_hits", ["--write-read-probs", "--min-hits", str(min_hits)])
    assert _files(cc) == _files(py)
    head, rows = _split(_files(py)[FILE])
    assert head[1:-1] == [b"#group\t%d\t%s" % (g, n.encode()) for g, n in enumerate(est)]      # the estimated rows
    assert {int(r.split(b"\t")[1]) for r in rows} <= set(range(len(est)))


def test_a_bootstrap_leaves_the_file_as_it_is(toy, mini_binary, plain_run):
    py = _run_py(toy, "py_boot", ["--write-read-probs", "--iters", "2", "--seed", "7"])
    cc, _ = _run_cc(toy, mini_binary, "cc_boot", ["--write-read-probs", "--iters", "2", "--seed", "7"])
    assert _files(cc) == _files(py)
    assert _files(py)[FILE] == _files(plain_run)[FILE]
    assert b"#bootstrap_iters:\t2" in _files(py)["r_abundances.txt"]


def test_the_other_outputs_do_not_change(toy):
    extra = ["--bin-reads", "--write-unassigned", "--write-assignment-table", "--write-probs", "--write-likelihood", "--iters", "2",
             "--seed", "7"]
    without = _files(_run_py(toy, "py_all_without", extra))
    with_flag = _files(_run_py(toy, "py_all_with", extra + ["--write-read-probs"]))
    assert set(with_flag) == set(without) | {FILE} and len(without) >= 8
    for f, data in without.items():
        assert with_flag[f] == data, f


def test_samples_write_a_file_per_sample(toy, mini_binary, plain_run):
    """--samples: every sample's file is the one a single run with its -o and --themisto writes, in both drivers"""
    d = toy["dir"]
    single = toy["dir"] / "py_single_strand"
    os.makedirs(single)
    assert main(["--themisto-1", str(d / "toy_1.txt"), "-i", str(d / "clustering.txt"), "-o", str(single / "r"), "--write-read-probs"]) == 0
    want = {"a": _files(plain_run), "b": _files(single)}
    assert want["a"][FILE] != want["b"][FILE]
    for driver in ("py", "cc"):
        outs = {k: d / f"{driver}_samples_{k}" for k in ("a", "b")}
        for o in outs.values():
            os.makedirs(o)
        m = d / f"{driver}_samples.tsv"
        m.write_text(f"{outs['a'] / 'r'}\t{d / 'toy_1.txt'},{d / 'toy_2.txt'}\n{outs['b'] / 'r'}\t{d / 'toy_1.txt'}\n")
        argv = ["-i", str(d / "clustering.txt"), "--samples", str(m), "--write-read-probs"]
        if driver == "py":
            assert main(argv) == 0
        else:
            p = subprocess.run([mini_binary] + argv, capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stdout + p.stderr
        for k, o in outs.items():
            assert _files(o) == want[k], (driver, k)

