"""GPU: the matrix outputs of both drivers with the text formatted on the device (msw_core_text_block) -- on the toy of
tests/test_gpu_cli_toy.py, in blocks of 37 classes (MSWEEP_TEXT_BLOCK), against the same run with the host formatting
kept (MSWEEP_HOST_TEXT=1); and --write-likelihood-bitseq against a Python rendering of include/Likelihood.hpp:275-311
from get_dense_logl and the read counts, `Ntotal` quirk included, identical between `python -m msweep_amd` and
msweep_mini.

probs.tsv holds "%g" of the DEVICE's exp(gamma) on one side and of the host's on the other: they can differ where a
rounding boundary of the six digits lies between two neighbouring doubles (about one cell in 10^10).  On this fixed
seeded toy they do not; a difference would show at the first run and is answered by another seed, not a looser
comparison."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from msweep_amd.__main__ import bitseq_total, main
from msweep_amd.core import Core
from msweep_amd.likelihood import from_device_alignment
from msweep_amd.reference import read_reference
from test_gpu_cli_toy import _toy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini_text") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _common(tmp_path):
    return ["--themisto-1", str(tmp_path / "toy_1.txt"), "--themisto-2", str(tmp_path / "toy_2.txt"),
            "-i", str(tmp_path / "clustering.txt")]


def _run_mini(mini_binary, args, env=None):
    p = subprocess.run([mini_binary] + args, capture_output=True, text=True, timeout=120, env={**os.environ, **(env or {})})
    assert p.returncode == 0, p.stdout + p.stderr
    return p


@pytest.mark.parametrize("extra", [[], ["--min-hits", "400"]])
def test_device_text_equals_host_text_in_both_drivers(tmp_path, mini_binary, monkeypatch, extra):
    _toy(tmp_path)
    args = _common(tmp_path) + ["--write-probs", "--write-likelihood"] + extra
    monkeypatch.setenv("MSWEEP_TEXT_BLOCK", "37")
    assert main(args + ["-o", str(tmp_path / "py_dev")]) == 0
    _run_mini(mini_binary, args + ["-o", str(tmp_path / "cc_dev")], {"MSWEEP_TEXT_BLOCK": "37"})
    monkeypatch.setenv("MSWEEP_HOST_TEXT", "1")
    assert main(args + ["-o", str(tmp_path / "py_host")]) == 0
    _run_mini(mini_binary, args + ["-o", str(tmp_path / "cc_host")], {"MSWEEP_HOST_TEXT": "1"})
    for name in ("likelihoods.tsv", "probs.tsv", "abundances.txt"):
        want = (tmp_path / ("py_host_" + name)).read_bytes()
        assert len(want) > 100 and want.count(b"\n") > (37 if name != "abundances.txt" else 4), name
        for run in ("py_dev", "cc_dev", "cc_host"):
            assert (tmp_path / (run + "_" + name)).read_bytes() == want, (run, name)
    if extra:
        head = (tmp_path / "py_dev_probs.tsv").read_text().splitlines()[0].split("\t")
        rows = (tmp_path / "py_dev_probs.tsv").read_text().splitlines()[1:-1]
        assert len(head) == 5 and all(len(r.split("\t")) == 5 for r in rows)      # the groups below --min-hits: "\t0"


def _render_bitseq(tmp_path):
    """include/Likelihood.hpp:275-311 from the library's own likelihood bits and the read counts"""
    with open(tmp_path / "clustering.txt") as f:
        grouping = read_reference(f)
    with Core(0) as core:
        aln = core.read_alignment([str(tmp_path / "toy_1.txt"), str(tmp_path / "toy_2.txt")], len(grouping.group_indicators))
        from_device_alignment(core, aln, grouping.group_indicators, grouping.get_sizes())
        L = core.get_dense_logl()
        counts = [int(c) for c in aln.ec_counts()]
    total = 0
    for c in counts:                                       # std::accumulate from an int 0: truncated after every class
        total = int(float(total) + math.exp(math.log(float(c))))
    G = L.shape[0]
    out = [f"# Ntotal {total}", f"# Nmap {total}", f"# M {G}", "# LOGFORMAT (probabilities saved on log scale.)",
           "# r_name num_alignments (tr_id prob )^*{num_alignments}"]
    read_id = 1
    for j, c in enumerate(counts):
        tail = f"{G + 1} " + "".join(f"{g + 1} {'%g' % L[g, j]} " for g in range(G)) + "0 -10000.00"
        for _ in range(c):
            out.append(f"{read_id} {tail}")
            read_id += 1
    return ("\n".join(out) + "\n").encode(), counts


def test_bitseq_likelihood_file(tmp_path, mini_binary, monkeypatch):
    _toy(tmp_path)
    want, counts = _render_bitseq(tmp_path)
    assert want.count(b"\n") == 5 + sum(counts)
    monkeypatch.setenv("MSWEEP_TEXT_BLOCK", "37")
    args = _common(tmp_path) + ["--write-likelihood-bitseq", "--no-fit-model"]
    assert main(args + ["-o", str(tmp_path / "py")]) == 0
    _run_mini(mini_binary, args + ["-o", str(tmp_path / "cc")], {"MSWEEP_TEXT_BLOCK": "37"})
    assert (tmp_path / "py_bitseq_likelihoods.tsv").read_bytes() == want
    assert (tmp_path / "cc_bitseq_likelihoods.tsv").read_bytes() == want
    assert not (tmp_path / "py_abundances.txt").exists() and not (tmp_path / "cc_abundances.txt").exists()
    # the host formatting of both drivers writes the same file
    monkeypatch.setenv("MSWEEP_HOST_TEXT", "1")
    assert main(args + ["-o", str(tmp_path / "pyh")]) == 0
    _run_mini(mini_binary, args + ["-o", str(tmp_path / "cch")], {"MSWEEP_HOST_TEXT": "1"})
    assert (tmp_path / "pyh_bitseq_likelihoods.tsv").read_bytes() == want
    assert (tmp_path / "cch_bitseq_likelihoods.tsv").read_bytes() == want


def test_both_likelihood_flags_write_only_the_bitseq_file(tmp_path, mini_binary):
    _toy(tmp_path, n_reads=300)
    args = _common(tmp_path) + ["--write-likelihood", "--write-likelihood-bitseq"]
    assert main(args + ["-o", str(tmp_path / "py")]) == 0
    _run_mini(mini_binary, args + ["-o", str(tmp_path / "cc")])
    for run in ("py", "cc"):
        assert (tmp_path / (run + "_bitseq_likelihoods.tsv")).exists() and (tmp_path / (run + "_abundances.txt")).exists()
        assert not (tmp_path / (run + "_likelihoods.tsv")).exists()
    assert (tmp_path / "py_bitseq_likelihoods.tsv").read_bytes() == (tmp_path / "cc_bitseq_likelihoods.tsv").read_bytes()


def test_bitseq_from_a_likelihood_file(tmp_path, mini_binary):
    """--read-likelihood ... --write-likelihood-bitseq --no-fit-model: the dense flavour, the counts of the file"""
    _toy(tmp_path, n_reads=300)
    assert main(_common(tmp_path) + ["--write-likelihood", "--no-fit-model", "-o", str(tmp_path / "w")]) == 0
    rows = [ln.split("\t") for ln in (tmp_path / "w_likelihoods.tsv").read_text().splitlines()]
    counts = [int(r[0]) for r in rows]
    rd = ["-i", str(tmp_path / "clustering.txt"), "--read-likelihood", str(tmp_path / "w_likelihoods.tsv"),
          "--write-likelihood-bitseq", "--no-fit-model"]
    assert main(rd + ["-o", str(tmp_path / "py")]) == 0
    _run_mini(mini_binary, rd + ["-o", str(tmp_path / "cc")])
    got = (tmp_path / "py_bitseq_likelihoods.tsv").read_bytes()
    assert got == (tmp_path / "cc_bitseq_likelihoods.tsv").read_bytes()
    lines = got.decode().splitlines()
    total = bitseq_total(counts)
    assert lines[:3] == [f"# Ntotal {total}", f"# Nmap {total}", "# M 4"] and len(lines) == 5 + sum(counts)
    # the six digits of the file survive the round trip: every class's tail repeats its line of the likelihood file
    first = np.cumsum([0] + counts[:-1])
    for j in (0, len(counts) // 2, len(counts) - 1):
        cells = lines[5 + first[j]].split(" ")
        assert cells[0] == str(first[j] + 1) and cells[1] == "5" and cells[-2:] == ["0", "-10000.00"]
        assert cells[2:-2] == [v for g in range(4) for v in (str(g + 1), rows[j][1 + g])]
    assert total <= sum(counts)


def test_ntotal_restates_the_truncating_sum():
    assert bitseq_total([5]) == 4                      # exp(log 5) = 4.999...: truncated
    assert bitseq_total([1, 2, 3]) == 6
    assert bitseq_total([3, 5]) == 7                   # 3 + 4.999... = 7.999...: truncated again
    assert bitseq_total([]) == 0
