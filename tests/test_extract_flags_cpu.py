"""CPU: --extract-reads of `python -m msweep_amd` is judged before a device is touched -- without --bin-reads, or with an
empty path in its list, it is refused with status 1 in the words of the other argument errors.  The restatement the GPU
tests of the extraction take their expected bytes from (extract_restated) is pinned here on a literal, and the host loops
behind MSWEEP_HOST_EXTRACT=1 are run by their stand-alone program."""
import os
import subprocess

import pytest

from conftest import ROOT
from msweep_amd import __main__ as cli
from msweep_amd import binning


def fastq_records(text):
    """The records of `text` (bytes of a FASTQ file): its lines with their line ends, grouped by four."""
    parts = bytes(text).split(b"\n")        # (on '\n' alone: a '\r' belongs to its line)
    lines = [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
    assert len(lines) % 4 == 0
    return [b"".join(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def extract_restated(text, ids):
    """The records of `text` whose 0-based number is in `ids`, verbatim, in file order, each once."""
    records = fastq_records(text)
    return b"".join(records[i] for i in sorted(set(int(x) for x in ids)))


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


def _args(tmp_path):
    return ["-i", str(tmp_path / "none.txt"), "--themisto-1", "a", "-o", str(tmp_path / "o")]


def test_extract_reads_needs_bin_reads(no_device, capsys, tmp_path):
    rc = cli.main(_args(tmp_path) + ["--extract-reads", "r1.fq,r2.fq"])
    err = capsys.readouterr().err
    assert rc == 1
    assert err == "Extracting the reads failed:\n  --extract-reads needs --bin-reads\nexiting\n"


@pytest.mark.parametrize("value", ["", "r1.fq,", ",r2.fq", "r1.fq,,r2.fq"])
def test_an_empty_path_in_the_list_is_refused(no_device, capsys, tmp_path, value):
    rc = cli.main(_args(tmp_path) + ["--bin-reads", "--extract-reads", value])
    err = capsys.readouterr().err
    assert rc == 1
    assert err == "Extracting the reads failed:\n  --extract-reads has an empty path in its list\nexiting\n"


def test_valid_flags_pass_the_check(monkeypatch, tmp_path):
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "Core", reached)
    with pytest.raises(Reached):
        cli.main(_args(tmp_path) + ["--bin-reads", "--extract-reads", "r1.fq,r2.fq.gz"])


def test_extract_path_lies_beside_the_bins():
    assert binning.extract_path("out/p", "clust1", 1) == "out/clust1_1.fastq"
    assert binning.extract_path("p", "g", 2) == "./g_2.fastq"


FIVE = (b"@r0\nACGT\n+\nIIII\n"
        b"@r1\nAC\n+r1\n@+\n"          # a quality line that begins with '@'
        b"@\n\n+\n\n"                    # six bytes
        b"@r3 x\nA\n+\n+\n"            # a quality line that is '+'
        b"@r4\nGG\n+\nII")               # no final line feed


def test_the_restatement_on_a_literal():
    assert extract_restated(FIVE, [3, 1, 1]) == b"@r1\nAC\n+r1\n@+\n@r3 x\nA\n+\n+\n"
    assert extract_restated(FIVE, [2]) == b"@\n\n+\n\n"
    assert extract_restated(FIVE, [4, 0]) == b"@r0\nACGT\n+\nIIII\n@r4\nGG\n+\nII"
    assert extract_restated(FIVE, []) == b""
    assert extract_restated(FIVE, range(5)) == FIVE
    crlf = FIVE.replace(b"\n", b"\r\n")
    assert extract_restated(crlf, [1, 4]) == b"@r1\r\nAC\r\n+r1\r\n@+\r\n@r4\r\nGG\r\n+\r\nII"
    assert extract_restated(crlf + b"\r\n", [4]) == b"@r4\r\nGG\r\n+\r\nII\r\n"


def test_host_loops_stand_alone(tmp_path):
    """msweep_amd/csrc/fastq_host.hpp -- index, validation, selection, gather, pieces -- against its own restatement in
    tests/cpp/fastq_host_test.cpp: no device, no library"""
    exe = str(tmp_path / "fastq_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fastq_host_test.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
