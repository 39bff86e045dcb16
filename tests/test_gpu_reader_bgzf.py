"""GPU: BGZF (bgzip) pseudoalignment files through the reader on the device (msw_alignment_read_device): the compressed
bytes are staged while the host walks headers and trailers, and the member kernel inflates them in front of the token
kernels (host_inflate_members.inc).  Two strands of 20 000 reads, as tests/test_gpu_reader_gzip.py draws them, written
plain, as BGZF and as single-member gzip: the BGZF pair gives the five arrays of the plain pair, element for element, in
both merge modes, with both files reported as served by the member kernel; a BGZF strand mixes with a single-member gzip
strand and with a plain one; text the token kernels do not judge still carries the host parser's message; both drivers
write the abundances.txt of the plain pair, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from msweep_amd.__main__ import main
from msweep_amd.core import Core, MswError
from test_gpu_reader_gzip import KEYS, N_GROUPS, N_TARGETS, _gzip, _strand_text
from test_inflate_members_cpu import bgzf

pytestmark = pytest.mark.gpu

N_READS = 20000


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_strands")
    paths = {"plain": [], "bgzf": [], "gzip": [], "members": []}
    for s in range(2):
        text = _strand_text(60 + s, N_READS + 13 * s)
        blocked = bgzf(text)
        paths["members"].append(-(-len(text) // 0xff00) + 1)
        for kind, name, data in (("plain", f"s{s}.txt", text), ("bgzf", f"s{s}.bgzf.txt.gz", blocked), ("gzip", f"s{s}.txt.gz", _gzip(text, 6))):
            (d / name).write_bytes(data)
            paths[kind].append(str(d / name))
    names = [f"g{i % N_GROUPS}" for i in range(N_TARGETS)]
    (d / "clustering.txt").write_text("\n".join(names) + "\n")
    paths["clustering"] = str(d / "clustering.txt")
    paths["dir"] = d
    return paths


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


@pytest.fixture(scope="module")
def plain_arrays(core, files):
    """the reference of this module, read once: the plain pair through the same entry, per merge mode"""
    out = {}
    for mode in ("intersection", "union"):
        aln = core.read_alignment(files["plain"], N_TARGETS, mode)
        assert aln.on_device
        out[mode] = (aln.n_reads, {k: np.array(v) for k, v in aln.arrays().items() if k in KEYS})
    return out


def _equal(aln, want):
    assert aln.n_reads == want[0]
    got = aln.arrays()
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[1][k], err_msg=k)


@pytest.mark.parametrize("mode", ["intersection", "union"])
def test_bgzf_pair_gives_the_plain_pairs_arrays(core, files, plain_arrays, mode):
    aln = core.read_alignment(files["bgzf"], N_TARGETS, mode)
    assert aln.on_device
    infos = core.last_inflate()
    print(infos)
    assert len(infos) == 2
    for path, plain, n_members, info in zip(files["bgzf"], files["plain"], files["members"], infos):
        assert info["on_device"] == 1 and info["fallback_reason"] == 0, info
        assert info["n_members"] == n_members > 1 and info["n_chunks"] == n_members and info["chunk_bytes"] == 0, info
        assert info["payload_bytes"] == os.path.getsize(path) - 26 * n_members and info["text_bytes"] == os.path.getsize(plain)
    _equal(aln, plain_arrays[mode])


@pytest.mark.parametrize("mode", ["intersection", "union"])
def test_a_bgzf_strand_beside_a_gzip_or_a_plain_strand(core, files, plain_arrays, mode):
    for pair, members in (([files["bgzf"][0], files["gzip"][1]], [True, False]), ([files["gzip"][0], files["bgzf"][1]], [False, True]),
                          ([files["bgzf"][0], files["plain"][1]], [True, False]), ([files["plain"][0], files["bgzf"][1]], [False, True])):
        aln = core.read_alignment(pair, N_TARGETS, mode)
        assert aln.on_device
        infos = core.last_inflate()
        assert [i["on_device"] for i in infos] == [int(p.endswith(".gz")) for p in pair], infos
        assert [i["n_members"] > 1 for i in infos] == members, infos
        _equal(aln, plain_arrays[mode])


def test_host_inflate_switch_serves_the_same_arrays(core, files, plain_arrays, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_INFLATE", "1")
    aln = core.read_alignment(files["bgzf"], N_TARGETS, "intersection")
    assert aln.on_device                                               # (the token kernels still parse the text)
    assert [i["reason"] for i in core.last_inflate()] == ["forced", "forced"]
    _equal(aln, plain_arrays["intersection"])


def test_malformed_line_inside_a_bgzf_file_carries_the_host_parsers_message(core, tmp_path):
    bad = tmp_path / "bad.bgzf.txt.gz"
    bad.write_bytes(bgzf(b"0 1 2\n1 x3\n2 4\n", piece=7))             # (the line lies across two members)
    with pytest.raises(MswError, match="File format not supported on line 2 with content: 1 x3"):
        core.read_alignment([str(bad)], 10)
    info = core.last_inflate()[0]
    assert info["on_device"] == 1 and info["n_members"] == 4           # inflated by the kernel, refused by the parser


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini_bgzf") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def test_both_drivers_write_the_plain_pairs_abundances(files, mini_binary, capfd):
    d = files["dir"]

    def args(pair, prefix):
        return ["--themisto-1", pair[0], "--themisto-2", pair[1], "-i", files["clustering"], "-o", str(d / prefix), "--verbose"]

    assert main(args(files["plain"], "py_plain")) == 0
    capfd.readouterr()
    assert main(args(files["bgzf"], "py_bgzf")) == 0
    err = capfd.readouterr().err
    assert err.count("gzip input inflated on the device") == 2 and err.count("BGZF members") == 2, err
    want = (d / "py_plain_abundances.txt").read_bytes()
    assert want.count(b"\n") > N_GROUPS and (d / "py_bgzf_abundances.txt").read_bytes() == want
    for pair, prefix in ((files["plain"], "cc_plain"), (files["bgzf"], "cc_bgzf")):
        p = subprocess.run([mini_binary] + args(pair, prefix), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stderr.count("gzip input inflated on the device") == (2 if prefix == "cc_bgzf" else 0), p.stderr
        assert (d / (prefix + "_abundances.txt")).read_bytes() == want, prefix
