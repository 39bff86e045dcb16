"""GPU: gzip pseudoalignment files through the reader on the device (msw_alignment_read_device): the compressed bytes
are inflated by the kernels (host_inflate.inc) in front of the token kernels.  Two strands of 200 000 reads with targets
out of order and repeated, written plain and as gzip at levels 1 and 6: the gzip pair gives the five arrays of the plain
pair, element for element, in both merge modes, with both files reported as served by the kernels; a plain and a gzip
strand mix; text the token kernels do not judge still carries the host parser's message; both drivers write the
abundances.txt of the plain pair, byte for byte."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from msweep_amd.__main__ import main
from msweep_amd.core import Core, MswError

pytestmark = pytest.mark.gpu

KEYS = ("ec_tptr", "ec_targets", "ec_counts", "ec_rptr", "ec_reads")
N_READS, N_TARGETS, N_GROUPS = 200000, 3000, 25


def _strand_text(seed, n_reads):
    """lines as tests/test_gpu_reader.py builds them -- unaligned reads, targets in any order, repeated targets, repeated
    read ids, lines shuffled -- drawn in bulk"""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 7, n_reads)
    k[rng.random(n_reads) < 0.2] = 0
    ptr = np.concatenate([[0], np.cumsum(k)]).tolist()
    draws = (rng.integers(0, 40, ptr[-1]) + np.repeat(rng.integers(0, N_TARGETS - 40, n_reads), k)).tolist()
    dup = (rng.random(n_reads) < 0.2).tolist()
    lines = []
    for r in range(n_reads):
        t = draws[ptr[r]:ptr[r + 1]]
        if t and dup[r]:
            t = t + [t[0]] + t[-1:]
        lines.append(" ".join(map(str, [r] + t)))
    for r in rng.choice(n_reads, n_reads // 20, replace=False).tolist():
        lines.append(f"{r} {(r * 7) % N_TARGETS}")
    order = rng.permutation(len(lines)).tolist()
    return ("\n".join(lines[i] for i in order) + "\n").encode()


def _gzip(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gz_strands")
    paths = {"plain": [], 1: [], 6: []}
    for s in range(2):
        text = _strand_text(40 + s, N_READS + 13 * s)
        for kind in paths:
            p = d / (f"s{s}.txt" if kind == "plain" else f"s{s}_l{kind}.txt.gz")
            p.write_bytes(text if kind == "plain" else _gzip(text, kind))
            paths[kind].append(str(p))
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
        infos = core.last_inflate()
        assert len(infos) == 2 and all(i["on_device"] == 0 and i["fallback_reason"] == 0 and i["payload_bytes"] == 0 for i in infos)
        out[mode] = (aln.n_reads, {k: np.array(v) for k, v in aln.arrays().items() if k in KEYS})
    return out


def _equal(aln, want):
    assert aln.n_reads == want[0]
    got = aln.arrays()
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[1][k], err_msg=k)


@pytest.mark.parametrize("mode", ["intersection", "union"])
@pytest.mark.parametrize("level", [1, 6])
def test_gzip_pair_gives_the_plain_pairs_arrays(core, files, plain_arrays, mode, level):
    aln = core.read_alignment(files[level], N_TARGETS, mode)
    assert aln.on_device
    infos = core.last_inflate()
    print(infos)
    assert len(infos) == 2
    for path, info in zip(files[level], infos):
        assert info["on_device"] == 1 and info["fallback_reason"] == 0, info
        assert info["payload_bytes"] == os.path.getsize(path) - 18 and info["n_starts"] >= 1
    _equal(aln, plain_arrays[mode])


@pytest.mark.parametrize("mode", ["intersection", "union"])
def test_one_plain_and_one_gzip_strand(core, files, plain_arrays, mode):
    for pair in ([files["plain"][0], files[6][1]], [files[1][0], files["plain"][1]]):
        aln = core.read_alignment(pair, N_TARGETS, mode)
        assert aln.on_device
        infos = core.last_inflate()
        assert [i["on_device"] for i in infos] == [int(p.endswith(".gz")) for p in pair]
        _equal(aln, plain_arrays[mode])


def test_host_inflate_switch_serves_the_same_arrays(core, files, plain_arrays, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_INFLATE", "1")
    aln = core.read_alignment(files[6], N_TARGETS, "intersection")
    assert aln.on_device                                               # (the token kernels still parse the text)
    assert [i["reason"] for i in core.last_inflate()] == ["forced", "forced"]
    _equal(aln, plain_arrays["intersection"])


def test_text_the_token_kernels_do_not_judge_carries_the_host_parsers_message(core, tmp_path, monkeypatch):
    bad = tmp_path / "bad.txt.gz"
    bad.write_bytes(_gzip(b"0 1 2\n1 x3\n2 4\n", 6))
    with pytest.raises(MswError, match="File format not supported on line 2 with content: 1 x3"):
        core.read_alignment([str(bad)], 10)
    assert core.last_inflate()[0]["on_device"] == 1                    # inflated by the kernels, refused by the parser
    cut = tmp_path / "cut.txt.gz"
    cut.write_bytes(_gzip(b"0 1 2\n" * 5000, 6)[:-20])                 # a file zlib rejects: its message, as before
    monkeypatch.setenv("MSWEEP_HOST_INFLATE", "1")                     # (corrupt streams are the host tests' business)
    with pytest.raises(MswError, match="cannot read gzip-compressed pseudoalignment file .*cut.txt.gz"):
        core.read_alignment([str(cut)], 10)


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini_gzin") / "msweep_mini")
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
    assert main(args(files[6], "py_gz")) == 0
    err = capfd.readouterr().err
    assert err.count("gzip input inflated on the device") == 2, err
    want = (d / "py_plain_abundances.txt").read_bytes()
    assert want.count(b"\n") > N_GROUPS and (d / "py_gz_abundances.txt").read_bytes() == want
    for pair, prefix in ((files["plain"], "cc_plain"), (files[6], "cc_gz")):
        p = subprocess.run([mini_binary] + args(pair, prefix), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert p.stderr.count("gzip input inflated on the device") == (2 if prefix == "cc_gz" else 0), p.stderr
        assert (d / (prefix + "_abundances.txt")).read_bytes() == want, prefix
