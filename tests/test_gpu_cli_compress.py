"""GPU: --compress z in both drivers -- on the toy of tests/test_gpu_cli_toy.py, in blocks of 37 classes
(MSWEEP_TEXT_BLOCK): every `.gz` decompresses to the bytes of the same run without --compress, the plain-named file is
not written, `_abundances.txt` stays plain ("Ignore request to compress", src/OutfileDesignator.cpp:107) and unchanged,
what goes to stdout stays plain, and `python -m msweep_amd` and msweep_mini -- which make the same calls on the gzip
stream -- write byte-identical files."""
import gzip
import os
import subprocess
import zlib

import pytest

from conftest import ROOT
from msweep_amd.__main__ import main
from test_gpu_cli_toy import _toy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini_gz") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _common(tmp_path):
    return ["--themisto-1", str(tmp_path / "toy_1.txt"), "--themisto-2", str(tmp_path / "toy_2.txt"),
            "-i", str(tmp_path / "clustering.txt")]


def _run_mini(mini_binary, args):
    p = subprocess.run([mini_binary] + args, capture_output=True, text=True, timeout=120, env={**os.environ, "MSWEEP_TEXT_BLOCK": "37"})
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def _inflate(path):
    raw = path.read_bytes()
    d = zlib.decompressobj(wbits=31)
    data = d.decompress(raw)
    assert d.eof and d.unused_data == b"" and gzip.decompress(raw) == data        # one member, nothing behind it
    return data


def _runs(tmp_path, mini_binary, monkeypatch, args):
    """plain and compressed runs of both drivers into tmp_path/<run>/o"""
    monkeypatch.setenv("MSWEEP_TEXT_BLOCK", "37")
    for run in ("py_plain", "cc_plain", "py_z", "cc_z"):
        os.mkdir(tmp_path / run)
        full = _common(tmp_path) + args + ["-o", str(tmp_path / run / "o")] + (["--compress", "z"] if run.endswith("_z") else [])
        if run.startswith("py"):
            assert main(full) == 0
        else:
            _run_mini(mini_binary, full)


def _check(tmp_path, names, plain_only=("o_abundances.txt",)):
    for name in names:
        want = (tmp_path / "py_plain" / name).read_bytes()
        assert (tmp_path / "cc_plain" / name).read_bytes() == want
        for run in ("py_z", "cc_z"):
            assert _inflate(tmp_path / run / (name + ".gz")) == want, (run, name)
            assert not (tmp_path / run / name).exists(), (run, name)
        assert (tmp_path / "py_z" / (name + ".gz")).read_bytes() == (tmp_path / "cc_z" / (name + ".gz")).read_bytes(), name
    for name in plain_only:
        want = (tmp_path / "py_plain" / name).read_bytes()
        for run in ("py_z", "cc_z"):
            assert (tmp_path / run / name).read_bytes() == want and not (tmp_path / run / (name + ".gz")).exists(), (run, name)
    for run in ("py_z", "cc_z"):        # nothing else was written
        assert sorted(os.listdir(tmp_path / run)) == sorted([n + ".gz" for n in names] + list(plain_only)), run


@pytest.mark.parametrize("extra", [[], ["--min-hits", "400"]])
def test_probs_and_likelihood(tmp_path, mini_binary, monkeypatch, extra):
    _toy(tmp_path)
    _runs(tmp_path, mini_binary, monkeypatch, ["--write-probs", "--write-likelihood"] + extra)
    _check(tmp_path, ["o_probs.tsv", "o_likelihoods.tsv"])
    assert (tmp_path / "py_plain" / "o_probs.tsv").read_bytes().count(b"\n") > 37


def test_bitseq_likelihood(tmp_path, mini_binary, monkeypatch):
    _toy(tmp_path)
    _runs(tmp_path, mini_binary, monkeypatch, ["--write-likelihood-bitseq", "--no-fit-model"])
    _check(tmp_path, ["o_bitseq_likelihoods.tsv"], plain_only=())


def test_bins_with_an_empty_one(tmp_path, mini_binary, monkeypatch):
    names = _toy(tmp_path)
    with open(tmp_path / "clustering.txt", "a") as f:      # a group no read aligns to: its bin is empty
        f.write("ghost\n" * 5)
    _runs(tmp_path, mini_binary, monkeypatch, ["--bin-reads"])
    _check(tmp_path, [n + ".bin" for n in names + ["ghost"]])
    assert (tmp_path / "py_plain" / "ghost.bin").read_bytes() == b""
    assert len((tmp_path / "py_z" / "ghost.bin.gz").read_bytes()) == 20           # header, final block, CRC and length
    assert any((tmp_path / "py_plain" / (n + ".bin")).stat().st_size > 0 for n in names)     # ... and not every bin


def test_level_0_and_the_host_switch_write_the_same_text(tmp_path, mini_binary, monkeypatch):
    _toy(tmp_path, n_reads=300)
    monkeypatch.setenv("MSWEEP_TEXT_BLOCK", "37")
    base = _common(tmp_path) + ["--write-probs", "--write-likelihood"]
    assert main(base + ["-o", str(tmp_path / "plain")]) == 0
    assert main(base + ["-o", str(tmp_path / "l0"), "--compress", "z", "--compression-level", "0"]) == 0
    monkeypatch.setenv("MSWEEP_HOST_TEXT", "1")            # the host-formatted text goes through gzip_append
    assert main(base + ["-o", str(tmp_path / "ht"), "--compress", "z"]) == 0
    _run_mini(mini_binary, base + ["-o", str(tmp_path / "htc"), "--compress", "z"] )
    monkeypatch.delenv("MSWEEP_HOST_TEXT")
    monkeypatch.setenv("MSWEEP_HOST_GZIP", "1")            # zlib on the host, the reference's method
    assert main(base + ["-o", str(tmp_path / "hz"), "--compress", "z", "--compression-level", "1"]) == 0
    for name in ("probs.tsv", "likelihoods.tsv"):
        want = (tmp_path / ("plain_" + name)).read_bytes()
        for run in ("l0", "ht", "hz"):
            assert _inflate(tmp_path / f"{run}_{name}.gz") == want, (run, name)
        assert (tmp_path / f"l0_{name}.gz").stat().st_size > len(want)


def test_stdout_stays_plain(tmp_path, mini_binary, monkeypatch, capfd):
    _toy(tmp_path, n_reads=300)
    monkeypatch.setenv("MSWEEP_TEXT_BLOCK", "37")
    args = _common(tmp_path) + ["--print-probs"]
    assert main(args + ["-o", str(tmp_path / "a")]) == 0
    want = capfd.readouterr().out
    assert main(args + ["-o", str(tmp_path / "b"), "--compress", "z"]) == 0
    assert capfd.readouterr().out == want and want.startswith("ec_id\t")
    p = _run_mini(mini_binary, args + ["-o", str(tmp_path / "c"), "--compress", "z"])
    assert p.stdout == want
    assert sorted(f for f in os.listdir(tmp_path) if f[:2] in ("a_", "b_", "c_")) == ["a_abundances.txt", "b_abundances.txt", "c_abundances.txt"]
    # no -o: the files go to stdout, plain, whatever --compress says
    assert main(_common(tmp_path) + ["--write-probs", "--compress", "z"]) == 0
    assert capfd.readouterr().out.startswith("ec_id\t")


def test_refusals_of_the_native_driver(mini_binary, tmp_path):
    for extra, words in ((["--compress", "bz2"], "unsupported compression type bz2"),
                         (["--compress", "z", "--compression-level", "10"], "unsupported compression level 10")):
        p = subprocess.run([mini_binary, "-i", str(tmp_path / "none.txt"), "-o", str(tmp_path / "o")] + extra,
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and words in p.stderr and "z only" in p.stderr, p.stderr
