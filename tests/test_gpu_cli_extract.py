"""GPU: --bin-reads --extract-reads through both drivers.  A toy of the shape tests/test_gpu_binning.py uses (4 clusters,
1 500 paired reads, plus a group no read aligns to, whose bin is empty) and two FASTQ files of 1 500 records, the second
gzip-compressed.  For every group `<g>_<k>.fastq` holds the records the restatement pinned in
tests/test_extract_flags_cpu.py picks with the ids read back from `<g>.bin`; the bins and the abundances are those of a
run without the flag; --compress z writes `<g>_<k>.fastq.gz` that inflate to the plain files, a valid empty gzip file for
the empty bin; msweep_mini writes the same bytes; a read file of another record count ends the run before any extraction
file is written; with two grouping columns a group name of both holds the second column's reads."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from msweep_amd.__main__ import main
from test_extract_flags_cpu import extract_restated

pytestmark = pytest.mark.gpu

N_READS = 1500
GROUPS = ["clust1", "clust2", "clust3", "clust4", "ghost"]


def _toy(d, n_reads=N_READS, seed=3):
    """4 clusters x ~10 reference sequences, paired-end reads drawn from theta = (.5,.3,.15,.05); five sequences of a
    fifth group, `ghost`, that no read aligns to"""
    rng = np.random.default_rng(seed)
    sizes = [12, 9, 10, 8]
    names = GROUPS[:4]
    indicators = [names[k] for k in range(4) for _ in range(sizes[k])]
    order = rng.permutation(len(indicators))
    indicators = [indicators[i] for i in order]
    members = {n: [i for i, x in enumerate(indicators) if x == n] for n in names}
    theta = [0.5, 0.3, 0.15, 0.05]
    l1, l2 = [], []
    for r in range(n_reads):
        g = rng.choice(4, p=theta)
        hit = set(rng.choice(members[names[g]], max(1, rng.binomial(sizes[g], 0.65)), replace=False).tolist())
        for o in range(4):
            if o != g and rng.random() < 0.3:
                hit |= set(rng.choice(members[names[o]], max(1, rng.binomial(sizes[o], 0.15)), replace=False).tolist())
        h1 = sorted(hit | ({int(rng.integers(0, len(indicators)))} if rng.random() < 0.1 else set()))
        h2 = sorted(hit) if rng.random() > 0.05 else []
        l1.append(" ".join(map(str, [r] + h1)))
        l2.append(" ".join(map(str, [r] + h2)))
    (d / "toy_1.txt").write_text("\n".join(l1) + "\n")
    (d / "toy_2.txt").write_text("\n".join(l2) + "\n")
    indicators += ["ghost"] * 5
    (d / "clustering.txt").write_text("\n".join(indicators) + "\n")
    # a second column: clust1 and clust2 together under the name clust1, the rest as `rest`
    second = ["clust1" if x in ("clust1", "clust2") else "rest" for x in indicators]
    (d / "two_columns.txt").write_text("\n".join(a + "\t" + b for a, b in zip(indicators, second)) + "\n")
    (d / "second_column.txt").write_text("\n".join(second) + "\n")


def _fastq(seed, n, mate):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        L = int(rng.integers(50, 251))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes()
        qual = rng.integers(33, 74, L, dtype=np.uint8).tobytes()        # '!' ... 'I': '@' and '+' among them
        out.append(b"@read%d/%d\n" % (r, mate) + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_toy")
    _toy(d)
    texts = [_fastq(21, N_READS, 1), _fastq(22, N_READS, 2)]
    (d / "r1.fq").write_bytes(texts[0])
    (d / "r2.fq.gz").write_bytes(gzip.compress(texts[1], 6))
    (d / "short.fq").write_bytes(_fastq(21, N_READS - 1, 1))
    return {"dir": d, "texts": texts, "reads": f"{d / 'r1.fq'},{d / 'r2.fq.gz'}"}


def _args(toy, clustering="clustering.txt"):
    d = toy["dir"]
    return ["--themisto-1", str(d / "toy_1.txt"), "--themisto-2", str(d / "toy_2.txt"), "-i", str(d / clustering)]


def _run_py(toy, name, extra, clustering="clustering.txt"):
    out = toy["dir"] / name
    os.makedirs(out)
    assert main(_args(toy, clustering) + ["--bin-reads", "-o", str(out / "p")] + extra) == 0
    return out


@pytest.fixture(scope="module")
def py_plain(toy):
    return _run_py(toy, "py_plain", ["--extract-reads", toy["reads"]])


@pytest.fixture(scope="module")
def py_z(toy):
    return _run_py(toy, "py_z", ["--extract-reads", toy["reads"], "--compress", "z"])


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    """msweep_amd/cpp/msweep_mini.cpp, built for this module"""
    out = str(tmp_path_factory.mktemp("extractmini") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


def _bin_ids(path):
    return [int(x) for x in open(path).read().split()]


def test_python_cli_extracts_the_bins_reads(toy, py_plain):
    names = sorted(os.listdir(py_plain))
    assert names == sorted([g + ".bin" for g in GROUPS] + [f"{g}_{k}.fastq" for g in GROUPS for k in (1, 2)] + ["p_abundances.txt"])
    sizes = []
    for g in GROUPS:
        ids = _bin_ids(py_plain / (g + ".bin"))
        sizes.append(len(ids))
        for k in (1, 2):
            assert (py_plain / f"{g}_{k}.fastq").read_bytes() == extract_restated(toy["texts"][k - 1], ids), (g, k)
    assert sum(n > 0 for n in sizes) >= 3 and sizes[-1] == 0        # ghost: an empty bin, two empty files
    # the bins and the abundances are those of a run without --extract-reads
    bare = _run_py(toy, "py_bare", [])
    for name in [g + ".bin" for g in GROUPS] + ["p_abundances.txt"]:
        assert (bare / name).read_bytes() == (py_plain / name).read_bytes(), name


def test_compress_z_writes_gzip_files(toy, py_plain, py_z):
    names = sorted(os.listdir(py_z))
    assert names == sorted([g + ".bin.gz" for g in GROUPS] + [f"{g}_{k}.fastq.gz" for g in GROUPS for k in (1, 2)] + ["p_abundances.txt"])
    for g in GROUPS:
        for k in (1, 2):
            assert gzip.decompress((py_z / f"{g}_{k}.fastq.gz").read_bytes()) == (py_plain / f"{g}_{k}.fastq").read_bytes(), (g, k)
    # the empty bin (checked on the restatement: no id, no byte): a valid empty gzip file
    assert _bin_ids(py_plain / "ghost.bin") == [] and extract_restated(toy["texts"][0], []) == b""
    z = (py_z / "ghost_1.fastq.gz").read_bytes()
    assert len(z) == 20 and gzip.decompress(z) == b""


@pytest.mark.parametrize("z", [False, True])
def test_native_driver_writes_the_same_bytes(toy, py_plain, py_z, mini_binary, z):
    want = py_z if z else py_plain
    out = toy["dir"] / ("cc_z" if z else "cc_plain")
    os.makedirs(out)
    p = subprocess.run([mini_binary] + _args(toy) + ["--bin-reads", "--extract-reads", toy["reads"], "-o", str(out / "p")] +
                       (["--compress", "z"] if z else []), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(out)) == sorted(os.listdir(want))
    for name in os.listdir(want):
        assert (out / name).read_bytes() == (want / name).read_bytes(), name


def test_a_read_file_of_another_record_count_is_refused(toy, mini_binary, capsys):
    d = toy["dir"]
    for driver in ("py", "cc"):
        out = d / ("short_" + driver)
        os.makedirs(out)
        extra = ["--bin-reads", "--extract-reads", f"{d / 'r1.fq'},{d / 'short.fq'}", "-o", str(out / "p")]
        if driver == "py":
            rc = main(_args(toy) + extra)
            err = capsys.readouterr().err
        else:
            p = subprocess.run([mini_binary] + _args(toy) + extra, capture_output=True, text=True, timeout=120)
            rc, err = p.returncode, p.stderr
        assert rc == 1
        assert err.startswith("Extracting the reads failed:\n  ") and err.endswith("\nexiting\n")
        assert "1499" in err and "1500" in err and "short.fq" in err
        left = sorted(os.listdir(out))
        assert left == sorted(g + ".bin" for g in GROUPS)          # the bins stay, no .fastq was written


def test_failures_of_the_extraction_carry_its_message(toy, capsys):
    d = toy["dir"]
    (d / "bad.fq").write_bytes(toy["texts"][0].replace(b"@read7/1\n", b"read7/1\n", 1))
    for k, (path, words) in enumerate(((d / "absent.fq", "cannot open read file"), (d / "bad.fq", "record 8"))):
        out = d / f"fail_{k}"
        os.makedirs(out)
        rc = main(_args(toy) + ["--bin-reads", "--extract-reads", str(path), "-o", str(out / "p")])
        err = capsys.readouterr().err
        assert rc == 1 and err.startswith("Extracting the reads failed:\n  ") and words in err
        assert sorted(os.listdir(out)) == sorted(g + ".bin" for g in GROUPS)


def test_verbose_notes_every_read_file(toy, capsys):
    out = toy["dir"] / "verbose"
    os.makedirs(out)
    assert main(_args(toy) + ["--bin-reads", "--extract-reads", toy["reads"], "-o", str(out / "p"), "--verbose"]) == 0
    err = capsys.readouterr().err
    assert f"note: {toy['dir'] / 'r1.fq'}: plain text; 1500 records\n" in err
    assert f"note: {toy['dir'] / 'r2.fq.gz'}: gzip input inflated on the " in err and "; 1500 records\n" in err


def test_two_grouping_columns_keep_the_second_columns_reads(toy, py_plain):
    """the files carry no grouping index, as the bins do not: a group name of both columns ends up with the reads of the
    column that ran last -- those of a run on that column alone"""
    both = _run_py(toy, "two_columns", ["--extract-reads", toy["reads"]], "two_columns.txt")
    second = _run_py(toy, "second_column", ["--extract-reads", toy["reads"]], "second_column.txt")
    for k in (1, 2):
        got = (both / f"clust1_{k}.fastq").read_bytes()
        assert got == (second / f"clust1_{k}.fastq").read_bytes()
        assert got == extract_restated(toy["texts"][k - 1], _bin_ids(both / "clust1.bin"))
        assert got != (py_plain / f"clust1_{k}.fastq").read_bytes()        # (the second column's clust1 holds clust2 as well)
        assert (both / f"rest_{k}.fastq").exists() and (both / f"clust3_{k}.fastq").exists()
