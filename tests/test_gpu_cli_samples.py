"""GPU: --samples runs a manifest of samples in one process on resident handles, and every file of every
sample is, byte for byte, the file of a single run with that sample's -o / --themisto / --extract-reads.

The oracle throughout is the project itself on single runs; solves are bit-reproducible, so every comparison is on bytes.
Three inputs over the same 39 reference sequences: the toy of tests/test_gpu_cli_toy.py (1 500 paired reads, plain), a
larger sample (3 000 reads, one strand, gzip) and a smaller one (300 paired reads, plain), both from msweep_amd.synth.
The manifest orders them large, toy, small, large again (under another prefix): a handle meets a smaller sample after a
larger one and then a larger one again -- the bug class is state the previous sample left on the handle."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from msweep_amd import synth
from msweep_amd.__main__ import main
from test_gpu_cli_toy import _toy, mini_binary  # noqa: F401 (mini_binary: the fixture)

pytestmark = pytest.mark.gpu

FLAGS = ["--write-probs", "--write-likelihood", "--iters", "3", "--seed", "11", "--bin-reads", "--min-abundance", "0.01"]
VARIANTS = {"plain": [], "gzip": ["--compress", "z"], "min_hits": ["--min-hits", "1"],
            "em_float": ["--algorithm", "emgpu", "--emprecision", "float"], "groupings": [],
            "assign": ["--write-unassigned", "--write-assignment-table"], "fastq": []}
ORDER = ["large", "toy", "small", "large"]      # the manifest; the fourth sample goes to the directory `again`
N_READS = {"large": 3000, "toy": 1500, "small": 300}


def _synthetic(root, name, n_reads, seed, paired):
    prob = synth.make_csr_problem(n_reads, 4, seed=seed, max_other=3, group_sizes=lambda rng, G: np.array([12, 9, 10, 8], np.uint64))
    aln = synth.csr_to_targets(prob)
    assert aln["n_targets"] == 39
    rng = np.random.default_rng(seed)
    ec_of = rng.permutation(np.repeat(np.arange(len(prob["ec_counts"]), dtype=np.int64), prob["ec_counts"].astype(np.int64)))
    paths = [str(root / f"{name}_{k + 1}.txt") for k in range(2 if paired else 1)]
    for k, path in enumerate(paths):
        synth.write_themisto(path, ec_of, aln["ec_tptr"], aln["ec_targets"], extra=(rng, 0.1, 39) if k else None)
    return paths


def _fastq(path, n, tag):
    text = "".join(f"@{tag}{i}\n{'ACGT'[i % 4] * (20 + i % 7)}\n+\n{'I' * (20 + i % 7)}\n" for i in range(n)).encode()
    with open(path, "wb") as f:
        f.write(gzip.compress(text) if str(path).endswith(".gz") else text)
    return str(path)


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    """The inputs, and the runs of the Python driver, made on first use and shared:
    study.single(variant, sample) / study.batch(variant, devices) -> the directory of a sample's files (prefix P)."""
    root = tmp_path_factory.mktemp("samples")
    _toy(root)
    clusters = (root / "clustering.txt").read_text().split("\n")[:-1]
    # the three columns of tests/test_gpu_groupings.py over the toy's 39 sequences and a 40th that no read hits
    cols = [clusters + ["lonely"], [f"s{i}" for i in range(40)], ["half_a" if i < 20 else "half_b" for i in range(40)]]
    (root / "multi.tsv").write_text("".join("\t".join(c[i] for c in cols) + "\n" for i in range(40)))
    large = _synthetic(root, "large", N_READS["large"], 5, False)
    with open(large[0], "rb") as f:
        data = f.read()
    with open(large[0] + ".gz", "wb") as f:
        f.write(gzip.compress(data))

    class Study:
        dir = root
        files = {"large": [large[0] + ".gz"], "toy": [str(root / "toy_1.txt"), str(root / "toy_2.txt")],
                 "small": _synthetic(root, "small", N_READS["small"], 6, True)}
        fastqs = {"large": [_fastq(root / "large.fq", N_READS["large"], "l")],
                  "toy": [_fastq(root / "toy_1.fq", N_READS["toy"], "a"), _fastq(root / "toy_2.fq.gz", N_READS["toy"], "b")],
                  "small": [_fastq(root / "small.fq", N_READS["small"], "s")]}
        _done = {}

        def flags(self, variant):
            return ["-i", str(root / ("multi.tsv" if variant == "groupings" else "clustering.txt"))] + FLAGS + VARIANTS[variant]

        def manifest(self, d, variant, order=ORDER):
            """<d>/manifest.tsv over `order`, every sample to a directory of its own; -> (path, the directories)"""
            dirs = []
            lines = ["# large, toy, small and large again", ""]
            for k, name in enumerate(order):
                dirs.append(d / (name if name not in order[:k] else f"{name}_again{k}"))
                dirs[-1].mkdir()
                cols = [str(dirs[-1] / "P"), ",".join(self.files[name])] + ([",".join(self.fastqs[name])] if variant == "fastq" else [])
                lines.append("\t".join(cols))
            (d / "manifest.tsv").write_text("\n".join(lines) + "\n")
            return str(d / "manifest.tsv"), dirs

        def single(self, variant, name):
            key = f"single_{variant}_{name}"
            if key not in self._done:
                d = root / key
                d.mkdir()
                extra = ["--extract-reads", ",".join(self.fastqs[name])] if variant == "fastq" else []
                assert main(self.flags(variant) + ["-o", str(d / "P"), "--themisto", ",".join(self.files[name])] + extra) == 0, key
                self._done[key] = d
            return self._done[key]

        def batch(self, variant, devices=None):
            key = f"batch_{variant}_{devices}"
            if key not in self._done:
                d = root / key
                d.mkdir()
                m, dirs = self.manifest(d, variant)
                assert main(self.flags(variant) + ["--samples", m] + (["--devices", devices] if devices else [])) == 0, key
                self._done[key] = dirs
            return self._done[key]
    return Study()


def _files(d):
    return sorted(os.listdir(d))


def _same_dirs(got, want):
    """the same files with the same bytes"""
    assert _files(got) == _files(want), (str(got), str(want))
    assert any(f.startswith("P_") and "abundances" in f for f in _files(got)), str(got)
    for f in _files(got):
        a, b = open(got / f, "rb").read(), open(want / f, "rb").read()
        assert a == b, (str(got / f), str(want / f))
        assert len(b) > 0 or ".bin" in f or ".fastq" in f, f


def _against_single_runs(study, variant, devices=None):
    dirs = study.batch(variant, devices)
    for name, d in zip(ORDER, dirs):
        _same_dirs(d, study.single(variant, name))
    _same_dirs(dirs[0], dirs[3])      # the large sample again, after the small one


def test_every_file_of_every_sample_is_the_single_runs_file(study):
    _against_single_runs(study, "plain")
    names = _files(study.batch("plain")[1])
    assert {"P_abundances.txt", "P_probs.tsv", "P_likelihoods.tsv", "clust1.bin"} <= set(names)


def test_two_workers_on_one_device_write_the_same_bytes(study):
    _against_single_runs(study, "plain", "0,0")
    for a, b in zip(study.batch("plain", "0,0"), study.batch("plain")):
        _same_dirs(a, b)


@pytest.mark.parametrize("variant", ["gzip", "min_hits", "em_float", "groupings", "assign", "fastq"])
def test_variants(study, variant):
    _against_single_runs(study, variant)
    names = set(_files(study.batch(variant)[1]))
    want = {"gzip": {"P_probs.tsv.gz", "clust1.bin.gz"}, "min_hits": {"P_abundances.txt"}, "em_float": {"P_abundances.txt"},
            "groupings": {"P_0_abundances.txt", "P_1_probs.tsv", "P_2_likelihoods.tsv", "half_a.bin", "s3.bin"},
            "assign": {"unassigned_reads.bin", "P_reads_to_groups.tsv"}, "fastq": {"clust1_1.fastq", "clust1_2.fastq"}}[variant]
    assert want <= names, names


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_native_driver_writes_the_same_files(study, mini_binary, devices):
    d = study.dir / f"cc_{devices}"
    d.mkdir()
    m, dirs = study.manifest(d, "plain")
    p = subprocess.run([mini_binary] + study.flags("plain") + ["--samples", m] + (["--devices", devices] if devices else []),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", p.stdout + p.stderr
    for got, want in zip(dirs, study.batch("plain")):
        _same_dirs(got, want)


def _failing(study, d, variant, bad_files=None, bad_fastqs=None):
    """toy, a sample that fails, toy again; -> (manifest, directories)"""
    d.mkdir()
    files, fastqs = dict(study.files), dict(study.fastqs)
    files["bad"], fastqs["bad"] = bad_files or study.files["toy"], bad_fastqs or study.fastqs["toy"]
    saved = study.files, study.fastqs
    study.files, study.fastqs = files, fastqs
    try:
        return study.manifest(d, variant, ["toy", "bad", "toy"])
    finally:
        study.files, study.fastqs = saved


@pytest.mark.parametrize("driver", ["python", "native"])
def test_the_first_failure_stops_the_queue(study, mini_binary, capsys, driver):
    bad = study.dir / "bad.txt"
    bad.write_text("0 1\n12 34 x\n2 3\n")
    assert main(study.flags("plain") + ["--themisto", str(bad), "-o", str(study.dir / "bad_single")]) == 1
    single = capsys.readouterr().err
    assert single.startswith("Reading the pseudoalignments failed:\n  ") and single.endswith("\nexiting\n")
    m, dirs = _failing(study, study.dir / f"fail_{driver}", "plain", bad_files=[str(bad)])
    argv = study.flags("plain") + ["--samples", m]
    if driver == "python":
        rc, err = main(argv), capsys.readouterr().err
    else:
        p = subprocess.run([mini_binary] + argv, capture_output=True, text=True, timeout=120)
        rc, err = p.returncode, p.stderr
    assert rc == 1
    assert err == f"sample {dirs[1] / 'P'}: " + single + "samples: 1 finished, 1 failed, 1 not started\n"
    _same_dirs(dirs[0], study.single("plain", "toy"))
    assert _files(dirs[1]) == [] and _files(dirs[2]) == []


def test_a_read_file_of_another_size_fails_the_same_way(study, capsys):
    wrong = _fastq(study.dir / "wrong.fq", N_READS["toy"] - 1, "w")
    m, dirs = _failing(study, study.dir / "fail_fastq", "fastq", bad_fastqs=[wrong])
    rc = main(study.flags("fastq") + ["--samples", m])
    err = capsys.readouterr().err
    assert rc == 1
    assert err == (f"sample {dirs[1] / 'P'}: Extracting the reads failed:\n  {wrong} holds {N_READS['toy'] - 1} records, the "
                   f"pseudoalignment {N_READS['toy']} reads\nexiting\nsamples: 1 finished, 1 failed, 1 not started\n")
    _same_dirs(dirs[0], study.single("fastq", "toy"))
    assert not any(f.endswith(".fastq") for f in _files(dirs[1])) and _files(dirs[2]) == []


def test_verbose_lines_carry_their_sample(study, capsys):
    """two workers: every line of a sample has `sample <prefix>: ` in front, and without it a sample's lines are those of
    its single run (the bound of every fifth iteration: the solves are the same to the last digit)"""
    flags = ["-i", str(study.dir / "multi.tsv"), "--verbose"]
    general = ["  read 3 groupings\n", "note: --algorithm rcgcpu is served by the GPU RCG kernels (same algorithm as rcggpu)\n"]
    single = {}
    for name in set(ORDER):
        d = study.dir / f"verbose_single_{name}"
        d.mkdir()
        assert main(flags + ["-o", str(d / "P"), "--themisto", ",".join(study.files[name])]) == 0
        single[name] = [ln for ln in capsys.readouterr().err.splitlines(True) if ln not in general]
        assert any("grouping 1: iter: 0, bound: " in ln for ln in single[name])
    assert any("gzip input inflated on" in ln for ln in single["large"])
    d = study.dir / "verbose_batch"
    d.mkdir()
    m, dirs = study.manifest(d, "plain")
    assert main(flags + ["--samples", m, "--devices", "0,0"]) == 0
    lines = capsys.readouterr().err.splitlines(True)
    assert lines[:2] == general and lines[-1] == "samples: 4 finished, 0 failed, 0 not started\n"
    for name, sd in zip(ORDER, dirs):
        tag = f"sample {sd / 'P'}: "
        assert [ln[len(tag):] for ln in lines[2:-1] if ln.startswith(tag)] == single[name], name
    assert all(any(ln.startswith(f"sample {sd / 'P'}: ") for sd in dirs) for ln in lines[2:-1])
