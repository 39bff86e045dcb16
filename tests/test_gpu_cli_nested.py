"""GPU: --nested -- the columns of -i as one hierarchy, every bin of a node estimated within its group from a
sub-alignment made on the device (msw_alignment_subset) -- against the manual pipeline made of this tree's own
single-column runs, byte for byte, and msweep_mini against the Python driver.

The fixture (written by the test): 8 reference sequences in three level-0 groups of 4 / 3 / 1 sequences, a second column
of lineages (spA: a1 a1 a2 a2, spB: b1 b2 b2, spC: c1) and a third one for the 3-level case; 300 reads on one strand,
most of them hitting sequences of ONE level-0 group (their gamma for it is 1: binned at any theta), twenty across groups.

The manual pipeline for a child: level 0 runs alone with --bin-reads; the test writes the restricted text from the `.bin`
-- one line per binned read, the READS RENUMBERED by rank among the ids of the bin (a text of n lines must number its reads
0 .. n - 1: the reader leaves other ids out), the targets those of the group, renumbered by rank -- and the sub `-i` file;
a single-column run follows.  Its abundances and probabilities are the child's, byte for byte, and its bins are the
child's through the parent's bin (rank -> original read id)."""
import contextlib
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

from msweep_amd.__main__ import main
from test_gpu_cli_toy import mini_binary  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

COL0 = ["spA"] * 4 + ["spB"] * 3 + ["spC"]
COL1 = ["a1", "a1", "a2", "a2", "b1", "b2", "b2", "c1"]
COL2 = ["s1", "s2", "s3", "s3", "t1", "t2", "t3", "u1"]
N_READS = 300


def _rows():
    """{read id: targets}: 150 reads within spA, 100 within spB, 30 on spC, 20 across groups -- among them {0,1,2,3,4}
    beside {0,1,2,3}: two classes that differ only in a sequence of another group"""
    rng = np.random.default_rng(5)
    in_a = [(0,), (1,), (0, 1), (2, 3), (0, 1, 2), (3,), (0, 1, 2, 3), (2,)]
    in_b = [(4,), (5, 6), (4, 5), (6,), (5,), (4, 5, 6)]
    across = [(0, 1, 2, 3, 4), (0, 1, 2, 3, 7), (4, 5, 6, 0), (3, 7), (2, 5, 7)]
    kinds = [in_a] * 150 + [in_b] * 100 + [[(7,)]] * 30 + [across] * 20
    order = rng.permutation(N_READS)
    return {int(order[i]): kinds[i][int(rng.integers(len(kinds[i])))] for i in range(N_READS)}


def _fastq(mate):
    rng = np.random.default_rng(100 + mate)
    out = []
    for r in range(N_READS):
        seq = bytes(rng.choice(list(b"ACGT"), size=20 + r % 7).tolist())
        out.append(b"@read%d/%d\n" % (r, mate) + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return out


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    root = tmp_path_factory.mktemp("nested")
    rows = _rows()
    (root / "toy.txt").write_text("".join(" ".join([str(i)] + [str(t) for t in rows[i]]) + "\n" for i in range(N_READS)))
    (root / "two.tsv").write_text("".join(f"{a}\t{b}\n" for a, b in zip(COL0, COL1)))
    (root / "three.tsv").write_text("".join(f"{a}\t{b}\t{c}\n" for a, b, c in zip(COL0, COL1, COL2)))
    (root / "col0.tsv").write_text("".join(a + "\n" for a in COL0))
    records = [_fastq(1), _fastq(2)]
    for k, rec in enumerate(records, 1):
        (root / f"reads_{k}.fastq").write_bytes(b"".join(rec))
    return dict(dir=root, rows=rows, records=records, reads=["--themisto-1", str(root / "toy.txt")])


def _run_py(toy, d, indicators, extra):
    """the Python driver, in this process; returns (directory, what it wrote to stderr)"""
    d.mkdir()
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        rc = main(toy["reads"] + ["-i", str(toy["dir"] / indicators), "-o", str(d / "P")] + extra)
    assert rc == 0, err.getvalue()
    return d, err.getvalue()


def _run_mini(toy, mini, d, indicators, extra):
    d.mkdir()
    p = subprocess.run([mini] + toy["reads"] + ["-i", str(toy["dir"] / indicators), "-o", str(d / "P")] + extra, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return d, p.stderr


def _same_dirs(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def _ids(path):
    data = gzip.decompress(path.read_bytes()) if str(path).endswith(".gz") else path.read_bytes()
    return [int(x) for x in data.split()]


FLAGS = ["--bin-reads", "--write-probs"]
VARIANTS = {"plain": ([], ""), "gzip": (["--compress", "z"], ".gz"), "bootstrap": (["--iters", "3", "--seed", "7"], "")}
CHILDREN = {"spA": ["a1", "a2"], "spB": ["b1", "b2"]}
_DONE = {}


def _once(key, make):
    """a run is made on first use and shared by the tests that need it (a run costs about two seconds)"""
    if key not in _DONE:
        _DONE[key] = make()
    return _DONE[key]


def _nested(toy, variant):
    return _once(("nested", variant), lambda: _run_py(toy, toy["dir"] / f"nested_{variant}", "two.tsv",
                                                       ["--nested", "--verbose"] + FLAGS + VARIANTS[variant][0]))


def _level0(toy, variant):
    return _once(("level0", variant), lambda: _run_py(toy, toy["dir"] / f"level0_{variant}", "col0.tsv", FLAGS + VARIANTS[variant][0]))[0]


def _manual_child(toy, variant, group):
    """The single-column run over the restricted text of `group`'s bin of the level-0 run: (its directory, the read ids
    behind the text's read numbers).  The reads are numbered by their rank among the bin's ids in ascending order."""
    def make():
        gz = VARIANTS[variant][1]
        ids = sorted(_ids(_level0(toy, variant) / f"{group}.bin{gz}"))
        seqs = [i for i, g in enumerate(COL0) if g == group]
        rank = {t: r for r, t in enumerate(seqs)}
        d = toy["dir"] / f"manual_{variant}_{group}"
        d.mkdir()
        (d / "restricted.txt").write_text("".join(
            " ".join([str(r)] + [str(rank[t]) for t in toy["rows"][i] if t in rank]) + "\n" for r, i in enumerate(ids)))
        (d / "sub.tsv").write_text("".join(COL1[i] + "\n" for i in seqs))
        assert main(["--themisto-1", str(d / "restricted.txt"), "-i", str(d / "sub.tsv"), "-o", str(d / "P")] + FLAGS + VARIANTS[variant][0]) == 0
        return d, ids
    return _once(("manual", variant, group), make)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_root_is_the_level_0_run(toy, variant):
    """the root's files carry the single-column names and bytes, and nothing is written for spC: one sequence, one lineage"""
    gz = VARIANTS[variant][1]
    nested_dir, err = _nested(toy, variant)
    level0 = _level0(toy, variant)
    names = ["P_abundances.txt", "P_probs.tsv" + gz] + [f"{g}.bin{gz}" for g in ("spA", "spB", "spC")]
    for f in names:
        assert (nested_dir / f).read_bytes() == (level0 / f).read_bytes(), f
    for g, lins in CHILDREN.items():
        names += [f"P_{g}_abundances.txt", f"P_{g}_probs.tsv{gz}"] + [f"{g}_{l}.bin{gz}" for l in lins]
    assert sorted(os.listdir(nested_dir)) == sorted(names)
    assert "note: node spC: skipped, its sequences carry fewer than two groups in column 1\n" in err
    assert "node spA:   iter: 0, bound: " in err and "node spB:   iter: 0, bound: " in err and "\n  iter: 0, bound: " in "\n" + err


@pytest.mark.parametrize("group", list(CHILDREN))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_child_is_the_single_run_over_its_bin(toy, variant, group):
    """abundances and probabilities byte for byte; the child's bins are the manual run's through the parent's bin"""
    gz = VARIANTS[variant][1]
    nested_dir, _ = _nested(toy, variant)
    child, ids = _manual_child(toy, variant, group)
    assert len(ids) > 50                                          # the bin the child is made from is not empty
    for f in ("abundances.txt", "probs.tsv" + gz):
        got, want = (nested_dir / f"P_{group}_{f}").read_bytes(), (child / f"P_{f}").read_bytes()
        assert len(want) > 40 and got == want, f
    for lin in CHILDREN[group]:
        assert _ids(nested_dir / f"{group}_{lin}.bin{gz}") == [ids[r] for r in _ids(child / f"{lin}.bin{gz}")], lin
    if variant == "bootstrap":
        assert all(ln.count("\t") == 4 for ln in (child / "P_abundances.txt").read_text().splitlines() if not ln.startswith("#"))


def test_at_least_one_child_merges_classes(toy):
    """classes of the parent that hold a binned read against the child's classes: fewer means some fell together"""
    level0 = _level0(toy, "plain")
    merged = 0
    for group in CHILDREN:
        seqs = {i for i, g in enumerate(COL0) if g == group}
        parent_classes = {toy["rows"][i] for i in _ids(level0 / f"{group}.bin")}
        merged += len({tuple(t for t in c if t in seqs) for c in parent_classes}) < len(parent_classes)
    assert merged >= 1


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_native_driver_writes_the_same_files_and_notes(toy, mini_binary, tmp_path, variant):
    py, err = _nested(toy, variant)
    cc, cc_err = _run_mini(toy, mini_binary, tmp_path / "cc", "two.tsv", ["--nested", "--verbose"] + FLAGS + VARIANTS[variant][0])
    _same_dirs(py, cc)
    assert cc_err == err


def test_without_bin_reads_the_bins_are_taken_but_not_written(toy, mini_binary, tmp_path):
    py, _ = _run_py(toy, tmp_path / "py", "two.tsv", ["--nested"])
    assert sorted(os.listdir(py)) == ["P_abundances.txt", "P_spA_abundances.txt", "P_spB_abundances.txt"]
    full, _ = _nested(toy, "plain")
    for f in os.listdir(py):
        assert (py / f).read_bytes() == (full / f).read_bytes(), f
    cc, _ = _run_mini(toy, mini_binary, tmp_path / "cc", "two.tsv", ["--nested"])
    _same_dirs(py, cc)


def test_nested_extracts_child_bins_from_the_samples_read_files(toy, mini_binary, tmp_path):
    """child bins hold original read ids: the FASTQ pair is opened once and serves every node"""
    fq = ",".join(str(toy["dir"] / f"reads_{k}.fastq") for k in (1, 2))
    py, _ = _run_py(toy, tmp_path / "py", "two.tsv", ["--nested", "--bin-reads", "--extract-reads", fq])
    for stem in ("spA", "spB", "spC", "spA_a1", "spA_a2", "spB_b1", "spB_b2"):
        ids = _ids(py / f"{stem}.bin")
        for k in (1, 2):
            assert (py / f"{stem}_{k}.fastq").read_bytes() == b"".join(toy["records"][k - 1][i] for i in sorted(ids)), (stem, k)
    assert len(_ids(py / "spA_a1.bin")) > 10 and max(_ids(py / "spB_b2.bin")) > len(_ids(py / "spB.bin"))
    cc, _ = _run_mini(toy, mini_binary, tmp_path / "cc", "two.tsv", ["--nested", "--bin-reads", "--extract-reads", fq])
    _same_dirs(py, cc)


def test_nested_per_sample_of_a_manifest(toy, mini_binary, tmp_path):
    single, _ = _run_py(toy, tmp_path / "single", "two.tsv", ["--nested"] + FLAGS)
    for who in ("py", "cc"):
        m = tmp_path / f"{who}.tsv"
        m.write_text(f"{tmp_path}/{who}_s1/P\t{toy['dir']}/toy.txt\n{tmp_path}/{who}_s2/P\t{toy['dir']}/toy.txt\n")
        (tmp_path / f"{who}_s1").mkdir(), (tmp_path / f"{who}_s2").mkdir()
        argv = ["-i", str(toy["dir"] / "two.tsv"), "--samples", str(m), "--nested"] + FLAGS
        if who == "py":
            assert main(argv) == 0
        else:
            p = subprocess.run([mini_binary] + argv, capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
        _same_dirs(tmp_path / f"{who}_s1", single)
        _same_dirs(tmp_path / f"{who}_s2", single)


def test_three_levels(toy, mini_binary, tmp_path):
    """column 2 below column 1: a1 -> s1 s2 and b2 -> t2 t3 are run, a2 (s3 s3) and b1 (one sequence) are skipped"""
    py, err = _run_py(toy, tmp_path / "py", "three.tsv", ["--nested", "--verbose"] + FLAGS)
    for stem in ("spA_a2", "spB_b1", "spC"):
        assert f"note: node {stem}: skipped, its sequences carry fewer than two groups in column" in err
    want = ["P_abundances.txt", "P_probs.tsv", "spA.bin", "spB.bin", "spC.bin"]
    for g, lins, deep, leaves in (("spA", ["a1", "a2"], "a1", ["s1", "s2"]), ("spB", ["b1", "b2"], "b2", ["t2", "t3"])):
        want += [f"P_{g}_abundances.txt", f"P_{g}_probs.tsv"] + [f"{g}_{l}.bin" for l in lins]
        want += [f"P_{g}_{deep}_abundances.txt", f"P_{g}_{deep}_probs.tsv"] + [f"{g}_{deep}_{s}.bin" for s in leaves]
    assert sorted(os.listdir(py)) == sorted(want)
    # a leaf bin lies inside its parent's bin, and the depth-1 files are those of the two-column run
    assert set(_ids(py / "spA_a1_s1.bin")) <= set(_ids(py / "spA_a1.bin")) <= set(_ids(py / "spA.bin"))
    assert len(_ids(py / "spA_a1_s1.bin")) > 5
    two, _ = _nested(toy, "plain")
    for f in os.listdir(two):
        assert (py / f).read_bytes() == (two / f).read_bytes(), f
    cc, cc_err = _run_mini(toy, mini_binary, tmp_path / "cc", "three.tsv", ["--nested", "--verbose"] + FLAGS)
    _same_dirs(py, cc)
    assert cc_err == err
