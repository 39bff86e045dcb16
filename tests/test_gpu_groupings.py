"""GPU: every column of the -i file is run from ONE resident alignment (the grouping loop of src/mSWEEP.cpp:282).

The oracle throughout is the project itself on a single column: a three-column indicator file against the three files
that each hold one of its columns.  Solves are bit-reproducible run to run, so every comparison is on bytes.

The toy of tests/test_gpu_cli_toy.py (39 sequences in four clusters, 1 500 paired reads) with a 40th sequence no read
hits, and three columns chosen so that consecutive builds differ in every way a build can:
  column 0  the four clusters (12 / 9 / 10 / 8) and the 40th sequence in a group of its own: --min-hits 1 masks it
  column 1  every sequence its own group (G = 40, all sizes 1)
  column 2  two groups of 20 sequences
"""
import os
import subprocess

import numpy as np
import pytest

from msweep_amd.__main__ import main
from msweep_amd.core import Core
from msweep_amd.reference import output_path, read_references
from test_gpu_cli_toy import _toy, mini_binary  # noqa: F401 (mini_binary: the fixture)

pytestmark = pytest.mark.gpu

K = 3
FLAGS = ["--write-probs", "--write-likelihood", "--iters", "3", "--seed", "11", "--bin-reads", "--min-abundance", "0.01"]
VARIANTS = {"plain": [], "min_hits": ["--min-hits", "1"], "gzip": ["--compress", "z"],
            "em_float": ["--algorithm", "emgpu", "--emprecision", "float"]}


def _columns(clusters):
    """the three columns over the toy's 39 sequences + one that no read hits"""
    n = len(clusters) + 1
    return [clusters + ["lonely"], [f"s{i}" for i in range(n)], ["half_a" if i < n // 2 else "half_b" for i in range(n)]]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The toy's files, `multi.tsv` (three columns) and `col<i>.tsv`; the runs of the Python driver, made on first use and
    shared: case.py_multi(variant) / case.py_single(variant, i) -> the directory the run wrote into (prefix P)."""
    root = tmp_path_factory.mktemp("groupings")
    _toy(root)
    cols = _columns((root / "clustering.txt").read_text().split("\n")[:-1])
    assert len(cols[0]) == 40
    (root / "multi.tsv").write_text("".join("\t".join(c[i] for c in cols) + "\n" for i in range(40)))
    for k, c in enumerate(cols):
        (root / f"col{k}.tsv").write_text("\n".join(c) + "\n")

    class Case:
        dir = root
        reads = ["--themisto-1", str(root / "toy_1.txt"), "--themisto-2", str(root / "toy_2.txt")]
        files = [str(root / "toy_1.txt"), str(root / "toy_2.txt")]
        _done = {}

        def run_py(self, name, indicators, extra):
            if name not in self._done:
                d = root / name
                d.mkdir()
                rc = main(self.reads + ["-i", str(root / indicators), "-o", str(d / "P")] + FLAGS + extra)
                assert rc == 0, name
                self._done[name] = d
            return self._done[name]

        def py_multi(self, variant):
            return self.run_py(f"py_multi_{variant}", "multi.tsv", VARIANTS[variant])

        def py_single(self, variant, i):
            return self.run_py(f"py_single{i}_{variant}", f"col{i}.tsv", VARIANTS[variant])
    return Case()


def _outputs(variant):
    gz = ".gz" if variant == "gzip" else ""
    return ["abundances.txt", "probs.tsv" + gz, "likelihoods.tsv" + gz]


def _bins(d):
    return sorted(f for f in os.listdir(d) if f.endswith((".bin", ".bin.gz")))


def _same_file(got, want):
    a, b = open(got, "rb").read(), open(want, "rb").read()
    assert len(b) > 0 or str(want).endswith((".bin", ".bin.gz")), want
    assert a == b, (str(got), str(want))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_python_cli_multi_column_against_single_column_runs(case, variant):
    """`P_<i>_...` of the three-column run are, byte for byte, the files of the run over column i alone -- under
    --min-hits 1 (another mask per column), --compress z (the gzip streams too) and the fp32 EM kernels as well.  The
    bins carry no index (src/OutfileDesignator.cpp:80-94); the three columns share no group name, so every bin of a
    single-column run has its counterpart in the one directory of the multi-column run."""
    multi = case.py_multi(variant)
    assert not (multi / "P_abundances.txt").exists()
    bins = []
    for i in range(K):
        single = case.py_single(variant, i)
        for name in _outputs(variant):
            assert len(open(single / ("P_" + name), "rb").read()) > 20
            _same_file(multi / f"P_{i}_{name}", single / ("P_" + name))
        assert _bins(single), i
        for b in _bins(single):
            _same_file(multi / b, single / b)
        bins += _bins(single)
    assert _bins(multi) == sorted(bins)
    assert sorted(f for f in os.listdir(multi) if f.startswith("P_")) == sorted(f"P_{i}_{n}" for i in range(K) for n in _outputs(variant))
    if variant == "min_hits":
        rows = [ln.split("\t") for ln in open(multi / "P_0_abundances.txt").read().splitlines() if not ln.startswith("#")]
        assert rows[-1] == ["lonely", "0", "0", "0", "0"]      # masked in column 0, written with the zeros behind the rest
        assert not os.path.exists(multi / "lonely.bin")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_native_driver_writes_the_same_files(case, mini_binary, variant):
    d = case.dir / f"cc_multi_{variant}"
    d.mkdir()
    p = subprocess.run([mini_binary] + case.reads + ["-i", str(case.dir / "multi.tsv"), "-o", str(d / "P")] + FLAGS + VARIANTS[variant],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    py = case.py_multi(variant)
    assert sorted(os.listdir(d)) == sorted(os.listdir(py))
    for f in os.listdir(py):
        _same_file(d / f, py / f)


def test_without_a_prefix_the_groupings_follow_each_other_on_stdout(case, mini_binary, capfd):
    """No -o: each grouping prints what a single-column run prints, in grouping order (the reference would write files
    named `_0_probs.tsv`: DESIGN.md)."""
    flags = ["--write-probs", "--iters", "3", "--seed", "11"]
    capfd.readouterr()
    want = ""
    for i in range(K):
        assert main(case.reads + ["-i", str(case.dir / f"col{i}.tsv")] + flags) == 0
        out = capfd.readouterr().out
        assert out.startswith("ec_id\t") and "#c_id\tmean_theta\tbootstrap_mean_thetas\n" in out
        want += out
    assert main(case.reads + ["-i", str(case.dir / "multi.tsv")] + flags) == 0
    assert capfd.readouterr().out == want
    p = subprocess.run([mini_binary] + case.reads + ["-i", str(case.dir / "multi.tsv")] + flags, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == want


def test_alphas_are_checked_when_a_grouping_is_reached(case, mini_binary, tmp_path, capfd):
    """--alphas of length 4 with --min-hits 1: grouping 0 keeps its four clusters and writes its files; grouping 1 (one
    group per sequence) ends the run with the message of today (src/mSWEEP.cpp:392-396)."""
    flags = ["-i", str(case.dir / "multi.tsv"), "--alphas", "1,1,1,1", "--min-hits", "1"]
    capfd.readouterr()
    assert main(case.reads + flags + ["-o", str(tmp_path / "py")]) == 1
    assert capfd.readouterr().err == "Error: --alphas must have the same number of values as there are groups."
    p = subprocess.run([mini_binary] + case.reads + flags + ["-o", str(tmp_path / "cc")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and p.stderr == "Error: --alphas must have the same number of values as there are groups."
    assert sorted(os.listdir(tmp_path)) == ["cc_0_abundances.txt", "py_0_abundances.txt"]
    _same_file(tmp_path / "cc_0_abundances.txt", tmp_path / "py_0_abundances.txt")
    assert len((tmp_path / "py_0_abundances.txt").read_text().splitlines()) == 4 + 5


def test_a_target_group_missing_from_a_grouping_fails_that_grouping(case, tmp_path, capfd):
    flags = ["-i", str(case.dir / "multi.tsv"), "--bin-reads", "--target-groups", "clust1", "-o", str(tmp_path / "P")]
    capfd.readouterr()
    assert main(case.reads + flags) == 1
    assert capfd.readouterr().err == "Binning the reads failed:\n  target group clust1 is not among the estimated groups\nexiting\n"
    assert sorted(os.listdir(tmp_path)) == ["P_0_abundances.txt", "clust1.bin"]


def test_verbose_counts_the_groupings_and_names_them_in_the_notes(case, mini_binary, tmp_path, capfd):
    """--verbose: `  read 3 groupings` (src/mSWEEP.cpp:265-267) and the grouping index in front of a grouping's notes;
    a single column keeps the lines of today.  Both drivers write the same lines."""
    capfd.readouterr()
    assert main(case.reads + ["-i", str(case.dir / "multi.tsv"), "-o", str(tmp_path / "py"), "--verbose"]) == 0
    err = capfd.readouterr().err
    assert "  read 3 groupings\n" in err
    for i in range(K):
        assert f"  grouping {i}: iter: 0, bound: " in err
    assert "\n  iter: " not in err
    p = subprocess.run([mini_binary] + case.reads + ["-i", str(case.dir / "multi.tsv"), "-o", str(tmp_path / "cc"), "--verbose"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == err
    assert main(case.reads + ["-i", str(case.dir / "col1.tsv"), "-o", str(tmp_path / "one"), "--verbose"]) == 0
    err = capfd.readouterr().err
    assert "groupings" not in err and "grouping " not in err and "  iter: 0, bound: " in err


def _export(core, aln):
    """the five arrays of an alignment, copied out now (msw_alignment_export)"""
    out = [np.empty(aln.n_ecs + 1, np.uint64), np.empty(aln.n_hits, np.uint32), np.empty(aln.n_ecs, np.uint64),
           np.empty(aln.n_ecs + 1, np.uint64), np.empty(aln.n_aligned, np.uint32)]
    assert core._L.msw_alignment_export(aln._h, *[a.ctypes.data for a in out]) == 0
    return out


def _build_and_use(core, aln, g, weights, min_hits):
    """one grouping on a handle: everything the drivers take from a build and its solve"""
    n_kept, mask, logc = core.build_likelihood_aln(aln, g.group_indicators, g.get_sizes(), min_hits=min_hits)
    prior = np.ones(n_kept)
    res = core.solve(None, prior)
    gamma = core.gamma()
    thetas, iters = core.bootstrap(weights, 11, int(weights.sum()), 0, 2, prior)
    rows = np.arange(n_kept, dtype=np.uint32)
    bin_ptr, reads, _ = core.bin_reads_aln(aln, rows, 1.0 - res["theta"])
    info = core.layout_info()
    return dict(n_kept=np.array(n_kept), mask=mask, logc=logc, theta=res["theta"], iters=np.array(res["iters"]),
                bound=np.array(res["bound"]), gamma=gamma, hash=np.array(core.layout_hash(), np.uint64), boot=thetas,
                boot_iters=iters, bin_ptr=bin_ptr, reads=reads, probs=np.frombuffer(core.text_block(0, 0, aln.n_ecs), np.uint8)), info


def _assert_same(got, want, what):
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert a.tobytes() == b.tobytes(), (what, k)


@pytest.mark.parametrize("min_hits", [0, 1])
def test_rebuild_on_one_handle(case, min_hits):
    """read_alignment once, build_likelihood_aln with column 0, 1, 0, 2, 0 on ONE handle: after every build the solve,
    gamma, the layout hash, two bootstrap replicates, the bins of every group and the text of the probabilities are,
    bit for bit, those of a fresh Core that read the files anew and built only that column -- so every result for
    column 0 is the first one -- and the alignment's arrays, copied out of device memory only after the last build, are
    those of a fresh read.

    Layouts seen on the MI355X (layout_info per grouping, printed below): all three columns get 4-byte narrow records
    with the group vectors and the whole slot table in LDS, pass B mode 2 -- 40 sequences cannot fill the LDS, so no
    choice of sizes on this toy reaches the wide or index encodings (the next test forces them).  What does change from
    build to build, columns 0 / 1 / 2: G 5 / 40 / 2 (--min-hits 1: 4 / 39 / 2), slot_entries 304 / 1 / 80, rows
    42 / 190 / 42, max_rows 4 / 16 / 2, pass B's register cells 8 / 16 / 8, 21 / 22 / 21 slices (column 1 has one
    slice of two lanes per class), and the --min-hits mask."""
    with open(case.dir / "multi.tsv") as f:
        groupings = read_references(f)
    fresh, weights, arrays0 = {}, None, None
    for i, g in enumerate(groupings):
        with Core(0) as core:
            aln = core.read_alignment(case.files, 40)
            if arrays0 is None:
                arrays0 = _export(core, aln)            # before any build
                weights = arrays0[2].astype(np.uint32)
            fresh[i], _ = _build_and_use(core, aln, g, weights, min_hits)
    with Core(0) as core:
        aln = core.read_alignment(case.files, 40)
        seen = []
        for step, i in enumerate([0, 1, 0, 2, 0]):
            got, info = _build_and_use(core, aln, groupings[i], weights, min_hits)
            print(f"min_hits {min_hits} build {step} column {i}: G {got['n_kept']} layout {info}")
            _assert_same(got, fresh[i], f"build {step}, column {i}")
            seen.append((int(got["n_kept"]), int(got["hash"]), info["slot_entries"]))
        for a, b in zip(seen, seen[1:]):
            assert a[0] != b[0] and a[1] != b[1], seen     # consecutive builds: another G, another layout
        assert seen[0] == seen[2] == seen[4]
        for a, b in zip(_export(core, aln), arrays0):      # (the first copy out of this alignment's device arrays)
            assert a.tobytes() == b.tobytes()
    assert fresh[0]["mask"].sum() == (4 if min_hits else 5) and fresh[2]["mask"].all()


def _layout(info):
    return tuple(info[k] for k in ("record_bytes", "index_records", "groups_in_lds", "table_in_lds", "passB_mode"))


def test_rebuild_across_record_encodings_and_lds_modes(case, monkeypatch):
    """The toy cannot leave the narrow records by itself (test_rebuild_on_one_handle), so the library's developer
    switches give every build of the sequence another record encoding and LDS mode, as tests/test_gpu_hybrid.py and
    tests/test_gpu_binning.py use them: column 0 as it comes (4-byte narrow records, groups and slot table in LDS),
    column 1 with MSWEEP_FORCE_LDS=10 (the slot table in memory: index records over the hybrid area), column 2 with
    MSWEEP_RECORD_BYTES=8 (wide records), column 1 with MSWEEP_FORCE_LDS=00 (group vectors in memory as well).  Every build
    on the used handle gives what a fresh handle gives under the same switch, bit for bit; no two consecutive builds
    share their layout."""
    with open(case.dir / "multi.tsv") as f:
        groupings = read_references(f)
    steps = [(0, {}), (1, {"MSWEEP_FORCE_LDS": "10"}), (0, {}), (2, {"MSWEEP_RECORD_BYTES": "8"}), (0, {}),
             (1, {"MSWEEP_FORCE_LDS": "00"}), (2, {"MSWEEP_RECORD_BYTES": "8"}), (0, {})]

    def build(core, aln, i, env, weights):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            return _build_and_use(core, aln, groupings[i], weights, 1)
    fresh, weights = {}, None
    for i, env in steps:
        key = (i, tuple(env.items()))
        if key in fresh:
            continue
        with Core(0) as core:
            aln = core.read_alignment(case.files, 40)
            if weights is None:
                weights = aln.ec_counts().astype(np.uint32)
            fresh[key] = build(core, aln, i, env, weights)
    with Core(0) as core:
        aln = core.read_alignment(case.files, 40)
        seen = []
        for step, (i, env) in enumerate(steps):
            got, info = build(core, aln, i, env, weights)
            want, want_info = fresh[(i, tuple(env.items()))]
            print(f"build {step} column {i} {env}: layout {_layout(info)} slot entries {info['slot_entries']} in LDS {info['slot_entries_in_lds']}")
            _assert_same(got, want, f"build {step}, column {i}, {env}")
            assert info == want_info, step
            seen.append(_layout(info))
        for a, b in zip(seen, seen[1:]):
            assert a != b, seen
        assert seen[0] == (4, 0, 1, 1, 2) and seen[1][1] == 1 and seen[3][0] == 8 and seen[5][2] == 0, seen


@pytest.fixture(scope="module")
def groupings_shim_binary(tmp_path_factory):
    from test_gpu_cpp_shim import _compile
    return _compile(tmp_path_factory, "groupings_shim_test")


def test_shim_reads_once_and_builds_per_column(case, groupings_shim_binary):
    """msw::DeviceLikelihood::read_files once + build_from_alignment per column (tests/cpp/groupings_shim_test.cpp): theta
    per column, as hex floats, equals the Python side's and what build_from_files gives on an object of its own; column 0
    built again after the others gives its first answer; after release_alignment() a build is refused."""
    with open(case.dir / "multi.tsv") as f:
        groupings = read_references(f)
    txt = f"40 {K}\n"
    for g in groupings:
        txt += f"{g.get_n_groups()}\n" + " ".join(map(str, g.group_indicators)) + "\n" + " ".join(map(str, g.get_sizes())) + "\n"
    r = subprocess.run([groupings_shim_binary, "1"] + case.files, input=txt, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split(" ") for ln in r.stdout.strip().splitlines()]
    out = {(ln[0], ln[1]): ln[2:] for ln in lines if ln[0] in ("loop", "files", "again")}
    with Core(0) as core:
        aln = core.read_alignment(case.files, 40)
        assert dict((ln[0], ln[1]) for ln in lines if len(ln) == 2) == {
            "n_ecs": str(aln.n_ecs), "n_reads": str(aln.n_reads), "n_aligned": str(aln.n_aligned), "released": "1"}
        for i, g in enumerate(groupings):
            n_kept, _, _ = core.build_likelihood_aln(aln, g.group_indicators, g.get_sizes(), min_hits=1)
            want = [float(x).hex() for x in core.solve(None, np.ones(n_kept))["theta"]]
            got = [float.fromhex(x).hex() for x in out[("loop", str(i))]]
            assert got == want, i
            assert out[("files", str(i))] == out[("loop", str(i))], i
    assert out[("again", "0")] == out[("loop", "0")]


def test_output_path_names_what_the_drivers_wrote(case):
    d = case.py_multi("plain")
    for i in range(K):
        assert os.path.exists(output_path(str(d / "P"), i, K, "abundances.txt"))
    assert os.path.exists(output_path(str(case.py_single("plain", 0) / "P"), 0, 1, "abundances.txt"))
