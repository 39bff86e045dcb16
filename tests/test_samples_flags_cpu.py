"""CPU: --samples / --devices of `python -m msweep_amd` are judged before a device is touched -- every refusal is the
three-line message of a parsing error with status 1 -- and the manifest's grammar (msweep_amd/samples.py): comments,
blank lines, two and three columns.  msweep_amd/cpp/samples_manifest.hpp, msweep_mini's parser, is held to the same
samples and the same messages through tests/cpp/samples_manifest_test.cpp, which also runs the workers' queue and the
library's table of dynamic-LDS limits (msweep_amd/csrc/lds_grants.hpp) on threads, under the sanitizers."""
import os
import subprocess

import pytest

from msweep_amd import __main__ as cli
from msweep_amd import samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


def _manifest(tmp_path, text, name="samples.tsv"):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


def _refused(capsys, argv, message):
    rc = cli.main(argv)
    err = capsys.readouterr().err
    assert rc == 1
    assert err == f"Parsing arguments failed:\n  {message}\nexiting\n"


GOOD = "a/p\tx_1.txt,x_2.txt\nb/p\ty.txt\n"


@pytest.mark.parametrize("flag, extra", [("--themisto", ["--themisto", "a,b"]), ("--themisto-1", ["--themisto-1", "a"]),
                                         ("--themisto-2", ["--themisto-2", "a"]), ("-o", ["-o", "out"]),
                                         ("--read-likelihood", ["--read-likelihood", "l.tsv"]), ("--print-probs", ["--print-probs"]),
                                         ("--extract-reads", ["--bin-reads", "--extract-reads", "r.fastq"])])
def test_samples_takes_the_place_of_the_single_run_flags(no_device, capsys, tmp_path, flag, extra):
    m = _manifest(tmp_path, GOOD)
    _refused(capsys, ["-i", "none.txt", "--samples", m] + extra, f"--samples can't be used with {flag}")


def test_the_first_colliding_flag_is_named(no_device, capsys, tmp_path):
    m = _manifest(tmp_path, GOOD)
    _refused(capsys, ["-i", "none.txt", "--print-probs", "-o", "x", "--samples", m], "--samples can't be used with -o")


def test_devices_needs_samples(no_device, capsys):
    _refused(capsys, ["-i", "none.txt", "--themisto-1", "a", "--devices", "0,0"], "--devices needs --samples")


@pytest.mark.parametrize("devices", ["0,", "a", "0,-1", "", "1 ", "0,,1"])
def test_devices_is_a_list_of_indices(no_device, capsys, tmp_path, devices):
    m = _manifest(tmp_path, GOOD)
    _refused(capsys, ["-i", "none.txt", "--samples", m, "--devices=" + devices], f"--devices: {devices} is not a list of device indices")


def test_a_manifest_that_cannot_be_opened(no_device, capsys, tmp_path):
    m = str(tmp_path / "missing.tsv")
    _refused(capsys, ["-i", "none.txt", "--samples", m], f"cannot open the sample manifest {m}")


@pytest.mark.parametrize("text", ["", "\n\n", "# only a comment\n\n#another\n"])
def test_a_manifest_without_a_sample(no_device, capsys, tmp_path, text):
    m = _manifest(tmp_path, text)
    _refused(capsys, ["-i", "none.txt", "--samples", m], f"the sample manifest {m} has no sample")


REFUSALS = [
    # (manifest, --bin-reads, the message after "<path>")
    ("a/p\tx.txt\n\nonly_a_prefix\n", False, ", line 3: 1 columns (a sample is <prefix> TAB <alignment files> [TAB <FASTQ files>])"),
    ("a/p\tx.txt\tr.fq\tmore\n", True, ", line 1: 4 columns (a sample is <prefix> TAB <alignment files> [TAB <FASTQ files>])"),
    ("# c\n\tx.txt\n", False, ", line 2: empty output prefix"),
    ("a/p\t\n", False, ", line 1: empty path in a list"),
    ("a/p\tx.txt,\n", False, ", line 1: empty path in a list"),
    ("a/p\tx.txt,,y.txt\n", False, ", line 1: empty path in a list"),
    ("a/p\tx.txt\t\n", True, ", line 1: empty path in a list"),
    ("a/p\tx.txt\tr.fq,\n", True, ", line 1: empty path in a list"),
    ("a/p\tx.txt\tr.fq\nb/p\ty.txt\n", True, ", line 2: FASTQ files on some lines and not on others"),
    ("a/p\tx.txt\n#\nb/p\ty.txt\tr.fq\n", True, ", line 3: FASTQ files on some lines and not on others"),
    ("a/p\tx.txt\tr.fq\nb/p\ty.txt\ts.fq\n", False, ": a FASTQ column needs --bin-reads"),
    ("a/p\tx.txt\nb/p\ty.txt\n\na/p\tz.txt\n", False, ", line 4: the output prefix a/p is that of line 1"),
    ("a/p\tx.txt\n./a//p\tz.txt\n", False, ", line 2: the output prefix ./a//p is that of line 1"),
    ("a/p\tx.txt\nb/p\ty.txt\na/q\tz.txt\n", True,
     ", line 3: with --bin-reads the prefix a/q lies in the directory of line 1: the bins would overwrite each other"),
    ("p\tx.txt\n./q\tz.txt\n", True,
     ", line 2: with --bin-reads the prefix ./q lies in the directory of line 1: the bins would overwrite each other"),
]


@pytest.mark.parametrize("text, bin_reads, message", REFUSALS)
def test_manifest_refusals(no_device, capsys, tmp_path, text, bin_reads, message):
    m = _manifest(tmp_path, text)
    _refused(capsys, ["-i", "none.txt", "--samples", m] + (["--bin-reads"] if bin_reads else []), m + message)


GRAMMAR = ("# a study\n"
           "\n"
           "out/s1/p\tin/s1_1.txt.gz,in/s1_2.txt.gz\tin/s1_1.fq,in/s1_2.fq.gz\n"
           "#out/skipped/p\tx\ty\n"
           "out/s2/p with blank\tin/s2.txt\tin/s2.fq\r\n"
           "\n"
           "/abs/s3/p\tin/s3_1.txt,in/s3_2.txt\tin/s3.fq")       # (no newline at the end)
GRAMMAR_SAMPLES = [("out/s1/p", ["in/s1_1.txt.gz", "in/s1_2.txt.gz"], ["in/s1_1.fq", "in/s1_2.fq.gz"], 3),
                   ("out/s2/p with blank", ["in/s2.txt"], ["in/s2.fq"], 5),
                   ("/abs/s3/p", ["in/s3_1.txt", "in/s3_2.txt"], ["in/s3.fq"], 7)]


def test_manifest_grammar(tmp_path):
    m = _manifest(tmp_path, GRAMMAR)
    got = samples.read_manifest(m)
    assert [tuple(s) for s in got] == GRAMMAR_SAMPLES
    samples.check_samples(m, got, True)
    two = samples.read_manifest(_manifest(tmp_path, GOOD, "two.tsv"))
    assert [tuple(s) for s in two] == [("a/p", ["x_1.txt", "x_2.txt"], None, 1), ("b/p", ["y.txt"], None, 2)]
    samples.check_samples(m, two, True)      # the same name below two parents: two directories
    samples.check_samples(m, samples.read_manifest(_manifest(tmp_path, "a/p\tx\na/q\ty\n", "same_dir.tsv")), False)


def test_valid_flags_reach_the_device(monkeypatch, tmp_path):
    """a good manifest passes every check: -i is read, then one handle per --devices entry is asked for"""
    made = []

    class Reached(Exception):
        pass

    def core(device):
        made.append(device)
        if len(made) == 3:
            raise Reached()
        return object()
    monkeypatch.setattr(cli, "Core", core)
    (tmp_path / "clustering.txt").write_text("a\nb\na\n")
    m = _manifest(tmp_path, GOOD)
    with pytest.raises(Reached):
        cli.main(["-i", str(tmp_path / "clustering.txt"), "--samples", m, "--devices", "1,0,1", "--bin-reads", "--compress", "z"])
    assert made == [1, 0, 1]


def test_without_devices_the_workers_run_on_device(monkeypatch, capsys, tmp_path):
    made = []

    def core(device):
        made.append(device)
        raise cli.MswError("no device here")
    monkeypatch.setattr(cli, "Core", core)
    (tmp_path / "clustering.txt").write_text("a\nb\na\n")
    rc = cli.main(["-i", str(tmp_path / "clustering.txt"), "--samples", _manifest(tmp_path, GOOD), "--device", "3"])
    assert rc == 1 and made == [3]       # (the first handle fails: no second one is asked for)
    assert capsys.readouterr().err == "Initialising the GPU failed:\n  no device here\nexiting\n"
    assert cli.DEFAULT_WORKERS in (1, 2)


# ---- msweep_mini's parser, the queue and the LDS table: a program of their own ---------------------------------------------
def _build(tmp_path, *flags):
    exe = str(tmp_path / ("samples_manifest_test" + ("_" + flags[-1].split("=")[-1].replace(",", "_") if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", *flags, "-I", os.path.join(ROOT, "msweep_amd", "cpp"),
                           "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "samples_manifest_test.cpp")])
    return exe


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("samples_cpp"), "-g", "-fno-sanitize-recover=all", "-fsanitize=address,undefined")


def _clean(out):
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "FAILED" not in out.stdout
    for word in ("runtime error", "AddressSanitizer", "ThreadSanitizer"):
        assert word not in out.stderr, out.stderr[-3000:]


def _cpp_parse(exe, path, bin_reads):
    out = subprocess.run([exe, "parse", path, "1" if bin_reads else "0"], capture_output=True, text=True, timeout=60)
    _clean(out)
    return out.stdout


def test_the_native_parser_reads_the_same_samples(asan_exe, tmp_path):
    m = _manifest(tmp_path, GRAMMAR)
    want = "".join(f"{n}\t{p}\t{','.join(f)}\t{','.join(q)}\n" for p, f, q, n in GRAMMAR_SAMPLES)
    assert _cpp_parse(asan_exe, m, True) == want
    assert _cpp_parse(asan_exe, _manifest(tmp_path, GOOD, "two.tsv"), True) == "1\ta/p\tx_1.txt,x_2.txt\n2\tb/p\ty.txt\n"


@pytest.mark.parametrize("text, bin_reads, message", REFUSALS + [("", False, None), ("#\n\n", True, None)])
def test_the_native_parser_gives_the_same_refusals(asan_exe, tmp_path, text, bin_reads, message):
    m = _manifest(tmp_path, text)
    with pytest.raises(samples.ManifestError) as ex:
        samples.check_samples(m, samples.read_manifest(m), bin_reads)
    if message is not None:
        assert str(ex.value) == m + message
    assert _cpp_parse(asan_exe, m, bin_reads) == f"refused: {ex.value}\n"


def test_the_native_parser_refuses_a_missing_manifest(asan_exe, tmp_path):
    m = str(tmp_path / "missing.tsv")
    assert _cpp_parse(asan_exe, m, False) == f"refused: cannot open the sample manifest {m}\n"


def test_queue_and_lds_table_under_asan_and_ubsan(asan_exe):
    out = subprocess.run([asan_exe], capture_output=True, text=True, timeout=300)
    _clean(out)
    assert "queue: ok" in out.stdout and "lds grants: ok" in out.stdout and "samples manifest: ok" in out.stdout


def test_queue_and_lds_table_under_tsan(tmp_path):
    out = subprocess.run([_build(tmp_path, "-g", "-fsanitize=thread")], capture_output=True, text=True, timeout=300)
    _clean(out)
    assert "queue: ok" in out.stdout and "lds grants: ok" in out.stdout


def test_path_spellings_compare_equal():
    assert samples.normal_path("./a//b/../c/") == "a/c" and samples.normal_path("/../x") == "/x"
    assert samples.normal_path("../x") == "../x"
    assert samples.bin_dir("p") == samples.bin_dir("./p") == "" and samples.bin_dir("a/p") == "a" and samples.bin_dir("/p") == "/"
