"""CPU: --write-read-probs / --probs-threshold are judged before a device is touched, in both drivers and in the same words
(msweep_amd/read_probs.py; msweep_amd/cpp/msweep_mini.cpp check_read_probs_flags holds the same rules for msweep_mini, which
is run here as a whole program: every refusal ends it before it asks for a device); the header of the file; and a valid set
of flags reaches the device."""
import os
import subprocess

import pytest

from msweep_amd import __main__ as cli
from msweep_amd import read_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--themisto-1", "x.txt"]
TWO = "a\tx\na\ty\nb\tz\nb\tw\n"


def _both(capsys, mini, argv, message):
    """the Python driver and msweep_mini refuse `argv` with the same three lines and status 1"""
    want = f"Parsing arguments failed:\n  {message}\nexiting\n"
    rc = cli.main(argv)
    assert rc == 1 and capsys.readouterr().err == want
    p = subprocess.run([mini] + argv, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr == want and p.stdout == ""


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


@pytest.fixture(scope="module")
def mini_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mini") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


@pytest.fixture
def indicators(tmp_path):
    p = tmp_path / "groups.tsv"
    p.write_text("a\nb\na\n")
    return str(p)


@pytest.mark.parametrize("text", ["nan", "0", "0.0", "-0.5", "1.0000001", "2", "inf", "abc", "", "0x1p-3", "1_0", " 0.5", "0.5 "])
def test_threshold_outside_the_unit_interval(no_device, capsys, mini_binary, indicators, text):
    argv = ["-i", indicators] + BASE + ["-o", "out/p", "--write-read-probs", "--probs-threshold", text]
    want = f"Parsing arguments failed:\n  --probs-threshold must be a probability in (0, 1] (got {text})\nexiting\n"
    p = subprocess.run([mini_binary] + argv, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr == want and p.stdout == ""
    with pytest.raises(read_probs.ReadProbsError, match=r"\(0, 1\]"):
        read_probs.threshold_of(text)
    if not text.startswith("-"):      # (argparse takes a value that starts with '-' only in the --flag=value form)
        assert cli.main(argv) == 1 and capsys.readouterr().err == want
    assert cli.main(argv[:-2] + [f"--probs-threshold={text}"]) == 1 and capsys.readouterr().err == want


def test_threshold_without_the_flag(no_device, capsys, mini_binary, indicators):
    _both(capsys, mini_binary, ["-i", indicators] + BASE + ["-o", "out/p", "--probs-threshold", "0.5"],
          "--probs-threshold needs --write-read-probs")
    # the value is judged first
    _both(capsys, mini_binary, ["-i", indicators] + BASE + ["-o", "out/p", "--probs-threshold", "7"],
          "--probs-threshold must be a probability in (0, 1] (got 7)")


def test_needs_a_prefix(no_device, capsys, mini_binary, indicators):
    _both(capsys, mini_binary, ["-i", indicators] + BASE + ["--write-read-probs"], "--write-read-probs needs -o")


@pytest.mark.parametrize("flag, extra", [("--read-likelihood", ["--read-likelihood", "l.tsv"]), ("--no-fit-model", ["--no-fit-model"])])
def test_flags_it_refuses(no_device, capsys, mini_binary, indicators, flag, extra):
    _both(capsys, mini_binary, ["-i", indicators] + BASE + ["-o", "out/p", "--write-read-probs"] + extra,
          f"--write-read-probs can't be used with {flag}")


def test_nested_is_refused(no_device, capsys, mini_binary, tmp_path):
    i = tmp_path / "two.tsv"
    i.write_text(TWO)
    _both(capsys, mini_binary, ["-i", str(i)] + BASE + ["-o", "out/p", "--nested", "--write-read-probs", "--probs-threshold", "0.01"],
          "--write-read-probs can't be used with --nested")


def test_the_first_refusal_is_named(no_device, capsys, mini_binary, indicators):
    _both(capsys, mini_binary, ["-i", indicators] + BASE + ["-o", "out/p", "--no-fit-model", "--write-read-probs", "--read-likelihood", "l.tsv"],
          "--write-read-probs can't be used with --read-likelihood")


def test_with_samples_the_manifest_names_the_prefixes(monkeypatch, capsys, mini_binary, tmp_path, indicators):
    """--samples takes the place of -o: no refusal for the missing prefix; the run goes on to the device"""
    class Reached(Exception):
        pass

    def core(device):
        raise Reached()
    monkeypatch.setattr(cli, "Core", core)
    m = tmp_path / "samples.tsv"
    m.write_text("s1/p\tx.txt\ns2/p\ty.txt\n")
    with pytest.raises(Reached):
        cli.main(["-i", indicators, "--samples", str(m), "--write-read-probs"])
    assert read_probs.check_flags(True, None, False, True, False, False, False) == read_probs.DEFAULT_THRESHOLD == 0.001
    with pytest.raises(read_probs.ReadProbsError, match="needs -o"):
        read_probs.check_flags(True, None, False, False, False, False, False)


def test_a_valid_flag_set_reaches_the_device(monkeypatch, indicators):
    class Reached(Exception):
        pass

    seen = {}

    def core(device):
        raise Reached()
    monkeypatch.setattr(cli, "Core", core)
    real = read_probs.check_flags

    def spy(*a):
        seen["tau"] = real(*a)
        return seen["tau"]
    monkeypatch.setattr(read_probs, "check_flags", spy)
    for extra, tau in (([], 0.001), (["--probs-threshold", "1"], 1.0), (["--probs-threshold", "1e-300"], 1e-300),
                       (["--probs-threshold", "0.25", "--compress", "z", "--iters", "2", "--bin-reads"], 0.25)):
        with pytest.raises(Reached):
            cli.main(["-i", indicators] + BASE + ["-o", "out/p", "--write-read-probs"] + extra)
        assert seen["tau"] == tau
    # without the flags nothing is asked of the rules but the default
    with pytest.raises(Reached):
        cli.main(["-i", indicators] + BASE)
    assert seen["tau"] == 0.001


def test_header_bytes():
    assert read_probs.header(0.001, ["sp1", "b c", ""]) == (b"#threshold\t0.001\n#group\t0\tsp1\n#group\t1\tb c\n#group\t2\t\n"
                                                            b"#read_id\tgroup\tprob\n")
    assert read_probs.header(0.1, []) == b"#threshold\t0.10000000000000001\n#read_id\tgroup\tprob\n"
    assert read_probs.header(1.0, ["g"]).startswith(b"#threshold\t1\n")
    assert read_probs.header(1e-300, ["g"]).startswith(b"#threshold\t1e-300\n")      # (the double is 1.000000000000000025e-300)
    assert read_probs.header(0.3, []).startswith(b"#threshold\t0.29999999999999999\n")
    assert cli.output_path("out/P", 0, 1, "read_probs.tsv") == "out/P_read_probs.tsv"
    assert cli.output_path("out/P", 1, 2, "read_probs.tsv") == "out/P_1_read_probs.tsv"
