"""CPU (g++ only): the decimal-to-double routine of msweep_amd/csrc/dec_parse.hpp, host build, against glibc's strtod
(tests/cpp/dec_parse_test.cpp) -- an adversarial list, malformed tokens, "%g" of 2 M random doubles from the four generators
of tests/cpp/g6_format_test.cpp and 1 M random tokens inside Clinger's exact case.  Every decided token has strtod's bits,
nothing outside the exact case is decided, everything inside it is (the rule is a theorem, not a measurement), and every
malformed token is bad."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, *flags):
    exe = str(tmp_path / ("dec_parse_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "dec_parse_test.cpp")])
    return exe


def _check_report(out):
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "MISMATCH" not in out.stdout and "FAILED" not in out.stdout
    rows = {m.group(1): tuple(int(x) for x in m.group(2, 3, 4, 5))
            for m in re.finditer(r"^(\S+): tokens=(\d+) wrong=(\d+) decided=(\d+) undecided=(\d+) ok$", out.stdout, re.M)}
    assert set(rows) == {"adversarial", "malformed", "random_bits", "uniform", "exp(-745U)", "-50U", "fast_domain"}, out.stdout
    assert all(r[1] == 0 for r in rows.values())
    for name in ("random_bits", "uniform", "exp(-745U)", "-50U"):
        assert rows[name][0] == 500000 and rows[name][2] + rows[name][3] == 500000, (name, rows[name])
    # "%g" of values a likelihood file holds (-50 < x < 0, nearly all with |x| >= 1e-4): six digits, |k| <= 9 -- decided
    assert rows["-50U"][3] * 1000 <= rows["-50U"][0], rows["-50U"]
    # random bit patterns are nearly all beyond 1e22 or below 1e-22: left to strtod, never decided wrongly
    assert rows["random_bits"][3] > rows["random_bits"][2]
    n, _, decided, undecided = rows["fast_domain"]
    assert n > 900000 and undecided == 0 and decided == n, rows["fast_domain"]
    return rows


def test_host_build_matches_strtod(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    _check_report(out)


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    _check_report(out)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
