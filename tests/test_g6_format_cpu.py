"""CPU (g++ only): the "%g" digit generator of msweep_amd/csrc/g6_format.hpp, host build, against glibc's
snprintf("%g") -- the adversarial list, 18 000 constructed ties, ties above 1e6 (left to snprintf) and 2 M random
values of four generators (tests/cpp/g6_format_test.cpp) -- and its power-of-ten table against fractions.Fraction."""
import os
import re
import subprocess
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, *flags):
    exe = str(tmp_path / ("g6_format_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "g6_format_test.cpp")])
    return exe


def _check_report(out):
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "MISMATCH" not in out.stdout and "FAILED" not in out.stdout
    rows = {m.group(1): tuple(int(x) for x in m.group(2, 3, 4))
            for m in re.finditer(r"^(\S+): values=(\d+) wrong=(\d+) undecided=(\d+) ok$", out.stdout, re.M)}
    assert set(rows) == {"adversarial", "ties", "ties_above_1e6", "random_bits", "uniform", "exp(-745U)", "-50U"}, out.stdout
    assert all(w == 0 for _, w, _ in rows.values())
    assert rows["ties"] == (18000, 0, 0)
    for name in ("random_bits", "uniform", "exp(-745U)", "-50U"):
        n, _, und = rows[name]
        assert n == 500000 and und * 10000 <= n, (name, rows[name])
    return rows


def test_host_build_matches_snprintf(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    rows = _check_report(out)
    # the ties the routine cannot resolve itself are all left to snprintf, none decided wrongly
    assert rows["ties_above_1e6"][2] == rows["ties_above_1e6"][0]


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    _check_report(out)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]


def test_power_table_is_exact(tmp_path):
    out = subprocess.run([_build(tmp_path), "--table"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(-310, 346))
    for k, p, q in rows:
        assert 1 << 63 <= p < 1 << 64, k
        exact = Fraction(10) ** k / Fraction(2) ** q
        assert p <= exact < p + 1, k                      # P = floor(10^k / 2^q)
        assert (exact == p) == (0 <= k <= 27), k          # ... exact where the header resolves ties itself


def test_exponent_estimate_is_never_above_the_true_exponent():
    """X0 = (t * 78913) >> 18 is floor(log10 2^t) for every binary exponent of a double: the true decimal exponent is X0
    or X0 + 1, so the routine corrects upward only."""
    for t in range(-1074, 1024):
        x0 = (t * 78913) >> 18
        v = Fraction(2) ** t
        assert Fraction(10) ** x0 <= v < Fraction(10) ** (x0 + 1), t
