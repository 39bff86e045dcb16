"""CPU (g++ only): msweep_amd/csrc/text_cells.hpp, host build (tests/cpp/text_cells_test.cpp) -- the undecided cells of a
text block printed with snprintf and placed for k_text_close: no cells, a cell at offset 0, a cell whose 13 blanks end the
block, cells back to back, printed values of 1 and of 13 bytes, and the refusals (a cell past the end, overlapping cells);
every result against a host gap-closer over a synthetic block.  A program of its own, once plain and once under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ("no cells:", "a cell at offset 0:", "a cell that ends at total:", "two cells back to back:", "a text of length 1:",
         "a text of length 13:", "a cell past the end: refused", "overlapping cells: refused")


def _run(tmp_path, *flags):
    exe = str(tmp_path / ("text_cells_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "text_cells_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "FAILED" not in out.stdout and "text cells: ok" in out.stdout, out.stdout
    for case in CASES:
        assert case in out.stdout, (case, out.stdout)
    return out


def test_cells_are_printed_and_placed(tmp_path):
    _run(tmp_path)


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path):
    out = _run(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
