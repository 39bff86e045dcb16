"""CPU (g++ only): msweep_amd/csrc/deflate_format.hpp, host build (tests/cpp/deflate_format_test.cpp) -- the length and
distance codes against RFC 1951 3.2.5 for every length and distance, the length-limited code-length builder on Fibonacci,
flat, single-symbol, two-symbol and random histograms (at most 15 bits, Kraft sum exactly 1 from two symbols on), the
CRC-32 pieces against zlib, and the reference encoder built from the same header -- the kernels' parse, codes, header and
framing written plainly -- whose streams zlib inflates to the input."""
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 32768


def _build(tmp_path, *flags):
    exe = str(tmp_path / ("deflate_format_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "deflate_format_test.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("deflate"))


def probs_text(n_bytes, seed=1):
    """probs-shaped text: "%g" of a row-normalised exp of normal draws, 30 % of the cells tiny"""
    rng = np.random.default_rng(seed)
    G = 40
    rows, size, j = [], 0, 0
    while size < n_bytes:
        x = np.exp(3.0 * rng.standard_normal(G))
        x[rng.random(G) < 0.3] *= 1e-30
        x /= x.sum()
        rows.append(str(j) + "\t" + "\t".join("%g" % v for v in x) + "\t0\t0\n")
        size += len(rows[-1])
        j += 1
    return "".join(rows).encode()[:n_bytes]


def inputs():
    rng = np.random.default_rng(7)
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    weighted = np.repeat(np.arange(22, dtype=np.uint8) + 65, fib)
    return {
        "empty": b"",
        "one_byte": b"x",
        "run_70000": b"a" * 70000,
        "random": rng.integers(0, 256, 3 * CHUNK + 7, dtype=np.uint8).tobytes(),
        "alternating": b"ab" * 20000,
        "fibonacci": rng.permutation(weighted)[:CHUNK].tobytes(),
        "probs": probs_text(200000),
    }


def _check_report(out):
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "FAILED" not in out.stdout
    for line in ("lengths: values=256 ok", "distances: values=32768 ok", "header: ok", "crc: ok"):
        assert line in out.stdout, out.stdout
    assert "builder: histograms=" in out.stdout and "limited=40 ok" in out.stdout, out.stdout


def _round_trips(exe, tmp_path):
    sizes = {}
    for name, data in inputs().items():
        src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
        src.write_bytes(data)
        for chunk, stored in ((CHUNK, 0), (CHUNK, 1), (70000, 0), (70000, 1)):
            r = subprocess.run([exe, "--encode", str(src), str(dst), str(chunk), str(stored)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-2000:]
            raw = dst.read_bytes()
            d = zlib.decompressobj(wbits=-15)
            assert d.decompress(raw) == data and d.eof and d.unused_data == b"", (name, chunk, stored)
            assert raw.endswith(b"\x00\x00\xff\xff\x03\x00") or data == b""
            sizes[name, chunk, stored] = len(raw)
        for piece in (1, 64, 4096, 1 << 20):
            r = subprocess.run([exe, "--crc", str(src), str(piece)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and int(r.stdout) == zlib.crc32(data), (name, piece)
    return sizes


def test_tables_builder_header_and_crc(exe):
    _check_report(subprocess.run([exe], capture_output=True, text=True, timeout=300))


def test_reference_encoder_round_trips_through_zlib(exe, tmp_path):
    sizes = _round_trips(exe, tmp_path)
    data = inputs()
    n = len(data["random"])
    # random bytes go stored: 10 bytes a chunk, 2 for the final block; 70 000 stored bytes take two stored blocks
    assert sizes["random", CHUNK, 0] == n + 10 * 4 + 2
    assert sizes["random", 70000, 0] == n + 15 + 10 + 2
    assert sizes["run_70000", CHUNK, 1] == 70000 + 10 * 3 + 2 and sizes["run_70000", 70000, 1] == 70000 + 15 + 2
    assert sizes["run_70000", CHUNK, 0] < 3 * 300
    # matches and dynamic codes both work: below the midpoint of zlib level 1 and zlib without matches
    text = data["probs"]
    huff = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    bound = (len(zlib.compress(text, 1)) + len(huff.compress(text) + huff.flush())) / 2
    print("probs-shaped text: ratio", sizes["probs", CHUNK, 0] / len(text), "bound", bound / len(text))
    assert sizes["probs", CHUNK, 0] < bound


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    _check_report(out)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    _round_trips(exe, tmp_path)
