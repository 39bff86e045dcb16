"""CPU (g++ only): msweep_amd/csrc/inflate_format.hpp, host build (tests/cpp/inflate_format_test.cpp) -- the member header,
the block headers, the block-start probe and the two symbol loops, put together as the plain reference the kernels follow
(probe per chunk, pass (a) against an unknown window, window chain, pass (b), trailer).  The reference inflates every
input below to zlib's bytes at every chunk size; the probe finds every non-final dynamic block start that lies first in
its chunk; mutated streams end in a fallback reason or in zlib's bytes, in a stand-alone build under ASan and UBSan."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1024, 4096, 16384, 65536, 0)      # 0: one chunk
STARTS_LINES = 58000                        # lines at which zlib's own blocks meet the bound on the starts (below)
WHY = {"none": 0, "forced": 1, "header": 2, "probe": 3, "status": 4, "crc": 5, "trailing": 6, "memory": 7, "long span": 8}


def themisto_text(n_lines=60000, seed=5, n_targets=2000):
    """Themisto-shaped text: the read id, then Poisson(4) ascending target ids below n_targets"""
    rng = np.random.default_rng(seed)
    k = rng.poisson(4.0, n_lines)
    ptr = np.concatenate([[0], np.cumsum(k)]).tolist()
    draws = rng.integers(0, n_targets, ptr[-1]).tolist()
    lines = []
    for i in range(n_lines):
        lines.append(" ".join([str(i)] + [str(v) for v in sorted(set(draws[ptr[i]:ptr[i + 1]]))]))
    return ("\n".join(lines) + "\n").encode()


def gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush=zlib.Z_FULL_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for o in range(0, len(data), flush_every):
        out += c.compress(data[o:o + flush_every]) + c.flush(flush)
    return out + c.flush()


def with_header_fields(member):
    """the same member behind a header with FEXTRA, FNAME, FCOMMENT and FHCRC"""
    assert member[3] == 0
    head = bytes([0x1f, 0x8b, 8, 4 | 8 | 16 | 2]) + member[4:10] + bytes([5, 0]) + b"extra" + b"name.aln\0" + b"a comment\0"
    return head + (zlib.crc32(head) & 0xffff).to_bytes(2, "little") + member[10:]


_cache = {}


def streams():
    """name -> (gzip member, its text): the inputs of the CPU tests and of tests/test_gpu_inflate.py"""
    if _cache:
        return _cache
    text = themisto_text()
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, 100000, dtype=np.uint8).tobytes()
    for level in (1, 6, 9):
        _cache[f"themisto_l{level}"] = (gz(text, level), text)
    _cache["themisto_fixed"] = (gz(text, 6, zlib.Z_FIXED), text)
    _cache["themisto_huffman_only"] = (gz(text, 6, zlib.Z_HUFFMAN_ONLY), text)
    _cache["themisto_rle"] = (gz(text, 6, zlib.Z_RLE), text)
    _cache["themisto_stored"] = (gz(text, 0), text)
    _cache["themisto_full_flush"] = (gz(text, 6, flush_every=100000), text)
    # a block start every 4 KB of text with the history kept: owners of 1 KiB chunks write far fewer than 32 768 bytes, so
    # a window is mostly its predecessors' and a marker passes through many windows before it meets its byte
    _cache["themisto_sync_flush"] = (gz(text[:400000], 6, flush_every=4096, flush=zlib.Z_SYNC_FLUSH), text[:400000])
    _cache["run_70000"] = (gz(b"a" * 70000), b"a" * 70000)
    _cache["ab_400000"] = (gz(b"ab" * 200000), b"ab" * 200000)
    mixed = text[:300000] + noise + text[300000:600000]
    _cache["noise_inside"] = (gz(mixed), mixed)
    _cache["empty"] = (gz(b""), b"")
    _cache["one_byte"] = (gz(b"x"), b"x")
    _cache["header_fields"] = (with_header_fields(gz(text[:200000])), text[:200000])
    for name, (member, data) in _cache.items():
        assert zlib.decompress(member, 31) == data, name
    return _cache


def _build(tmp_path, *flags):
    exe = str(tmp_path / ("inflate_format_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "inflate_format_test.cpp"), "-lz"])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("inflate"))


def _report(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def run_reference(exe, tmp_path, name, member, chunk):
    src, dst = tmp_path / (name + ".gz"), tmp_path / (name + ".out")
    src.write_bytes(member)
    r = subprocess.run([exe, "--inflate", str(src), str(dst), str(chunk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return _report(r.stdout), dst.read_bytes()


def test_tables_order_and_member_header(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    for line in ("tables: ok", "order: ok", "member: ok"):
        assert line in out.stdout


def test_reference_equals_zlib_at_every_chunk_size(exe, tmp_path):
    false_total = 0
    for name, (member, data) in streams().items():
        for chunk in CHUNKS:
            if name == "ab_400000" and chunk != 1024:
                continue
            rep, text = run_reference(exe, tmp_path, name, member, chunk)
            print(name, chunk, rep)
            false_total += rep["false"]
            # every non-final dynamic block start that lies first in its chunk is found
            assert rep["missed"] == 0, (name, chunk, rep)
            if rep["false"] == 0:
                assert rep["why"] == WHY["none"] and text == data, (name, chunk, rep)
            else:
                # a position the probe accepted where no block starts: the run says so and vouches for nothing
                assert (rep["why"] == WHY["none"] and text == data) or (rep["why"] == WHY["probe"] and text == b""), (name, chunk, rep)
    print("false starts accepted over all inputs and chunk sizes:", false_total)


def test_themisto_streams_have_a_start_in_most_chunks(exe, tmp_path):
    """zlib closes a dynamic block about every 30 KB of compressed Themisto text (33 KB at level 1: two chunks of 16 KiB
    and a little, so the line count decides on which side of one half that level falls -- 20 blocks in 41 chunks at
    60 000 lines, 20 in 39 at 58 000): at 16 KiB chunks at least half of the chunks begin an owner, which is what
    tests/test_gpu_inflate.py asks of the kernels on the same text"""
    text_in = themisto_text(STARTS_LINES)
    for level in (1, 6, 9):
        member, data = gz(text_in, level), text_in
        rep, text = run_reference(exe, tmp_path, f"l{level}", member, 16384)
        print("level", level, len(member), rep)
        assert text == data and 2 * rep["starts"] >= rep["chunks"], rep
        assert rep["chunks"] == -(-(len(member) - 18) // 16384)


def test_trailer_and_framing_decide(exe, tmp_path):
    member, data = streams()["themisto_l6"]
    bad_crc = member[:-8] + bytes([member[-8] ^ 1]) + member[-7:]
    rep, text = run_reference(exe, tmp_path, "bad_crc", bad_crc, 65536)
    assert rep["why"] == WHY["crc"] and text == b""
    bad_len = member[:-1] + bytes([member[-1] ^ 1])
    rep, text = run_reference(exe, tmp_path, "bad_len", bad_len, 65536)
    assert rep["why"] == WHY["crc"] and text == b""
    rep, text = run_reference(exe, tmp_path, "two_members", member + member, 65536)
    assert rep["why"] != WHY["none"] and text == b""
    rep, text = run_reference(exe, tmp_path, "garbage", member + b"\0" * 5, 65536)
    assert rep["why"] != WHY["none"] and text == b""
    rep, text = run_reference(exe, tmp_path, "not_gzip", b"BZh91AY&SY" + b"\0" * 30, 65536)
    assert rep["why"] == WHY["header"]


def test_mutated_streams_stand_alone_under_asan_and_ubsan(tmp_path):
    """2 000 mutated copies of the level-6 stream (byte flips, truncations, bit insertions) through the stand-alone
    program built with the sanitizers: every copy ends in a fallback reason or in zlib's bytes, and nothing is reported"""
    exe = _build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout + out.stderr
    member, data = streams()["themisto_l6"]
    src = tmp_path / "l6.gz"
    src.write_bytes(member)
    for chunk, copies, seed in ((65536, 1000, 1), (4096, 1000, 2)):
        r = subprocess.run([exe, "--fuzz", str(src), str(copies), str(seed), str(chunk)], capture_output=True, text=True, timeout=1200)
        print(r.stdout[-500:])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        rep = _report(r.stdout.splitlines()[-1])
        assert rep["copies"] == copies and rep["bad"] == 0 and rep["error"] + rep["same"] == copies
    rep, text = run_reference(exe, tmp_path, "l6_san", member, 16384)
    assert rep["why"] == 0 and text == data
