"""CPU (g++ only): the member layer of msweep_amd/csrc/inflate_format.hpp, host build (tests/cpp/inflate_members_test.cpp)
-- BGZF files (bgzip: gzip files of many small members that state their compressed length in the 'BC' subfield of their
header) walked into a member table and decoded one member at a time by the plain reference the member kernel follows
(members_reference: the walk, inflate_owner per member from an empty window, the per-member trailer check).  The inputs
are built here from raw deflate, as tests/test_gpu_inflate_members.py builds them; gzip.decompress of the whole file is
the expected text.  The walk takes headers with other subfields and optional fields and refuses, as "header", whatever
does not walk member by member to the end of the file; a damaged trailer is "crc"; mutated files end in a reason or in
zlib's bytes, in a stand-alone build under ASan and UBSan."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_inflate_format_cpu import WHY, themisto_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 0xff00                              # bgzip's block of text
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def raw_deflate(piece, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(piece) + c.flush()


def member(piece, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra_before=b"", fields_behind=False):
    """one BGZF member: the 18-byte header with the 'BC' subfield (other subfields in front of it, FNAME and FCOMMENT behind
    the extra field on request), the raw deflate stream, CRC-32 and length"""
    payload = raw_deflate(piece, level, strategy)
    names = b"name.aln\0a comment\0" if fields_behind else b""
    xlen = len(extra_before) + 6
    total = 12 + xlen + len(names) + len(payload) + 8
    assert total <= 65536, total
    head = bytes([0x1f, 0x8b, 8, 4 | (0x18 if fields_behind else 0), 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra_before
    head += b"BC" + struct.pack("<HH", 2, total - 1) + names
    return head + payload + struct.pack("<II", zlib.crc32(piece), len(piece))


def bgzf(data, piece=PIECE, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """data in members of `piece` bytes of text, htslib's end-of-file marker (the member of the empty piece) behind them"""
    out = [member(data[o:o + piece], level, strategy) for o in range(0, len(data), piece)]
    if eof:
        out.append(member(b""))
    return b"".join(out)


def members_of(data, piece=PIECE, eof=True):
    return -(-len(data) // piece) + int(eof)


_cache = {}


def files():
    """name -> (BGZF file, its text, its member count)"""
    if _cache:
        return _cache
    text = themisto_text()
    noise = np.random.default_rng(9).integers(0, 256, 100000, dtype=np.uint8).tobytes()
    for level in (1, 6, 9):
        _cache[f"themisto_l{level}"] = (bgzf(text, level=level), text, members_of(text))
    _cache["themisto_fixed"] = (bgzf(text, strategy=zlib.Z_FIXED), text, members_of(text))
    _cache["themisto_stored"] = (bgzf(text, PIECE - 64, level=0), text, members_of(text, PIECE - 64))
    _cache["no_eof_marker"] = (bgzf(text, eof=False), text, members_of(text, eof=False))
    _cache["pieces_4096"] = (bgzf(text, 4096), text, members_of(text, 4096))
    _cache["one_byte"] = (bgzf(b"x", eof=False), b"x", 1)
    _cache["only_eof_marker"] = (bgzf(b""), b"", 1)
    full = text[:65536]
    _cache["member_of_65536"] = (bgzf(full, 65536), full, 2)
    _cache["run_65536"] = (bgzf(b"a" * 65536, 65536), b"a" * 65536, 2)
    _cache["ab_60000"] = (bgzf(b"ab" * 30000, 60000), b"ab" * 30000, 2)
    _cache["noise"] = (bgzf(noise, 30000), noise, members_of(noise, 30000))
    _cache["no_final_line_feed"] = (bgzf(text[:200000 - 1] + b"7"), text[:200000 - 1] + b"7", members_of(text[:200000]))
    two = bgzf(text[:150000]) + bgzf(text[150000:400000])
    _cache["two_files"] = (two, text[:400000], members_of(text[:150000]) + members_of(text[150000:400000]))
    for name, (f, data, n) in _cache.items():
        assert gzip.decompress(f) == data, name
    assert member(b"") == EOF_MARKER and len(EOF_MARKER) == 28
    assert _cache["themisto_l6"][2] == 23 and len(text) == 1415197
    return _cache


def _build(tmp_path, *flags):
    exe = str(tmp_path / ("inflate_members_test" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", os.path.join(ROOT, "msweep_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "inflate_members_test.cpp"), "-lz"])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("inflate_members"))


def _report(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def run_reference(exe, tmp_path, name, data):
    src, dst = tmp_path / (name + ".gz"), tmp_path / (name + ".out")
    src.write_bytes(data)
    r = subprocess.run([exe, "--inflate", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return _report(r.stdout), dst.read_bytes()


def split_members(f):
    """the members of a BGZF file built here (18-byte headers)"""
    out, o = [], 0
    while o < len(f):
        size = struct.unpack_from("<H", f, o + 16)[0] + 1
        out.append(f[o:o + size])
        o += size
    assert o == len(f)
    return out


def test_members_reference_equals_zlib(exe, tmp_path):
    for name, (f, data, n_members) in files().items():
        rep, text = run_reference(exe, tmp_path, name, f)
        print(name, len(f), rep)
        assert rep["why"] == WHY["none"] and text == data and rep["members"] == n_members, (name, rep)
        assert rep["payload"] == len(f) - 26 * n_members, (name, rep)


def test_walk_takes_other_subfields_and_optional_fields(exe, tmp_path):
    text = themisto_text()[:150000]
    pieces = [text[o:o + PIECE] for o in range(0, len(text), PIECE)]
    other = b"XY" + struct.pack("<H", 5) + b"hello"                   # a subfield in front of 'BC': no fixed offset
    f = member(pieces[0], extra_before=other) + member(pieces[1], fields_behind=True) + \
        member(pieces[2], extra_before=other, fields_behind=True) + EOF_MARKER
    assert gzip.decompress(f) == text
    rep, got = run_reference(exe, tmp_path, "fields", f)
    assert rep["why"] == WHY["none"] and got == text and rep["members"] == 4, rep


def test_walk_refuses_what_does_not_walk_to_the_end(exe, tmp_path):
    f, data, _ = files()["themisto_l6"]
    ms = split_members(f)
    plain = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain = plain.compress(b"0 1 2\n") + plain.flush()
    isize_65537 = ms[3][:-4] + struct.pack("<I", 65537)
    cases = {
        "bsize_plus_one": b"".join(ms[:3]) + ms[3][:16] + struct.pack("<H", len(ms[3])) + ms[3][18:] + b"".join(ms[4:]),
        "bsize_minus_one": b"".join(ms[:3]) + ms[3][:16] + struct.pack("<H", len(ms[3]) - 2) + ms[3][18:] + b"".join(ms[4:]),
        "plain_member_in_the_middle": b"".join(ms[:5]) + plain + b"".join(ms[5:]),
        "plain_member_behind": f + plain,
        "five_trailing_bytes": f + b"\0" * 5,
        "cut_last_member": f[:-3],
        "cut_inside_a_member": b"".join(ms[:7]) + ms[7][:1000],
        "isize_65537": b"".join(ms[:3]) + isize_65537 + b"".join(ms[4:]),
        "plain_gzip": plain,
        "empty_file": b"",
    }
    for name, bad in cases.items():
        rep, text = run_reference(exe, tmp_path, name, bad)
        assert rep["why"] == WHY["header"] and text == b"", (name, rep)


def test_a_members_trailer_decides(exe, tmp_path):
    f, data, _ = files()["themisto_l6"]
    ms = split_members(f)
    assert len(ms) == 23
    m = ms[11]
    for name, bad in (("crc", m[:-8] + bytes([m[-8] ^ 0x40]) + m[-7:]), ("isize", m[:-4] + bytes([m[-4] ^ 1]) + m[-3:])):
        rep, text = run_reference(exe, tmp_path, "bad_" + name, b"".join(ms[:11]) + bad + b"".join(ms[12:]))
        assert rep["why"] == WHY["crc"] and rep["bad_member"] == 11 and text == b"", (name, rep)
    # a final block that ends in front of the member's last payload byte: two bytes of padding inside the member
    padded = m[:16] + struct.pack("<H", len(m) + 1) + m[18:-8] + b"\0\0" + m[-8:]
    rep, text = run_reference(exe, tmp_path, "padded", b"".join(ms[:11]) + padded + b"".join(ms[12:]))
    assert rep["why"] == WHY["trailing"] and rep["bad_member"] == 11 and text == b"", rep
    # a payload cut short inside the member (BSIZE says so): the decode's status
    short = m[:16] + struct.pack("<H", len(m) - 101) + m[18:-108] + m[-8:]
    rep, text = run_reference(exe, tmp_path, "short", b"".join(ms[:11]) + short + b"".join(ms[12:]))
    assert rep["why"] == WHY["status"] and rep["bad_member"] == 11 and rep["status"] != 0 and text == b"", rep


def test_mutated_files_stand_alone_under_asan_and_ubsan(tmp_path):
    """2 000 mutated copies of the level-6 file (byte flips, truncations, insertions, half of them in headers and
    trailers) through the stand-alone program built with the sanitizers: every copy ends in a reason or in zlib's bytes,
    and nothing is reported"""
    exe = _build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    f, data, _ = files()["themisto_l6"]
    src = tmp_path / "l6.bgzf.gz"
    src.write_bytes(f)
    for copies, seed in ((1000, 1), (1000, 2)):
        r = subprocess.run([exe, "--fuzz", str(src), str(copies), str(seed)], capture_output=True, text=True, timeout=1200)
        print(r.stdout[-500:])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        rep = _report(r.stdout.splitlines()[-1])
        assert rep["copies"] == copies and rep["bad"] == 0 and rep["error"] + rep["same"] == copies
    for name in ("themisto_l6", "themisto_fixed", "themisto_stored", "only_eof_marker"):
        f, data, _ = files()[name]
        rep, text = run_reference(exe, tmp_path, name + "_san", f)
        assert rep["why"] == 0 and text == data, name
