"""GPU: gzip inflated on the device (msw_core_inflate_gzip: inflate_kernels.hpp behind host_inflate.inc) against zlib on the
inputs of tests/test_inflate_format_cpu.py -- Themisto-shaped text at levels 1, 6, 9, under Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE,
stored, with full flushes; long runs, marker chains, stored blocks between dynamic ones, the empty file, one byte, a
header with every optional field -- at chunk sizes of 1, 4, 16 KiB and the default; which path served (on_device, the
fallback reason), how many chunks begin an owner, the device compressor's own stream, two members, a damaged trailer and
the switch that forces the host path."""
import zlib

import pytest

from msweep_amd.core import Core, MswError
from test_inflate_format_cpu import STARTS_LINES, gz, streams, themisto_text

pytestmark = pytest.mark.gpu

CHUNKS = (1024, 4096, 16384, 0)     # 0: the default
# one owner would walk the whole payload (no dynamic block starts inside): beyond 256 KiB that goes to the host
LONG_SPAN = ("themisto_fixed", "themisto_stored")


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


def test_equals_zlib_on_the_device_at_every_chunk_size(core):
    """every input, the single-block ones (one byte, the run of 70 000) and those whose blocks span many chunks (30 KB
    blocks in 1 KiB chunks) and the one whose owners write less than a window (sync flushes every 4 KB) included: zlib's
    bytes, from the kernels -- but for the two streams without a block start inside (fixed-Huffman, stored; 0.76 and 1.4 MB in
    one stretch), which zlib serves with the reason "long span"""
    for name, (member, data) in streams().items():
        for chunk in CHUNKS:
            text, info = core.inflate_gzip(member, chunk)
            print(name, chunk, {k: info[k] for k in ("n_chunks", "n_starts", "on_device", "reason", "kernel_ms")})
            assert text == data, (name, chunk, info)
            if name in LONG_SPAN:
                assert info["on_device"] == 0 and info["reason"] == "long span" and info["n_starts"] == 1, (name, chunk, info)
                continue
            assert info["on_device"] == 1 and info["fallback_reason"] == 0, (name, chunk, info)
            head = 38 if name == "header_fields" else 10                 # 10 + FEXTRA 2 + 5, FNAME 9, FCOMMENT 10, FHCRC 2
            assert info["text_bytes"] == len(data) and info["payload_bytes"] == len(member) - 8 - head
            assert info["chunk_bytes"] == (chunk or 65536) and 1 <= info["n_starts"] <= info["n_chunks"]


def test_most_chunks_of_themisto_streams_begin_an_owner(core):
    """at 16 KiB chunks at least half of the chunks have a block start (zlib's own blocks allow it at this line count:
    tests/test_inflate_format_cpu.py::test_themisto_streams_have_a_start_in_most_chunks)"""
    data = themisto_text(STARTS_LINES)
    for level in (1, 6, 9):
        member = gz(data, level)
        text, info = core.inflate_gzip(member, 16384)
        print("level", level, info)
        assert text == data and info["on_device"] == 1 and info["fallback_reason"] == 0
        assert info["n_chunks"] == -(-(len(member) - 18) // 16384) and 2 * info["n_starts"] >= info["n_chunks"], info


def test_stream_of_the_device_compressor_comes_back(core):
    data = streams()["themisto_l6"][1][:300000]
    out = core.gzip_begin(6) + core.gzip_append(data[:100000]) + core.gzip_append(data[100000:]) + core.gzip_end()
    assert zlib.decompress(out, 31) == data
    for chunk in (4096, 0):
        text, info = core.inflate_gzip(out, chunk)
        assert text == data and info["on_device"] == 1 and info["fallback_reason"] == 0, info


def test_long_stretch_without_a_block_start_goes_to_the_host_path(core, monkeypatch):
    """a fixed-Huffman stream has no dynamic block start inside: one owner.  Below the bound on an owner's stretch (256 KiB
    of payload, or a 64th of the payload) the kernels serve it; with the bound lowered under its length, zlib does"""
    data = streams()["themisto_l6"][1][:100000]
    member = gz(data, 6, zlib.Z_FIXED)
    assert 40000 < len(member) < 200000
    text, info = core.inflate_gzip(member)
    assert text == data and info["on_device"] == 1 and info["n_starts"] == 1, info
    monkeypatch.setenv("MSWEEP_INFLATE_MAX_SPAN", "16384")
    text, info = core.inflate_gzip(member)
    assert text == data and info["on_device"] == 0 and info["reason"] == "long span" and info["n_starts"] == 1, info
    dyn, dyn_text = streams()["themisto_l6"]                           # blocks of ~30 KB: beyond the lowered bound too
    text, info = core.inflate_gzip(dyn, 4096)
    assert text == dyn_text and info["reason"] == "long span"
    monkeypatch.setenv("MSWEEP_INFLATE_MAX_SPAN", "65536")
    text, info = core.inflate_gzip(dyn, 4096)
    assert text == dyn_text and info["on_device"] == 1


def test_two_members_go_to_the_host_path(core):
    (a, ta), (b, tb) = streams()["themisto_l6"], streams()["run_70000"]
    text, info = core.inflate_gzip(a + b)
    assert text == ta + tb
    assert info["on_device"] == 0 and info["reason"] == "trailing bytes", info
    text, info = core.inflate_gzip(b + a + b)
    assert text == tb + ta + tb and info["on_device"] == 0 and info["reason"] == "trailing bytes"


def test_damaged_trailer_is_the_host_paths_error(core):
    member, data = streams()["themisto_l6"]
    bad = member[:-8] + bytes([member[-8] ^ 0x40]) + member[-7:]      # (the payload itself decodes: nothing is provoked)
    with pytest.raises(MswError, match="cannot read gzip-compressed bytes: incorrect data check"):
        core.inflate_gzip(bad)
    bad = member[:-4] + bytes([member[-4] ^ 1]) + member[-3:]
    with pytest.raises(MswError, match="cannot read gzip-compressed bytes: incorrect length check"):
        core.inflate_gzip(bad)
    text, info = core.inflate_gzip(member)                             # the handle is usable afterwards
    assert text == data and info["on_device"] == 1


def test_host_inflate_switch(core, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_INFLATE", "1")
    for name in ("themisto_l6", "empty", "noise_inside"):
        member, data = streams()[name]
        text, info = core.inflate_gzip(member)
        assert text == data and info["on_device"] == 0 and info["reason"] == "forced", (name, info)
    monkeypatch.delenv("MSWEEP_HOST_INFLATE")                          # read at the call
    text, info = core.inflate_gzip(streams()["themisto_l6"][0])
    assert info["on_device"] == 1


def test_chunk_size_from_the_environment(core, monkeypatch):
    member, data = streams()["themisto_l6"]
    monkeypatch.setenv("MSWEEP_INFLATE_CHUNK", "8192")
    text, info = core.inflate_gzip(member)
    assert text == data and info["chunk_bytes"] == 8192 and info["on_device"] == 1
    text, info = core.inflate_gzip(member, 32768)                      # the argument decides when given
    assert text == data and info["chunk_bytes"] == 32768
