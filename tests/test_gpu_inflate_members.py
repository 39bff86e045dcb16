"""GPU: BGZF (bgzip) input inflated on the device per member (msw_core_inflate_gzip: inflate_member_kernels.hpp behind
host_inflate_members.inc) against zlib on the files of tests/test_inflate_members_cpu.py -- Themisto-shaped text in
members of 0xff00 bytes at levels 1, 6, 9, under Z_FIXED and stored, with and without htslib's end-of-file marker, in
members of 4 096 bytes, one byte, nothing, a member of exactly 64 KiB, runs and pairs across the ring's wrap, noise, a text
without a final line feed, two files concatenated: zlib's bytes, from the kernel, with the member count.  What does not
walk member by member to the end of the file, or fails a member's trailer, is the host path's, with the handle usable
afterwards."""
import struct
import zlib

import pytest

from msweep_amd.core import Core, MswError
from test_inflate_members_cpu import EOF_MARKER, files, split_members

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


def test_every_file_is_zlibs_bytes_from_the_kernel(core):
    for name, (f, data, n_members) in files().items():
        text, info = core.inflate_gzip(f)
        print(name, len(f), {k: info[k] for k in ("n_members", "on_device", "reason", "write_ms", "kernel_ms")})
        assert text == data, (name, info)
        assert info["on_device"] == 1 and info["fallback_reason"] == 0 and info["n_members"] == n_members, (name, info)
        assert info["n_chunks"] == n_members and info["n_starts"] == n_members and info["chunk_bytes"] == 0, (name, info)
        assert info["text_bytes"] == len(data) and info["payload_bytes"] == len(f) - 26 * n_members, (name, info)
        assert info["probe_ms"] == 0 and info["window_ms"] == 0 and info["chain_ms"] == 0 and info["crc_ms"] == 0, (name, info)
        assert info["kernel_ms"] == info["write_ms"], (name, info)


def test_single_member_path_reports_no_members(core):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    data = files()["themisto_l6"][1][:200000]
    text, info = core.inflate_gzip(c.compress(data) + c.flush())
    assert text == data and info["on_device"] == 1 and info["n_members"] == 0 and info["chunk_bytes"] == 65536, info


def test_what_does_not_walk_to_the_end_is_the_host_paths(core):
    f, data, n_members = files()["themisto_l6"]
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain = c.compress(b"0 1 2\n") + c.flush()
    text, info = core.inflate_gzip(f + plain)                          # a BGZF file followed by one plain member
    assert text == data + b"0 1 2\n" and info["on_device"] == 0 and info["reason"] == "header", info
    ms = split_members(f)
    bad = b"".join(ms[:3]) + ms[3][:16] + struct.pack("<H", len(ms[3])) + ms[3][18:] + b"".join(ms[4:])
    text, info = core.inflate_gzip(bad)                                # BSIZE damaged in member 3: zlib ignores the field
    assert text == data and info["on_device"] == 0 and info["reason"] == "header", info
    text, info = core.inflate_gzip(f)                                  # the handle is usable afterwards
    assert text == data and info["on_device"] == 1 and info["n_members"] == n_members


def test_damaged_member_trailer_is_the_host_paths_error(core):
    f, data, n_members = files()["themisto_l6"]
    ms = split_members(f)
    assert len(ms) == 23
    m = ms[11]                                                         # (the payload itself decodes: nothing is provoked)
    bad = b"".join(ms[:11]) + m[:-8] + bytes([m[-8] ^ 0x40]) + m[-7:] + b"".join(ms[12:])
    with pytest.raises(MswError, match="cannot read gzip-compressed bytes: incorrect data check"):
        core.inflate_gzip(bad)
    text, info = core.inflate_gzip(f)                                  # the handle is usable afterwards
    assert text == data and info["on_device"] == 1 and info["n_members"] == n_members


def test_host_inflate_switch(core, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_INFLATE", "1")
    for name in ("themisto_l6", "only_eof_marker", "two_files"):
        f, data, _ = files()[name]
        text, info = core.inflate_gzip(f)
        assert text == data and info["on_device"] == 0 and info["reason"] == "forced" and info["n_members"] == 0, (name, info)
    monkeypatch.delenv("MSWEEP_HOST_INFLATE")                          # read at the call
    text, info = core.inflate_gzip(EOF_MARKER)
    assert text == b"" and info["on_device"] == 1 and info["n_members"] == 1
