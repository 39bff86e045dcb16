"""GPU: the records of a FASTQ file by read id on the device (msw_fastq_* through Core.fastq_open: fastq_kernels.hpp behind
host_fastq.inc).  The expected bytes come from the restatement pinned in tests/test_extract_flags_cpu.py -- the lines in
fours, the records of sorted(set(ids)) joined.  A synthetic file of about 600 records whose lines straddle tile edges and
span up to three tiles, with quality lines that begin with '@' or '+': index and gather against the restatement for
several selections, with and without a final line feed and with CRLF, the same under MSWEEP_HOST_EXTRACT=1, as gzip and as
BGZF, in pieces, inside a gzip stream; files outside the grammar and ids out of range are refused by name and leave the
handle usable."""
import bz2
import gzip
import struct
import zlib

import numpy as np
import pytest

from msweep_amd import synth
from msweep_amd.core import Core, MswError
from msweep_amd.likelihood import from_grouped_counts
from test_extract_flags_cpu import extract_restated, fastq_records

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 35, 151, 4095, 4096, 4097, 10000)
N_RECORDS = 600
SIX = b"@\n\n+\n\n"
MIB = 1 << 20


def _record(rng, r, L, eol):
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes()
    qual = bytearray(rng.integers(35, 74, L, dtype=np.uint8).tobytes())     # '#' ... 'I': no '@', no '+'
    kind = rng.integers(0, 10)
    if L and kind == 0:
        qual[0] = ord("@")
    elif L and kind == 1:
        qual[0] = ord("+")
    name = b"read%d/1" % r
    plus = b"+" + (name if rng.integers(0, 10) == 0 else b"")
    return b"@" + name + eol + seq + eol + plus + eol + bytes(qual) + eol


def _fastq(seed, eol=b"\n"):
    """N_RECORDS records; 300 and 301 are the six-byte record, placed at an odd offset"""
    rng = np.random.default_rng(seed)
    recs = [_record(rng, r, int(rng.choice(LENGTHS)), eol) for r in range(N_RECORDS)]
    if eol == b"\n":
        if sum(map(len, recs[:300])) % 2 == 0:
            recs[299] = b"@x" + recs[299][1:]
        recs[300] = recs[301] = SIX
        assert sum(map(len, recs[:300])) % 2 == 1
    return b"".join(recs)


def _bgzf(data, block=0xff00):
    """BGZF: gzip members of at most `block` bytes of text, each stating its own length in the 'BC' subfield; the empty
    member at the end"""
    out = []
    for o in list(range(0, len(data), block)) + [len(data)]:
        piece = data[o:o + block] if o < len(data) else b""
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out)


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


@pytest.fixture(scope="module")
def texts():
    """the module's files, drawn once: with a final line feed, without, CRLF"""
    t = _fastq(11)
    return {"nl": t, "no_nl": t[:-1], "crlf": _fastq(12, b"\r\n")}


@pytest.fixture(scope="module")
def selections():
    rng = np.random.default_rng(5)
    return {"all": np.arange(N_RECORDS), "none": np.zeros(0, np.int64), "first": [0], "last": [N_RECORDS - 1],
            "odd": np.arange(1, N_RECORDS, 2), "random": rng.integers(0, N_RECORDS, 200), "six": [301, 300]}


def _gather(fq, ids, max_bytes=256 * MIB):
    n, nbytes = fq.select(np.asarray(ids, np.uint32))
    got = b"".join(fq.pieces(max_bytes))
    return n, nbytes, got


def _toy_solves(core):
    """the handle still works: a small solve ends normalised"""
    p = synth.make_csr_problem(2000, 8, seed=3, max_other=3)
    lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    res = core.solve(lik.log_counts(), np.ones(8), tol=1e-6, max_iters=500)
    assert abs(res["theta"].sum() - 1.0) < 1e-9


# ---- 1. index and gather against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("variant", ["nl", "no_nl", "crlf"])
def test_index_and_gather(core, texts, selections, tmp_path, monkeypatch, variant, host):
    if host:
        monkeypatch.setenv("MSWEEP_HOST_EXTRACT", "1")
    text = texts[variant]
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    with core.fastq_open(path) as fq:
        assert fq.info["n_records"] == N_RECORDS and fq.info["text_bytes"] == len(text) and fq.info["reason"] == 0
        for name, ids in selections.items():
            want = extract_restated(text, ids)
            n, nbytes, got = _gather(fq, ids)
            assert (n, nbytes) == (len(set(int(x) for x in ids)), len(want)), name
            assert got == want, name
        if variant == "nl":
            assert extract_restated(text, [300, 301]) == SIX + SIX
        ms, nb = core.last_fastq_timing()
        assert nb == len(extract_restated(text, selections["six"])) and ms >= 0.0        # (of the last selection)


# ---- 2. input forms ------------------------------------------------------------------------------------------------------
def test_gzip_and_bgzf_give_the_plain_files_bytes(core, texts, selections, tmp_path):
    text = texts["no_nl"]
    want = extract_restated(text, selections["random"])
    (tmp_path / "r.fq.gz").write_bytes(gzip.compress(text, 6))
    (tmp_path / "r.bgzf.fq.gz").write_bytes(_bgzf(text))
    with core.fastq_open(tmp_path / "r.fq.gz") as fq:
        info = fq.info["inflate"]
        print("gzip:", info)
        assert info["on_device"] in (0, 1)              # reported; a file this small may go to zlib
        assert fq.info["n_records"] == N_RECORDS and fq.info["text_bytes"] == len(text)
        assert _gather(fq, selections["random"])[2] == want
    with core.fastq_open(tmp_path / "r.bgzf.fq.gz") as fq:
        info = fq.info["inflate"]
        print("bgzf:", info)
        assert info["on_device"] == 1 and info["n_members"] == -(-len(text) // 0xff00) + 1
        assert fq.info["n_records"] == N_RECORDS
        assert _gather(fq, selections["random"])[2] == want
        assert _gather(fq, selections["all"])[2] == text


# ---- 3. pieces -------------------------------------------------------------------------------------------------------------
def test_pieces_end_at_record_ends(core, texts, tmp_path):
    text = texts["nl"]
    assert len(text) > 5 * MIB // 2
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    ends = set(np.cumsum([len(r) for r in fastq_records(text)]).tolist())
    with core.fastq_open(path) as fq:
        fq.select(np.arange(N_RECORDS, dtype=np.uint32))
        pieces = list(fq.pieces(MIB))
    assert len(pieces) >= 3 and b"".join(pieces) == text
    at = 0
    for p in pieces:
        at += len(p)
        assert 0 < len(p) <= MIB and at in ends


def test_a_record_longer_than_a_piece_is_refused(core, tmp_path):
    L = (MIB + 1 - 7) // 2
    giant = b"@g\n" + b"A" * L + b"\n+\n" + b"I" * L + b"\n"
    assert len(giant) == MIB + 1
    small = b"@s\nAC\n+\nII\n"
    text = small + giant + small
    (tmp_path / "g.fq").write_bytes(text)
    with core.fastq_open(tmp_path / "g.fq") as fq:
        fq.select([0, 1, 2])
        it = fq.pieces(MIB)
        assert next(it) == small                       # the piece ends in front of the record that does not fit
        with pytest.raises(MswError, match=r"record 2 .*1048577 bytes"):
            next(it)
        assert _gather(fq, [2, 0])[2] == small + small       # the handle and the file stay usable
        assert _gather(fq, [1], 2 * MIB)[2] == giant
    _toy_solves(core)


# ---- 4. gzip out ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("which", ["none", "all"])
def test_pieces_inside_a_gzip_stream(core, texts, selections, tmp_path, monkeypatch, which, host):
    if host:
        monkeypatch.setenv("MSWEEP_HOST_EXTRACT", "1")
    text = texts["nl"]
    path = tmp_path / "reads.fq"
    path.write_bytes(text)
    with core.fastq_open(path) as fq:
        fq.select(np.asarray(selections[which], np.uint32))
        z = core.gzip_begin(6) + b"".join(fq.pieces_gzip(MIB)) + core.gzip_end()
    want = extract_restated(text, selections[which])
    assert gzip.decompress(z) == want
    if which == "all":
        assert len(want) > 5 * MIB // 2 and len(z) < len(want)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
GOOD = b"@a\nACGT\n+\nIIII\n"
MANY = b"".join(b"@r%d\n" % i + b"A" * 151 + b"\n+\n" + b"I" * 151 + b"\n" for i in range(40))


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("text,record,words", [
    (GOOD + GOOD + b"@c\nAC\n", 3, "10 lines"),                       # a line count of 4 k + 2
    (GOOD + b"a\nACGT\n+\nIIII\n" + GOOD, 2, "'@'"),
    (GOOD + GOOD + b"@a\nACGT\n\nIIII\n", 3, "'+'"),
    (b"@a\nACGTA\n+\nIIII\n" + GOOD, 1, "differ in length"),         # a sequence one byte longer than its quality
    (MANY + b"@z\nACGT\n+\nIII\n", 41, "differ in length"),           # the bad record last, beyond the first tile
    (MANY + b"x\nACGT\n+\nIIII", 41, "'@'"),
])
def test_files_outside_the_grammar_are_refused(core, tmp_path, monkeypatch, text, record, words, host):
    if host:
        monkeypatch.setenv("MSWEEP_HOST_EXTRACT", "1")
    (tmp_path / "bad.fq").write_bytes(text)
    with pytest.raises(MswError) as ex:
        core.fastq_open(tmp_path / "bad.fq")
    msg = str(ex.value)
    assert f"record {record}" in msg and words in msg and "bad.fq" in msg
    assert len(MANY) > 2 * 4096
    _toy_solves(core)


def test_ids_out_of_range_and_other_compressions_are_refused(core, tmp_path):
    (tmp_path / "two.fq").write_bytes(GOOD + GOOD)
    with core.fastq_open(tmp_path / "two.fq") as fq:
        assert _gather(fq, [1])[2] == GOOD
        with pytest.raises(MswError, match=r"read id 2 .*2 records"):
            fq.select([0, 2])
        assert b"".join(fq.pieces(MIB)) == b""          # (the selection of before, exhausted)
        assert _gather(fq, [0, 1])[2] == GOOD + GOOD
    (tmp_path / "r.fq.bz2").write_bytes(bz2.compress(GOOD))
    with pytest.raises(MswError, match="bzip2"):
        core.fastq_open(tmp_path / "r.fq.bz2")
    with pytest.raises(MswError, match="cannot open read file"):
        core.fastq_open(tmp_path / "absent.fq")
    _toy_solves(core)


# ---- 6. an empty file --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True])
def test_an_empty_file(core, tmp_path, monkeypatch, host):
    if host:
        monkeypatch.setenv("MSWEEP_HOST_EXTRACT", "1")
    (tmp_path / "empty.fq").write_bytes(b"")
    with core.fastq_open(tmp_path / "empty.fq") as fq:
        assert fq.info["n_records"] == 0
        assert _gather(fq, []) == (0, 0, b"")
        with pytest.raises(MswError, match=r"read id 0 .*0 records"):
            fq.select([0])
