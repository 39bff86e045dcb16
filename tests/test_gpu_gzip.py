"""GPU: --compress z in the library -- msw_core_gzip_begin / _append / _end and msw_core_text_block_gzip.  The stream the
device writes (deflate_kernels.hpp) is an ordinary single-member gzip file: Python's gzip and zlib read it back to the
input, for host bytes of every size around the 32 KiB chunk and of every kind of content, and for the three text flavours
on the layouts of tests/test_gpu_text_format.py; the conditions on its size (stored chunks for random bytes, matches and
dynamic codes on probs-shaped text), determinism, level 0, the zlib path behind MSWEEP_HOST_GZIP=1, and the refusals."""
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from msweep_amd.core import TEXT_BITSEQ, TEXT_LOGL, TEXT_PROBS, Core, MswError
from msweep_amd.likelihood import from_dense
from test_deflate_format_cpu import probs_text
from test_gpu_text_format import LAYOUTS, build

pytestmark = pytest.mark.gpu

C = 32768       # the chunk (deflate_format.hpp kChunk)


def _contents(n, kind, rng):
    if kind == "repeat":
        return b"a" * n
    if kind == "alternate":
        return (b"ab" * (n // 2 + 1))[:n]
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(11)
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    weighted = np.repeat(np.arange(22, dtype=np.uint8) + 65, fib)      # 46 367 symbols; a chunk of them after the shuffle
    cases = {"empty": b"", "one_byte": b"x", "fibonacci": rng.permutation(weighted)[:C].tobytes(), "probs": probs_text(1_000_000)}
    for kind in ("repeat", "alternate", "random"):
        for n in (C - 1, C, C + 1, 3 * C + 7):
            cases[f"{kind}_{n}"] = _contents(n, kind, rng)
    return cases


def one_member(out, data):
    assert out[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255])
    assert gzip.decompress(out) == data
    d = zlib.decompressobj(wbits=31)
    assert d.decompress(out) == data and d.eof and d.unused_data == b""     # one member, nothing behind it


def stream(core, pieces, level=6):
    out = core.gzip_begin(level)
    for p in pieces:
        out += core.gzip_append(p)
    return out + core.gzip_end()


@pytest.fixture(scope="module")
def core():
    with Core(0) as c:
        yield c


def test_host_bytes_round_trip(core, inputs):
    for name, data in inputs.items():
        out = stream(core, [data])
        one_member(out, data)
        ms, n_in, n_out = core.last_gzip_timing()
        assert (n_in, n_out) == (len(data), len(out)) and ms >= 0.0, name
        if name.startswith("random"):
            # stored chunks: random bytes grow by the stored overhead only
            assert len(out) <= len(data) + 10 * -(-len(data) // C) + 20, name
        if name.startswith("repeat") or name.startswith("alternate"):
            assert len(out) < len(data) // 50 + 400, name                   # matches of 258 and short codes
    assert len(stream(core, [])) == 20 and len(stream(core, [b""])) == 20


def test_uneven_appends_and_determinism(core, inputs):
    for kind in ("repeat", "alternate", "random"):
        data = inputs[f"{kind}_{3 * C + 7}"]
        cuts = [data[:5], data[5:C + 4000], data[C + 4000:]]
        out = stream(core, cuts)
        one_member(out, data)
        assert stream(core, cuts) == out                                    # the same calls, the same bytes
    data = inputs["probs"]
    first = stream(core, [data])
    assert stream(core, [data]) == first
    with Core(0) as other:
        assert stream(other, [data]) == first


def test_probs_shaped_text_needs_matches_and_dynamic_codes(core, inputs):
    data = inputs["probs"]
    out = stream(core, [data])
    one_member(out, data)
    huff = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    z1, zh = len(zlib.compress(data, 1)), len(huff.compress(data) + huff.flush())
    print(f"probs-shaped text: device {len(out) / len(data):.4f}, zlib level 1 {z1 / len(data):.4f}, Z_HUFFMAN_ONLY {zh / len(data):.4f}")
    assert len(out) < (z1 + zh) / 2


def test_fibonacci_alphabet_reaches_long_codes(core, inputs):
    data = inputs["fibonacci"]
    out = stream(core, [data])
    one_member(out, data)
    assert len(out) < len(data) // 2                                        # 22 symbols of Fibonacci weights: ~2.6 bits each


def test_level_0_stores(core, inputs):
    for name in ("probs", "one_byte", f"repeat_{3 * C + 7}"):
        data = inputs[name]
        out = stream(core, [data], level=0)
        one_member(out, data)
        assert len(out) == len(data) + 10 * -(-len(data) // C) + 20 > len(data)
    for level in (1, 9):
        assert stream(core, [inputs["probs"][:100000]], level) == stream(core, [inputs["probs"][:100000]], 6)   # one effort setting


def test_host_gzip_switch_round_trips(inputs, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_GZIP", "1")
    with Core(0) as core:
        for name in ("empty", "one_byte", "probs", f"random_{3 * C + 7}"):
            data = inputs[name]
            for level in (1, 6):
                out = stream(core, [data[:len(data) // 3], data[len(data) // 3:]], level)
                assert gzip.decompress(out) == data
                d = zlib.decompressobj(wbits=31)
                assert d.decompress(out) == data and d.eof and d.unused_data == b""
        monkeypatch.delenv("MSWEEP_HOST_GZIP")
        one_member(stream(core, [inputs["one_byte"]]), inputs["one_byte"])  # read at begin: the device path again


def test_refusals_leave_the_handle_usable(core, inputs):
    with pytest.raises(MswError, match="no gzip stream is open"):
        core.gzip_append(b"abc")
    with pytest.raises(MswError, match="no gzip stream is open"):
        core.gzip_end()
    with pytest.raises(MswError, match="outside 0 ... 9"):
        core.gzip_begin(10)
    with pytest.raises(MswError, match="outside 0 ... 9"):
        core.gzip_begin(-1)
    head = core.gzip_begin(6)
    with pytest.raises(MswError, match="open on this handle already"):
        core.gzip_begin(6)
    with pytest.raises(MswError, match="no likelihood resident"):
        core.text_block_gzip(TEXT_BITSEQ, 0, 1)
    out = head + core.gzip_append(b"still here") + core.gzip_end()
    one_member(out, b"still here")
    with pytest.raises(MswError, match="no gzip stream is open"):
        core.gzip_end()


def _gz_blocks(core, what, E, step=37, **kw):
    """the stream of text_block_gzip over [0, E) in ranges of `step` classes, and the plain text of the same ranges"""
    out, plain, cells, cells_plain, text_len = core.gzip_begin(6), b"", 0, 0, 0
    for e0 in range(0, E, step):
        e1 = min(E, e0 + step)
        k = dict(kw)
        if "line_prefix" in k:
            k["line_prefix"] = k["line_prefix"][e0:e1]
        z, nh, nt = core.text_block_gzip(what, e0, e1, with_info=True, **k)
        out, cells, text_len = out + z, cells + nh, text_len + nt
    out += core.gzip_end()
    for e0 in range(0, E, step):
        e1 = min(E, e0 + step)
        k = dict(kw)
        if "line_prefix" in k:
            k["line_prefix"] = k["line_prefix"][e0:e1]
        t, nh = core.text_block(what, e0, e1, with_host_cells=True, **k)
        plain, cells_plain = plain + t, cells_plain + nh
    assert cells == cells_plain and text_len == len(plain)
    return out, plain, cells


@pytest.mark.parametrize("layout", LAYOUTS)
def test_text_blocks_of_all_flavours(monkeypatch, layout):
    # the smallest shape of test_text_block_all_flavours, and one with several ranges of 37 classes
    for G, E in ((1, 1), (3, 1000)):
        with Core(0) as core:
            logc = build(core, monkeypatch, layout, G, E)
            prefix = np.arange(E, dtype=np.uint64) * np.uint64(977) + np.uint64(1)
            with pytest.raises(MswError, match="no gzip stream is open"):
                core.text_block_gzip(TEXT_BITSEQ, 0, E)
            core.gzip_begin(6)
            with pytest.raises(MswError, match="no solve has run on this handle"):
                core.text_block_gzip(TEXT_PROBS, 0, E)
            with pytest.raises(MswError, match="out of bounds"):
                core.text_block_gzip(TEXT_BITSEQ, 0, E + 1)
            assert core.gzip_end() != b""
            for what, kw in ((TEXT_LOGL, {"line_prefix": prefix}), (TEXT_BITSEQ, {})):
                out, plain, cells = _gz_blocks(core, what, E, **kw)
                one_member(out, plain)
                assert cells == 0 and len(plain) > 0
            core.solve(logc, np.ones(G))
            out, plain, _ = _gz_blocks(core, TEXT_PROBS, E, n_zero_cols=3)
            one_member(out, plain)
            assert plain.count(b"\n") == E


@pytest.mark.parametrize("cap", [None, "2", "0"])
def test_undecided_cells_are_closed_on_the_device(monkeypatch, cap):
    """the dense matrix with ties above 1e6 of test_text_block_undecided_cells_in_a_matrix: the cells the formatter leaves
    to the host are put in on the device (k_text_close); with a list of two entries, or none, the host formats whole blocks
    and their text is uploaded -- the same text under every setting"""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    if cap is not None:
        monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", cap)
    rng = np.random.default_rng(3)
    G, E = 5, 300
    L = -50.0 * rng.random((G, E))
    L[rng.integers(0, G, 60), rng.integers(0, E, 60)] = [-float((2 * int(n) + 1) * 5) for n in rng.integers(100000, 1000000, 60)]
    prefix = np.arange(E, dtype=np.uint64)
    n_ties = int((L < -1e6).sum())
    with Core(0) as core:
        from_dense(core, L, np.zeros(E))
        for step in (37, E):
            out, plain, cells = _gz_blocks(core, TEXT_LOGL, E, step=step, line_prefix=prefix)
            one_member(out, plain)
            want = b"".join(str(j).encode() + b"".join(b"\t" + ("%g" % v).encode() for v in L[:, j]) + b"\n" for j in range(E))
            assert plain == want
            if cap is None:
                assert cells == n_ties
            else:
                assert cells >= n_ties          # whole blocks (those with more undecided cells than the list holds)
        out, plain, _ = _gz_blocks(core, TEXT_BITSEQ, 290, step=41)
        one_member(out, plain)


# ---- the streams pinned ------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gzip_streams.json")


def pinned_streams(setenv, delenv):
    """(name, stream) of the calls tests/golden/gzip_streams.json pins: a fixed gzip_append input, and the 5 x 300 tie matrix
    of test_undecided_cells_are_closed_on_the_device as LOGL in ranges of 37 classes and of E, with the whole list and with
    a list of two entries.  Only the Core API: the same function runs on any build of the library."""
    setenv("MSWEEP_DENSE_COMPRESS", "0")
    delenv("MSWEEP_TEXT_HOST_CAP", raising=False)
    delenv("MSWEEP_HOST_GZIP", raising=False)
    rng = np.random.default_rng(3)
    G, E = 5, 300
    L = -50.0 * rng.random((G, E))
    L[rng.integers(0, G, 60), rng.integers(0, E, 60)] = [-float((2 * int(n) + 1) * 5) for n in rng.integers(100000, 1000000, 60)]
    prefix = np.arange(E, dtype=np.uint64)
    with Core(0) as core:
        yield "append_probs_text", stream(core, [probs_text(3 * C + 7, seed=5)])
        from_dense(core, L, np.zeros(E))
        for cap in (None, "2"):
            if cap:
                setenv("MSWEEP_TEXT_HOST_CAP", cap)
            for step in (37, E):
                out, plain, _ = _gz_blocks(core, TEXT_LOGL, E, step=step, line_prefix=prefix)
                one_member(out, plain)
                yield f"ties_logl_step{step}_cap{cap}", out


def test_compressed_streams_are_the_recorded_ones(monkeypatch):
    """the compressed bytes are a function of the text, the chunk size and the call boundaries: length and SHA-256 of the
    streams above against tests/golden/gzip_streams.json, recorded once from the library as it was before the text and
    gzip outputs shared their block pipeline"""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = {name: {"len": len(out), "sha256": hashlib.sha256(out).hexdigest()} for name, out in pinned_streams(monkeypatch.setenv, monkeypatch.delenv)}
    assert len(got) == 5
    assert got == want
