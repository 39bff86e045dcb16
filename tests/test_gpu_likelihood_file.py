"""GPU: --read-likelihood files parsed on the device (msw_core_set_dense_logl_file / _text: likelihood_text_kernels.hpp,
host_likelihood_file.inc).  The yardstick is the host parser, read_likelihood_file, followed by set_dense_logl on a second
handle: a SERVED file leaves the same resident likelihood -- get_dense_logl bit for bit (compared as uint64: NaN sign and
-0 included), layout hash, shape, counts --, a file outside the strict grammar is NOT SERVED, returns 0 and leaves the handle
as it was.  No test here looks for a fault: malformed text only ever yields "not served"."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from msweep_amd.__main__ import main, read_likelihood_file
from msweep_amd.core import Core, MswError
from msweep_amd.likelihood import from_dense, from_likelihood_file

pytestmark = pytest.mark.gpu

TILE = 4096
COUNT_RE = re.compile(rb"[0-9]{1,18}\Z")
CELL_RE = re.compile(rb"(-?(inf|nan)|-?[0-9]+(\.[0-9]+)?(e[+-]?[0-9]+)?)\Z")


def grammar_ok(text, G):
    """the grammar the device serves (include/msweep_core.h), restated"""
    if not text:
        return False
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    for ln in lines:
        parts = ln.split(b"\t")
        if len(parts) != G + 1 or not COUNT_RE.match(parts[0]):
            return False
        if any(len(c) > 24 or not CELL_RE.match(c) for c in parts[1:]):
            return False
    return bool(lines)


@pytest.fixture(scope="module")
def host_core():
    c = Core(0)
    yield c
    c.close()


def _layout(core):
    """the layout hash of the CSR-of-ECs flavour, "dense" for a matrix kept dense"""
    try:
        return core.layout_hash()
    except MswError:
        return "dense"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _host(tmp_path, text, G, host_core, name="lik.tsv"):
    p = tmp_path / name
    p.write_bytes(text)
    counts, L = read_likelihood_file(str(p), G)
    host_core.set_dense_logl(L)
    return counts, L


def _assert_same(dev, host_core, counts, want_counts):
    assert dev.shape() == host_core.shape()
    assert _layout(dev) == _layout(host_core)
    assert np.array_equal(_bits(dev.get_dense_logl()), _bits(host_core.get_dense_logl()))
    assert counts.dtype == np.uint64 and np.array_equal(counts, want_counts)


def _check_served(tmp_path, gpu_core, host_core, text, G, n_host=None):
    info, counts = gpu_core.set_dense_logl_text(text, G)
    assert info["served"] == 1 and info["reason"] == 0, info
    assert info["text_bytes"] == len(text)
    want_counts, L = _host(tmp_path, text, G, host_core)
    assert info["n_ecs"] == L.shape[1]
    if n_host is not None:
        assert info["n_host_cells"] == n_host, info
    _assert_same(gpu_core, host_core, counts, want_counts)
    return info, L


def _random_text(G, E, seed):
    """cells "%g" of seeded values whose tokens are 1 to 13 bytes long; one kind in seven has a three-digit exponent, which
    is outside the kernels' exact case: those cells come back through the host's strtod"""
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 7, size=(E, G))
    gens = [rng.integers(0, 10, size=(E, G)).astype(float),              # "7", "0": 1 byte
            -np.exp(rng.uniform(-30, 5, size=(E, G))),                   # "-1.23457e-09": 12 bytes
            -rng.uniform(0, 50, size=(E, G)),                            # "-23.4567"
            np.round(-rng.uniform(0, 50, size=(E, G)), 1),               # "-23.4"
            -rng.integers(1, 10**6, size=(E, G)).astype(float),          # "-123456"
            rng.uniform(0, 1e-3, size=(E, G)),                           # "0.000123457"
            -np.exp(rng.uniform(-290, -231, size=(E, G)))]               # "-1.23457e-110": 13 bytes
    vals = np.choose(kinds, gens)
    counts = rng.integers(1, 5000, size=E)
    lines = [str(int(counts[j])) + "\t" + "\t".join("%g" % x for x in vals[j]) for j in range(E)]
    return ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def text_7x700():
    return _random_text(7, 700, 11)


def test_handwritten_file(tmp_path, gpu_core, host_core):
    text = (b"3\t-4.60517\t-0.5\t-12\n1\t-4.60517\t-4.60517\t-1e-05\n10\t-0.25\t-4.60517\t-3.5e+00\n"
            b"7\t0\t-4.60517\t-100\n2\t-4.60517\t-7.25\t-4.60517\n")
    info, L = _check_served(tmp_path, gpu_core, host_core, text, 3, n_host=0)
    assert L.shape == (3, 5) and L[2, 0] == -12.0 and info["n_ecs"] == 5


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_files(tmp_path, gpu_core, host_core, seed):
    text = _random_text(7, 700, seed)
    lens = {len(c) for ln in text.split(b"\n")[:-1] for c in ln.split(b"\t")[1:]}
    assert min(lens) == 1 and max(lens) == 13
    assert len(text) > 8 * TILE                                          # several tiles
    n_host = len(re.findall(rb"e-[0-9]{3}[\t\n]", text))          # the three-digit exponents
    _check_served(tmp_path, gpu_core, host_core, text, 7, n_host=n_host)
    _check_served(tmp_path, gpu_core, host_core, text[:-1], 7, n_host=n_host)    # the last line without its '\n'


def _fill_lines(n, head, unit):
    """exactly n bytes of well-formed lines: 16-byte `unit` lines, then one line `head` + digits + '\\n' (n >= 16)"""
    out = b""
    while n > len(head) + 24 + 1:
        out += unit
        n -= len(unit)
    digits = n - len(head) - 1
    assert len(unit) == 16 and 1 <= digits <= 24
    return out + head + b"7" * digits + b"\n"


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_text_of_exactly_whole_tiles(tmp_path, gpu_core, host_core, seed):
    """lines added until the text is exactly a multiple of the 4 096-byte tile: no padding byte inside the last tile"""
    text = _random_text(7, 700, seed)
    out = text[:text.index(b"\n", 6 * TILE) + 1]
    rest = -len(out) % TILE
    out += _fill_lines(rest if rest >= 16 else rest + TILE, b"1\t0\t0\t0\t0\t0\t0\t", b"1\t0\t0\t0\t0\t0\t0\t5\n")
    assert len(out) % TILE == 0 and len(out) >= 7 * TILE and grammar_ok(out, 7)
    _check_served(tmp_path, gpu_core, host_core, out, 7)


def test_shapes(tmp_path, gpu_core, host_core):
    _check_served(tmp_path, gpu_core, host_core, _random_text(1, 1000, 21), 1)       # G = 1
    wide = _random_text(1025, 3, 22)                                                          # lines longer than two tiles
    assert min(len(ln) for ln in wide.split(b"\n")[:-1]) > 2 * TILE
    _check_served(tmp_path, gpu_core, host_core, wide, 1025)
    _check_served(tmp_path, gpu_core, host_core, b"5\t-1.5\t-2.5\t-4.60517\n", 3, n_host=0)    # E = 1
    _check_served(tmp_path, gpu_core, host_core, b"5\t-1.5\t-2.5\t-4.60517", 3, n_host=0)


def _filler(n):
    """n bytes of well-formed G = 2 lines"""
    return _fill_lines(n, b"1\t0\t", b"1\t0\t-1234567890\n")


def test_tokens_at_segment_and_tile_boundaries(tmp_path, gpu_core, host_core):
    long_cell = b"-0.123456789012345678901"                      # 24 bytes, 21 significant digits
    line15 = b"1\t-123456789.5\t-0.75\n"                         # "-0.75" starts 15 bytes into the line
    assert len(long_cell) == 24 and line15.index(b"-0.75") == 15
    cases = {
        "a token starts at byte 15 of a segment": _filler(80) + line15 + b"2\t-1\t-2\n",
        "a token starts at the last byte of a tile": _filler(TILE - 16) + line15 + b"2\t-1\t-2\n",
        "a line feed is the last byte of a tile": _filler(TILE) + b"3\t-1.5\t-2.5\n",
        "a 24-byte token crosses a tile boundary": _filler(TILE - 16) + b"1\t0\t" + long_cell + b"\n2\t-1\t-2\n",
    }
    assert cases["a token starts at byte 15 of a segment"].index(b"-0.75") == 80 + 15
    assert cases["a token starts at the last byte of a tile"].index(b"-0.75") == TILE - 1
    assert cases["a line feed is the last byte of a tile"][TILE - 1:TILE + 1] == b"\n3"
    assert cases["a 24-byte token crosses a tile boundary"].index(long_cell) == TILE - 12
    for name, text in cases.items():
        assert grammar_ok(text, 2), name
        # (the 24-byte cell has 21 significant digits: the host's strtod converts it)
        _check_served(tmp_path, gpu_core, host_core, text, 2, n_host=1 if "24-byte" in name else 0)


def test_values_decided_on_the_device(gpu_core):
    tokens = ["0", "-0", "inf", "-inf", "nan", "-nan", "1e-05", "1e+06", "-4.60517", "123456789012345"]
    text = ("9\t" + "\t".join(tokens) + "\n").encode()
    info, counts = gpu_core.set_dense_logl_text(text, len(tokens))
    assert info["served"] == 1 and info["n_host_cells"] == 0 and counts.tolist() == [9]
    got = _bits(gpu_core.get_dense_logl())[:, 0]
    want = np.array([struct.unpack("<Q", struct.pack("<d", float(t)))[0] for t in tokens], np.uint64)
    assert got.tolist() == want.tolist()


def test_values_outside_the_fast_domain_go_to_the_host(tmp_path, gpu_core, host_core):
    planted = ["-1.23457e-308", "123456789012345678", "1e23", "1e-23", "2.5e-320"]
    rng = np.random.default_rng(5)
    G, E = 5, 300
    cells = [["%g" % x for x in -rng.uniform(0, 50, G)] for _ in range(E)]
    where = [(3, 0), (77, 4), (150, 2), (299, 1), (299, 3)]
    for (j, g), tok in zip(where, planted):
        cells[j][g] = tok
    text = "".join(f"{j + 1}\t" + "\t".join(cells[j]) + "\n" for j in range(E)).encode()
    info, L = _check_served(tmp_path, gpu_core, host_core, text, G, n_host=5)
    got = _bits(gpu_core.get_dense_logl())
    for (j, g), tok in zip(where, planted):
        assert got[g, j] == struct.unpack("<Q", struct.pack("<d", float(tok)))[0], tok
    # a value strtod cannot represent: not served, each driver's own parser decides
    bad = text.replace(b"1e23", b"1e400")
    before = _layout(gpu_core), gpu_core.shape()
    info, counts = gpu_core.set_dense_logl_text(bad, G)
    assert info["served"] == 0 and info["reason_text"] == "range error" and counts is None
    assert (_layout(gpu_core), gpu_core.shape()) == before


def _background_text():
    rng = np.random.default_rng(40)
    G, E = 40, 3000
    vals = np.round(-rng.uniform(0.1, 30, 50), 3)
    cells = np.where(rng.random((E, G)) < 0.9, -4.60517, vals[rng.integers(0, 50, (E, G))])
    counts = rng.integers(1, 200, E)
    return ("".join(f"{int(counts[j])}\t" + "\t".join("%g" % x for x in cells[j]) + "\n" for j in range(E))).encode(), G, E


@pytest.mark.parametrize("compress", ["default", "0"])
def test_background_structure_and_solve(tmp_path, gpu_core, host_core, monkeypatch, compress):
    """a matrix of the shape the reference writes (one background value, few others): both paths re-express it alike
    (the background is sampled from the stage, not from a host matrix) and solve to the same bits; MSWEEP_DENSE_COMPRESS=0:
    both keep it dense"""
    if compress == "0":
        monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    text, G, E = _background_text()
    info, counts = gpu_core.set_dense_logl_text(text, G)
    assert info["served"] == 1
    want_counts, L = _host(tmp_path, text, G, host_core)
    _assert_same(gpu_core, host_core, counts, want_counts)
    nnz_dev, nnz_host = gpu_core.shape()[2], host_core.shape()[2]
    assert nnz_dev == nnz_host
    assert (nnz_dev < G * E) if compress == "default" else (nnz_dev == G * E and _layout(gpu_core) == "dense")
    logc = np.log(want_counts.astype(np.float64))
    a = gpu_core.solve(logc, np.ones(G), tol=1e-6)
    b = host_core.solve(logc, np.ones(G), tol=1e-6)
    assert a["iters"] == b["iters"] and np.array_equal(_bits(a["theta"]), _bits(b["theta"]))


GOOD = b"".join(b"%d\t-4.60517\t-1.5\t-0.25\n" % (j + 1) for j in range(400))      # G = 3, 22 bytes a line: > 2 tiles


def _with_defect(defect, later):
    lines = GOOD.split(b"\n")[:-1]
    k = 250 if later else 2            # line 250 starts beyond byte 4 096
    if later:
        assert len(b"\n".join(lines[:k])) > TILE
    ln = lines[k]
    cell = {"0x10": b"0x10", "1_0": b"1_0", "1E5": b"1E5", "Inf": b"Inf", "leading blank": b" 1", ".": b".",
            "25-byte token": b"-0.1234567890123456789012"}
    if defect in cell:
        assert defect != "25-byte token" or len(cell[defect]) == 25
        lines[k] = ln.replace(b"-1.5", cell[defect])
    elif defect == "extra column":
        lines[k] = ln + b"\t-1"
    elif defect == "missing column":
        lines[k] = ln.rsplit(b"\t", 1)[0]
    elif defect == "crlf":
        lines[k] = ln + b"\r"
    elif defect == "blank line":
        lines.insert(k, b"")
    elif defect == "+5 as count":
        lines[k] = b"+5" + ln[ln.index(b"\t"):]
    elif defect == "19-digit count":
        lines[k] = b"1234567890123456789" + ln[ln.index(b"\t"):]
    return b"\n".join(lines) + b"\n"


REASON = {"extra column": "column count", "missing column": "column count", "crlf": "bad byte", "blank line": "column count",
          "+5 as count": "bad token", "19-digit count": "bad token", "0x10": "bad byte", "1_0": "bad byte", "1E5": "bad byte",
          "Inf": "bad byte", "leading blank": "bad byte", ".": "bad token", "25-byte token": "bad token"}


@pytest.fixture(scope="module")
def resident(gpu_core):
    """a likelihood set before the calls that are not served: it must still be there afterwards"""
    info, _ = gpu_core.set_dense_logl_text(GOOD, 3)
    assert info["served"] == 1
    return _layout(gpu_core), gpu_core.shape(), _bits(gpu_core.get_dense_logl()).copy()


def _assert_untouched(gpu_core, resident):
    assert (_layout(gpu_core), gpu_core.shape()) == resident[:2]
    assert np.array_equal(_bits(gpu_core.get_dense_logl()), resident[2])


@pytest.mark.parametrize("later", [False, True], ids=["first tile", "later tile"])
@pytest.mark.parametrize("defect", sorted(REASON))
def test_not_served(gpu_core, resident, defect, later):
    text = _with_defect(defect, later)
    assert not grammar_ok(text, 3)
    info, counts = gpu_core.set_dense_logl_text(text, 3)            # returns: rc = 0
    assert info["served"] == 0 and counts is None and info["reason_text"] == REASON[defect], info
    _assert_untouched(gpu_core, resident)


def test_not_served_whole_file_cases(tmp_path, gpu_core, resident):
    info, counts = gpu_core.set_dense_logl_text(GOOD + b"\n", 3)    # a blank line at the end
    assert info["served"] == 0 and info["reason_text"] == "column count"
    info, counts = gpu_core.set_dense_logl_text(b"", 3)
    assert info["served"] == 0 and info["reason_text"] == "empty"
    (tmp_path / "empty.tsv").write_bytes(b"")
    info, counts = gpu_core.set_dense_logl_file(str(tmp_path / "empty.tsv"), 3)
    assert info["served"] == 0 and info["reason_text"] == "empty"
    info, counts = gpu_core.set_dense_logl_file(str(tmp_path / "no_such_file.tsv"), 3)
    assert info["served"] == 0 and info["reason_text"] == "open / read" and counts is None
    info, counts = gpu_core.set_dense_logl_text(GOOD, 4)            # the wrong number of groups
    assert info["served"] == 0 and info["reason_text"] == "column count"
    _assert_untouched(gpu_core, resident)


def test_forced_to_the_host(gpu_core, resident, monkeypatch):
    monkeypatch.setenv("MSWEEP_HOST_LIKELIHOOD_FILE", "1")
    info, counts = gpu_core.set_dense_logl_text(GOOD, 3)
    assert info["served"] == 0 and info["reason_text"] == "forced" and counts is None
    _assert_untouched(gpu_core, resident)


FUZZ_SEED = 2024
FUZZ_ALPHABET = b"0123456789012345678901234567890123456789.-+e\t\n infaxE_\r"


def _mutations(text, n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        kind, at, b = int(rng.integers(0, 3)), int(rng.integers(0, len(text))), FUZZ_ALPHABET[int(rng.integers(0, len(FUZZ_ALPHABET)))]
        if kind == 0:
            yield text[:at] + bytes([b]) + text[at + 1:]
        elif kind == 1:
            yield text[:at] + bytes([b]) + text[at:]
        else:
            yield text[:at] + text[at + 1:]


def test_mutation_fuzz(tmp_path, gpu_core):
    """300 single-byte mutations of a G = 7, E = 60 file: served and bit-equal to the host parser's matrix, or not served;
    never served where the host parser raises or returns other bits, and never refused inside the grammar but for a value
    strtod cannot represent"""
    base = _random_text(7, 60, 31)
    path = tmp_path / "m.tsv"
    served = 0
    for text in _mutations(base, 300, FUZZ_SEED):
        info, counts = gpu_core.set_dense_logl_text(text, 7)
        if not info["served"]:
            assert not grammar_ok(text, 7) or info["reason_text"] == "range error", (text[:200], info)
            continue
        assert grammar_ok(text, 7)
        served += 1
        path.write_bytes(text)
        want_counts, L = read_likelihood_file(str(path), 7)        # (raises: the test fails -- served where the host refuses)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(_bits(gpu_core.get_dense_logl()), _bits(L))
    print("served", served, "of 300")
    assert served >= 100


def _bgzf(text):
    out = b""
    for o in list(range(0, len(text), 0xff00)) + [None]:
        chunk = b"" if o is None else text[o:o + 0xff00]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        bsize = 12 + 6 + len(payload) + 8 - 1
        out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + payload +
                struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return out


def test_compressed_files(tmp_path, gpu_core, host_core, text_7x700):
    want_counts, L = _host(tmp_path, text_7x700, 7, host_core)
    half = text_7x700.index(b"\n", len(text_7x700) // 2) + 1
    files = {"single.gz": gzip.compress(text_7x700, 6), "bgzf.gz": _bgzf(text_7x700),
             "pair.gz": gzip.compress(text_7x700[:half], 6) + gzip.compress(text_7x700[half:], 6)}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        info, counts = gpu_core.set_dense_logl_file(str(tmp_path / name), 7)
        assert info["served"] == 1 and info["text_bytes"] == len(text_7x700), (name, info)
        _assert_same(gpu_core, host_core, counts, want_counts)
        if name == "bgzf.gz":
            assert info["inflate"]["on_device"] == 1 and info["inflate"]["n_members"] >= 2
        if name == "pair.gz":
            assert info["inflate"]["on_device"] == 0        # several members without declared lengths: zlib
        # the host parser reads the same file (gzip.open)
        c2, L2 = read_likelihood_file(str(tmp_path / name), 7)
        assert np.array_equal(c2, want_counts) and np.array_equal(_bits(L2), _bits(L))
    (tmp_path / "plain.tsv").write_bytes(text_7x700)
    info, counts = gpu_core.set_dense_logl_file(str(tmp_path / "plain.tsv"), 7)
    assert info["served"] == 1 and info["inflate"]["payload_bytes"] == 0
    _assert_same(gpu_core, host_core, counts, want_counts)


# ---- drivers ------------------------------------------------------------------------------------------------------------
from test_gpu_cli_toy import _toy  # noqa: E402


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from conftest import ROOT
    out = str(tmp_path_factory.mktemp("mini_likfile") / "msweep_mini")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", out, os.path.join(lib, "cpp", "msweep_mini.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return out


@pytest.fixture(scope="module")
def toy_files(tmp_path_factory, mini):
    """the toy input, its likelihood file plain and gzip (--compress z), written by the Python driver"""
    d = tmp_path_factory.mktemp("likfile_toy")
    _toy(d, n_reads=600)
    base = ["--themisto-1", str(d / "toy_1.txt"), "--themisto-2", str(d / "toy_2.txt"), "-i", str(d / "clustering.txt")]
    assert main(base + ["-o", str(d / "w"), "--write-likelihood", "--no-fit-model"]) == 0
    assert main(base + ["-o", str(d / "z"), "--write-likelihood", "--no-fit-model", "--compress", "z"]) == 0
    assert gzip.decompress((d / "z_likelihoods.tsv.gz").read_bytes()) == (d / "w_likelihoods.tsv").read_bytes()
    return d


def _run_driver(which, mini, args, env_switch, monkeypatch):
    if which == "python":
        if env_switch:
            monkeypatch.setenv("MSWEEP_HOST_LIKELIHOOD_FILE", "1")
        else:
            monkeypatch.delenv("MSWEEP_HOST_LIKELIHOOD_FILE", raising=False)
        return main(args), ""
    env = dict(os.environ)
    env.pop("MSWEEP_HOST_LIKELIHOOD_FILE", None)
    if env_switch:
        env["MSWEEP_HOST_LIKELIHOOD_FILE"] = "1"
    p = subprocess.run([mini] + args, capture_output=True, text=True, timeout=120, env=env)
    return p.returncode, p.stderr


@pytest.mark.parametrize("which", ["python", "mini"])
def test_drivers_read_the_file_on_either_path(tmp_path, toy_files, mini, gpu_core, which, monkeypatch, capfd):
    d = toy_files
    outs = {}
    for name, lf in (("plain", "w_likelihoods.tsv"), ("gz", "z_likelihoods.tsv.gz")):
        for switch in (False, True):
            pre = str(tmp_path / f"{name}_{int(switch)}")
            rc, err = _run_driver(which, mini, ["-i", str(d / "clustering.txt"), "--read-likelihood", str(d / lf), "-o", pre,
                                                "--write-probs", "--verbose"], switch, monkeypatch)
            err += capfd.readouterr().err
            assert rc == 0, err
            note = [ln for ln in err.splitlines() if ln.startswith("note: ") and "likelihood file parsed on" in ln]
            assert len(note) == 1, err
            assert note[0] == f"note: {d / lf}: likelihood file parsed on " + ("the host (forced)" if switch else "the device (0 cells on the host)")
            outs[name, switch] = (open(pre + "_abundances.txt").read(), open(pre + "_probs.tsv").read())
    assert outs["plain", False] == outs["plain", True] == outs["gz", False] == outs["gz", True]
    # ... and what read_likelihood_file + from_dense give directly
    monkeypatch.delenv("MSWEEP_HOST_LIKELIHOOD_FILE", raising=False)
    from msweep_amd.__main__ import write_probs
    from msweep_amd.reference import read_reference
    from msweep_amd.sample import PlainSample
    grouping = read_reference(open(d / "clustering.txt"))
    counts, L = read_likelihood_file(str(d / "w_likelihoods.tsv"), grouping.get_n_groups())
    gpu_core.set_pack_schedule(False)        # (as the drivers choose for a run without bootstrap)
    try:
        lik = from_dense(gpu_core, L, np.log(counts.astype(np.float64)))
    finally:
        gpu_core.set_pack_schedule(True)
    res = gpu_core.solve(lik.log_counts(), np.ones(L.shape[0]), 1e-6, 5000)
    total = int(counts.sum())
    sample = PlainSample(total, total)
    sample.store_abundances(res["theta"])
    with open(tmp_path / "direct_abundances.txt", "w") as f:
        sample.write_abundances(grouping.get_names(), f)
    with open(tmp_path / "direct_probs.tsv", "w") as f:
        write_probs(f, grouping.get_names(), [], gpu_core)
    assert outs["plain", False] == (open(tmp_path / "direct_abundances.txt").read(), open(tmp_path / "direct_probs.tsv").read())


@pytest.mark.parametrize("which", ["python", "mini"])
def test_drivers_keep_their_message_for_a_wrong_column_count(tmp_path, toy_files, mini, which, monkeypatch, capfd):
    d = toy_files
    rc, err = _run_driver(which, mini, ["-i", str(d / "clustering.txt"), "--read-likelihood", str(d / "toy_1.txt")], False, monkeypatch)
    err += capfd.readouterr().err
    assert rc == 1 and "Building the log-likelihood array failed" in err and "Could not read from the likelihoods file." in err


def test_from_likelihood_file(toy_files, gpu_core, host_core, monkeypatch):
    G = 4
    lik = from_likelihood_file(gpu_core, str(toy_files / "z_likelihoods.tsv.gz"), G)
    assert lik.file_info["served"] == 1 and lik.groups_considered().all() and lik.n_groups == G
    monkeypatch.setenv("MSWEEP_HOST_LIKELIHOOD_FILE", "1")
    ref = from_likelihood_file(host_core, str(toy_files / "w_likelihoods.tsv"), G)
    assert ref.file_info["served"] == 0 and ref.file_info["reason_text"] == "forced"
    assert np.array_equal(lik.ec_counts, ref.ec_counts) and np.array_equal(lik.log_counts(), ref.log_counts())
    assert np.array_equal(_bits(lik.log_mat()), _bits(ref.log_mat())) and lik.n_ecs == ref.n_ecs


def test_cpp_shim_from_file(tmp_path, toy_files):
    """msw::DeviceLikelihood::from_file (rcgpar_hip.hpp), the mirror of LL_WOR21::from_file: the same theta as the matrix
    route (set_dense of the host-parsed matrix), and the reference's message for a file that cannot be opened"""
    from conftest import ROOT
    exe = str(tmp_path / "likelihood_file_test")
    lib = os.path.join(ROOT, "msweep_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "likelihood_file_test.cpp"),
                           "-L" + lib, "-lmsweep_core", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    for lf in ("w_likelihoods.tsv", "z_likelihoods.tsv.gz"):
        p = subprocess.run([exe, str(toy_files / lf), "4"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out = dict(ln.split(" ", 1) for ln in p.stdout.strip().splitlines())
        assert out["served"] == "1" and out["theta_file"] == out["theta_matrix"] and out["iters_file"] == out["iters_matrix"]
    p = subprocess.run([exe, str(tmp_path / "missing.tsv"), "4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "exception Could not read from the likelihoods file." in p.stdout
    # text the device does not serve reaches the shim's own parser: the reference's message for what that does not take either
    good = (toy_files / "w_likelihoods.tsv").read_text().splitlines()
    for name, bad_line in (("cell", good[1].replace("\t", "\tx", 1)), ("count", "-5" + good[1][good[1].index("\t"):]),
                           ("columns", good[1] + "\t-1"), ("empty cell", good[1].replace("\t", "\t\t", 1))):
        (tmp_path / "bad.tsv").write_text("\n".join([good[0], bad_line] + good[2:]) + "\n")
        p = subprocess.run([exe, str(tmp_path / "bad.tsv"), "4"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "exception Could not read from the likelihoods file." in p.stdout, (name, p.stdout)
    # ... and a well-formed file outside the device's grammar ("1E1": upper case) is read by it
    (tmp_path / "upper.tsv").write_text("\n".join([good[0].replace("\t", "\t-1E1\t", 1).rsplit("\t", 1)[0]] + good[1:]) + "\n")
    p = subprocess.run([exe, str(tmp_path / "upper.tsv"), "4"], capture_output=True, text=True, timeout=60)
    out = dict(ln.split(" ", 1) for ln in p.stdout.strip().splitlines())
    assert p.returncode == 0 and out["served"] == "0" and out["theta_file"] == out["theta_matrix"], p.stdout
