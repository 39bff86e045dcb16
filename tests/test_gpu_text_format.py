"""GPU: the text of the matrix outputs formatted on the device (msweep_amd/csrc/text_kernels.hpp, g6_format.hpp).

msw_core_format_g6 against Python's "%g" (the same correctly rounded six digits glibc prints), byte for byte: random
values of four generators, the adversarial list, exact ties, sizes around every boundary of the kernels.
msw_core_text_block -- PROBS, LOGL, BITSEQ -- on the four record encodings and the dense flavour against a host
rendering of get_dense_logl / gamma_block, and its refusals."""
import math
from fractions import Fraction

import numpy as np
import pytest

from msweep_amd import synth
from msweep_amd.core import TEXT_BITSEQ, TEXT_LOGL, TEXT_PROBS, Core, MswError
from msweep_amd.likelihood import from_dense, from_grouped_counts

pytestmark = pytest.mark.gpu


def g6(x):
    return ("%g" % x).encode()


def lines_of(values):
    return b"".join(g6(float(x)) + b"\n" for x in values)


# ---- 2a. random values ---------------------------------------------------------------------------------------------
def test_format_random_values(gpu_core):
    rng = np.random.default_rng(20240611)
    bits = rng.integers(0, 2**64, 260_000, dtype=np.uint64)
    bits = bits[((bits >> np.uint64(52)) & np.uint64(0x7ff)) != np.uint64(0x7ff)][:200_000]
    assert len(bits) == 200_000
    x = np.concatenate([bits.view(np.float64), rng.random(200_000), np.exp(-745.0 * rng.random(200_000)),
                        -50.0 * rng.random(100_000)])
    text, n_host = gpu_core.format_g6(x, with_host_cells=True)
    want = lines_of(x)
    if text != want:
        got = text.split(b"\n")
        bad = [(float(v), g, w) for v, g, w in zip(x, got, want.split(b"\n")) if g != w][:10]
        raise AssertionError(f"{len(got) - 1} lines, first differences {bad}")
    assert n_host <= 1e-4 * len(x), n_host


# ---- 2b. the adversarial list --------------------------------------------------------------------------------------
def test_format_adversarial_list(gpu_core):
    x = [0.0, -0.0, 0.5, 1.0, 100000.0, 1e6, 123456.7, 0.0001, 1e-5, 0.9999995, 0.99999951, 999999.5, 999999.4999999999,
         9.9999995e-5, 0.000099999949, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308]
    for k in range(-323, 309):
        p = float("1e%d" % k)
        x += [p, math.nextafter(p, 0.0), math.nextafter(p, math.inf), -p]
    assert gpu_core.format_g6(x) == lines_of(x)
    special = np.array([0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000,
                        0x7ff0000000000001, 0xfff0000000000001], np.uint64).view(np.float64)
    assert gpu_core.format_g6(special) == b"inf\n-inf\nnan\n-nan\nnan\n-nan\n"


# ---- 2c. ties --------------------------------------------------------------------------------------------------------
def test_format_exact_ties_round_half_even(gpu_core):
    rng = np.random.default_rng(7)
    x, want = [100000.5, 12345.25, 1.015625, 13 / 128], [b"100000", b"12345.2", b"1.01562", b"0.101562"]
    for X in range(-3, 6):
        unit = Fraction(1, 2 ** (6 - X))
        lo, hi = Fraction(10) ** X, Fraction(10) ** (X + 1)
        m0, m1 = math.ceil(lo / unit) | 1, math.floor(hi / unit)
        for m in (m0 + 2 * rng.integers(0, (m1 - m0) // 2, 200)):
            m = int(m) | 1
            v = m * unit
            assert lo <= v < hi
            scaled = v * Fraction(10) ** (5 - X)                       # the six digits and a half: a tie
            assert scaled.denominator == 2
            n = scaled.numerator // 2
            n += n & 1                                                   # half to even
            xf = float(v)
            assert Fraction(xf) == v
            x.append(xf)
            want.append(g6(float(Fraction(n) / Fraction(10) ** (5 - X))))
            assert want[-1] == g6(xf)                                    # (Python's own rounding agrees)
    text = gpu_core.format_g6(x)
    assert text == b"".join(w + b"\n" for w in want)


def test_format_ties_the_device_leaves_to_the_host(gpu_core, monkeypatch):
    """(2 N + 1) 5 10^j: ties above 1e6, where the power of ten is not exact in 64 bits -- the device leaves 13 blanks
    and the host fills them in and closes the gaps; with a list of two entries the host formats the whole block."""
    rng = np.random.default_rng(9)
    ties = [float((2 * int(n) + 1) * 5 * 10 ** j) for j in range(0, 9) for n in rng.integers(100000, 1000000, 40)]
    x = np.array([1.0, 0.25] * len(ties) + [1e-300])
    x[1:2 * len(ties):2] = ties
    text, n_host = gpu_core.format_g6(x, with_host_cells=True)
    assert text == lines_of(x)
    assert n_host == len(ties)
    monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", "2")
    text, n_host = gpu_core.format_g6(x, with_host_cells=True)
    assert text == lines_of(x)
    assert n_host == len(x)


# ---- 2d. sizes -------------------------------------------------------------------------------------------------------
WIDTHS = [1.0, -1.0, 0.5, -0.5, 1e-5, -1e-5, 1.5e-5, 1.25e-5, 1.125e-5, 1.0625e-5, 1.03125e-5, -1.03125e-5, -1.03125e-300]

# 4096 * 64 + 1: one line past the 64-line tile of the write pass, past the 256-lane workgroup of the length pass, past
# the last of the 256 CUs x 16 workgroups of the write pass (its first workgroup takes a second tile) and past every
# power-of-two block of the scan up to 2^18
N_BOUNDARY = 4096 * 64 + 1


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, N_BOUNDARY])
def test_format_sizes_and_irregular_offsets(gpu_core, n):
    assert [len(g6(v)) for v in WIDTHS] == list(range(1, 14))
    x = np.resize(np.array(WIDTHS), n) if n else np.zeros(0)
    assert gpu_core.format_g6(x) == lines_of(x)
    if n > 1:
        assert gpu_core.format_g6(x[::-1].copy()) == lines_of(x[::-1])


# ---- 3. msw_core_text_block ------------------------------------------------------------------------------------------
# "dense_compressed": the dense boundary's CSR form with shared table slots.  The issue's shapes (G <= 257, E <= 1000)
# cannot reach 12-byte VALUE records -- those need more than 65 536 distinct values in at most G E / 4 listed cells --
# so value records are tested at the smallest shape that has them (test_text_block_value_records)
LAYOUTS = ["narrow", "wide", "index", "dense_compressed", "dense"]


def build(core, monkeypatch, layout, G, E, seed=5):
    """a likelihood of exactly G groups and E classes in the asked layout; returns the log counts"""
    rng = np.random.default_rng(seed + 131 * G + E)
    counts = rng.integers(1, 6, E)
    if layout in ("dense_compressed", "dense"):
        if layout == "dense":
            monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
        d = synth.make_dense_problem(E, G, seed=seed, max_support=min(G, 12))
        from_dense(core, d["logl"], np.log(counts))
        if layout == "dense_compressed" and G == 257 and E == 1000:
            assert core.shape()[2] < G * E and core.layout_info()["record_bytes"] != 12    # listed cells, no value records
        return np.log(counts)
    if layout == "wide":
        monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    if layout == "index":
        monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
        monkeypatch.setenv("MSWEEP_HYBRID_HOT", "48")
    sizes = synth.diverse_group_sizes(rng, G) if layout == "index" else rng.integers(1, 20, G)
    sizes = np.asarray(sizes, np.uint64)
    k = rng.integers(1, min(G, 6) + 1, E)
    rowptr = np.zeros(E + 1, np.uint64)
    rowptr[1:] = np.cumsum(k)
    grp = np.concatenate([np.sort(rng.choice(G, kk, replace=False)) for kk in k]).astype(np.uint32)
    cnt = (1 + rng.integers(0, 1 << 30, len(grp)) % sizes[grp].astype(np.int64)).astype(np.uint32)
    from_grouped_counts(core, rowptr, grp, cnt, counts, sizes)
    if G == 257 and E == 1000:
        info = core.layout_info()
        assert info["record_bytes"] == (8 if layout == "wide" else 4)
        assert info["index_records"] == (1 if layout == "index" else 0)
    return np.log(counts)


def ranges(E):
    r = [(0, E), (0, 1), (E - 1, E), (0, 0), (E, E)]
    if E >= 2:
        r.append((1, E - 1))
    if E > 260:
        r += [(250, 260), (255, 257), (500, 501)]
    return r


def render_logl(L, e0, e1, prefix):
    return b"".join(str(int(prefix[j - e0])).encode() + b"".join(b"\t" + g6(v) for v in L[:, j]) + b"\n"
                    for j in range(e0, e1))


def render_bitseq(L, e0, e1):
    G = L.shape[0]
    return b"".join(str(G + 1).encode() + b" " + b"".join(str(g + 1).encode() + b" " + g6(v) + b" " for g, v in enumerate(L[:, j]))
                    + b"0 -10000.00\n" for j in range(e0, e1))


@pytest.mark.parametrize("E", [1, 1000])
@pytest.mark.parametrize("G", [1, 3, 257])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_text_block_all_flavours(monkeypatch, layout, G, E):
    rng = np.random.default_rng(G * 7 + E)
    with Core(0) as core:
        logc = build(core, monkeypatch, layout, G, E)
        L = core.get_dense_logl()
        assert L.shape == (G, E)
        prefix_all = rng.integers(0, 2**63, E).astype(np.uint64)
        prefix_all[::2] = 2**64 - 1
        prefix_all[1::3] = 0
        prefix_all[0] = 0 if G == 1 else 2**64 - 1
        for e0, e1 in ranges(E):
            text, n_host = core.text_block(TEXT_LOGL, e0, e1, line_prefix=prefix_all[e0:e1], with_host_cells=True)
            assert text == render_logl(L, e0, e1, prefix_all[e0:e1]), (e0, e1)
            assert n_host == 0
            assert core.text_block(TEXT_BITSEQ, e0, e1) == render_bitseq(L, e0, e1), (e0, e1)
        # refusals before a solve and on the arguments; the handle stays usable
        with pytest.raises(MswError, match="no solve has run on this handle"):
            core.text_block(TEXT_PROBS, 0, E)
        with pytest.raises(MswError, match="line_prefix"):
            core._check(core._L.msw_core_text_block(core._h, TEXT_LOGL, 0, E, None, 0, *_outs()))
        with pytest.raises(MswError, match="line_prefix"):
            core._check(core._L.msw_core_text_block(core._h, TEXT_BITSEQ, 0, E, prefix_all.ctypes.data, 0, *_outs()))
        with pytest.raises(MswError, match="n_zero_cols"):
            core.text_block(TEXT_BITSEQ, 0, E, n_zero_cols=3)
        with pytest.raises(MswError, match="out of bounds"):
            core.text_block(TEXT_BITSEQ, 0, E + 1)
        with pytest.raises(MswError, match="out of bounds"):
            core.text_block(TEXT_BITSEQ, 1, 0)
        assert core.text_block(TEXT_BITSEQ, 0, 1) == render_bitseq(L, 0, 1)

        core.solve(logc, np.ones(G))
        with pytest.raises(MswError, match=r"1 GiB; at most \d+ classes"):
            core.text_block(TEXT_PROBS, 0, E, n_zero_cols=2**30)
        with pytest.raises(MswError, match="unknown kind of text"):
            core.text_block(7, 0, E)
        for e0, e1 in ranges(E):
            gam = core.gamma_block(e0, e1)
            p = np.exp(gam)
            ok = [[[g6(v) for v in col] for col in c.T] for c in (p, np.nextafter(p, -np.inf), np.nextafter(p, np.inf))]
            for nz in (0, 3):
                text = core.text_block(TEXT_PROBS, e0, e1, n_zero_cols=nz)
                rows = text.split(b"\n")
                assert rows[-1] == b"" and len(rows) == e1 - e0 + 1, (e0, e1)
                for jj, row in enumerate(rows[:-1]):
                    cells = row.split(b"\t")
                    assert len(cells) == 1 + G + nz
                    assert cells[0] == str(e0 + jj).encode()
                    assert cells[1 + G:] == [b"0"] * nz
                    if cells[1:1 + G] != ok[0][jj]:
                        for g in range(G):
                            assert cells[1 + g] in (ok[0][jj][g], ok[1][jj][g], ok[2][jj][g]), (e0 + jj, g, cells[1 + g], p[g, jj])


def test_text_block_value_records():
    """12-byte value records (as tests/test_gpu_binning.py builds them): the smallest shape that reaches them is beyond
    the grid above, so they get a case of their own -- every line of the likelihood, and PROBS / BITSEQ on a range that
    straddles a 64-line tile and a 256-class boundary"""
    d = synth.make_dense_problem(20000, 40, seed=31, max_support=12)
    G, E = 40, 20000
    prefix = np.arange(E, dtype=np.uint64) * np.uint64(1_000_003)
    with Core(0) as core:
        from_dense(core, d["logl"], d["logc"])
        assert core.layout_info()["record_bytes"] == 12
        L = core.get_dense_logl()
        assert core.text_block(TEXT_LOGL, 0, E, line_prefix=prefix) == render_logl(L, 0, E, prefix)
        e0, e1 = 9950, 10300
        assert core.text_block(TEXT_BITSEQ, e0, e1) == render_bitseq(L, e0, e1)
        core.solve(d["logc"], np.ones(G))
        p = np.exp(core.gamma_block(e0, e1))
        ok = [[[g6(v) for v in col] for col in c.T] for c in (p, np.nextafter(p, -np.inf), np.nextafter(p, np.inf))]
        rows = core.text_block(TEXT_PROBS, e0, e1, n_zero_cols=2).split(b"\n")
        assert rows[-1] == b"" and len(rows) == e1 - e0 + 1
        for jj, row in enumerate(rows[:-1]):
            cells = row.split(b"\t")
            assert cells[0] == str(e0 + jj).encode() and cells[1 + G:] == [b"0", b"0"] and len(cells) == G + 3
            for g in range(G):
                assert cells[1 + g] in (ok[0][jj][g], ok[1][jj][g], ok[2][jj][g]), (e0 + jj, g)


def _outs():
    import ctypes as C
    keep = (C.c_void_p(), C.c_size_t(), C.c_size_t())
    _outs.keep = keep
    return C.byref(keep[0]), C.byref(keep[1]), C.byref(keep[2])


def test_text_block_undecided_cells_in_a_matrix(monkeypatch):
    """a dense likelihood that holds ties above 1e6: the device leaves them to the host, which closes the gaps (and,
    with a list of two entries, formats the whole block) -- the same bytes either way"""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    rng = np.random.default_rng(3)
    G, E = 5, 300
    L = -50.0 * rng.random((G, E))
    L[rng.integers(0, G, 60), rng.integers(0, E, 60)] = [-float((2 * int(n) + 1) * 5) for n in rng.integers(100000, 1000000, 60)]
    prefix = np.arange(E, dtype=np.uint64)
    with Core(0) as core:
        from_dense(core, L, np.zeros(E))
        Ld = core.get_dense_logl()
        np.testing.assert_array_equal(Ld, L)
        n_ties = int((L < -1e6).sum())
        for cap in (None, "2"):
            if cap:
                monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", cap)
            text, n_host = core.text_block(TEXT_LOGL, 0, E, line_prefix=prefix, with_host_cells=True)
            assert text == render_logl(L, 0, E, prefix)
            assert n_host == (G * E if cap else n_ties)
            assert core.text_block(TEXT_BITSEQ, 3, 290) == render_bitseq(L, 3, 290)


# ---- 4. the smallest blocks with undecided cells: their gaps are closed on the device -----------------------------------
T_LONG, T_SHORT, X = 1234565.0, 1000005.0, 0.25       # two ties of the kind above (11 bytes and, half to even, "1e+06"); X is ordinary


def _tie_arrays():
    for t in (T_LONG, T_SHORT):
        yield [t]
        yield [t, t, t]
        yield [X, t]
        yield [t, X]
        x = [X, -X, 1e-5] * 21 + [X, X]                 # 65 values: ties at 0, 63 and 64, the edge of k_text_write's 64-line tile
        x[0], x[63], x[64] = t, T_LONG, t
        yield x


def _caps(monkeypatch, n_ties, n_cells):
    """(n_host expected) under the whole list, a list of exactly n_ties entries (the list path still) and one entry fewer
    (the host formats the block)"""
    monkeypatch.delenv("MSWEEP_TEXT_HOST_CAP", raising=False)
    yield n_ties
    monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", str(n_ties))
    yield n_ties
    monkeypatch.setenv("MSWEEP_TEXT_HOST_CAP", str(n_ties - 1))
    yield n_cells


def test_format_smallest_blocks_with_ties(gpu_core, monkeypatch):
    assert g6(T_LONG) == b"1.23456e+06" and g6(T_SHORT) == b"1e+06"
    for x in _tie_arrays():
        n_ties = sum(v in (T_LONG, T_SHORT) for v in x)
        for want_host in _caps(monkeypatch, n_ties, len(x)):
            text, n_host = gpu_core.format_g6(np.array(x), with_host_cells=True)
            assert text == lines_of(x), x
            assert n_host == want_host, x


@pytest.mark.parametrize("n", [1, 2])
def test_text_block_smallest_all_tie_matrices(monkeypatch, n):
    """dense n x n, every cell a tie: LOGL, and BITSEQ where a suffix follows the last cell"""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    L = -np.array([[T_LONG, T_SHORT], [T_SHORT, T_LONG]])[:n, :n]
    prefix = np.arange(n, dtype=np.uint64) + np.uint64(7)
    with Core(0) as core:
        from_dense(core, L, np.zeros(n))
        np.testing.assert_array_equal(core.get_dense_logl(), L)
        for want_host in _caps(monkeypatch, n * n, n * n):
            text, n_host = core.text_block(TEXT_LOGL, 0, n, line_prefix=prefix, with_host_cells=True)
            assert text == render_logl(L, 0, n, prefix)
            assert n_host == want_host
            text, n_host = core.text_block(TEXT_BITSEQ, 0, n, with_host_cells=True)
            assert text == render_bitseq(L, 0, n)
            assert n_host == want_host
