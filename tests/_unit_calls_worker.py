"""One process of tests/test_gpu_units.py: a fresh process that creates ONE handle and at once makes one smallest call
of every family of the library, in the given order -- so that each translation unit of libmsweep_core.so (a code
object of its own) is entered first by a different call from process to process.
usage: _unit_calls_worker.py forward|reverse OUT.pickle [--time]     (--time: wall ms of the handle's creation and of
every call go into the pickle under "ms")"""
import gzip
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msweep_amd.core import ALGO_EM, PREC_FLOAT, TEXT_PROBS, Core  # noqa: E402
from msweep_amd.likelihood import from_dense, from_grouped_counts  # noqa: E402

G, E = 4, 64
GROUP_SIZES = np.array([10, 7, 12, 5], np.uint64)


def csr_problem():
    """64 ECs over 4 groups: EC j hits group j % 4 and, two times in three, a second group; counts within the sizes."""
    rowptr, grp, cnt = [0], [], []
    for j in range(E):
        g0 = j % G
        cells = {g0: 1 + (j * 7) % int(GROUP_SIZES[g0])}
        if j % 3:
            g1 = (g0 + 1 + j % 2) % G
            cells[g1] = 1 + (j * 5) % int(GROUP_SIZES[g1])
        for g in sorted(cells):
            grp.append(g)
            cnt.append(cells[g])
        rowptr.append(len(grp))
    ec_counts = 1 + (np.arange(E) * 13) % 9
    return np.array(rowptr, np.uint64), np.array(grp, np.uint32), np.array(cnt, np.uint32), ec_counts.astype(np.uint64)


def dense_matrix(n_groups, n_ecs, listed):
    """log(0.01) everywhere but `listed` cells per EC, every one of them a value of its own"""
    L = np.full((n_groups, n_ecs), np.log(0.01))
    j = np.arange(n_ecs)
    for k in range(listed):
        L[(j + 3 * k) % n_groups, j] = -0.1 - (j * listed + k + 1) * (11.0 / (n_ecs * listed + 1))
    return L


def solve_csr(core, env=None, check=None, **kw):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        rowptr, grp, cnt, ec_counts = csr_problem()
        lik = from_grouped_counts(core, rowptr, grp, cnt, ec_counts, GROUP_SIZES)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    li = core.layout_info()
    if check:
        assert check(li), li
    res = core.solve(lik.log_counts(), np.ones(G), **kw)
    return dict(theta=res["theta"].tobytes(), iters=res["iters"], bound=np.float64(res["bound"]).tobytes(),
                record_bytes=li["record_bytes"], index_records=li["index_records"])


def rcg_narrow(core):
    return solve_csr(core, check=lambda li: li["record_bytes"] == 4 and li["index_records"] == 0)


def rcg_wide(core):
    return solve_csr(core, {"MSWEEP_RECORD_BYTES": "8"}, check=lambda li: li["record_bytes"] == 8)


def rcg_index(core):
    return solve_csr(core, {"MSWEEP_FORCE_LDS": "10"}, check=lambda li: li["record_bytes"] == 4 and li["index_records"] == 1)


def rcg_value(core):
    """value records have no forcing switch: the smallest dense matrix whose listed cells exceed the 2^16 values that
    still share slots (host_compress.inc)"""
    n_ecs = 34000
    L = dense_matrix(16, n_ecs, 2)
    from_dense(core, L, np.zeros(n_ecs))
    li = core.layout_info()
    assert li["record_bytes"] == 12, li
    res = core.solve(np.zeros(n_ecs), np.ones(16), max_iters=30)
    return dict(theta=res["theta"].tobytes(), iters=res["iters"])


def dense(core):
    os.environ["MSWEEP_DENSE_COMPRESS"] = "0"
    try:
        from_dense(core, dense_matrix(G, E, 1), np.zeros(E))
    finally:
        del os.environ["MSWEEP_DENSE_COMPRESS"]
    res = core.solve(np.zeros(E), np.ones(G))
    return dict(theta=res["theta"].tobytes(), iters=res["iters"])


def em_float(core):
    out = solve_csr(core, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=50)
    out["float_kernels"] = int(core.last_timing()["em_float_kernels"])
    assert out["float_kernels"] == 1, out
    return out


def alignment(core, tmp):
    path = os.path.join(tmp, "aln.txt")
    with open(path, "w") as f:
        f.write("0 1 2\n1 3\n2 1 2\n3\n4 0 7\n5 3\n6 1 2\n7 5 6 7\n8 0 7\n9 4\n")
    aln = core.read_alignment([path], 8)
    assert aln.on_device
    return {k: np.asarray(v).tobytes() for k, v in sorted(aln.arrays().items()) if isinstance(v, np.ndarray)}


def text_block(core):
    rcg_narrow(core)
    return dict(text=core.text_block(TEXT_PROBS, 0, E))


def gzip_stream(core):
    out = core.gzip_begin(6) + core.gzip_append(b"abc\nabc\n") + core.gzip_end()
    assert gzip.decompress(out) == b"abc\nabc\n"
    return dict(gz=out)


def fastq(core, tmp):
    path = os.path.join(tmp, "r.fq")
    recs = [b"@r%d\nACGT%s\n+\nIIII%s\n" % (i, b"A" * i, b"I" * i) for i in range(4)]
    with open(path, "wb") as f:
        f.write(b"".join(recs))
    with core.fastq_open(path) as fq:
        n, nb = fq.select([2, 0])
        plain = b"".join(fq.pieces())
        assert (n, nb) == (2, len(recs[0]) + len(recs[2])) and plain == recs[0] + recs[2]
        gz = core.gzip_begin(6)
        fq.select([1, 3])
        gz += b"".join(fq.pieces_gzip()) + core.gzip_end()
        assert gzip.decompress(gz) == recs[1] + recs[3]
    return dict(plain=plain, gz=gz)


def bin_reads(core):
    rcg_narrow(core)
    bin_ptr, reads, log_thr = core.bin_reads(np.arange(E + 1, dtype=np.uint64), np.arange(E, dtype=np.uint32), [0, 1, 3],
                                             [0.5, 0.3, 0.9])
    return dict(bin_ptr=bin_ptr.tobytes(), reads=reads.tobytes(), log_thr=log_thr.tobytes())


def main():
    order, out_path = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        calls = [("rcg_narrow", rcg_narrow), ("rcg_wide", rcg_wide), ("rcg_index", rcg_index), ("rcg_value", rcg_value),
                 ("dense", dense), ("em_float", em_float), ("alignment", lambda c: alignment(c, tmp)),
                 ("text_block", text_block), ("gzip", gzip_stream), ("fastq", lambda c: fastq(c, tmp)),
                 ("bin_reads", bin_reads)]
        if order == "reverse":
            calls.reverse()
        out, ms = {}, {}
        t0 = time.perf_counter()
        with Core(0) as core:
            ms["create"] = (time.perf_counter() - t0) * 1e3
            for name, fn in calls:
                t0 = time.perf_counter()
                out[name] = fn(core)
                ms[name] = (time.perf_counter() - t0) * 1e3
    if "--time" in sys.argv:
        out["ms"] = ms
    with open(out_path, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    main()
