"""Shared by tests/test_alignment_subset_cpu.py and tests/test_gpu_alignment_subset.py: generated alignments in which
every case msw_alignment_subset has to get right is CONSTRUCTED (and asserted to be there), the restricted text of the
contract (include/msweep_core.h), and the comparison of a subset against the existing readers on that text:
  - the pure-Python mirror (msweep_amd/alignment.py), always, on the text as the contract words it: one line per
    selected id;
  - msw_alignment_read on the host.  That reader leaves out read ids at or beyond the text's line count (its guard
    against malformed text), which the mirror and the subset do not.  So it reads the same text where every selected
    id is below the number of selected ids, and otherwise the text PADDED with a bare line for every id that is not
    selected, up to the largest selected one: bare lines add no read to any class, the five arrays must be equal
    and only n_reads counts the padding."""
import io
import os

import numpy as np

from msweep_amd import core
from msweep_amd.alignment import Alignment, ec_hash

N_TARGETS = 40
N_LINES = 300
DROPPED = (0, 12, 30, 31, 32, 33, 34)
X, Y, Z, P, Q = (2, 7), (2, 7, 30), (30, 31), (1, 4, 9), (5, 6)


def keep_default(n_targets=N_TARGETS, dropped=DROPPED):
    k = np.ones(n_targets, np.uint8)
    k[list(dropped)] = 0
    return k


def source_rows():
    """{read id: target tuple} of a 300-line file; the constructed classes override the generated ones"""
    rng = np.random.default_rng(20240611)
    pool = [tuple(sorted(rng.choice(N_TARGETS, size=int(rng.integers(1, 7)), replace=False).tolist())) for _ in range(25)]
    rows = {}
    for i in range(N_LINES):
        rows[i] = () if rng.random() < 0.1 else pool[int(rng.integers(len(pool)))]
    # X and Y differ only in a dropped target: the class that stands LATER in the source gets the smallest read id
    later, earlier = (X, Y) if ec_hash(X) > ec_hash(Y) else (Y, X)
    for i in (3, 12):
        rows[i] = later
    for i in (10, 11):
        rows[i] = earlier
    for i in (20, 21):
        rows[i] = Z           # loses every target
    for i in (40, 41, 42, 43):
        rows[i] = P           # selected in part
    for i in (31, 32, 63, 64):
        rows[i] = Q           # the words of the selection bitmap end between them
    for i in (70, 71):
        rows[i] = ()          # in no class
    return rows


def write_rows(path, rows, n_lines):
    with open(path, "w") as f:
        for i in range(n_lines):
            f.write(" ".join([str(i)] + [str(t) for t in rows.get(i, ())]) + "\n")


def copy_arrays(aln):
    """the five arrays and n_reads of an alignment handle, as arrays of their own"""
    a = aln.arrays()
    return {k: (np.array(v) if k != "n_reads" else int(v)) for k, v in a.items()}


def class_of_read(arr):
    rp = arr["ec_rptr"].astype(np.int64)
    out = {}
    for e in range(len(rp) - 1):
        for r in arr["ec_reads"][rp[e]:rp[e + 1]].tolist():
            out[r] = e
    return out


def class_targets(arr, e):
    tp = arr["ec_tptr"].astype(np.int64)
    return tuple(arr["ec_targets"][tp[e]:tp[e + 1]].tolist())


def restricted_text(arr, ids, keep, pad=False):
    """the text of the contract: one line per selected id with the kept targets of its class, renumbered by rank"""
    keep = np.asarray(keep) != 0
    rank = np.cumsum(keep) - keep
    cls = class_of_read(arr)
    lines = []
    for i in ids:
        i = int(i)
        tg = class_targets(arr, cls[i]) if i in cls else ()
        lines.append(" ".join([str(i)] + [str(int(rank[t])) for t in tg if keep[t]]))
    if pad and len(ids):
        sel = set(int(i) for i in ids)
        lines += [str(i) for i in range(max(sel) + 1) if i not in sel]
    return "".join(ln + "\n" for ln in lines), int(keep.sum())


def mirror_arrays(text, n_keep):
    m = Alignment(n_keep)
    m.read("intersection", [io.StringIO(text)])
    m.collapse()
    reads = [r for v in m.ec_read_ids for r in v]
    rptr = np.concatenate([[0], np.cumsum([len(v) for v in m.ec_read_ids])]).astype(np.uint64)
    return dict(ec_tptr=np.asarray(m.ec_tptr, np.uint64), ec_targets=np.asarray(m.ec_targets, np.uint32),
                ec_counts=np.asarray(m.ec_counts, np.uint64), ec_rptr=rptr, ec_reads=np.asarray(reads, np.uint32),
                n_reads=m.n_queries)


ARRAYS = ("ec_tptr", "ec_targets", "ec_counts", "ec_rptr", "ec_reads")


def assert_same(got, want, what, n_reads=True):
    for k in ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k, g[:20], w[:20])
    if n_reads:
        assert got["n_reads"] == want["n_reads"], (what, got["n_reads"], want["n_reads"])


def check_against_readers(got, src, ids, keep, tmp_path, what):
    """`got`: the arrays of subset(src, ids, keep); src: the source's arrays"""
    ids = [int(i) for i in ids]
    text, n_keep = restricted_text(src, ids, keep)
    assert got["n_reads"] == len(ids), what
    assert_same(got, mirror_arrays(text, n_keep), what + ": python mirror")
    exact = not ids or max(ids) < len(ids)
    if not exact:
        text, _ = restricted_text(src, ids, keep, pad=True)
    p = os.path.join(str(tmp_path), "restricted.txt")
    with open(p, "w") as f:
        f.write(text)
    assert_same(got, core.read_alignment([p], n_keep, copy=True), what + ": msw_alignment_read", n_reads=exact)


def selections():
    """(name, read ids, keep) -- the ids in an order of their own: the outcome does not depend on it"""
    kd = keep_default()
    every = list(range(N_LINES))
    base = [3, 10, 11, 12, 20, 21, 41, 43, 70, 71, 5, 6, 7, 8, 100, 150, 151, 152, 200, 250, 299]
    return [
        ("constructed", base + [31, 64, 1000, 5000], kd),                 # 31 | 32 and 63 | 64: the left one of each pair ..
        ("constructed, other side", [32, 63] + base[::-1] + [400], kd),   # .. and the right one
        ("all four boundary ids", [64, 63, 32, 31, 3, 10], kd),
        ("a prefix of the ids", list(range(120)), kd),                    # (every id below the line count)
        ("every read, some targets", every, kd),
        ("some reads, every target", base, np.ones(N_TARGETS, np.uint8)),
        ("no read keeps a target", [20, 21, 70, 1000], kd),
        ("one target kept", every[::3], (np.arange(N_TARGETS) == 5).astype(np.uint8)),
    ]


def assert_constructed(src):
    """the constructed cases are in the source alignment, and the first selection meets each of them"""
    cls = class_of_read(src)
    name, ids, keep = selections()[0]
    sel = set(ids)
    # two classes that differ only in dropped targets; the smallest read id lies in the one that stands later
    assert class_targets(src, cls[3]) in (X, Y) and class_targets(src, cls[10]) in (X, Y) and cls[3] != cls[10]
    assert cls[3] > cls[10] and cls[12] == cls[3] and cls[11] == cls[10]
    assert {3, 10, 11, 12} <= sel and not keep[30] and keep[2] and keep[7]
    # a class of which only some reads are selected
    members = [r for r, e in cls.items() if e == cls[41]]
    assert class_targets(src, cls[41]) == P and set(members) & sel and set(members) - sel
    # a class that loses every target
    assert class_targets(src, cls[20]) == Z and not any(keep[t] for t in Z) and {20, 21} <= sel
    # selected ids in no class, and beyond the largest id of the source
    assert 70 not in cls and 71 not in cls and {70, 71} <= sel
    assert max(cls) < 1000 and src["n_reads"] == N_LINES and {1000, 5000} <= sel
    # ids 31, 32, 63, 64 share a class; the selections cut between them on both sides
    assert len({cls[i] for i in (31, 32, 63, 64)}) == 1 and all(keep[t] for t in Q)
    other = set(selections()[1][1])
    assert {31, 64} <= sel and not {32, 63} & sel and {32, 63} <= other and not {31, 64} & other
