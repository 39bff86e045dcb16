"""CPU, no compiler run: the staleness logic and the job count of msweep_amd/buildlib.py on a temporary directory of
fake sources, depfiles and stored hashes.  An object is stale when the hash over its flags and the contents of the files
its depfile names differs from the hash stored beside it -- content, never mtime."""
import os

import pytest

from msweep_amd import buildlib

FLAGS = ["-O3", "-std=c++17"]
# unit -> the files its depfile names (a.hip includes one.inc and common.hpp; b.hip two.inc, common.hpp and only.hpp)
DEPS = {"a": ["a.hip", "one.inc", "common.hpp"], "b": ["b.hip", "two.inc", "common.hpp", "only.hpp"],
        "c": ["c.hip", "dir with space/three.inc"]}


@pytest.fixture()
def tree(tmp_path):
    src, bld = tmp_path / "src", tmp_path / "build"
    (src / "dir with space").mkdir(parents=True)
    bld.mkdir()
    for names in DEPS.values():
        for n in names:
            (src / n).write_text("// " + n + "\n")
    for u, names in DEPS.items():       # what a compile leaves: the object, its depfile (make syntax), the stored hash
        obj = str(bld / (u + ".o"))
        open(obj, "wb").write(b"\x7fELF")
        esc = [n.replace(" ", "\\ ") for n in names]
        open(obj + ".d", "w").write(f"{u}.o: {esc[0]} \\\n  " + " \\\n  ".join(esc[1:]) + "\n")
        buildlib.record(obj, FLAGS, cwd=str(src))
    return src, bld


def stale(tree, flags=FLAGS):
    src, bld = tree
    return sorted(u for u in DEPS if buildlib.is_stale(str(bld / (u + ".o")), flags, cwd=str(src)))


def test_nothing_is_stale_after_a_build(tree):
    assert stale(tree) == []
    src, _ = tree
    os.utime(src / "common.hpp", (1, 1))        # mtime is no evidence
    os.utime(src / "one.inc", (2_000_000_000, 2_000_000_000))
    assert stale(tree) == []


def test_an_inc_edit_marks_exactly_its_unit(tree):
    src, _ = tree
    (src / "one.inc").write_text("// one.inc, edited\n")
    assert stale(tree) == ["a"]
    (src / "dir with space" / "three.inc").write_text("// edited\n")
    assert stale(tree) == ["a", "c"]


def test_a_header_edit_marks_exactly_the_units_that_name_it(tree):
    src, _ = tree
    (src / "only.hpp").write_text("// edited\n")
    assert stale(tree) == ["b"]
    (src / "common.hpp").write_text("// edited\n")
    assert stale(tree) == ["a", "b"]


def test_a_changed_flag_marks_all_units(tree):
    assert stale(tree, FLAGS + ["-DMSW_FX=0"]) == ["a", "b", "c"]
    assert stale(tree, list(reversed(FLAGS))) == ["a", "b", "c"]


def test_a_missing_depfile_object_or_hash_marks_its_unit(tree):
    _, bld = tree
    os.remove(bld / "b.o.d")
    assert stale(tree) == ["b"]
    os.remove(bld / "a.o.hash")
    assert stale(tree) == ["a", "b"]
    os.remove(bld / "c.o")
    assert stale(tree) == ["a", "b", "c"]


def test_a_deleted_source_marks_its_unit(tree):
    src, _ = tree
    os.remove(src / "two.inc")
    assert stale(tree) == ["b"]


def test_the_source_hash_goes_to_the_abi_unit_only():
    for u in buildlib.UNITS:
        has = any(f.startswith("-DMSW_SRC_HASH=") for f in buildlib.unit_flags(u, ["-DX=1"], "0123456789abcdef"))
        assert has == (u == buildlib.ABI_UNIT)
        assert os.path.exists(os.path.join(buildlib.CSRC, u + ".hip"))
    assert len(set(buildlib.UNITS)) == len(buildlib.UNITS)


def test_job_count_is_capped(monkeypatch):
    monkeypatch.setenv("MAX_JOBS", "64")
    monkeypatch.setattr(buildlib, "cpu_share", lambda: 256)
    monkeypatch.setattr(os, "cpu_count", lambda: 1024)
    assert buildlib.job_count(100) == 16
    assert buildlib.job_count(100, jobs=64) == 16
    assert buildlib.job_count(5) == 5               # no more jobs than units
    assert buildlib.job_count(100, jobs=8) == 8
    monkeypatch.setenv("MAX_JOBS", "4")
    assert buildlib.job_count(100) == 4
    monkeypatch.delenv("MAX_JOBS")
    monkeypatch.setattr(buildlib, "cpu_share", lambda: 3)
    assert buildlib.job_count(100) == 3
