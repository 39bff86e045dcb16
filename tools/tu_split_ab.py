#!/usr/bin/env python3
"""Developer A/B tool: what a fresh process pays for the library's code objects, this build against another one (the
parent commit's, built apart and given as --parent-lib; it is loaded through MSWEEP_CORE_LIB).  Each repeat starts one
fresh process per side, the sides alternated, and each process creates a handle and at once makes one smallest call of
every family (tests/_unit_calls_worker.py --time).  Printed: median and (min - max) of msw_core_create, of every
family's first call and of their sum, per side; and whether the two sides' outputs are equal byte for byte.
A family whose first call stands out on this side has a translation unit that msw_core_create does not warm.
usage: tu_split_ab.py --parent-lib PATH [--repeats 5]"""
import argparse
import os
import pickle
import statistics
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(R, "tests", "_unit_calls_worker.py")


def one(lib, tmp):
    env = dict(os.environ)
    env.pop("MSWEEP_CORE_LIB", None)
    if lib:
        env["MSWEEP_CORE_LIB"] = lib
    path = os.path.join(tmp, "out.pickle")
    subprocess.run([sys.executable, WORKER, "forward", path, "--time"], check=True, env=env, cwd=R, timeout=300)
    with open(path, "rb") as f:
        out = pickle.load(f)
    ms = out.pop("ms")
    ms["sum"] = sum(ms.values())
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sides = {"parent": os.path.abspath(a.parent_lib), "this": None}
    ms = {s: [] for s in sides}
    outs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.repeats):
            for s in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
                t, out = one(sides[s], tmp)
                ms[s].append(t)
                assert outs.setdefault(s, out) == out, f"{s}: outputs differ between two runs"
    print(f"{a.repeats} fresh processes per side, alternated; wall ms: median (min - max)")
    print(f"{'':12s} {'parent':>28s} {'this':>28s}")
    for k in ms["this"][0]:
        cells = []
        for s in sides:
            v = [t[k] for t in ms[s]]
            cells.append(f"{statistics.median(v):9.2f} ({min(v):8.2f} - {max(v):8.2f})")
        print(f"{k:12s} {cells[0]:>28s} {cells[1]:>28s}")
    print("outputs of the two sides equal byte for byte:", outs["parent"] == outs["this"])


if __name__ == "__main__":
    main()
