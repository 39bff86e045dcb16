"""GPU: libmsweep_core.so is built from several translation units, each a code object of its own.  Two
fresh processes each create a handle and at once make one smallest call of every family -- an RCG solve per record
encoding, a dense solve, an --emprecision float EM solve, the device reader, a text block, a gzip stream, the FASTQ
calls, the bin pass -- the second in the reverse order.  Every call must succeed and the two processes' outputs must be
equal byte for byte: a kernel registered in no code object fails its launch, a launch through another unit's stub or
state that the cut turned into one copy per unit shows as a failure or as a difference between the two orders."""
import os
import pickle
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FAMILIES = ["rcg_narrow", "rcg_wide", "rcg_index", "rcg_value", "dense", "em_float", "alignment", "text_block", "gzip",
            "fastq", "bin_reads"]


def test_every_family_from_a_fresh_process_in_either_order(tmp_path):
    outs = []
    for order in ("forward", "reverse"):        # one after the other: each a fresh child process with the GPU to itself
        path = tmp_path / (order + ".pickle")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_unit_calls_worker.py"), order, str(path)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, f"{order}: {p.stdout[-2000:]}{p.stderr[-4000:]}"
        with open(path, "rb") as f:
            outs.append(pickle.load(f))
    fwd, rev = outs
    assert sorted(fwd) == sorted(FAMILIES) == sorted(rev)
    for name in FAMILIES:
        assert fwd[name] == rev[name], name
    import numpy as np
    for name in ("rcg_narrow", "rcg_wide", "rcg_index", "rcg_value", "dense", "em_float"):
        theta = np.frombuffer(fwd[name]["theta"])
        # (the float EM leaves every weight rounded to fp32: up to 2^-24 of a weight below 1 each)
        assert abs(theta.sum() - 1.0) < (len(theta) * 2.0 ** -24 if name == "em_float" else 1e-9), name
