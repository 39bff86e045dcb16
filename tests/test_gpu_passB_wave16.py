"""GPU: pass B's 16-row kernel (RC = 16) at SIXTEEN wavefronts per workgroup -- offset records with the group vectors,
the column sums and the slot table in LDS (sweep_kernels.hpp pass_threads_B_of) -- in lock-step with the CSR oracle.

Every case first asserts through layout_info that pass B IS that kernel at 16 wavefronts (on_path): a case that is not on
the path fails.  Problems whose slices have at most 8 rows get the short-slice instantiation by default; MSWEEP_PASSB_RC=16
(read at set_csr) gives them the 16-row one, as in test_gpu_ec_length_boundaries.py part B.  Then the solve is held for
the conditioned iterations at rel 1e-9, theta summing to 1 within 1e-12 (run_lockstep: the tolerances of
test_gpu_ec_length_boundaries.py).

  uniform   ECs of exactly 1, 2, 7, 8, 9, 15, 16 cells (both sides of the 8-row half of the record buffers, odd lengths
            whose last row is the null record) x 3 ECs (most wavefronts own no slice), 64 (one full slice), 65 (a second
            slice of one EC) and 300 000 (4688 slices over the 4096 wavefronts of 256 workgroups: some wavefronts walk two
            slices -- both buffers of the ping-pong; a 64-slice geometry refill needs 16.7 M ECs and is not reached by any
            test of a few seconds).
  mixture   lengths 1..16 shuffled (a wavefront's slices go from 8 to 9 rows), ECs of 17..64 cells (the multi-lane
            instantiation) and a few above 1024 cells (a wavefront per EC behind the slices).
  counts    0; 1..3; 4..15; 16..254; 255, fractional and larger (the escape byte); one EC with a quarter of all reads
            (an EC with more than about 2^-10 of the reads fails the narrow-add test fxt1 = 2^51 / 2^K ~ sum c / 1024 and
            takes the two-part add, so here the counts from about 80 on do, the smaller ones do not).
  guarded   tests/golden/fuzz/seed2_case1348 (guarded ECs, counts in the tens of thousands) on this kernel.
  flush     more than 32 deferred logarithms per wavefront on the wavefront-per-EC path, with 16 wavefronts.
  determinism  two solves of the mixture return the same bits."""
import os

import numpy as np
import pytest

import ec_length_cases as ec
from conftest import ROOT
from test_gpu_group_boundaries import compute_units, conditioned_iters, run_lockstep

pytestmark = pytest.mark.gpu

ITERS = 8
G = 300
LENGTHS = (1, 2, 7, 8, 9, 15, 16)
N_ECS = (3, 64, 65, 300_000)


@pytest.fixture(autouse=True)
def rc16(monkeypatch):
    for name in ("MSWEEP_RECORD_BYTES", "MSWEEP_FORCE_LDS", "MSWEEP_HYBRID_HOT", "MSWEEP_MULTILANE", "MSWEEP_HOST_PACK",
                 "MSWEEP_LONG_ROW"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MSWEEP_PASSB_RC", "16")


def on_path(core, multilane=None):
    li = core.layout_info()
    assert li["record_bytes"] == 4 and li["index_records"] == 0, li
    assert li["groups_in_lds"] == 1 and li["table_in_lds"] == 1 and li["passB_mode"] in (1, 2), li
    assert li["passB_reg_cells"] == 16 and li["passB_waves"] == 16, li
    if multilane is not None:
        assert (sum(li["slices_by_lanes"][:-1]) > 0) == multilane, li
    return li


def strided_groups(rng, lens, n_groups):
    """distinct groups per EC without an n_ecs x G table of random numbers: start + k * stride mod G, stride coprime to G"""
    lens = np.asarray(lens, np.int64)
    assert lens.max() <= n_groups
    coprime = np.array([s for s in range(1, n_groups) if np.gcd(s, n_groups) == 1])
    start = rng.integers(0, n_groups, len(lens))
    stride = coprime[rng.integers(0, len(coprime), len(lens))]
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    j = np.repeat(np.arange(len(lens)), lens)
    k = np.arange(rowptr[-1]) - rowptr[j]
    return rowptr, (start[j] + k * stride[j]) % n_groups


def make_case(seed, lens, counts=None, n_groups=G):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    sizes = (1 + rng.poisson(4, n_groups)).astype(np.uint64)
    rowptr, grp = strided_groups(rng, lens, n_groups)
    cnt = rng.integers(1, sizes[grp].astype(np.int64) + 1)
    if counts is None:
        counts, logc = ec.multiplicities(rng, len(lens))
    with np.errstate(divide="ignore"):
        logc = np.log(np.asarray(counts, np.float64))
    return ec._csr_case(rng, n_groups, sizes, rowptr, grp, cnt, np.asarray(counts, np.float64), logc)


def held(core, oracle, c, min_iters):
    trace = ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"]
    # (a toy problem driven on with tol -1 can diverge in the oracle itself: the seeds are chosen so that none does)
    assert np.isfinite(trace["bound"]).all() and np.isfinite(trace["theta"]).all(), "the oracle's own solve is not finite"
    k = run_lockstep(core, c["logc"], c["alpha0"], trace, ITERS, rel=1e-9)
    print(f"E = {c['E']}: {k} iterations in lock-step; rejected steps {trace['didreset'].tolist()}")
    assert k == conditioned_iters(trace, ITERS) >= min_iters, f"{k} iterations in lock-step"
    return k


@pytest.mark.parametrize("n_ecs", N_ECS)
@pytest.mark.parametrize("L", LENGTHS)
def test_uniform_lengths(gpu_core, oracle, L, n_ecs):
    c = make_case(2003 * L + n_ecs, [L] * n_ecs)
    ec.set_csr(gpu_core, c)
    li = on_path(gpu_core, multilane=False)
    assert li["max_rows"] == L and li["n_slices"] == -(-n_ecs // 64) and li["n_long_ecs"] == 0, li
    held(gpu_core, oracle, c, ec.min_held(n_ecs, 64))


@pytest.fixture(scope="module")
def mixture():
    rng = np.random.default_rng(77)
    lens = np.concatenate([rng.integers(1, 17, 6000), rng.integers(17, 65, 300), [1025, 1100, 1500]])
    rng.shuffle(lens)
    return make_case(78, lens, n_groups=1600)


def test_mixture_of_lengths(gpu_core, oracle, mixture):
    ec.set_csr(gpu_core, mixture)
    li = on_path(gpu_core, multilane=True)
    assert li["max_rows"] == 16 and li["n_long_ecs"] == 3 and li["slices_by_lanes"][-1] >= 90, li
    held(gpu_core, oracle, mixture, 4)


def test_mixture_is_deterministic(gpu_core, mixture):
    ec.set_csr(gpu_core, mixture)
    on_path(gpu_core, multilane=True)
    a = gpu_core.solve(mixture["logc"], mixture["alpha0"], tol=-1.0, max_iters=ITERS)
    b = gpu_core.solve(mixture["logc"], mixture["alpha0"], tol=-1.0, max_iters=ITERS)
    assert a["iters"] == b["iters"] == ITERS and a["bound"] == b["bound"]
    np.testing.assert_array_equal(a["theta"], b["theta"])


def test_multiplicities(gpu_core, oracle):
    rng = np.random.default_rng(5)
    n = 2000
    lens = rng.integers(1, 17, n)
    counts = np.concatenate([np.zeros(200), rng.integers(1, 4, 800), rng.integers(4, 16, 600), rng.integers(16, 255, 380),
                             [255.0, 256.0, 1000.0, 2.5, 0.5, 300.25], np.full(13, 255.0), [20000.0]])
    assert len(counts) == n
    rng.shuffle(counts)
    c = make_case(6, lens, counts)
    # the narrow-add test of an EC (k_passB): c < sum c / 1024, roughly -- both sides among the counts of 16..254
    thr = counts.sum() / 1024
    assert 16 < thr < 254 and np.sum((counts >= 16) & (counts < thr / 2)) > 20 and np.sum((counts > 2 * thr) & (counts < 255)) > 20
    ec.set_csr(gpu_core, c)
    on_path(gpu_core, multilane=False)
    held(gpu_core, oracle, c, 4)


def test_guarded_ecs(gpu_core, oracle):
    d = np.load(os.path.join(ROOT, "tests", "golden", "fuzz", "seed2_case1348.npz"))
    n_groups, n = len(d["alpha0"]), 5
    gpu_core.set_csr(d["rowptr"], d["grp"], d["cnt"], d["lut"], ec.LOGZI, n_groups)
    on_path(gpu_core, multilane=False)
    lutidx = (d["grp"] * d["lut"].shape[1] + d["cnt"]).astype(np.uint32)
    ref = oracle.rcg_optl_csr(d["rowptr"], d["grp"], lutidx, d["lut"], ec.LOGZI, n_groups, d["logc"], d["alpha0"], tol=-1.0,
                              max_iters=n, trace=n)["trace"]
    k = run_lockstep(gpu_core, d["logc"], d["alpha0"], ref, n, rel=1e-9)
    assert k == conditioned_iters(ref, n)
    assert gpu_core.guarded_visits() > 0, "no EC went through the deferral queue"


def test_long_path_flush_at_16_wavefronts(gpu_core, oracle, monkeypatch):
    """test_long_path_flushes_deferred_logarithms with this kernel's wavefront count: 33 or 34 deferred logarithms per
    wavefront"""
    monkeypatch.setenv("MSWEEP_LONG_ROW", "16")
    nw = compute_units() * 16
    n_long = 33 * nw + 5
    assert n_long * 17 < 3_000_000
    c = make_case(11, [17] * n_long, np.random.default_rng(12).integers(1, 16, n_long).astype(np.float64), n_groups=200)
    ec.set_csr(gpu_core, c)
    li = on_path(gpu_core)
    assert li["n_long_ecs"] == n_long and li["n_slices"] == 0, li
    held(gpu_core, oracle, c, 4)
