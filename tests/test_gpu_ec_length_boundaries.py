"""GPU: the solve at every number of cells of an equivalence class at which the SELL layout, the packers or the sweeps
change strategy (tests/ec_length_cases.py lists them), against the CPU oracle in lock-step.  Every case is a problem
whose ECs all have exactly that length, so an error on the path of a length touches every EC of the problem.

  A  default build (narrow records, tables in LDS), both sides of every boundary from 1 to 2049 cells; the host packer
     builds the same layout bit for bit.
  B  pass B's two instantiations (RC = 8: 16 wavefronts, longer slices stream in chunks of 8 rows; RC = 16) on 1..16 cells.
  C  the other record encodings: wide, index records (hybrid slot area; cold segments of exactly 0, 1, 2 and 3 cells per
     EC), value records.
  D  MSWEEP_MULTILANE=0: one lane per EC, streaming slices of up to 256 rows, the wavefront-per-EC path beyond.
  E  EM, double and --emprecision float, on the layouts of A and of C's index records.
  F  a mixture with empty ECs that has every class boundary inside one permutation; more than 32 deferred logarithms per
     wavefront on the wavefront-per-EC path (flush_logs).

What each case checks: (1) through layout_info that it is on the path it names -- a case whose precondition fails tests
nothing and says so; (2) get_dense_logl bit-equal to the matrix of the input (the decoder for_each_cell on that layout);
(3) 8 iterations of RCG with tol -1 in lock-step with the oracle (run_lockstep: rel 1e-9, part A's tolerance of
test_gpu_group_boundaries.py; value records: test_value_records_lockstep's, also 1e-9, against the structured dense
oracle), the returned theta through assert_theta and summing to 1 within 1e-12; (4) exp(gamma) at atol 1e-7
(test_mid_length_ecs_slice_classes_and_streaming_path's) in parts A and C, where the lock-step ends (see
test_dense_instantiation_edge: afterwards a step rejected by rounding, by one side only, moves gamma).

Iterations held in lock-step (conditioned_iters; printed per case): at least 4 whenever a problem has more ECs than a slice
of its class holds -- except the problems of TWO ECs (the classes of one EC per slice, from 513 cells on), which the stop
rule at --tol 1e-6 ends after 3: the oracle's bound gains 4e-4, 7e-8, 0 there (1025 cells), and at 1536, 1537, 2048 and
2049 cells no seed of 1500 gives a fourth iteration.  Those are held for 3.  Problems of a single EC converge at once;
their first iterations are still compared."""
import numpy as np
import pytest

import ec_length_cases as ec
from msweep_amd.core import ALGO_EM, PREC_FLOAT
from msweep_amd.likelihood import from_dense
from test_gpu_group_boundaries import compute_units, conditioned_iters, rel_above, run_lockstep

pytestmark = pytest.mark.gpu

ITERS, ITERS_EM = 8, 25
SWITCHES = ("MSWEEP_PASSB_RC", "MSWEEP_RECORD_BYTES", "MSWEEP_FORCE_LDS", "MSWEEP_HYBRID_HOT", "MSWEEP_MULTILANE",
            "MSWEEP_HOST_PACK", "MSWEEP_LONG_ROW")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    """every case starts from the default build: the developer switches are read at set_csr"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def uniform_refs(oracle):
    """case, 8-iteration oracle trace and the iterations it allows, per (L, n_ecs): computed once, shared by the parts"""
    made = {}

    def get(L, n_ecs):
        if (L, n_ecs) not in made:
            c = ec.uniform_case(L, n_ecs)
            tr = ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"]
            made[L, n_ecs] = (c, tr, conditioned_iters(tr, ITERS))
        return made[L, n_ecs]
    return get


def check_layout(core, want):
    li = core.layout_info()
    for key, v in want.items():
        assert li[key] == v, f"{key} = {li[key]}, expected {v}: {li}"
    return li


def uniform_layout(c, multilane=True, **more):
    """what layout_info has to say of a uniform case; defaults: narrow records, every table entry from LDS"""
    L, n = c["L"], c["E"]
    geo = ec.expected_layout([L] * n, multilane)
    lone = ec.lanes(L, multilane)
    assert geo["n_long_ecs"] in (0, n) and sum(1 for s in geo["slices_by_lanes"] if s) == (0 if geo["n_long_ecs"] else 1)
    assert geo["max_rows"] == (0 if geo["n_long_ecs"] else -(-L // lone))
    # pass B's short-slice instantiation: narrow records, one lane per EC, the slices of more than 8 rows at most a
    # twentieth of the rows (finish_sell) -- all or none of them here
    rc = 8 if geo["n_slices"] and geo["max_rows"] <= 8 else 16
    want = dict(geo, record_bytes=4, index_records=0, rows_from_memory=0, passB_reg_cells=rc, table_in_lds=1, groups_in_lds=1)
    want.update(more)
    return want


def lockstep_case(core, c, trace, per, rel=1e-9):
    """checks 2 and 3"""
    np.testing.assert_array_equal(core.get_dense_logl(), ec.dense_of(c))
    k = run_lockstep(core, c["logc"], c["alpha0"], trace, ITERS, rel=rel)
    print(f"E = {c['E']}: {k} iterations in lock-step; rejected steps {trace['didreset'].tolist()}")
    assert k == conditioned_iters(trace, ITERS) >= ec.min_held(c["E"], per), f"{k} iterations in lock-step"
    return k


def gamma_case(core, oracle, c, k):
    """check 4, after the k iterations the lock-step holds"""
    res = core.solve(c["logc"], c["alpha0"], tol=-1.0, max_iters=k)
    assert res["iters"] == k
    ref = ec.csr_oracle(oracle, c, k, want_gamma=True)
    np.testing.assert_allclose(np.exp(core.gamma()), np.exp(ref["gamma"]), atol=1e-7)


# ---- A: the default build -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_A))
def test_default_build_at_ec_length(gpu_core, oracle, uniform_refs, monkeypatch, L, n_ecs):
    c, trace, _ = uniform_refs(L, n_ecs)
    assert np.isneginf(c["logc"]).sum() == n_ecs // 5
    want = uniform_layout(c)
    ec.set_csr(gpu_core, c)
    li = check_layout(gpu_core, want)
    h = gpu_core.layout_hash()
    k = lockstep_case(gpu_core, c, trace, ec.per_slice(L))
    gamma_case(gpu_core, oracle, c, k)
    monkeypatch.setenv("MSWEEP_HOST_PACK", "1")        # the packers' own boundaries are the same numbers
    ec.set_csr(gpu_core, c)
    assert gpu_core.layout_info() == li and gpu_core.layout_hash() == h, "the host packer builds another layout"


# ---- B: pass B's two instantiations -------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_B))
def test_passB_instantiations_at_ec_length(gpu_core, uniform_refs, monkeypatch, L, n_ecs):
    """RC = 8 on slices of 9..16 rows streams them in two chunks (8 | 9, an odd 15, a full 16); RC = 16 on slices of up to 8
    rows is the instantiation the default build does not pick for them.  Both in lock-step with the oracle and with
    each other at rtol 1e-11 (test_passB_short_slice_instantiation's)."""
    c, trace, _ = uniform_refs(L, n_ecs)
    thetas = {}
    for rc in (8, 16):
        monkeypatch.setenv("MSWEEP_PASSB_RC", str(rc))
        ec.set_csr(gpu_core, c)
        check_layout(gpu_core, uniform_layout(c, passB_reg_cells=rc))
        lockstep_case(gpu_core, c, trace, ec.per_slice(L))
        gpu_core.set_trace_theta(ITERS)
        gpu_core.solve(c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS)
        thetas[rc] = gpu_core.trace(ITERS, with_theta=True)["theta"].copy()
        gpu_core.set_trace_theta(0)
    assert thetas[8].shape == thetas[16].shape == (ITERS, c["G"])
    np.testing.assert_allclose(thetas[8], thetas[16], rtol=1e-11, atol=1e-18)


# ---- C: the other record encodings ------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_C))
def test_wide_records_at_ec_length(gpu_core, oracle, uniform_refs, monkeypatch, L, n_ecs):
    monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    c, trace, _ = uniform_refs(L, n_ecs)
    ec.set_csr(gpu_core, c)
    check_layout(gpu_core, uniform_layout(c, record_bytes=8, passB_reg_cells=16))
    k = lockstep_case(gpu_core, c, trace, ec.per_slice(L))
    gamma_case(gpu_core, oracle, c, k)


def index_records(monkeypatch):
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", str(ec.HYBRID_HOT))


@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_C))
def test_index_records_at_ec_length(gpu_core, oracle, uniform_refs, monkeypatch, L, n_ecs):
    """The 16 most used (group size, count) pairs in LDS: slices with hot and cold segments and slices taken from memory
    as a whole, as the frequencies have it (ec_length_cases.index_rows_from_memory restates the packer's rule)."""
    index_records(monkeypatch)
    c, trace, _ = uniform_refs(L, n_ecs)
    ec.set_csr(gpu_core, c)
    li = check_layout(gpu_core, uniform_layout(c, index_records=1, table_in_lds=0, passB_reg_cells=16,
                                               rows_from_memory=ec.index_rows_from_memory(c)))
    assert li["slot_entries_in_lds"] == min(ec.HYBRID_HOT, li["slot_entries"] // 16 * 16), li
    k = lockstep_case(gpu_core, c, trace, ec.per_slice(L))
    gamma_case(gpu_core, oracle, c, k)


@pytest.mark.parametrize("n_ecs", [65, 323])
@pytest.mark.parametrize("L,k_cold", ec.PART_C_COLD)
def test_index_records_cold_segment(gpu_core, oracle, monkeypatch, L, k_cold, n_ecs):
    """Exactly k cold cells in every EC: no cold segment, one of one row, one of kColdRows = 2 rows, and one cell more --
    nhot = 0, the whole slice from memory.  Which entries are LDS-resident follows from the frequencies
    (ec_length_cases.cold_cells), asserted here before the layout is asked."""
    index_records(monkeypatch)
    c = ec.cold_case(L, k_cold, n_ecs)
    cold = ec.cold_cells(c).reshape(c["E"], L).sum(1)
    assert np.all(cold[:n_ecs] == k_cold) and np.all(cold[n_ecs:] == 0), cold
    ec.set_csr(gpu_core, c)
    geo = ec.expected_layout([L] * c["E"])
    li = check_layout(gpu_core, dict(geo, record_bytes=4, index_records=1, slot_entries_in_lds=ec.HYBRID_HOT, groups_in_lds=1))
    assert li["rows"] == geo["n_slices"] * L
    assert li["rows_from_memory"] == (k_cold * geo["n_slices"] if k_cold <= ec.COLD_ROWS else li["rows"]), li
    trace = ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"]
    k = lockstep_case(gpu_core, c, trace, 64)
    gamma_case(gpu_core, oracle, c, k)


@pytest.mark.parametrize("L", ec.PART_C_VALUE)
def test_value_records_at_ec_length(gpu_core, oracle, L):
    c = ec.value_case(L)
    from_dense(gpu_core, c["logl"], c["logc"])
    assert gpu_core.shape() == (c["G"], c["E"], L * c["E"])
    geo = ec.expected_layout([L] * c["E"])
    check_layout(gpu_core, dict(geo, record_bytes=12, index_records=0, rows_from_memory=0, passB_reg_cells=16, slot_entries=0))
    np.testing.assert_array_equal(gpu_core.get_dense_logl(), c["logl"])
    s = oracle.rcg_optl_dense_structured(c["logl"], c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS, trace=ITERS)
    k = run_lockstep(gpu_core, c["logc"], c["alpha0"], s["trace"], ITERS, rel=1e-9)    # (test_value_records_lockstep's)
    print(f"{c['G']} x {c['E']}: {k} iterations in lock-step; rejected steps {s['trace']['didreset'].tolist()}")
    assert k >= 4
    res = gpu_core.solve(c["logc"], c["alpha0"], tol=-1.0, max_iters=k)
    assert res["iters"] == k
    sk = oracle.rcg_optl_dense_structured(c["logl"], c["logc"], c["alpha0"], tol=-1.0, max_iters=k, want_gamma=True)
    np.testing.assert_allclose(np.exp(gpu_core.gamma()), np.exp(sk["gamma"]), atol=1e-7)


# ---- D: one lane per EC -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_D, multilane=False))
def test_one_lane_per_ec_at_ec_length(gpu_core, uniform_refs, monkeypatch, L, n_ecs):
    """Slices of 16 rows in registers; of 17..256 rows streamed in chunks of 16 (one chunk and a row, an odd 31, two chunks,
    two and a row, 255 | 256); 257 and 513 cells on the wavefront-per-EC path with one and two steps of 512."""
    monkeypatch.setenv("MSWEEP_MULTILANE", "0")
    c, trace, _ = uniform_refs(L, n_ecs)
    ec.set_csr(gpu_core, c)
    want = uniform_layout(c, multilane=False)
    assert want["max_rows"] == (L if L <= ec.LONG_ROW_ONE_LANE else 0) and want["slices_by_lanes"][:6] == [0] * 6
    check_layout(gpu_core, want)
    lockstep_case(gpu_core, c, trace, ec.per_slice(L, multilane=False))


# ---- E: EM ------------------------------------------------------------------------------------------------------------

def em_case(core, oracle, c):
    """test_em_at_group_boundary's tolerances and sum rule (the MAP weights of a prior with alpha < 1 do not sum to 1
    once groups are clamped at 0: the sum is held to the oracle's own)"""
    L, logc, alpha0 = ec.dense_of(c), c["logc"], c["alpha0"]
    d = core.solve(logc, alpha0, tol=-1.0, max_iters=ITERS_EM, algo=ALGO_EM)
    assert core.last_timing()["em_float_kernels"] == 0
    ref = oracle.em_dense(L, logc, alpha0, tol=-1.0, max_iters=ITERS_EM)
    assert d["iters"] == ITERS_EM == ref["iters"]
    np.testing.assert_allclose(d["theta"], ref["theta"], rtol=1e-6, atol=1e-9)
    assert d["theta"].sum() == pytest.approx(ref["theta"].sum(), abs=1e-12)
    core.set_trace_theta(ITERS_EM)
    f = core.solve(logc, alpha0, tol=-1.0, max_iters=ITERS_EM, algo=ALGO_EM, prec=PREC_FLOAT)
    fp32 = core.last_timing()["em_float_kernels"]
    tr = core.trace(ITERS_EM, with_theta=True)
    core.set_trace_theta(0)
    assert fp32 == 1, "the fp32 EM kernels serve this layout"
    assert f["iters"] == ITERS_EM
    o = oracle.em_dense_f32(L, logc, alpha0, tol=-1.0, max_iters=ITERS_EM, trace=ITERS_EM)
    for k in (0, 4, 19, ITERS_EM - 1):
        r, a = rel_above(tr["theta"][k], o["theta_trace"][k])
        assert r < 1e-4 and a < 1e-7, (k, r, a)
    r, a = rel_above(f["theta"], o["theta"])
    assert r < 1e-4 and a < 1e-7, (r, a)
    assert abs(f["theta"].sum() - o["theta"].sum()) < 1e-5


@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_E))
def test_em_at_ec_length(gpu_core, oracle, uniform_refs, L, n_ecs):
    c, _, _ = uniform_refs(L, n_ecs)
    ec.set_csr(gpu_core, c)
    check_layout(gpu_core, uniform_layout(c))
    em_case(gpu_core, oracle, c)


@pytest.mark.parametrize("L,n_ecs", ec.case_ids(ec.PART_E_INDEX))
def test_em_index_records_at_ec_length(gpu_core, oracle, uniform_refs, monkeypatch, L, n_ecs):
    index_records(monkeypatch)
    c, _, _ = uniform_refs(L, n_ecs)
    ec.set_csr(gpu_core, c)
    check_layout(gpu_core, uniform_layout(c, index_records=1, table_in_lds=0, passB_reg_cells=16,
                                          rows_from_memory=ec.index_rows_from_memory(c)))
    em_case(gpu_core, oracle, c)


# ---- F: two shapes a single class cannot make -----------------------------------------------------------------------

def test_mixture_with_empty_ecs(gpu_core, oracle):
    c = ec.mixture_case()
    empty = np.nonzero(c["lens"] == 0)[0]
    assert len(empty) == 2 and sorted(c["counts"][empty]) == [0.0, 3.0]
    ec.set_csr(gpu_core, c)
    geo = ec.expected_layout(c["lens"])
    assert geo["slices_by_lanes"] == [0, 0, 0, 0, 0, 2, 2] and geo["n_long_ecs"] == 3 and geo["max_rows"] == 16
    check_layout(gpu_core, dict(geo, record_bytes=4, index_records=0, rows_from_memory=0, passB_reg_cells=16, table_in_lds=1))
    trace = ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"]
    k = lockstep_case(gpu_core, c, trace, 1)
    gamma_case(gpu_core, oracle, c, k)


def test_long_path_flushes_deferred_logarithms(gpu_core, oracle, monkeypatch):
    """MSWEEP_LONG_ROW=16 puts ECs of 17 cells on the wavefront-per-EC path; with counts in 1..15 every one defers its
    logarithm, and 33 nw + 5 of them give every wavefront of pass B's launch 33 or 34: flush_logs() after the 32nd, the
    rest at the end."""
    monkeypatch.setenv("MSWEEP_LONG_ROW", "16")
    n_cu = compute_units()
    nw = ec.passB_wavefronts(0, 10**9, n_cu)
    assert nw == n_cu * ec.PASS_B_WAVES
    n_long = 33 * nw + 5
    assert n_long > 32 * nw and ec.passB_wavefronts(0, n_long, n_cu) == nw and n_long * 17 < 3_000_000
    c = ec.uniform_case(17, n_long, G=200, small_only=True)
    assert c["counts"].min() >= 1 and c["counts"].max() <= 15 and np.all(c["counts"] == np.rint(c["counts"]))
    ec.set_csr(gpu_core, c)
    check_layout(gpu_core, dict(n_long_ecs=n_long, n_slices=0, max_rows=0, slices_by_lanes=[0] * 7, record_bytes=4,
                                index_records=0, rows_from_memory=0, passB_reg_cells=16, table_in_lds=1))
    trace = ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"]
    lockstep_case(gpu_core, c, trace, 1)
