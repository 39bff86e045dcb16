"""GPU: the solve at every group count at which one of its kernels changes strategy (tests/group_boundary_cases.py lists
them), against the CPU oracle in lock-step.

  A  CSR flavour, the O(G) chain (k_finstep, k_redfin, k_init_state, k_prepB, k_em_init / k_em_fin) on both sides of
     16, 64, 512, every k * 1024 of the register paths and 6144 | 6145, where those paths give way to the looping ones
     and --emprecision float to the fp64 kernels; rejected steps on either path, the closing verdict on the looping one.
  B  CSR flavour, pass B's modes 2 -> 1 -> 3 -> 4: the switch points found from layout_info, both sides solved.
  C  dense flavour at 1..67 ECs: both sides of every edge between k_dense_pass<1..16> / k_dense_big_pass<32..128>.
  D  dense flavour with more ECs than a launch has wavefronts: what the sweeps carry from a wavefront's first EC to
     its second, in every instantiation; rejected steps of the dense flavour on both paths of k_finstep.

Every precondition of a case (a rejected step being there, the modes around a switch, E > nw, the matrix kept dense)
is an assertion: a case whose precondition fails tests nothing and says so.  Tolerances are those of the existing test
of the same quantity, named where they are applied."""
import numpy as np
import pytest

import group_boundary_cases as gb
from conftest import dense_from_csr
from msweep_amd.core import ALGO_EM, PREC_FLOAT
from msweep_amd.likelihood import from_dense
from test_gpu_rcg import assert_theta, lockstep

pytestmark = pytest.mark.gpu

ITERS_CSR, ITERS_DENSE, ITERS_EM, ITERS_EM_DENSE = 12, 8, 25, 10


def conditioned_iters(ref_trace, iters, tol=1e-6):
    """How many of `iters` iterations the lock-step can hold: those the stop rule at its default --tol 1e-6 lets the
    solve run (a gain of the bound below tol after an accepted step ends it), read off the oracle's trace.  The cases
    run on with tol -1 so that every one executes the same chain, but a converged solve moves its bound by ulps, the
    verdict `bound < oldbound` on a step is then decided by rounding, and the fp64 and the extended oracle reject
    different steps there (e.g. iterations 9..11 at 18941 groups).  test_gpu_rcg.lockstep cuts the comparison at the
    iteration count of the solve for the same reason; every other test calls it on solves that stop by --tol."""
    for i in range(1, iters):
        if ref_trace["bound"][i] - ref_trace["bound"][i - 1] < tol and ref_trace["didreset"][i] == 0:
            return i + 1
    return iters


def run_lockstep(core, logc, alpha0, ref_trace, iters, rel):
    """`iters` iterations of RCG on the resident likelihood (tol -1: no early stop) against the oracle's trace
    (test_gpu_rcg.lockstep: bound and theta at `rel`, equal reset decisions) through conditioned_iters, the returned
    theta at the north-star tolerance and summing to 1.  Returns the number of iterations held in lock-step."""
    core.set_trace_theta(iters)
    res = core.solve(logc, alpha0, tol=-1.0, max_iters=iters)
    tr = core.trace(iters, with_theta=True)
    core.set_trace_theta(0)
    assert res["iters"] == iters and tr["n"] == iters and int(np.sum(ref_trace["didreset"] >= 0)) == iters
    k = conditioned_iters(ref_trace, iters)
    lockstep(tr, ref_trace, k, rel=rel)
    assert_theta(res["theta"], ref_trace["theta"][iters - 1])     # what the solve returns: the last iteration's weights
    assert res["theta"].sum() == pytest.approx(1.0, abs=1e-12)
    return k


def closing_verdict(core, logc, alpha0, ref_trace, upto):
    """test_rejected_step_at_the_last_allowed_iteration on the resident likelihood: --max-iters ends the run on every
    iteration up to `upto` in turn -- among them a rejected step, whose steepest-descent retry has to be evaluated
    before the run may end -- with that test's tolerances."""
    for n in range(1, upto + 1):
        core.set_trace_theta(n)
        res = core.solve(logc, alpha0, tol=-1.0, max_iters=n)
        tr = core.trace(n, with_theta=True)
        assert res["iters"] == n and tr["n"] == n
        assert tr["didreset"].tolist() == ref_trace["didreset"][:n].tolist(), n
        np.testing.assert_allclose(tr["bound"], ref_trace["bound"][:n], rtol=1e-9, err_msg=str(n))
        np.testing.assert_allclose(res["theta"], ref_trace["theta"][n - 1], rtol=1e-6, atol=1e-13, err_msg=str(n))
        assert res["theta"].sum() == pytest.approx(1.0, abs=1e-12)
    core.set_trace_theta(0)


# ---- A: the O(G) chain of the CSR flavour -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def csr_refs(oracle):
    """case and 12-iteration oracle trace per group count, computed once"""
    made = {}

    def get(G):
        if G not in made:
            c = gb.csr_case(G)
            made[G] = (c, gb.csr_oracle(oracle, c, ITERS_CSR)["trace"])
        return made[G]
    return get


@pytest.mark.parametrize("G", gb.CSR_GROUPS)
def test_csr_lockstep_at_group_boundary(gpu_core, csr_refs, G):
    c, ref = csr_refs(G)
    assert np.isneginf(c["logc"]).sum() == c["E"] // 5
    gb.set_csr(gpu_core, c)
    k = run_lockstep(gpu_core, c["logc"], c["alpha0"], ref, ITERS_CSR, rel=1e-9)
    assert k == ITERS_CSR or G <= 2, f"G = {G}: {k} iterations in lock-step"     # (1 and 2 groups converge in 2 and 7)


def test_csr_cases_reject_steps_on_both_paths_of_finstep(csr_refs):
    """What makes the cases above a test of the rejected step (u -= oldstep, a re-evaluation by the same slot's pass B):
    the oracle rejects one within the 12 iterations on the register path (G <= 6144) and on the looping path (6145),
    and not at the first iteration, whose step has no oldstep to take back."""
    resets = {G: csr_refs(G)[1]["didreset"][:conditioned_iters(csr_refs(G)[1], ITERS_CSR)].tolist() for G in gb.CSR_GROUPS}
    in_regs = [G for G in gb.CSR_GROUPS if G <= gb.IN_REGS_MAX and 1 in resets[G][1:]]
    assert in_regs, f"no rejected step at any G <= {gb.IN_REGS_MAX}: {resets}"
    for G in (gb.IN_REGS_MAX - 1, gb.IN_REGS_MAX, gb.IN_REGS_MAX + 1):
        assert 1 in resets[G][1:], f"no rejected step at G = {G}: {resets[G]}"


def test_closing_verdict_on_the_looping_path(gpu_core, csr_refs):
    """G = 6145, where k_finstep loops over the groups: the run ends on iterations 1..5, the rejected one among them
    (the closing verdict-only launch takes u -= oldstep and leaves the re-evaluation to the next run); then the same
    through fixed-iteration runs continued in pieces, one of which ends on the rejected step."""
    G = gb.IN_REGS_MAX + 1
    c, ref = csr_refs(G)
    k = ref["didreset"][:5].tolist().index(1) if 1 in ref["didreset"][:5].tolist() else -1
    assert k >= 1, f"no rejected step within iterations 1..4 at G = {G}: {ref['didreset'].tolist()}"
    assert conditioned_iters(ref, ITERS_CSR) >= 5
    gb.set_csr(gpu_core, c)
    closing_verdict(gpu_core, c["logc"], c["alpha0"], ref, 5)
    gpu_core.set_fixed_iters(True)
    try:
        gpu_core.prepare(c["logc"], c["alpha0"])
        gpu_core.run(max_iters=k)
        r = gpu_core.continue_(1)           # ends on the rejected step
        assert r["iters"] == k + 1
        np.testing.assert_allclose(r["theta"], ref["theta"][k], rtol=1e-6, atol=1e-13)
        r = gpu_core.continue_(2)
        assert r["iters"] == k + 3 and r["bound"] == pytest.approx(ref["bound"][k + 2], rel=1e-9)
        np.testing.assert_allclose(r["theta"], ref["theta"][k + 2], rtol=1e-6, atol=1e-13)
        assert r["theta"].sum() == pytest.approx(1.0, abs=1e-12)
    finally:
        gpu_core.set_fixed_iters(False)


def rel_above(got, ref, floor=1e-4):
    """worst relative error on weights >= floor, worst absolute error below (test_gpu_bootstrap_em._rel_above)"""
    big = ref >= floor
    return float(np.max(np.abs(got - ref)[big] / ref[big], initial=0.0)), float(np.max(np.abs(got - ref)[~big], initial=0.0))


@pytest.mark.parametrize("G", gb.EM_GROUPS)
def test_em_at_group_boundary(gpu_core, oracle, G):
    """k_em_init / k_em_fin on both sides of their boundaries, 25 iterations.  Double against em_dense with the
    tolerance of test_em_csr_matches_oracle_and_rcg_region; --emprecision float against em_dense_f32 with the tolerances
    of test_emprecision_float_is_fp32_arithmetic where the fp32 kernels serve it -- they do at 6144 groups and not at
    6145, where the float run is the double run bit for bit.

    (The MAP weights max(0, Nc + alpha - 1) / (sum c + sum(alpha - 1)) of a prior with alpha < 1 do not sum to 1 once
    groups are clamped at 0 -- 0.27 over at 6144 groups, in the oracle as in the kernels: the sum is held to the
    oracle's own, which is 1 where nothing is clamped.)"""
    c = gb.csr_case(G, reads=600)
    L = dense_from_csr(c["p"], c["lut"])
    assert L.size < 5_000_000
    logc, alpha0 = c["logc"], c["alpha0"]
    gb.set_csr(gpu_core, c)
    d = gpu_core.solve(logc, alpha0, tol=-1.0, max_iters=ITERS_EM, algo=ALGO_EM)
    assert gpu_core.last_timing()["em_float_kernels"] == 0
    ref = oracle.em_dense(L, logc, alpha0, tol=-1.0, max_iters=ITERS_EM)
    assert d["iters"] == ITERS_EM == ref["iters"]
    np.testing.assert_allclose(d["theta"], ref["theta"], rtol=1e-6, atol=1e-9)
    if not np.any(ref["theta"] == 0.0):
        assert ref["theta"].sum() == pytest.approx(1.0, abs=1e-12)
    assert d["theta"].sum() == pytest.approx(ref["theta"].sum(), abs=1e-12)

    gpu_core.set_trace_theta(ITERS_EM)
    f = gpu_core.solve(logc, alpha0, tol=-1.0, max_iters=ITERS_EM, algo=ALGO_EM, prec=PREC_FLOAT)
    fp32 = gpu_core.last_timing()["em_float_kernels"]
    tr = gpu_core.trace(ITERS_EM, with_theta=True)
    gpu_core.set_trace_theta(0)
    if G == gb.IN_REGS_MAX:
        assert fp32 == 1, "the fp32 EM kernels serve 6144 groups"
    if G > gb.IN_REGS_MAX:
        assert fp32 == 0, "the fp32 EM kernels hold their groups in registers: not beyond 6144"
    assert f["iters"] == ITERS_EM
    if fp32 == 0:
        np.testing.assert_array_equal(f["theta"], d["theta"])    # the fp64 kernels ran
        assert f["bound"] == d["bound"]
        return
    o = oracle.em_dense_f32(L, logc, alpha0, tol=-1.0, max_iters=ITERS_EM, trace=ITERS_EM)
    for k in (0, 4, 19, ITERS_EM - 1):
        r, a = rel_above(tr["theta"][k], o["theta_trace"][k])
        assert r < 1e-4 and a < 1e-7, (k, r, a)
    r, a = rel_above(f["theta"], o["theta"])
    assert r < 1e-4 and a < 1e-7, (r, a)
    assert abs(f["bound"] - o["bound"]) <= 4 * np.spacing(np.float32(abs(o["bound"])))
    assert f["bound"] == float(np.float32(f["bound"]))
    assert np.all(f["theta"] == f["theta"].astype(np.float32))
    assert abs(f["theta"].sum() - o["theta"].sum()) < 1e-5    # (floats: the bound of the fp32 test, not 1e-12)


# ---- B: pass B's modes ---------------------------------------------------------------------------------------------------

G_LO, G_HI = 1000, 40000
# (what ends at the switch, the mode on either side of it)
SWITCHES = {"mode2": (lambda li: li["passB_mode"] == 2, 2, 1),             # the column sums leave the fixed distance
            "groups_in_lds": (lambda li: li["groups_in_lds"] == 1, 1, 3),  # the group vectors leave LDS
            "mode3": (lambda li: li["passB_mode"] != 4, 3, 4)}             # the column sums take ranges of 16 k groups


@pytest.fixture(scope="module")
def passB_switches(gpu_core):
    """For each of SWITCHES: the G* in (1000, 40000) with the property at G* and not at G* + 1, by bisection over
    set_csr + layout_info on the input family of part A (the slot table, and with it the switch, depends on the
    input), and the layouts on both sides."""
    cases, infos = {}, {}

    def info(G):
        if G not in infos:
            cases[G] = gb.csr_case(G)
            gb.set_csr(gpu_core, cases[G])
            infos[G] = gpu_core.layout_info()
        return infos[G]

    found = {}
    for name, (holds, _, _) in SWITCHES.items():
        lo, hi = G_LO, G_HI
        assert holds(info(lo)), f"{name}: does not hold at G = {lo}: {info(lo)}"
        assert not holds(info(hi)), f"{name}: still holds at G = {hi}: {info(hi)}"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if holds(info(mid)):
                lo = mid
            else:
                hi = mid
        found[name] = lo
    return found, info, cases


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", list(SWITCHES))
def test_passB_mode_switch(gpu_core, oracle, passB_switches, name, side):
    """the largest group count of one mode (side 0) and the smallest of the next (side 1), in lock-step as in part A"""
    found, info, cases = passB_switches
    Gs = found[name]
    assert G_LO < Gs < G_HI - 1, f"{name}: switch at {Gs}, not strictly inside ({G_LO}, {G_HI})"
    holds, mode_below, mode_above = SWITCHES[name]
    assert holds(info(Gs)) and not holds(info(Gs + 1))
    assert (info(Gs)["passB_mode"], info(Gs + 1)["passB_mode"]) == (mode_below, mode_above), \
        f"{name}: modes {info(Gs)['passB_mode']} | {info(Gs + 1)['passB_mode']} at G = {Gs} | {Gs + 1}"
    G = Gs + side
    c = cases[G]
    gb.set_csr(gpu_core, c)
    assert gpu_core.layout_info()["passB_mode"] == (mode_above if side else mode_below)
    print(f"{name}: G = {G}, pass B mode {gpu_core.layout_info()['passB_mode']}")
    ref = gb.csr_oracle(oracle, c, ITERS_CSR)["trace"]
    run_lockstep(gpu_core, c["logc"], c["alpha0"], ref, ITERS_CSR, rel=1e-9)


@pytest.mark.parametrize("G,modes", [(16384, (3, 4)), (16385, (3, 4)), (32768, (4,)), (32769, (4,))])
def test_passB_group_range_edges(gpu_core, oracle, G, modes):
    """Mode 4 sweeps one range of 16384 groups per run: two runs begin at 16385 groups, three at 32769.  (Around
    16384 the column sums of all groups may still fit, mode 3: the solve is held to the oracle all the same.)"""
    c = gb.csr_case(G)
    gb.set_csr(gpu_core, c)
    mode = gpu_core.layout_info()["passB_mode"]
    assert mode in modes, f"G = {G}: pass B mode {mode}, expected one of {modes}"
    print(f"G = {G}: pass B mode {mode}")
    ref = gb.csr_oracle(oracle, c, ITERS_CSR)["trace"]
    run_lockstep(gpu_core, c["logc"], c["alpha0"], ref, ITERS_CSR, rel=1e-9)


# ---- C: the dense flavour at a handful of ECs ---------------------------------------------------------------------------

def gamma_excess(a, b):
    """worst |a - b| in units of the bound 1e-9 + 1e-9 |b| (test_value_records_lockstep's on gamma_block): > 1 fails it"""
    return float(np.max(np.abs(a - b) / (1e-9 + 1e-9 * np.abs(b))))


@pytest.mark.parametrize("E", gb.DENSE_TINY_ECS)
@pytest.mark.parametrize("G", gb.DENSE_GROUPS)
def test_dense_instantiation_edge(gpu_core, oracle, monkeypatch, G, E):
    """Kept dense, 8 iterations against the structured oracle (rel 1e-8 as the other dense tests), the matrix read
    back bit for bit, gamma in the log domain at rtol = atol = 1e-9 (test_value_records_lockstep's on gamma_block).

    gamma is compared where the lock-step ends (conditioned_iters: many of these small problems converge within the 8
    iterations, and a step rejected by rounding afterwards -- by one side only -- moves gamma by 2e-8).  Should the
    oracle's own gamma not be good to the bound at some shape -- the fp64 structured oracle against the dense-state
    oracle in extended precision, measured in the case -- its bound is four times their distance.  Measured on the
    host: at most 4e-5 of the bound at every shape (after all 8 iterations: 1.1, 2.1 and 3.2 times the bound at
    2049 x 3, 4096 x 67 and 4097 x 67, each with a step rejected at iteration 6 or 7)."""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    c = gb.dense_case(E, G)
    logl, logc, alpha0 = c["logl"], c["logc"], c["alpha0"]
    from_dense(gpu_core, logl, logc)
    assert gpu_core.shape() == (G, E, G * E), "not kept dense"
    s = oracle.rcg_optl_dense_structured(logl, logc, alpha0, tol=-1.0, max_iters=ITERS_DENSE, trace=ITERS_DENSE)
    k = run_lockstep(gpu_core, logc, alpha0, s["trace"], ITERS_DENSE, rel=1e-8)
    np.testing.assert_array_equal(gpu_core.get_dense_logl(), logl)
    res = gpu_core.solve(logc, alpha0, tol=-1.0, max_iters=k)
    assert res["iters"] == k
    sk = oracle.rcg_optl_dense_structured(logl, logc, alpha0, tol=-1.0, max_iters=k, want_gamma=True)
    xk = oracle.rcg_optl_dense(logl, logc, alpha0, tol=-1.0, max_iters=k, extended=True)
    apart = gamma_excess(sk["gamma"], xk["gamma"])
    widen = 1.0 if apart <= 1.0 else 4.0 * apart
    print(f"{G} x {E}: gamma after {k} iterations; the fp64 and the extended oracle are {apart:.2e} of the bound apart")
    np.testing.assert_allclose(gpu_core.gamma(), sk["gamma"], rtol=1e-9 * widen, atol=1e-9 * widen)
    assert res["theta"].sum() == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("matrix", ["unstructured", "background"])
def test_dense_one_group_past_the_dense_sweeps(gpu_core, oracle, matrix):
    """8193 x 5 is re-expressed as CSR-of-ECs whatever its shape.  unstructured: every cell its own value, (nearly)
    every cell listed, as in test_unstructured_dense_matrix_beyond_the_dense_sweeps; background: the matrix of the other
    cases of this part, whose cells off the background value are the listed ones."""
    G, E = gb.DENSE_MAX_GROUPS + 1, 5
    c = gb.dense_case(E, G)
    if matrix == "unstructured":
        L = np.random.default_rng(0).normal(-3.0, 1.0, size=(G, E))
    else:
        L = c["logl"]
    gpu_core.set_dense_logl(L)
    g_, e_, nnz = gpu_core.shape()
    assert (g_, e_) == (G, E)
    if matrix == "unstructured":
        assert nnz >= G * E - E
    else:
        assert nnz == np.count_nonzero(L != np.log(0.01))
    s = oracle.rcg_optl_dense_structured(L, c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS_DENSE, trace=ITERS_DENSE)
    run_lockstep(gpu_core, c["logc"], c["alpha0"], s["trace"], ITERS_DENSE, rel=1e-8)
    np.testing.assert_array_equal(gpu_core.get_dense_logl(), L)


# ---- D: wavefronts of the dense sweeps that take more than one EC -----------------------------------------------------

DENSE_MULTI = [("reg", G) for G in gb.DENSE_REG_GROUPS] + [("big", G) for G in gb.DENSE_BIG_GROUPS]


def compute_units():
    """hipDeviceAttributeMultiprocessorCount of device 0, through the HIP runtime this process already uses -- not through
    torch.cuda, whose wheel brings a second ROCm runtime: a process that used both aborts at exit (see
    test_gpu_multi.n_devices)."""
    import ctypes
    from msweep_amd.core import load_library
    load_library()
    n = ctypes.c_int(0)
    rc = ctypes.CDLL(None).hipDeviceGetAttribute(ctypes.byref(n), 63, 0)    # hipDeviceAttributeMultiprocessorCount
    assert rc == 0 and 1 <= n.value <= 1024, (rc, n.value)
    return n.value


def multi_ec_shape(kind, G):
    """E, nw of a part D case on this GPU: nw = 4 * nblk_dense wavefronts, wavefront w sweeps the ECs w, w + nw, ...
    (dense_from_stage, msweep_amd/csrc/host_likelihood.inc: nblk_dense = max(1, min((E + 3) / 4, n_cu * (nreg >= 32 ?
    2 : 8))); restated in group_boundary_cases.dense_wavefronts).
      reg: E = 2 nw + 3 -- the register kernels prefetch the next EC's row: wavefronts 0..2 take three ECs (prefetch,
           prefetch, none), all others two (prefetch, none);
      big: E = nw + 3 -- wavefronts 0..2 take a second EC into the sums they carry, all others one."""
    n_cu = compute_units()
    nw = gb.dense_full_wavefronts(G, n_cu)
    E = 2 * nw + 3 if kind == "reg" else nw + 3
    assert (gb.dense_nreg(G) >= 32) == (kind == "big")
    assert gb.dense_wavefronts(E, G, n_cu) == nw and E > nw, f"{kind} {G}: E = {E} leaves every wavefront one EC (nw = {nw})"
    assert G * E <= 16_900_000, f"{kind} {G}: {G * E} cells"
    return E, nw


@pytest.fixture(scope="module")
def multi_ec_refs(oracle):
    """input and oracle results of a part D case; the small results are kept for the tests that share them"""
    kept = {}

    def get(kind, G, want_input=True):
        E, nw = multi_ec_shape(kind, G)
        if (kind, G) in kept and not want_input:
            return None, kept[kind, G]
        c = gb.dense_multi_ec_case(E, G, nw)
        zeros = np.nonzero(c["counts"][nw:min(2 * nw, E)] == 0)[0] + nw
        assert len(zeros) and np.any(c["counts"][:nw] == 0), "no zero count on a wavefront's second EC / first EC"
        assert np.any(c["counts"][nw:min(2 * nw, E)] != 0)
        if (kind, G) not in kept:
            # (the structured oracle: the dense-state one forms |g|^2 less accurately -- at 2051 x 8192 its value of
            # iteration 7 is 1.1e-7 from the extended oracle's, beyond lockstep's 1e-7, the structured one's 2e-11)
            r = oracle.rcg_optl_dense_structured(c["logl"], c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS_DENSE,
                                                 trace=ITERS_DENSE)
            em = oracle.em_dense(c["logl"], c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS_EM_DENSE)
            kept[kind, G] = dict(trace=r["trace"], em_theta=em["theta"], em_iters=em["iters"], E=E, nw=nw, zero_at=int(zeros[0]))
        return c, kept[kind, G]
    return get


@pytest.mark.parametrize("kind,G", DENSE_MULTI)
def test_dense_wavefront_sweeps_several_ecs(gpu_core, multi_ec_refs, monkeypatch, kind, G):
    """8 iterations against the structured oracle (rel 1e-8), 10 of EM against em_dense (the tolerance of part A).
    (EM: the prior has alpha < 1, so weights are clamped at 0 and their u = log theta is -inf in the sweeps.)"""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    c, ref = multi_ec_refs(kind, G)
    E = ref["E"]
    print(f"{kind} G = {G}: E = {E}, nw = {ref['nw']}; EC {ref['zero_at']} (the second of wavefront {ref['zero_at'] - ref['nw']}) has a "
          f"zero count; rejected steps {ref['trace']['didreset'].tolist()}")
    from_dense(gpu_core, c["logl"], c["logc"])
    assert gpu_core.shape() == (G, E, G * E), "not kept dense"
    run_lockstep(gpu_core, c["logc"], c["alpha0"], ref["trace"], ITERS_DENSE, rel=1e-8)
    em = gpu_core.solve(c["logc"], c["alpha0"], tol=-1.0, max_iters=ITERS_EM_DENSE, algo=ALGO_EM)
    assert em["iters"] == ITERS_EM_DENSE == ref["em_iters"]
    np.testing.assert_allclose(em["theta"], ref["em_theta"], rtol=1e-6, atol=1e-9)
    assert em["theta"].sum() == pytest.approx(ref["em_theta"].sum(), abs=1e-12)   # (see test_em_at_group_boundary)


def test_dense_cases_reject_steps_on_both_paths_of_finstep(multi_ec_refs):
    """The dense flavour's rejected step (no prepB_block, coef = 1) is in the cases above for the register kernels, the
    two-sweep kernels and beyond 6144 groups (the looping path of k_finstep) -- at an iteration that has an oldstep."""
    resets = {}
    for kind, G in DENSE_MULTI:
        tr = multi_ec_refs(kind, G, want_input=False)[1]["trace"]
        resets[kind, G] = tr["didreset"][:conditioned_iters(tr, ITERS_DENSE)].tolist()
    assert any(1 in r[1:] for (kind, G), r in resets.items() if kind == "reg"), resets
    assert any(1 in r[1:] for (kind, G), r in resets.items() if kind == "big"), resets
    assert any(1 in r[1:] for (kind, G), r in resets.items() if G > gb.IN_REGS_MAX), resets


def test_dense_closing_verdict_on_the_looping_path(gpu_core, multi_ec_refs, monkeypatch):
    """8192 groups, dense flavour: the run ends on iterations 1..4, the rejected one among them"""
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    G = gb.DENSE_MAX_GROUPS
    c, ref = multi_ec_refs("big", G)
    assert 1 in ref["trace"]["didreset"][1:4].tolist(), f"no rejected step within iterations 1..3: {ref['trace']['didreset'].tolist()}"
    assert conditioned_iters(ref["trace"], ITERS_DENSE) >= 4
    from_dense(gpu_core, c["logl"], c["logc"])
    assert gpu_core.shape() == (G, ref["E"], G * ref["E"]), "not kept dense"
    closing_verdict(gpu_core, c["logc"], c["alpha0"], ref["trace"], 4)
