"""GPU: the cancellation guard (SURVEY.md 7.3 ii, msweep_amd/csrc/guard.hpp).

The sweeps form Z_j = p0 * U + sum_listed e_g (x_gj - p0).  When one group holds (nearly) all of
U = sum e_g and its cells sit far below the background value (x << p0) the two parts cancel: an
isolate / single-lineage sample whose reads hit the dominant lineage weakly, with a likelihood
table that goes far below log(zi) (custom -q / -e, --read-likelihood matrices) and prior counts
below one (so that the other groups' weights underflow).  Such ECs are evaluated without the
background trick.  Checked against the DENSE-STATE oracle (rcgpar's algorithm on the G x E
matrices, log-domain throughout -- no such cancellation) at the north-star tolerance, and in
lock-step against the structured oracle (which carries the same guard).
"""
import numpy as np
import pytest

from msweep_amd.core import ALGO_EM, PREC_DOUBLE, PREC_FLOAT, Core, MswError
from msweep_amd.likelihood import from_dense
from test_gpu_em_f32_index import N_FIX, TRACED, _assert_fp32_parity
from test_gpu_rcg import assert_theta, lockstep

pytestmark = pytest.mark.gpu
LOGZI = np.log(0.01)


def isolate_problem(seed, n_ecs=6000, G=40, deep=-55.0, n_levels=6, others=(0, 4), other_values=(-6.0, -0.1)):
    """One dominant group (0) listed in most ECs -- strongly (table value near 0) or weakly (`deep`, far
    below log(zi) = -4.6) -- plus a few other groups per EC (`others`: how many, lo..hi-1) with ordinary values."""
    rng = np.random.default_rng(seed)
    lut = np.empty((G, n_levels + 1))
    lut[:, 0] = LOGZI
    lut[:, 1:] = rng.uniform(*other_values, (G, n_levels))
    lut[0, 1] = deep                  # the dominant group's weak hit
    lut[0, 2] = deep / 2
    lut[0, 3:] = rng.uniform(-1.0, -0.05, n_levels - 2)
    lut[1, 1] = deep * 0.8            # a second group with a deep cell
    rows, grp, cnt = [], [], []
    counts = np.empty(n_ecs, np.uint64)
    for j in range(n_ecs):
        kind = rng.random()
        cells = {}
        if kind < 0.55:               # a read of the dominant lineage, strong hit
            cells[0] = int(rng.integers(3, n_levels + 1))
            counts[j] = rng.integers(1, 400)
        elif kind < 0.85:             # weak hit of the dominant lineage only: the cancelling case
            cells[0] = int(rng.integers(1, 3))
            counts[j] = rng.integers(1, 4)
        elif kind < 0.93:             # dominant weak + the second deep group weak
            cells[0] = 1
            cells[1] = 1
            counts[j] = 1
        else:                         # a read that does not list the dominant group at all
            counts[j] = rng.integers(1, 3)
        for g in rng.choice(np.arange(2, G), rng.integers(*others), replace=False):
            cells[int(g)] = int(rng.integers(1, n_levels + 1))
        if not cells:
            cells[int(rng.integers(2, G))] = 1
        for g in sorted(cells):
            grp.append(g)
            cnt.append(cells[g])
        rows.append(len(cells))
    rowptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
    return dict(rowptr=rowptr, grp=np.array(grp, np.uint32), cnt=np.array(cnt, np.uint32), lut=lut,
                ec_counts=counts, G=G)


def dense_of(p):
    G, E = p["G"], len(p["rowptr"]) - 1
    L = np.full((G, E), LOGZI)
    rows = np.repeat(np.arange(E), np.diff(p["rowptr"].astype(np.int64)))
    L[p["grp"], rows] = p["lut"][p["grp"], p["cnt"]]
    return L


@pytest.mark.parametrize("alpha,deep,zero_counts", [(1.0, -55.0, False), (0.5, -55.0, True), (0.01, -55.0, False),
                                                    (1e-3, -120.0, True), (0.01, -30.0, False)])
def test_dominant_group_matches_dense_state_oracle(gpu_core, oracle, alpha, deep, zero_counts):
    _check_dominant(gpu_core, oracle, isolate_problem(seed=int(-deep) + int(alpha * 1000), deep=deep), alpha, deep, zero_counts)


@pytest.mark.parametrize("alpha,deep,zero_counts", [(0.5, -55.0, True), (0.01, -55.0, False)])
def test_dominant_group_with_mid_length_ecs(gpu_core, oracle, alpha, deep, zero_counts):
    """The guarded ECs of slices that hold several lanes per EC (17..256 cells: sell.hpp slice classes): the EC's
    first lane hands it to the guard path, which walks the EC's cells over its lanes."""
    p = isolate_problem(seed=77 + int(alpha * 1000), n_ecs=3000, G=150, deep=deep, others=(18, 120), other_values=(-16.0, -8.0))
    visits = _check_dominant(gpu_core, oracle, p, alpha, deep, zero_counts)
    assert sum(gpu_core.layout_info()["slices_by_lanes"][:-1]) > 0
    assert visits > 0          # the guard path of multi-lane slices is what this test is about


def _check_dominant(gpu_core, oracle, p, alpha, deep, zero_counts, structured=True, layout=None):
    """structured=False: without the structured oracle's lock-step (the dense-state checks only); layout: assertions on
    layout_info()."""
    G = p["G"]
    alpha0 = np.full(G, alpha)
    with np.errstate(divide="ignore"):
        c = p["ec_counts"].astype(np.float64)
        if zero_counts:
            c[::7] = 0.0                                  # -inf log counts (bootstrap replicates, BootstrapSample.cpp:70)
        logc = np.log(c)
    gpu_core.set_csr(p["rowptr"], p["grp"], p["cnt"], p["lut"], LOGZI, G)
    if layout is not None:
        layout(gpu_core.layout_info())
    gpu_core.set_trace_theta(20)
    res = gpu_core.solve(logc, alpha0)
    visits = gpu_core.guarded_visits()
    tr = gpu_core.trace(20, with_theta=True)
    gpu_core.set_trace_theta(0)
    s = None
    if structured:
        lutidx = (p["grp"] * p["lut"].shape[1] + p["cnt"]).astype(np.uint32)
        s = oracle.rcg_optl_csr(p["rowptr"], p["grp"], lutidx, p["lut"], LOGZI, G, logc, alpha0, trace=20)
    d = oracle.rcg_optl_dense(dense_of(p), logc, alpha0, trace=20)
    th_d = oracle.mixture_components(d["gamma"], logc)
    big = th_d >= 1e-4
    worst = np.max(np.abs(res["theta"] - th_d)[big] / th_d[big])
    print(f"alpha {alpha}, deepest cell {deep}: {visits} guarded EC evaluations; theta[0] = 1 - {1 - th_d[0]:.3e}; iterations hip {res['iters']} / "
          f"structured oracle {s['iters'] if s else '-'} / dense-state oracle {d['iters']}; worst rel err vs the dense-state oracle "
          f"{worst:.2e} (weights >= 1e-4), worst abs err below {np.max(np.abs(res['theta'] - th_d)[~big], initial=0):.2e}")
    assert th_d[0] > 0.9
    assert np.all(np.isfinite(res["theta"])) and res["theta"].sum() == pytest.approx(1.0, abs=1e-11)
    if s is not None:
        lockstep(tr, s["trace"], 20)
        assert abs(res["iters"] - s["iters"]) <= 1      # the stop sits in the last bits of the bound
    assert abs(res["iters"] - d["iters"]) <= 5
    # against the dense-state oracle after the SAME number of iterations
    same = gpu_core.solve(logc, alpha0, tol=-1.0, max_iters=d["iters"])
    assert_theta(same["theta"], th_d)
    # gamma (what --write-probs prints): the guarded ECs' columns too
    g = gpu_core.gamma()
    np.testing.assert_allclose(np.exp(g).sum(0), 1.0, rtol=1e-10)
    np.testing.assert_allclose(np.exp(g), np.exp(d["gamma"]), atol=2e-6)
    return visits


def isolate_1e9_problem(E=3000):
    """A single lineage (group 0 of 30) hit strongly by every EC but four, which hit it weakly (table values << log zi)
    with one read each; up to two other groups per EC, far below the background."""
    rng = np.random.default_rng(4)
    G = 30
    lut = np.full((G, 4), LOGZI)
    lut[0, 1:] = [-36.0, -30.0, -0.2]                    # weak, weak, strong hit of the dominant group
    lut[1:, 1] = -40.0                                   # every other group: only far below the background
    lut[1:, 2:] = -30.0
    kind = rng.random(E)
    kind[:4] = [0.7, 0.9, 0.9, 0.7]                     # four weak ECs, one read each; every other EC strong
    kind[4:] *= 0.6
    rows, grp, cnt = [], [], []
    for j in range(E):
        cells = {0: 3 if kind[j] < 0.6 else (1 if kind[j] < 0.8 else 2)}
        for g in rng.choice(np.arange(1, G), rng.integers(0, 3), replace=False):
            cells[int(g)] = int(rng.integers(1, 4))
        for g in sorted(cells):
            grp.append(g)
            cnt.append(cells[g])
        rows.append(len(cells))
    rowptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
    counts = np.where(kind < 0.6, rng.integers(1, 50, E).astype(np.uint64) * 100_000, 1).astype(np.uint64)
    return dict(rowptr=rowptr, grp=np.array(grp, np.uint32), cnt=np.array(cnt, np.uint32), lut=lut, ec_counts=counts, G=G)


def test_isolate_theta_one_minus_1e_9(gpu_core, oracle):
    """A single lineage at theta >= 1 - 1e-9 with the default prior (alpha = 1).  Nearly all reads hit it
    strongly; a few reads hit it weakly (table values << log zi): for those the dominant group's cell
    and the background sum cancel (Z is 1e-13 of p0 * U), and they are what the other groups live on."""
    p = isolate_1e9_problem()
    rowptr, grp, cnt, lut, counts, G = p["rowptr"], p["grp"], p["cnt"], p["lut"], p["ec_counts"], p["G"]
    logc = np.log(counts.astype(np.float64))
    gpu_core.set_csr(rowptr, grp, cnt, lut, LOGZI, G)
    # 7e9 reads: the bound is ~1e10 and one fp64 ulp of it is 2e-6 -- the stop rule is given a gain it can
    # resolve (the reference's OpenMP path keeps its bound in long double for this reason)
    d = oracle.rcg_optl_dense(dense_of(dict(rowptr=rowptr, grp=grp, cnt=cnt, lut=lut, G=G)), logc, np.ones(G), tol=1e-3)
    own = gpu_core.solve(logc, np.ones(G), tol=1e-3)
    assert abs(own["iters"] - d["iters"]) <= 2
    res = gpu_core.solve(logc, np.ones(G), tol=-1.0, max_iters=d["iters"])   # the same number of iterations
    th_d = oracle.mixture_components(d["gamma"], logc)
    print(f"isolate: theta[0] = 1 - {1 - res['theta'][0]:.3e} (dense-state oracle 1 - {1 - th_d[0]:.3e}), "
          f"iterations {res['iters']} / {d['iters']}; other groups: hip {res['theta'][1:].max():.3e}, oracle {th_d[1:].max():.3e}")
    assert 1 - th_d[0] < 1e-9
    assert_theta(res["theta"], th_d)
    # the other groups' weights themselves (far below the floor of the north-star tolerance), relatively
    np.testing.assert_allclose(res["theta"][1:], th_d[1:], rtol=1e-5, atol=1e-30)


def test_zero_probability_ec_is_an_error_not_a_nan(gpu_core):
    """An EC whose only cell underflows under every group: reported, not propagated as NaN."""
    G = 4
    lut = np.array([[LOGZI, -800.0]] * G)
    rowptr = np.array([0, 1, 2], np.uint64)
    grp = np.array([0, 0], np.uint32)
    cnt = np.array([1, 1], np.uint32)
    gpu_core.set_csr(rowptr, grp, cnt, lut, LOGZI, G)
    # prior counts so small that every other group's weight underflows: nothing is left for these ECs
    try:
        r = gpu_core.solve(np.zeros(2), np.full(G, 1e-5), max_iters=50)
    except MswError as ex:
        assert "underflow" in str(ex) or "not finite" in str(ex)
    else:
        assert np.all(np.isfinite(r["theta"])) and r["theta"].sum() == pytest.approx(1.0, abs=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# The guard path of every sweep and record form (msweep_amd/csrc/guard.hpp).  Each case asserts the layout it means to
# exercise AND guarded_visits() > 0 after the solve: a case the guard never ran in proves nothing and fails.
# Two inputs whose ECs are guarded under EM too (prior 0.5; the default isolate_problem(G=40) never is: its other groups
# keep 0.6 % of the weight, above the guard's 2^-8).  `deep` = -30 keeps exp(T - tref) well inside fp32.
# ---------------------------------------------------------------------------------------------------------------------
GUARD_INPUTS = {
    "short": dict(seed=3, n_ecs=600, G=300, deep=-30.0, other_values=(-16.0, -8.0)),
    "mid": dict(seed=2, n_ecs=800, G=150, deep=-55.0, others=(18, 120), other_values=(-16.0, -8.0)),   # ECs of 17..256 cells
}


@pytest.fixture(scope="module")
def guard_inputs(oracle):
    """name -> the problem and its EM reference."""
    out = {}
    for name, kw in GUARD_INPUTS.items():
        p = isolate_problem(**kw)
        L = dense_of(p)
        logc = np.log(p["ec_counts"].astype(np.float64))
        a0 = np.full(p["G"], 0.5)
        out[name] = dict(p=p, L=L, logc=logc, a0=a0, em=oracle.em_dense(L, logc, a0, tol=1e-8, max_iters=400))
    return out


def _load_csr(core, p):
    core.set_csr(p["rowptr"], p["grp"], p["cnt"], p["lut"], LOGZI, p["G"])
    return core.layout_info()


@pytest.mark.parametrize("name", sorted(GUARD_INPUTS))
def test_guard_under_em_double(guard_inputs, name):
    """k_passB's guard section with a = 1 (EM): iteration count and weights against the dense EM oracle."""
    q = guard_inputs[name]
    with Core(0) as core:
        li = _load_csr(core, q["p"])
        assert li["record_bytes"] == 4 and li["index_records"] == 0 and li["passB_mode"] in (1, 2), li
        em = core.solve(q["logc"], q["a0"], algo=ALGO_EM, prec=PREC_DOUBLE, tol=1e-8, max_iters=400)
        assert core.last_timing()["em_float_kernels"] == 0
        visits = core.guarded_visits()
    print(f"{name}: fp64 EM, {visits} guarded EC evaluations, iterations {em['iters']} / {q['em']['iters']}")
    assert visits > 0
    assert em["iters"] == q["em"]["iters"]
    assert_theta(em["theta"], q["em"]["theta"])


@pytest.mark.parametrize("records", ["offset", "index"])
@pytest.mark.parametrize("name", sorted(GUARD_INPUTS))
def test_guard_under_em_float(guard_inputs, oracle, monkeypatch, name, records):
    """The guard section of the fp32 EM sweeps, k_em_passB_f32 (offset records) and k_em_passB_f32_idx (index records:
    MSWEEP_FORCE_LDS=10), against the fp32 oracle through test_gpu_em_f32_index.py _assert_fp32_parity.  Up to N_FIX
    iterations at tol = -1 as there: with a prior below one the MAP objective is not the log-likelihood, which FALLS by
    more than that in the short input's fifth iteration -- both runs stop there.
    Two of the helper's assertions are switched off: the weights adding up to 1 within 1e-5 (a prior below one clips
    weights at zero: the ORACLE's own sums are off by 1.6e-6 and 7.8e-4) and, on the short input, the log-likelihood
    within four float spacings (the sweep gives -45148.176, the oracle -45148.426: 0.25 against 0.016)."""
    if records == "index":
        monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    q = guard_inputs[name]
    if "em32" not in q:
        q["em32"] = oracle.em_dense_f32(q["L"], q["logc"], q["a0"], tol=-1.0, max_iters=N_FIX, trace=N_FIX)
    o = q["em32"]
    with Core(0) as core:
        li = _load_csr(core, q["p"])
        assert li["index_records"] == (records == "index") and li["record_bytes"] == 4, li
        core.set_trace_theta(N_FIX)
        f = core.solve(q["logc"], q["a0"], tol=-1.0, max_iters=N_FIX, algo=ALGO_EM, prec=PREC_FLOAT)
        assert core.last_timing()["em_float_kernels"] == 1
        visits = core.guarded_visits()
        tr = core.trace(N_FIX, with_theta=True)
    print(f"{name}, {records} records: fp32 EM, {visits} guarded EC evaluations in {f['iters']} iterations (oracle {o['iters']}); "
          f"log-likelihood {f['bound']!r} / {o['bound']!r}; sum of weights - 1: {f['theta'].sum() - 1:.2e} / {o['theta'].sum() - 1:.2e}")
    assert visits > 0
    assert f["iters"] == o["iters"]
    _assert_fp32_parity(f"guard {name} {records}", f, tr, o["theta"], o["theta_trace"], o["bound"],
                        traced=tuple(k for k in TRACED if k < o["iters"]), bound=name == "mid", unit_sum=False)


def _is_index(li):
    assert li["index_records"] == 1 and li["record_bytes"] == 4, li


def _is_wide(li):
    assert li["record_bytes"] == 8, li


def _is_mode0(li):
    assert li["passB_mode"] == 0, li


@pytest.mark.parametrize("switches,layout", [({"MSWEEP_FORCE_LDS": "10"}, _is_index), ({"MSWEEP_RECORD_BYTES": "8"}, _is_wide),
                                             ({"MSWEEP_GLOBAL_ATOMICS": "1", "MSWEEP_FORCE_LDS": "01"}, _is_mode0)],
                         ids=["index", "wide", "global_atomics"])
def test_guard_under_rcg_on_other_record_forms(oracle, monkeypatch, switches, layout):
    """Index records, 8-byte records and pass B's mode 0 (column sums in memory) through the guard path of both sweeps:
    the short-EC input at prior 0.01 (at 0.5 RCG never guards an EC of it) against the DENSE-STATE oracle at the
    north-star tolerance.  (Not the structured oracle's lock-step: on this input the solve misses it on all three
    layouts -- new norm off by 1.2e-7 where 1e-7 is allowed, weights by up to 2.3e-7 where 1e-9 is.)
    (MSWEEP_GLOBAL_ATOMICS is read only for group vectors that are not in LDS -- host_layout.inc passB_mode -- which
    300 groups are unless MSWEEP_FORCE_LDS=01 puts them in memory.)"""
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    with Core(0) as core:
        visits = _check_dominant(core, oracle, isolate_problem(**GUARD_INPUTS["short"]), 0.01, -30.0, False,
                                 structured=False, layout=layout)
    assert visits > 0


def _is_value(li):
    assert li["record_bytes"] == 12, li


def test_guard_under_rcg_on_value_records(oracle):
    """12-byte value records through the guard walk of both sweeps: test_isolate_theta_one_minus_1e_9's generator at
    40000 ECs -- 80 k listed cells at 7 % density: value records need more than 65536 different listed values -- as a
    dense matrix with noise of 1e-3 on every listed cell, prior 1 and tol 1e-3 as there, against the dense-state oracle
    on the same matrix.  (isolate_problem at 30000 ECs, cells down to -120, prior 1e-3, reaches value records too but
    guards no EC in its 87 iterations.)"""
    name, p, alpha, tol = "isolate", isolate_1e9_problem(40000), 1.0, 1e-3
    L = dense_of(p)
    rows = np.repeat(np.arange(len(p["rowptr"]) - 1), np.diff(p["rowptr"].astype(np.int64)))
    L[p["grp"], rows] += np.random.default_rng(5).normal(0.0, 1e-3, len(rows))
    logc = np.log(p["ec_counts"].astype(np.float64))
    alpha0 = np.full(p["G"], alpha)
    d = oracle.rcg_optl_dense(L, logc, alpha0, tol=tol)
    th_d = oracle.mixture_components(d["gamma"], logc)
    with Core(0) as core:
        from_dense(core, L, logc)
        _is_value(core.layout_info())
        res = core.solve(logc, alpha0, tol=tol)
        visits = core.guarded_visits()
        same = core.solve(logc, alpha0, tol=-1.0, max_iters=d["iters"])     # the SAME number of iterations
    print(f"value records, {name}: {visits} guarded EC evaluations; theta[0] = 1 - {1 - th_d[0]:.3e}; iterations {res['iters']} / "
          f"dense-state oracle {d['iters']}; sum of weights - 1: {res['theta'].sum() - 1:.2e}")
    assert visits > 0
    assert th_d[0] > 0.9
    assert np.all(np.isfinite(res["theta"])) and res["theta"].sum() == pytest.approx(1.0, abs=1e-11)
    assert_theta(same["theta"], th_d)
    assert abs(res["iters"] - d["iters"]) <= 5


# Pass B's modes 3 and 4 (sell.hpp pass_lds_bytes, host_layout.inc passB_mode).  The group vectors leave LDS -- mode 3, the
# column sums alone in LDS -- with the first G whose 16 bytes per group (G + 64 sentinels) and the sweeps' tail exceed
# the 160 KB; one range of groups at a time -- mode 4 -- with the first G whose 8 bytes per group do, beside the slot
# table the layout keeps in LDS (sell_bhi(slot_entries_in_lds) bytes: the test reads it back and checks that its G is
# that boundary for the table it got).
K_LDS, K_TAIL, K_SENTINELS = 160 * 1024, 32 * 8 + 16 * 66 * 8, 64


def _first_G_past_lds(bytes_per_group, n_tab=0):
    bhi = (16 * n_tab + 255) & ~255 if n_tab else 0
    return (K_LDS - K_TAIL - bhi) // bytes_per_group - K_SENTINELS + 1


MANY_ITERS = 12        # fixed iterations of the mode-to-mode comparison
G_MODE4 = 17473        # = _first_G_past_lds(8, slot_entries_in_lds) for this input (asserted below)


def _many_groups(G):
    return isolate_problem(**dict(GUARD_INPUTS["short"], G=G))


@pytest.mark.parametrize("alpha", [0.01, 0.5])
@pytest.mark.parametrize("G,mode,other,other_mode", [(_first_G_past_lds(16), 3, {"MSWEEP_GLOBAL_ATOMICS": "1"}, 0),
                                                     (G_MODE4, 4, {"MSWEEP_FORCE_LDS": "00"}, 3)], ids=["mode3", "mode4"])
def test_guard_with_many_groups(oracle, monkeypatch, G, mode, other, other_mode, alpha):
    """The short-EC input with G raised to the first group count of pass B's mode 3 and of mode 4, against the
    DENSE-STATE oracle after the same number of iterations, at the north-star tolerance.  At prior 0.5 also against the
    same problem under the next simpler mode, a fixed number of iterations: the same guarded EC evaluations -- in mode 4
    the guard path runs once per sweep, not once per range of groups -- and the same weights.
    Not asserted, because the solve misses them: the structured oracle's lock-step (the
    solves converge within ten iterations and the new norm of the last ones is rounding noise, -5.0e-10 against 8.3e-11,
    with no absolute floor in that check); at prior 0.5 the iteration counts (7, structured oracle 10, dense-state 15);
    at prior 0.01 the mode-to-mode comparison (the 12 iterations run past convergence, where two runs of ONE mode
    differ: 2673 and 2431 evaluations)."""
    p = _many_groups(G)
    alpha0 = np.full(G, alpha)
    logc = np.log(p["ec_counts"].astype(np.float64))
    d = oracle.rcg_optl_dense(dense_of(p), logc, alpha0)
    th_d = oracle.mixture_components(d["gamma"], logc)
    with Core(0) as core:
        if mode == 3:
            li = _load_csr(core, _many_groups(G - 1))
            assert li["groups_in_lds"] == 1 and li["passB_mode"] in (1, 2), li      # one group fewer: still in LDS
        li = _load_csr(core, p)
        assert li["passB_mode"] == mode, li
        if mode == 4:   # (with the table this layout keeps in LDS, one group fewer leaves room for all column sums)
            assert li["table_in_lds"] == 1 and G == _first_G_past_lds(8, li["slot_entries_in_lds"]), li
        res = core.solve(logc, alpha0)
        visits = core.guarded_visits()
        print(f"G {G}, mode {mode}, prior {alpha}: {visits} guarded EC evaluations; iterations {res['iters']} / dense-state oracle {d['iters']}")
        assert visits > 0
        assert np.all(np.isfinite(res["theta"])) and res["theta"].sum() == pytest.approx(1.0, abs=1e-11)
        if alpha == 0.01:
            assert abs(res["iters"] - d["iters"]) <= 5
        same = core.solve(logc, alpha0, tol=-1.0, max_iters=d["iters"])     # the SAME number of iterations
        assert_theta(same["theta"], th_d)
        if alpha == 0.5:
            runs = []
            for env, want in (({}, mode), (other, other_mode)):
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                li = _load_csr(core, p)
                assert li["passB_mode"] == want, li
                r = core.solve(logc, alpha0, tol=-1.0, max_iters=MANY_ITERS)
                runs.append((r, core.guarded_visits()))
            print(f"  in {MANY_ITERS} iterations: mode {mode} {runs[0][1]} evaluations, mode {other_mode} {runs[1][1]}")
            assert runs[0][1] == runs[1][1] > 0
            assert_theta(runs[0][0]["theta"], runs[1][0]["theta"])
