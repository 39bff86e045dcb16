"""GPU: bootstrap resampling (bit-exact with libstdc++'s stream), the bootstrap driver, and the EM
variant, against the oracle and the committed golden vectors."""
import numpy as np
import pytest

from conftest import dense_from_csr, load_golden, lutidx_of
from msweep_amd import synth
from msweep_amd.core import ALGO_EM, ALGO_RCG
from msweep_amd.likelihood import from_dense, from_grouped_counts, precalc_lls
from test_gpu_rcg import assert_theta

pytestmark = pytest.mark.gpu


def test_resample_counts_match_libstdcxx_golden(gpu_core):
    g = load_golden("bootstrap_golden.json")
    for c in g["cases"]:
        exp = np.array(c["counts"], np.uint32)
        got = gpu_core.resample_counts(c["weights"], c["seed"], c["draws"], 0, len(exp))
        np.testing.assert_array_equal(got, exp)
        # any slice of the ONE sequential stream, asked for on its own (what rank r of N does)
        if len(exp) > 1:
            got1 = gpu_core.resample_counts(c["weights"], c["seed"], c["draws"], 1, len(exp))
            np.testing.assert_array_equal(got1, exp[1:])


def test_resample_counts_match_oracle_large(gpu_core, oracle):
    rng = np.random.default_rng(21)
    w = rng.integers(0, 500, 200_000).astype(np.uint32)
    w[rng.random(len(w)) < 0.3] = 0
    exp = oracle.bootstrap_counts(w, -99, 300_000, 3)
    got = gpu_core.resample_counts(w, -99, 300_000, 0, 3)
    np.testing.assert_array_equal(got, exp)
    # backwards seek re-seeds the stream
    np.testing.assert_array_equal(gpu_core.resample_counts(w, -99, 300_000, 1, 2), exp[1:2])
    assert np.all(got.sum(1) == 300_000)


def test_far_seek_jumps_ahead_like_stepping(gpu_core, monkeypatch):
    """Rank r of a multi-GPU bootstrap starts r * (B / P) * draws words into the stream: beyond 2^27
    words the seek is a GF(2) jump on the host; same counts as stepping there on the device."""
    rng = np.random.default_rng(3)
    w = rng.integers(1, 50, 5000).astype(np.uint32)
    draws, first = 100_000, 1500            # 1.5e8 words in
    jumped = gpu_core.resample_counts(w, 11, draws, first, first + 2)
    jumped_on = gpu_core.resample_counts(w, 11, draws, first + 2, first + 3)   # short forward seek after a jump
    monkeypatch.setenv("MSWEEP_MT_NOJUMP", "1")
    stepped = gpu_core.resample_counts(w, 11, draws, first, first + 3)
    np.testing.assert_array_equal(jumped, stepped[:2])
    np.testing.assert_array_equal(jumped_on, stepped[2:])
    assert np.all(stepped.sum(1) == draws)


def test_bootstrap_driver_matches_replicate_by_replicate_oracle(gpu_core, oracle):
    p = synth.make_csr_problem(30000, 80, seed=14, max_other=6)
    G = 80
    alpha0 = np.ones(G)
    lik = from_grouped_counts(gpu_core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    w = p["ec_counts"].astype(np.uint32)
    draws = int(w.sum())
    theta, iters = gpu_core.bootstrap(w, 42, draws, 0, 4, alpha0)
    counts = oracle.bootstrap_counts(w, 42, draws, 4)
    lut = precalc_lls(p["group_sizes"])
    for b in range(4):
        with np.errstate(divide="ignore"):
            logc = np.log(counts[b].astype(float))       # -inf for ECs drawn zero times (:70)
        ref = oracle.rcg_optl_csr(p["rowptr"], p["grp"], lutidx_of(p, lut), lut, np.log(0.01), G, logc, alpha0)
        assert iters[b] == ref["iters"]
        assert_theta(theta[b], ref["theta"])
        assert theta[b].sum() == pytest.approx(1.0, abs=1e-12)   # normalised by the resampled total
    # a slice of the replicate stream equals the same rows of the full run (N-GPU invariance)
    # (identical resampled counts; the solves differ only by the order of the LDS atomic adds of
    # the column sums, i.e. by rounding)
    theta2, _ = gpu_core.bootstrap(w, 42, draws, 2, 4, alpha0)
    for b in range(2):
        assert_theta(theta2[b], theta[2 + b])
    # --bootstrap-count smaller than the number of reads
    theta3, _ = gpu_core.bootstrap(w, 7, 5000, 0, 1, alpha0)
    c3 = oracle.bootstrap_counts(w, 7, 5000, 1)[0]
    with np.errstate(divide="ignore"):
        r3 = oracle.rcg_optl_csr(p["rowptr"], p["grp"], lutidx_of(p, lut), lut, np.log(0.01), G,
                                 np.log(c3.astype(float)), alpha0)
    assert_theta(theta3[0], r3["theta"])


@pytest.mark.parametrize("idx", [1, 2, 3, 6])
def test_em_dense_matches_oracle(gpu_core, oracle, idx):
    c = load_golden("rcg_golden.json")["cases"][idx]
    L = np.array(c["logl"])
    logc = np.array([-np.inf if x is None else x for x in c["logc"]])
    alpha0 = np.array(c["alpha0"])
    from_dense(gpu_core, L, logc)
    res = gpu_core.solve(logc, alpha0, tol=1e-9, max_iters=5000, algo=ALGO_EM)
    ref = oracle.em_dense(L, logc, alpha0, tol=1e-9, max_iters=5000, want_gamma=True)
    assert abs(res["iters"] - ref["iters"]) <= 2
    np.testing.assert_allclose(res["theta"], ref["theta"], rtol=1e-6, atol=1e-9)
    assert res["bound"] == pytest.approx(ref["bound"], rel=1e-10)
    np.testing.assert_allclose(np.exp(gpu_core.gamma()), np.exp(ref["gamma"]), atol=1e-6)


def test_em_csr_matches_oracle_and_rcg_region(gpu_core, oracle):
    p = synth.make_csr_problem(20000, 60, seed=15, max_other=6)
    G = 60
    alpha0 = np.ones(G)
    lik = from_grouped_counts(gpu_core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    em = gpu_core.solve(lik.log_counts(), alpha0, tol=1e-8, max_iters=20000, algo=ALGO_EM)
    lut = precalc_lls(p["group_sizes"])
    ref = oracle.em_dense(dense_from_csr(p, lut), lik.log_counts(), alpha0, tol=1e-8, max_iters=20000)
    assert abs(em["iters"] - ref["iters"]) <= 2
    np.testing.assert_allclose(em["theta"], ref["theta"], rtol=1e-6, atol=1e-9)
    rcg = gpu_core.solve(lik.log_counts(), alpha0, algo=ALGO_RCG)
    np.testing.assert_allclose(em["theta"], rcg["theta"], atol=5e-3)   # different objectives, same region
    # --emprecision float: fp32 arithmetic, stops where the float log-likelihood stops growing -- earlier, in the same
    # region (test_emprecision_float_is_fp32_arithmetic holds it against the fp32 oracle)
    em32 = gpu_core.solve(lik.log_counts(), alpha0, tol=1e-8, max_iters=20000, algo=ALGO_EM, prec=1)
    assert gpu_core.last_timing()["em_float_kernels"] == 1 and em32["iters"] < em["iters"]
    np.testing.assert_allclose(em32["theta"], em["theta"], atol=5e-3)


def test_large_slot_area_em_and_bootstrap(gpu_core, oracle):
    """A dense matrix with continuous listed values is re-expressed with one table slot per listed
    cell: far more than 16384 slots, so the per-slot tables are rebuilt by k_tables (many workgroups)
    instead of inside k_step / k_fin / k_em_fin.  EM, RCG and the bootstrap driver on that form."""
    E, G = 12000, 300
    p = synth.make_dense_problem(E, G, seed=23)
    rng = np.random.default_rng(5)
    w = rng.integers(1, 40, E).astype(np.uint32)
    logc = np.log(w.astype(float))
    alpha0 = np.ones(G)
    from_dense(gpu_core, p["logl"], logc)
    assert 16384 < gpu_core.shape()[2] < G * E // 4
    em = gpu_core.solve(logc, alpha0, tol=1e-4, max_iters=5000, algo=ALGO_EM)
    ref = oracle.em_dense(p["logl"], logc, alpha0, tol=1e-4, max_iters=5000)
    assert abs(em["iters"] - ref["iters"]) <= max(2, ref["iters"] // 200)   # a flat tail: the stop is soft
    np.testing.assert_allclose(em["theta"], ref["theta"], rtol=1e-5, atol=1e-8)
    rcg = gpu_core.solve(logc, alpha0)
    s = oracle.rcg_optl_dense_structured(p["logl"], logc, alpha0)
    assert abs(rcg["iters"] - s["iters"]) <= 2
    assert_theta(rcg["theta"], s["theta"])
    # bootstrap replicates: each equals a solve on the oracle's resampled counts
    draws = int(w.sum())
    theta, iters = gpu_core.bootstrap(w, 7, draws, 0, 2, alpha0)
    counts = oracle.bootstrap_counts(w, 7, draws, 2)
    for b in range(2):
        with np.errstate(divide="ignore"):
            lc = np.log(counts[b].astype(float))
        rb = oracle.rcg_optl_dense_structured(p["logl"], lc, alpha0)
        assert abs(iters[b] - rb["iters"]) <= 2
        assert_theta(theta[b], rb["theta"])


@pytest.mark.parametrize("streams", ["1", "3", "16"])
def test_replicates_in_flight_do_not_change_results(gpu_core, monkeypatch, streams):
    """The driver runs several replicates at a time (solver states sharing the resident likelihood,
    one stream each, contiguous blocks of the one random stream): same counts, same solves."""
    p = synth.make_csr_problem(20000, 50, seed=41, max_other=6)
    G = 50
    lik = from_grouped_counts(gpu_core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    w = p["ec_counts"].astype(np.uint32)
    draws = int(w.sum())
    monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", "1")
    ref, it_ref = gpu_core.bootstrap(w, 5, draws, 1, 8, np.ones(G))
    monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", streams)
    got, it = gpu_core.bootstrap(w, 5, draws, 1, 8, np.ones(G))
    assert it.tolist() == it_ref.tolist()
    for b in range(7):
        assert_theta(got[b], ref[b])
    # the handle's own state still serves a plain solve afterwards
    res = gpu_core.solve(lik.log_counts(), np.ones(G))
    assert res["theta"].sum() == pytest.approx(1.0, abs=1e-12)


def test_replicates_in_flight_across_likelihood_changes(gpu_core, monkeypatch):
    """The extra solver states outlive a likelihood: a larger CSR likelihood, then a dense one (kept on
    the dense sweeps), on the same handle -- each time the same replicates as with one in flight."""
    def both(w, draws, G):
        monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", "1")
        ref, it_ref = gpu_core.bootstrap(w, 9, draws, 0, 5, np.ones(G))
        monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", "3")
        got, it = gpu_core.bootstrap(w, 9, draws, 0, 5, np.ones(G))
        assert it.tolist() == it_ref.tolist()
        for b in range(5):
            assert_theta(got[b], ref[b])

    for R, G, seed in [(5000, 20, 51), (60000, 120, 52)]:
        p = synth.make_csr_problem(R, G, seed=seed, max_other=5)
        from_grouped_counts(gpu_core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
        w = p["ec_counts"].astype(np.uint32)
        both(w, int(w.sum()), G)
    monkeypatch.setenv("MSWEEP_DENSE_COMPRESS", "0")
    d = synth.make_dense_problem(3000, 70, seed=53)
    from_dense(gpu_core, d["logl"], d["logc"])
    w = np.random.default_rng(2).integers(1, 9, 3000).astype(np.uint32)
    both(w, int(w.sum()), 70)


def test_bootstrap_keeps_the_handles_solve_and_not_its_settings(monkeypatch):
    """The replicates run beside the handle's own solve: gamma, the trace, the timing record and the guarded visits
    after msw_core_bootstrap still describe the solve before it (the drivers write --write-probs after the
    replicates).  And the replicates do not take the handle's fixed_iters, profiling or trace_theta: they solve to
    tol whatever those say."""
    from msweep_amd.core import Core
    p = synth.make_csr_problem(20000, 40, seed=61, max_other=6)
    G, n, max_iters = 40, 12, 5000
    alpha0 = np.ones(G)
    w = p["ec_counts"].astype(np.uint32)
    draws = int(w.sum())

    def state(core):
        return core.gamma(), core.trace(n, with_theta=True), core.last_timing(), core.guarded_visits()

    def assert_same_state(a, b):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1].keys() == b[1].keys()
        for k in a[1]:
            np.testing.assert_array_equal(a[1][k], b[1][k])
        assert a[2] == b[2] and a[3] == b[3]

    with Core(0) as core:
        lik = from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
        core.set_profiling(True)
        core.set_trace_theta(n)
        res = core.solve(lik.log_counts(), alpha0, max_iters=max_iters)
        assert n < res["iters"] < max_iters
        before = state(core)
        assert before[1]["n"] == n and before[2]["passA_ms"] > 0.0
        core.set_fixed_iters(True)
        reps = {}
        for streams in ("1", "4"):
            monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", streams)
            reps[streams] = core.bootstrap(w, 3, draws, 0, 4, alpha0, max_iters=max_iters)
            assert_same_state(state(core), before)
        core.set_fixed_iters(False)
        core.set_profiling(False)
        core.set_trace_theta(0)
        for streams in ("1", "4"):
            monkeypatch.setenv("MSWEEP_BOOTSTRAP_STREAMS", streams)
            theta, iters = core.bootstrap(w, 3, draws, 0, 4, alpha0, max_iters=max_iters)
            np.testing.assert_array_equal(theta, reps[streams][0])
            np.testing.assert_array_equal(iters, reps[streams][1])
            assert np.all(iters < max_iters)
        assert reps["1"][1].tolist() == reps["4"][1].tolist()



def _float_problem(R, G, seed, max_other):
    p = synth.make_csr_problem(R, G, seed=seed, max_other=max_other)
    lut = precalc_lls(p["group_sizes"])
    return p, dense_from_csr(p, lut), np.log(p["ec_counts"].astype(float))


def _rel_above(got, ref, floor=1e-4):
    big = ref >= floor
    return float(np.max(np.abs(got - ref)[big] / ref[big], initial=0.0)), float(np.max(np.abs(got - ref)[~big], initial=0.0))


@pytest.mark.parametrize("R,G,seed,mo", [(20000, 60, 33, 5), (150000, 400, 34, 15)])
def test_emprecision_float_is_fp32_arithmetic(gpu_core, oracle, R, G, seed, mo):
    """--emprecision float (src/mSWEEP.cpp:129,202) as REAL fp32 (msweep_amd/csrc/em_f32_kernels.hpp; until round 4 it ran
    the fp64 kernels).  Against orc_em_dense_f32 (rcgpar::em_torch with float tensors restated): (i) a fixed number of
    iterations: every weight >= 1e-4 within 1e-4 relative (two fp32 evaluation orders), (ii) to --tol 1e-6: the float
    log-likelihood stops growing at float resolution after a fraction of the double run's iterations -- the behaviour
    the reference publishes (335 iterations against the 5000 cap, docs/gpubenchmarks.md:20-22) -- within a few iterations
    of the oracle (+-6 or 15 %: the gains there are one or two float steps of the log-likelihood, and which iteration
    rounds to no gain depends on the rounding of 10^4 .. 10^7 fp32 terms on either side; measured 30 / 34 and 50 / 55);
    (iii) the answer differs from the double run's at the level such an early stop implies."""
    from msweep_amd.core import PREC_DOUBLE, PREC_FLOAT
    p, L, logc = _float_problem(R, G, seed, mo)
    lik = from_grouped_counts(gpu_core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])
    a0 = np.ones(G)
    n = 40
    gpu_core.set_trace_theta(n)
    f_fix = gpu_core.solve(lik.log_counts(), a0, tol=-1.0, max_iters=n, algo=ALGO_EM, prec=PREC_FLOAT)
    assert gpu_core.last_timing()["em_float_kernels"] == 1
    tr = gpu_core.trace(n, with_theta=True)
    gpu_core.set_trace_theta(0)
    o_fix = oracle.em_dense_f32(L, logc, a0, tol=-1.0, max_iters=n, trace=n)
    for k in (0, 4, 19, n - 1):
        r, a = _rel_above(tr["theta"][k], o_fix["theta_trace"][k])
        assert r < 1e-4 and a < 1e-7, (k, r, a)
    r, a = _rel_above(f_fix["theta"], o_fix["theta"])
    print(f"float EM, {n} iterations: worst rel err vs the fp32 oracle {r:.2e} (abs below 1e-4: {a:.2e}); "
          f"log-likelihood {f_fix['bound']!r} / {o_fix['bound']!r}")
    assert abs(f_fix["bound"] - o_fix["bound"]) <= 4 * np.spacing(np.float32(abs(o_fix["bound"])))
    assert f_fix["bound"] == float(np.float32(f_fix["bound"]))          # the log-likelihood IS a float
    assert np.all(f_fix["theta"] == f_fix["theta"].astype(np.float32))  # and so are the weights
    assert abs(f_fix["theta"].sum() - 1.0) < 1e-5
    # (ii) the stop
    f = gpu_core.solve(lik.log_counts(), a0, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=5000)
    o = oracle.em_dense_f32(L, logc, a0, max_iters=5000)
    d = gpu_core.solve(lik.log_counts(), a0, algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=5000)
    assert gpu_core.last_timing()["em_float_kernels"] == 0
    print(f"to --tol 1e-6: float {f['iters']} iterations (fp32 oracle {o['iters']}), double {d['iters']}")
    assert abs(int(f["iters"]) - int(o["iters"])) <= max(6, int(0.15 * o["iters"]))
    assert f["iters"] < 0.6 * d["iters"] and o["iters"] < 0.6 * d["iters"]
    r, a = _rel_above(f["theta"], o["theta"])
    print(f"at their own stops: worst rel diff float hip / fp32 oracle {r:.2e} (abs below 1e-4: {a:.2e})")
    assert r < 5e-2 and a < 1e-5, (r, a)     # (stops a few iterations apart: the weights still move there)
    # (iii) float is not double
    assert np.max(np.abs(f["theta"] - d["theta"])) > 1e-7


def test_emprecision_float_other_shapes_and_fallback(oracle, monkeypatch):
    """The fp32 sweep over ECs of 17..700 cells (slice classes: several lanes per EC, DPP sums of floats), ECs beyond
    1024 cells (a wavefront each), zero counts, multiplicities beyond a byte, an EC holding a third of all reads (the
    two-part fixed-point adds) -- against the fp32 oracle; bootstrap replicates under float; and the layouts the fp32
    kernels do not serve (8-byte records here) run the fp64 kernels under MSW_PREC_FLOAT: the double run's bits."""
    from msweep_amd.core import Core, PREC_DOUBLE, PREC_FLOAT
    rng = np.random.default_rng(19)
    G = 1300
    sizes = (1 + rng.poisson(4, G)).astype(np.uint64)
    lut = precalc_lls(sizes)
    lens = np.concatenate([rng.integers(1, 17, 600), rng.integers(17, 700, 60), [1100, 1250, 3, 1]])
    rng.shuffle(lens)
    cols = [np.sort(rng.choice(G, int(n), replace=False)) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    grp = np.concatenate(cols).astype(np.uint32)
    cnt = rng.integers(1, sizes[grp] + 1).astype(np.uint32)
    E = len(lens)
    c = rng.integers(1, 40, E).astype(float)
    c[rng.random(E) < 0.2] = 0.0
    c[5] = 700.0
    c[11] = float(int(c.sum()) // 2)          # one EC with a third of all reads
    with np.errstate(divide="ignore"):
        logc = np.log(c)
    a0 = rng.uniform(1.0, 2.0, G)
    L = np.full((G, E), np.log(0.01))
    L[grp, np.repeat(np.arange(E), lens)] = lut[grp, cnt]
    n = 25
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, lut, np.log(0.01), G)
        li = core.layout_info()
        assert li["n_long_ecs"] == 2 and sum(li["slices_by_lanes"][:6]) > 0
        f = core.solve(logc, a0, tol=-1.0, max_iters=n, algo=ALGO_EM, prec=PREC_FLOAT)
        assert core.last_timing()["em_float_kernels"] == 1
        o = oracle.em_dense_f32(L, logc, a0, tol=-1.0, max_iters=n)
        r, a = _rel_above(f["theta"], o["theta"])
        print(f"mixed EC lengths, {n} float iterations: worst rel err {r:.2e}, abs {a:.2e}")
        assert r < 1e-4 and a < 1e-7
        # bootstrap replicates under --emprecision float: finite, normalised, close to the double replicates
        w = np.maximum(c, 1).astype(np.uint32)
        tf, itf = core.bootstrap(w, 7, int(w.sum()), 0, 3, a0, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=200)
        td, itd = core.bootstrap(w, 7, int(w.sum()), 0, 3, a0, algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=200)
        assert np.all(np.isfinite(tf)) and np.all(np.abs(tf.sum(1) - 1.0) < 1e-5)
        assert np.all(itf <= itd) and np.max(np.abs(tf - td)) < 5e-2
    monkeypatch.setenv("MSWEEP_RECORD_BYTES", "8")
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, lut, np.log(0.01), G)
        assert core.layout_info()["record_bytes"] == 8
        f8 = core.solve(logc, a0, tol=-1.0, max_iters=n, algo=ALGO_EM, prec=PREC_FLOAT)
        assert core.last_timing()["em_float_kernels"] == 0
        d8 = core.solve(logc, a0, tol=-1.0, max_iters=n, algo=ALGO_EM, prec=PREC_DOUBLE)
        np.testing.assert_array_equal(f8["theta"], d8["theta"])
