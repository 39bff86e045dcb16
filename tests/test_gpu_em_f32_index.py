"""GPU: `--algorithm emgpu --emprecision float` on INDEX-RECORD layouts (sell.hpp ENC 2: groupings with sizes up to
hundreds, whose fp64 slot table does not fit LDS and is kept as the hybrid area) served by the fp32 sweep
k_em_passB_f32_idx (msweep_amd/csrc/em_f32_kernels.hpp): the float image of the WHOLE slot area sits in LDS, both record
forms of a slice address it.  Every case asserts index records AND msw_timing::em_float_kernels == 1 right after the
float solve: none can pass through the fp64 kernels.  Tolerances are those of test_gpu_bootstrap_em.py
test_emprecision_float_is_fp32_arithmetic for two fp32 evaluation orders of one arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, dense_from_csr
from msweep_amd import synth
from msweep_amd.core import ALGO_EM, ALGO_RCG, PREC_DOUBLE, PREC_FLOAT, Core
from msweep_amd.likelihood import from_device_alignment, from_grouped_counts, precalc_lls
from test_gpu_cli_toy import _parse, mini_binary  # noqa: F401  (mini_binary: the fixture that builds msweep_mini)

pytestmark = pytest.mark.gpu

N_FIX = 25                      # fixed iterations of the parity runs
TRACED = (0, 4, 19, N_FIX - 1)  # iterations whose weights are compared


def _rel_above(got, ref, floor=1e-4):
    big = ref >= floor
    return float(np.max(np.abs(got - ref)[big] / ref[big], initial=0.0)), float(np.max(np.abs(got - ref)[~big], initial=0.0))


def _index_float(core):
    """The two facts every case stands on, read right after a float solve."""
    li = core.layout_info()
    assert li["index_records"] == 1, li
    assert core.last_timing()["em_float_kernels"] == 1
    return li


def _fixed_float(core, logc, a0, n=N_FIX):
    core.set_trace_theta(n)
    f = core.solve(logc, a0, tol=-1.0, max_iters=n, algo=ALGO_EM, prec=PREC_FLOAT)
    li = _index_float(core)
    tr = core.trace(n, with_theta=True)
    core.set_trace_theta(0)
    return f, tr, li


def _assert_fp32_parity(what, f, tr, ref_theta, ref_trace, ref_bound, traced=TRACED, bound=True, unit_sum=True):
    """f / tr: a fixed-iteration float solve and its trace; ref_*: the same iterations of another fp32 evaluation.
    bound / unit_sum = False (test_gpu_guard.py, priors below one): without the log-likelihood within four float
    spacings / the weights adding up to 1 within 1e-5."""
    for k in traced:
        r, a = _rel_above(tr["theta"][k], ref_trace[k])
        print(f"{what}: iteration {k}: worst rel err {r:.2e} (abs below 1e-4: {a:.2e})")
        assert r < 1e-4 and a < 1e-7, (what, k, r, a)
    if ref_theta is not None:
        r, a = _rel_above(f["theta"], ref_theta)
        print(f"{what}: result: worst rel err {r:.2e} (abs below 1e-4: {a:.2e}); log-likelihood {f['bound']!r} / {ref_bound!r}")
        assert r < 1e-4 and a < 1e-7, (what, r, a)
        if bound:
            assert abs(f["bound"] - ref_bound) <= 4 * np.spacing(np.float32(abs(ref_bound)))
    assert f["bound"] == float(np.float32(f["bound"]))          # the log-likelihood IS a float
    assert np.all(f["theta"] == f["theta"].astype(np.float32))  # and so are the weights
    if unit_sum:
        assert abs(f["theta"].sum() - 1.0) < 1e-5


@pytest.fixture(scope="module")
def prob21(oracle):
    """The shape test_gpu_hybrid.py shows to be index records under MSWEEP_FORCE_LDS=10, and its fp32 oracle runs
    (they do not depend on the layout: computed once)."""
    G = 500
    p = synth.make_csr_problem(60_000, G, seed=21, max_other=12, group_sizes=synth.diverse_group_sizes)
    L = dense_from_csr(p, precalc_lls(p["group_sizes"]))
    logc = np.log(p["ec_counts"].astype(float))
    a0 = np.ones(G)
    o_fix = oracle.em_dense_f32(L, logc, a0, tol=-1.0, max_iters=N_FIX, trace=N_FIX)
    o_tol = oracle.em_dense_f32(L, logc, a0, max_iters=5000)
    return dict(p=p, G=G, logc=logc, a0=a0, o_fix=o_fix, o_tol=o_tol)


def _load(core, p):
    return from_grouped_counts(core, p["rowptr"], p["grp"], p["cnt"], p["ec_counts"], p["group_sizes"])


@pytest.mark.parametrize("hot", [0, 48, 4096])
def test_float_on_forced_index_layouts_matches_the_fp32_oracle(prob21, monkeypatch, hot):
    """All rows in the plain record form (hot = 0), a mixed hot / cold cut (48), every entry hot (4096 > the area)."""
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", str(hot))
    q = prob21
    with Core(0) as core:
        _load(core, q["p"])
        f, tr, li = _fixed_float(core, q["logc"], q["a0"])
        print(li)
        assert li["slot_entries_in_lds"] == min(hot, li["slot_entries"]) // 16 * 16
        if hot == 48:
            assert 0 < li["rows_from_memory"] < li["rows"]      # (the fp64 sweeps' view: the cut is really mixed)
        o = q["o_fix"]
        _assert_fp32_parity(f"hot {hot}", f, tr, o["theta"], o["theta_trace"], o["bound"])
        if hot == 48:
            # the stop: the float log-likelihood stops growing at float resolution, a fraction of the double run's count
            ft = core.solve(q["logc"], q["a0"], algo=ALGO_EM, prec=PREC_FLOAT, max_iters=5000)
            _index_float(core)
            d = core.solve(q["logc"], q["a0"], algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=5000)
            assert core.last_timing()["em_float_kernels"] == 0
            ot = q["o_tol"]
            print(f"to --tol 1e-6: float {ft['iters']} iterations (fp32 oracle {ot['iters']}), double {d['iters']}")
            assert abs(int(ft["iters"]) - int(ot["iters"])) <= max(6, int(0.15 * ot["iters"]))
            assert ft["iters"] < 0.6 * d["iters"] and ot["iters"] < 0.6 * d["iters"]


def test_float_on_the_natural_hybrid_layout(oracle, monkeypatch):
    """No override: the fp64 passes are hybrid (a part of the slot area in LDS, the rest in memory) while the float image
    holds all of it.  The dense oracle is too slow for 25 iterations at this size: the natural layout against the all-cold
    decode of the same problem (whose oracle parity the forced case establishes) -- two evaluation orders of one
    arithmetic -- and against the fp32 oracle for the first two iterations."""
    G = 4000
    p = synth.make_csr_problem(100_000, G, seed=21, max_other=12, group_sizes=synth.diverse_group_sizes)
    logc = np.log(p["ec_counts"].astype(float))
    a0 = np.ones(G)
    with Core(0) as core:
        _load(core, p)
        f, tr, li = _fixed_float(core, logc, a0)
        print(li)
        assert 0 < li["slot_entries_in_lds"] < li["slot_entries"], li
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "0")
    with Core(0) as core:
        _load(core, p)
        fc, trc, lic = _fixed_float(core, logc, a0)
        assert lic["slot_entries_in_lds"] == 0, lic
    _assert_fp32_parity("natural / all-cold", f, tr, fc["theta"], trc["theta"], fc["bound"])
    L = dense_from_csr(p, precalc_lls(p["group_sizes"]))
    o2 = oracle.em_dense_f32(L, logc, a0, tol=-1.0, max_iters=2, trace=2)
    del L
    _assert_fp32_parity("natural / fp32 oracle", f, tr, None, o2["theta_trace"], None, traced=(0, 1))


@pytest.mark.parametrize("multilane", ["1", "0"])
def test_float_on_index_records_with_other_ec_shapes(oracle, monkeypatch, multilane):
    """Index records AND ECs of 17..256 cells (slices of several lanes per EC; MSWEEP_MULTILANE=0: the streaming
    branch), a few beyond 256 (a wavefront each), a fifth of the ECs with count zero, a count beyond a byte, one EC
    holding a third of all reads (the two-part fixed-point adds)."""
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "256")
    monkeypatch.setenv("MSWEEP_MULTILANE", multilane)
    rng = np.random.default_rng(8)
    G, E = 600, 4000
    sizes = np.minimum(1 + rng.lognormal(3.0, 1.2, G).astype(np.int64), 400).astype(np.uint64)
    lens = rng.integers(0, 17, E)
    lens[rng.choice(E, 1500, replace=False)] = rng.integers(17, 257, 1500)
    lens[rng.choice(E, 6, replace=False)] = rng.integers(257, 500, 6)
    lut = precalc_lls(sizes)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    grp = np.concatenate([np.sort(rng.choice(G, k, replace=False)) for k in lens]).astype(np.uint32)
    cnt = rng.integers(1, sizes[grp] + 1).astype(np.uint32)
    c = rng.integers(1, 40, E).astype(float)
    c[rng.random(E) < 0.2] = 0.0
    c[5] = 700.0
    c[11] = float(int(c.sum()) // 2)          # one EC with a third of all reads
    with np.errstate(divide="ignore"):
        logc = np.log(c)
    a0 = rng.uniform(1.0, 2.0, G)
    L = np.full((G, E), np.log(0.01))
    L[grp, np.repeat(np.arange(E), lens)] = lut[grp, cnt]
    with Core(0) as core:
        core.set_csr(rowptr, grp, cnt, lut, np.log(0.01), G)
        f, tr, li = _fixed_float(core, logc, a0)
        assert li["slot_entries_in_lds"] == 256, li
        assert (li["n_long_ecs"] > 0) == (multilane == "0")     # (beyond 256 cells: a wavefront each when every EC is one lane)
        assert (sum(li["slices_by_lanes"][:-1]) > 0) == (multilane == "1")
    o = oracle.em_dense_f32(L, logc, a0, tol=-1.0, max_iters=N_FIX, trace=N_FIX)
    _assert_fp32_parity(f"ragged, multilane {multilane}", f, tr, o["theta"], o["theta_trace"], o["bound"])


def test_float_is_float_and_leaves_nothing_behind(prob21, monkeypatch):
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    monkeypatch.setenv("MSWEEP_HYBRID_HOT", "48")
    q = prob21
    logc, a0 = q["logc"], q["a0"]
    with Core(0) as core:                      # a handle that never ran float
        _load(core, q["p"])
        d0 = core.solve(logc, a0, algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=300)
        r0 = core.solve(logc, a0, algo=ALGO_RCG)
    with Core(0) as core:
        _load(core, q["p"])
        f = core.solve(logc, a0, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=300)
        _index_float(core)
        d = core.solve(logc, a0, algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=300)
        assert core.last_timing()["em_float_kernels"] == 0
        r = core.solve(logc, a0, algo=ALGO_RCG)
        # float is not double ...
        assert np.max(np.abs(f["theta"] - d["theta"])) > 1e-7
        # ... and the float run leaves no state behind: the same bits as on the fresh handle
        assert d["iters"] == d0["iters"] and r["iters"] == r0["iters"]
        np.testing.assert_array_equal(d["theta"], d0["theta"])
        np.testing.assert_array_equal(r["theta"], r0["theta"])
        # the developer switch still puts the flag on the fp64 kernels: the double run's bits
        monkeypatch.setenv("MSWEEP_EM_FLOAT_AS_DOUBLE", "1")
        fd = core.solve(logc, a0, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=300)
        assert core.last_timing()["em_float_kernels"] == 0
        assert fd["iters"] == d["iters"]
        np.testing.assert_array_equal(fd["theta"], d["theta"])
        monkeypatch.delenv("MSWEEP_EM_FLOAT_AS_DOUBLE")
        # bootstrap replicates under float on the index layout
        w = q["p"]["ec_counts"].astype(np.uint32)
        tf, itf = core.bootstrap(w, 7, int(w.sum()), 0, 3, a0, algo=ALGO_EM, prec=PREC_FLOAT, max_iters=300)
        td, itd = core.bootstrap(w, 7, int(w.sum()), 0, 3, a0, algo=ALGO_EM, prec=PREC_DOUBLE, max_iters=300)
        assert np.all(np.isfinite(tf)) and np.all(np.abs(tf.sum(1) - 1.0) < 1e-5)
        assert np.all(itf <= itd), (itf, itd)
        # (msw_timing describes the handle's last SOLVE, not the replicates' workers: that these ran the fp32 kernels
        # shows in their weights, which are floats -- the double replicates' are not)
        assert np.all(tf == tf.astype(np.float32)) and not np.all(td == td.astype(np.float32))


def _toy_diverse(tmp_path, n_reads=2500, seed=4):
    """A Themisto plaintext pair over 30 clusters of 2..120 reference sequences (a diverse grouping)."""
    rng = np.random.default_rng(seed)
    sizes = np.clip(1 + rng.lognormal(2.6, 1.0, 30).astype(int), 2, 120)
    names = [f"clust{k + 1}" for k in range(len(sizes))]
    indicators = [names[k] for k in range(len(sizes)) for _ in range(sizes[k])]
    order = rng.permutation(len(indicators))
    indicators = [indicators[i] for i in order]
    members = {n: [i for i, x in enumerate(indicators) if x == n] for n in names}
    theta = rng.dirichlet(np.full(len(sizes), 0.4))
    l1, l2 = [], []
    for r in range(n_reads):
        g = rng.choice(len(sizes), p=theta)
        hit = set(rng.choice(members[names[g]], max(1, rng.binomial(sizes[g], 0.65)), replace=False).tolist())
        for o in rng.choice(len(sizes), 3, replace=False):
            if o != g and rng.random() < 0.5:
                hit |= set(rng.choice(members[names[o]], max(1, rng.binomial(sizes[o], 0.15)), replace=False).tolist())
        h2 = sorted(hit) if rng.random() > 0.05 else []
        l1.append(" ".join(map(str, [r] + sorted(hit))))
        l2.append(" ".join(map(str, [r] + h2)))
    (tmp_path / "toy_1.txt").write_text("\n".join(l1) + "\n")
    (tmp_path / "toy_2.txt").write_text("\n".join(l2) + "\n")
    (tmp_path / "clustering.txt").write_text("\n".join(indicators) + "\n")


def test_drivers_float_on_an_index_layout(tmp_path, mini_binary, monkeypatch):  # noqa: F811
    """`python -m msweep_amd` and msweep_mini with --algorithm emgpu --emprecision float on an input whose likelihood is
    index records (MSWEEP_FORCE_LDS=10 in the children's environment; confirmed through Core on the same classes): the
    same abundances byte for byte, and not the --emprecision double file."""
    from msweep_amd.__main__ import parse
    from msweep_amd.reference import read_reference
    _toy_diverse(tmp_path)
    files = [str(tmp_path / "toy_1.txt"), str(tmp_path / "toy_2.txt")]
    common = ["--themisto-1", files[0], "--themisto-2", files[1], "-i", str(tmp_path / "clustering.txt"),
              "--algorithm", "emgpu"]
    env = dict(os.environ, MSWEEP_FORCE_LDS="10", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = {}
    for tag, driver in (("py", [sys.executable, "-m", "msweep_amd"]), ("cc", [mini_binary])):
        for prec in ("float", "double"):
            pre = str(tmp_path / f"{tag}_{prec}")
            r = subprocess.run(driver + common + ["--emprecision", prec, "-o", pre], capture_output=True, text=True,
                               timeout=300, env=env, cwd=ROOT)
            assert r.returncode == 0, r.stdout + r.stderr
            out[tag, prec] = open(pre + "_abundances.txt").read()
            assert len(out[tag, prec]) > 200
    assert out["py", "float"] == out["cc", "float"]
    assert out["py", "double"] == out["cc", "double"]
    assert out["py", "float"] != out["py", "double"]
    _, rows = _parse(str(tmp_path / "py_float_abundances.txt"))
    assert abs(sum(v[0] for _, v in rows) - 1.0) < 1e-4
    # the same classes through Core, the same environment: index records, served by the fp32 kernels
    monkeypatch.setenv("MSWEEP_FORCE_LDS", "10")
    a = parse(common)
    with open(a.indicators) as fh:
        grouping = read_reference(fh)
    with Core(0) as core:
        aln = core.read_alignment(files, len(grouping.group_indicators), a.themisto_mode)
        lik = from_device_alignment(core, aln, grouping.group_indicators, grouping.get_sizes(), a.q, a.e, a.zero_inflation,
                                    a.min_hits)
        core.solve(None, np.ones(lik.n_groups), a.tol, a.max_iters, ALGO_EM, PREC_FLOAT)
        _index_float(core)
