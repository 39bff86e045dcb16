"""GPU: distinct handles may be used concurrently from distinct threads (include/msweep_core.h).  Two Cores in two
Python threads -- ctypes releases the GIL for the length of a call -- each read a different alignment from text, build,
solve and format the probabilities, started together on a barrier; the results are those of the same calls made one after
the other.  The two likelihoods differ in their number of groups (4 and 39), so the two solves ask for different amounts of
dynamic LDS for the same sweep kernels.  Then one thread's text is malformed: its error arrives on that thread and the
other thread's results are untouched."""
import gzip
import threading

import numpy as np
import pytest

from msweep_amd import synth
from msweep_amd.core import TEXT_PROBS, Core, MswError
from test_gpu_cli_toy import _toy

pytestmark = pytest.mark.gpu


def _work(core, files, indicators, sizes, rounds=1):
    """read from text, build, solve, text_block -- `rounds` times on the one handle; the last round's results"""
    for _ in range(rounds):
        aln = core.read_alignment(files, len(indicators))
        n_kept, mask, _ = core.build_likelihood_aln(aln, indicators, sizes, want_logc=False)
        res = core.solve(None, np.ones(n_kept))
        text = core.text_block(TEXT_PROBS, 0, aln.n_ecs)
        counts = aln.ec_counts().copy()
        aln.close()
        core.trim()
    return dict(theta=res["theta"], iters=res["iters"], bound=res["bound"], text=text, counts=counts, mask=mask)


def _same(a, b):
    assert a["iters"] == b["iters"] and a["bound"] == b["bound"] and a["text"] == b["text"] and len(a["text"]) > 1000
    np.testing.assert_array_equal(a["theta"], b["theta"])
    np.testing.assert_array_equal(a["counts"], b["counts"])
    np.testing.assert_array_equal(a["mask"], b["mask"])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    root = tmp_path_factory.mktemp("two_handles")
    _toy(root)
    clusters = (root / "clustering.txt").read_text().split("\n")[:-1]
    ids = {n: i for i, n in enumerate(dict.fromkeys(clusters))}
    four = (np.array([ids[c] for c in clusters], np.uint32), np.bincount([ids[c] for c in clusters]).astype(np.uint64))
    each = (np.arange(39, dtype=np.uint32), np.ones(39, np.uint64))
    prob = synth.make_csr_problem(3000, 4, seed=5, max_other=3, group_sizes=lambda rng, G: np.array([12, 9, 10, 8], np.uint64))
    aln = synth.csr_to_targets(prob)
    ec_of = np.random.default_rng(5).permutation(np.repeat(np.arange(len(prob["ec_counts"]), dtype=np.int64),
                                                           prob["ec_counts"].astype(np.int64)))
    synth.write_themisto(str(root / "large.txt"), ec_of, aln["ec_tptr"], aln["ec_targets"])
    (root / "large.txt.gz").write_bytes(gzip.compress((root / "large.txt").read_bytes()))
    (root / "bad.txt").write_text("0 1\n12 34 x\n2 3\n")
    # thread 0: the toy (paired, plain) in four groups; thread 1: the larger sample (gzip) with every sequence a group
    return dict(jobs=[([str(root / "toy_1.txt"), str(root / "toy_2.txt")], *four), ([str(root / "large.txt.gz")], *each)],
                bad=[str(root / "bad.txt")])


@pytest.fixture(scope="module")
def one_after_the_other(inputs):
    out = []
    for job in inputs["jobs"]:
        with Core(0) as core:
            out.append(_work(core, *job))
    assert out[0]["text"] != out[1]["text"]
    return out


def _in_threads(jobs):
    """jobs: callables taking a Core; each on a thread and a handle of its own, started together -> results / exceptions"""
    cores = [Core(0) for _ in jobs]
    barrier = threading.Barrier(len(jobs))
    out = [None] * len(jobs)

    def run(k):
        try:
            barrier.wait(timeout=60)
            out[k] = jobs[k](cores[k])
        except Exception as ex:      # handed to the test's thread
            out[k] = ex
    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in cores:
        c.close()
    return out


def test_two_handles_in_two_threads(inputs, one_after_the_other):
    got = _in_threads([lambda core, job=job: _work(core, *job, rounds=3) for job in inputs["jobs"]])
    for g, want in zip(got, one_after_the_other):
        assert not isinstance(g, Exception), g
        _same(g, want)


def test_a_larger_layout_after_a_smaller_one_on_the_other_handle(inputs, one_after_the_other):
    """one thread: the handles take turns, so each solve follows one that asked for another amount of LDS"""
    with Core(0) as a, Core(0) as b:
        for _ in range(2):
            _same(_work(a, *inputs["jobs"][0]), one_after_the_other[0])
            _same(_work(b, *inputs["jobs"][1]), one_after_the_other[1])
            _same(_work(b, *inputs["jobs"][0]), one_after_the_other[0])
            _same(_work(a, *inputs["jobs"][1]), one_after_the_other[1])


def test_an_error_stays_on_its_thread(inputs, one_after_the_other):
    with Core(0) as core:
        with pytest.raises(MswError) as alone:
            core.read_alignment(inputs["bad"], 39)
    assert len(str(alone.value)) > 10

    def bad(core):
        for _ in range(3):
            try:
                core.read_alignment(inputs["bad"], 39)
            except MswError as ex:
                last = ex
            else:
                raise AssertionError("the malformed text was read")
        raise last
    got = _in_threads([lambda core: _work(core, *inputs["jobs"][1], rounds=3), bad])
    assert not isinstance(got[0], Exception), got[0]
    _same(got[0], one_after_the_other[1])
    assert isinstance(got[1], MswError) and str(got[1]) == str(alone.value)
