"""Shared by tests/test_gpu_group_boundaries.py: the inputs of its cases, built the same way for every group count, and
the launch geometry of the dense sweeps restated from the host code, so that a case can say which wavefront takes
which EC.

The kernels that run once per group (k_finstep, k_redfin, k_init_state, k_prepB, k_em_init / k_em_fin) and the dense
sweeps change strategy at fixed group counts:
  16                      groups per workgroup of k_redfin
  64                      a wavefront
  512, 1024               the thread blocks of the O(G) kernels
  k * 1024, k = 1..6      the register paths of k_finstep / k_em_fin hold group tid + k * nt (state_kernels.hpp)
  6144 = kStepRegs * 1024 the last group count of the register paths; beyond it they loop, and --emprecision float
                          is served by the fp64 kernels
  64 * nreg               the dense instantiation: nreg = the smallest power of two with 64 * nreg >= G; <1>..<16> hold
                          an EC in registers, <32>..<128> sweep it twice; beyond 8192 the matrix is re-expressed as CSR
"""
import numpy as np

from conftest import lutidx_of
from msweep_amd import synth
from msweep_amd.likelihood import precalc_lls

LOGZI = np.log(0.01)

# part A: both sides of every boundary of the O(G) chain
CSR_GROUPS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097,
              5120, 5121, 6143, 6144, 6145, 7168, 7169)
EM_GROUPS = (1, 2, 64, 65, 1024, 1025, 6144, 6145)
IN_REGS_MAX = 6144           # kStepRegs * 1024 (state_kernels.hpp)

# part C: both sides of every instantiation edge of the dense sweeps, at fewer ECs than a workgroup has wavefronts,
# partial 64 x 64 tiles of k_transpose in both directions, one and two workgroups
DENSE_GROUPS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
DENSE_TINY_ECS = (1, 3, 5, 67)
DENSE_MAX_GROUPS = 8192      # beyond: re-expressed as CSR-of-ECs whatever the shape (host_likelihood.inc)

# part D: the smallest group count of every instantiation (1024: the largest of <16>, whose smallest is in part C)
DENSE_REG_GROUPS = (1, 65, 129, 257, 513, 1024)       # <1> <2> <4> <8> <16> <16>
DENSE_BIG_GROUPS = (1025, 2049, 4097, 8192)           # <32> <64> <128> <128>


def csr_case(G, reads=4000, seed=3):
    """The CSR input of parts A and B at G groups: a fifth of the ECs with a zero count (logc = -inf), a prior that is
    not flat.  The same generators for every G, so neighbouring group counts are different problems of one family."""
    p = synth.make_csr_problem(reads, G, seed=seed, max_other=min(6, G - 1))
    rng = np.random.default_rng(seed)
    E = len(p["ec_counts"])
    counts = p["ec_counts"].astype(np.float64)
    counts[rng.choice(E, E // 5, replace=False)] = 0.0
    assert counts.sum() > 0
    alpha0 = rng.uniform(0.5, 2.0, G)
    with np.errstate(divide="ignore"):
        logc = np.log(counts)
    lut = precalc_lls(p["group_sizes"])
    return dict(p=p, G=G, E=E, logc=logc, alpha0=alpha0, lut=lut, lutidx=lutidx_of(p, lut))


def set_csr(core, c):
    p = c["p"]
    core.set_csr(p["rowptr"], p["grp"], p["cnt"], c["lut"], LOGZI, c["G"])


def csr_oracle(oracle, c, iters, **kw):
    p = c["p"]
    return oracle.rcg_optl_csr(p["rowptr"], p["grp"], c["lutidx"], c["lut"], LOGZI, c["G"], c["logc"], c["alpha0"], tol=-1.0,
                               max_iters=iters, trace=iters, **kw)


def dense_case(E, G, seed=3):
    """The dense input of parts C and D: counts 0..5 (zeros give logc = -inf; at least one is not), a prior that is
    not flat."""
    p = synth.make_dense_problem(E, G, seed=seed)
    counts = np.random.default_rng(1).integers(0, 6, E).astype(np.float64)
    if not counts.any():
        counts[0] = 1.0
    alpha0 = np.random.default_rng(seed).uniform(0.5, 2.0, G)
    with np.errstate(divide="ignore"):
        logc = np.log(counts)
    return dict(logl=p["logl"], G=G, E=E, counts=counts, logc=logc, alpha0=alpha0)


def dense_multi_ec_case(E, G, nw, seed=3):
    """dense_case for part D, with a zero count on a wavefront's SECOND EC (the ECs nw .. 2 nw - 1).  Where the counts
    of dense_case leave none there -- E = nw + 3 has three such ECs only -- the middle one of them gets it."""
    c = dense_case(E, G, seed)
    assert nw < E
    second = c["counts"][nw:min(2 * nw, E)]
    if second.all():
        second[len(second) // 2] = 0.0       # (a view: writes c["counts"])
        with np.errstate(divide="ignore"):
            c["logc"] = np.log(c["counts"])
    return c


def dense_nreg(G):
    """dense_from_stage (msweep_amd/csrc/host_likelihood.inc): the smallest power of two with 64 * nreg >= G"""
    nreg = 1
    while nreg * 64 < G:
        nreg *= 2
    return nreg


def dense_wavefronts(E, G, n_cu):
    """Wavefronts of one launch of the dense sweeps, restated from dense_from_stage (msweep_amd/csrc/host_likelihood.inc):
      nblk_dense = max(1, min((E + 3) / 4, n_cu * (nreg >= 32 ? 2 : 8))),  four wavefronts per workgroup.
    Wavefront w sweeps the ECs w, w + nw, w + 2 nw, ... (dense_kernels.hpp)."""
    per_cu = 2 if dense_nreg(G) >= 32 else 8
    return 4 * max(1, min((E + 3) // 4, n_cu * per_cu))


def dense_full_wavefronts(G, n_cu):
    """nw of a launch with at least one EC for every wavefront"""
    return 4 * n_cu * (2 if dense_nreg(G) >= 32 else 8)
