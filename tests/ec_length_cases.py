"""Shared by tests/test_gpu_ec_length_boundaries.py: the inputs of its cases, built the same way for every EC length,
and the SELL geometry restated from the host code, so that a case can say which path its ECs take.

The sweeps, the packers and the fp32 EM kernels change strategy at fixed numbers of cells of an EC:
  16 m, m = 1, 2, .. 64    lanes per EC (sell.hpp slice_class_of: the smallest m with cells <= 16 m): 16 | 17 .. 512 | 513
  ceil(cells / m)          rows of a slice, worked through two at a time; load_slice makes the missing last row of an odd
                           slice in registers: 1, 2, odd | even, 15 | 16
  cells mod m != 0         the last row of a multi-lane EC partly filled: 17, 31, 33, 1023
  8                        rows pass B's short-slice instantiation holds (RC = 8); longer slices stream in chunks of 8
  1024 (256)               kLongRow (kLongRowOneLane, MSWEEP_MULTILANE=0): beyond it a wavefront per EC
  256, 512                 a quad of 4 x 64 cells, a step of kLongStep x 64 cells on that path: 1280 | 1281, 1536 | 1537,
                           2048 | 2049
  kColdRows = 2            index records: cold cells per EC a slice's cold segment holds; beyond, nhot = 0
  32                       deferred logarithms of one wavefront before flush_logs() on the wavefront-per-EC path
"""
import numpy as np

from msweep_amd.likelihood import precalc_lls

LOGZI = np.log(0.01)
G_UNIFORM = 2200             # 2049 cells fit; narrow records with the tables in LDS (asserted through layout_info)
ROWS_PER_LANE = 16           # kRowsPerLane (sell.hpp)
LONG_ROW, LONG_ROW_ONE_LANE = 1024, 256      # kLongRow, kLongRowOneLane (sell.hpp)
COLD_ROWS = 2                # kColdRows (sell.hpp)
PASS_B_WAVES = 12            # kPassThreadsB / 64 (common.hpp)
PASS_A_WAVES = 16            # kPassThreads / 64
HYBRID_HOT = 16              # MSWEEP_HYBRID_HOT of the index-record cases
VALUE_RECORDS_ABOVE = 65536  # kCompressShared (host_compress.inc): more distinct listed values -> value records

PART_A = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024,
          1025, 1087, 1088, 1089, 1280, 1281, 1536, 1537, 2048, 2049)
PART_B = (1, 7, 8, 9, 15, 16)
PART_C = (1, 2, 15, 16, 17, 33, 1024, 1025, 1281)
PART_C_VALUE = tuple(L for L in PART_C if L != 33)
PART_C_COLD = tuple((L, k) for L in (3, 16) for k in (0, 1, 2, 3))
PART_D = (16, 17, 31, 32, 33, 255, 256, 257, 513)
PART_E = (1, 2, 16, 17, 33, 1024, 1025, 1281)
PART_E_INDEX = (2, 17, 1025)
ALSO_ONE_AND_PER = (1, 16, 17, 1024, 1025)   # lengths that also take a single EC and exactly one full slice


def long_row(multilane=True, env=None):
    """reset_likelihood (host_likelihood.inc): ECs of more cells take the wavefront-per-EC path; env = MSWEEP_LONG_ROW"""
    lr = LONG_ROW if multilane else LONG_ROW_ONE_LANE
    return lr if env is None else min(max(env, 16), lr)


def lanes(L, multilane=True):
    """slice_class_of (sell.hpp): lanes an EC of L cells takes in its slice"""
    m = 1
    while multilane and m < 64 and L > ROWS_PER_LANE * m:
        m *= 2
    return m


def per_slice(L, multilane=True, env_long_row=None):
    """ECs a slice of the class holds; 1 for the wavefront-per-EC path"""
    return 1 if L > long_row(multilane, env_long_row) else 64 // lanes(L, multilane)


def ec_counts_of(L, multilane=True):
    """n_ecs of the cases of one length: one full slice and a slice of one EC; five full slices and three ECs; for the
    lengths of ALSO_ONE_AND_PER a single EC and exactly one full slice"""
    per = per_slice(L, multilane)
    n = [per + 1, 5 * per + 3]
    if L in ALSO_ONE_AND_PER:
        n = [1, per] + n
    return sorted(set(n))


def case_ids(lengths, multilane=True):
    return [(L, n) for L in lengths for n in ec_counts_of(L, multilane)]


def min_held(n_ecs, per):
    """Iterations a case has to stay in lock-step (test_gpu_group_boundaries.conditioned_iters on the oracle's trace): 4
    when it has more ECs than a slice of its class holds; 3 for the problems of two ECs, which the stop rule ends there
    (tests/test_gpu_ec_length_boundaries.py says why); a single slice's worth of ECs or less: what there is."""
    return 1 if n_ecs <= per else (3 if n_ecs == 2 else 4)


def expected_layout(lens, multilane=True, env_long_row=None):
    """slices_by_lanes, max_rows, n_long_ecs, n_slices of layout_info for ECs of these lengths (make_slice_classes,
    upload_sell: a slice has the rows of its longest EC, ceil(cells / m))"""
    lens = np.asarray(lens)
    lr = long_row(multilane, env_long_row)
    by_lanes, max_rows = [0] * 7, 0
    for m_log in range(7):
        m = 64 >> m_log
        mine = [int(n) for n in lens if n <= lr and lanes(int(n), multilane) == m]
        per = 64 // m
        by_lanes[m_log] = -(-len(mine) // per)
        if mine:
            max_rows = max(max_rows, -(-max(mine) // m))
    return dict(slices_by_lanes=by_lanes, max_rows=max_rows, n_long_ecs=int(np.sum(lens > lr)), n_slices=sum(by_lanes))


def passB_wavefronts(n_slices, n_long, n_cu):
    """Wavefronts of pass B's launch, restated from finish_sell (host_likelihood.inc): nblk = max(1, min(max(ceil(n_slices
    / 16), n_long), n_cu)) workgroups of kPassThreadsB = 768 threads.  Wavefront w takes the long ECs w, w + nw, ..."""
    nblk = max(1, min(max(-(-n_slices // PASS_A_WAVES), n_long), n_cu))
    return nblk * PASS_B_WAVES


def distinct_groups(rng, n_ecs, G, L):
    """L of G groups per EC, drawn without replacement, sorted: [n_ecs, L]"""
    r = rng.random((n_ecs, G))
    pick = np.argpartition(r, L - 1, axis=1)[:, :L] if L < G else np.tile(np.arange(G), (n_ecs, 1))
    return np.sort(pick, axis=1)


def multiplicities(rng, n_ecs, small_only=False):
    """A fifth zero (logc = -inf); one fractional and one of exactly 255 -- the escape byte kC8Escape itself -- whenever
    n_ecs >= 5; the rest 1..15: the deferred-logarithm path.  small_only: 1..15 throughout."""
    counts = rng.integers(1, 16, n_ecs).astype(np.float64)
    if not small_only:
        order = rng.permutation(n_ecs)
        nz = n_ecs // 5
        counts[order[:nz]] = 0.0
        if n_ecs >= 5:
            counts[order[nz]] += 0.5
            counts[order[nz + 1]] = 255.0
    with np.errstate(divide="ignore"):
        return counts, np.log(counts)


def _csr_case(rng, G, sizes, rowptr, grp, cnt, counts, logc):
    lut = precalc_lls(sizes)
    grp, cnt = grp.astype(np.uint32), cnt.astype(np.uint32)
    return dict(G=G, E=len(rowptr) - 1, sizes=sizes, rowptr=rowptr.astype(np.uint64), grp=grp, cnt=cnt, lut=lut,
                lutidx=(grp * np.uint32(lut.shape[1]) + cnt).astype(np.uint32), counts=counts, logc=logc,
                alpha0=rng.uniform(0.5, 2.0, G))


def uniform_case(L, n_ecs, seed=None, G=G_UNIFORM, small_only=False):
    """n_ecs ECs of exactly L cells: groups without replacement, sorted; group sizes 1 + Poisson(4); hit counts uniform
    in 1..size; multiplicities as above; a prior uniform in [0.5, 2].  The same generators for every length."""
    rng = np.random.default_rng(100003 * L + n_ecs if seed is None else seed)
    sizes = (1 + rng.poisson(4, G)).astype(np.uint64)
    grp = distinct_groups(rng, n_ecs, G, L).ravel()
    cnt = rng.integers(1, sizes[grp].astype(np.int64) + 1)
    counts, logc = multiplicities(rng, n_ecs, small_only)
    c = _csr_case(rng, G, sizes, np.arange(n_ecs + 1) * L, grp, cnt, counts, logc)
    c["L"] = L
    return c


def mixture_case(seed=7, G=G_UNIFORM):
    """Part F: two empty ECs, one of them counted, among ECs of 1, 16, 17 and 1025 cells in shuffled order: every class
    boundary inside one permutation (the wavefront-per-EC part, slices of two lanes per EC, a 16-row slice that ends
    in ECs of one cell, a last slice that ends in the empty ECs)."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 0] + [1] * 40 + [16] * 40 + [17] * 33 + [1025] * 3)
    rng.shuffle(lens)
    sizes = (1 + rng.poisson(4, G)).astype(np.uint64)
    grp = np.concatenate([distinct_groups(rng, 1, G, int(n))[0] for n in lens if n]).astype(np.int64)
    cnt = rng.integers(1, sizes[grp].astype(np.int64) + 1)
    counts, logc = multiplicities(rng, len(lens))
    empty = np.nonzero(lens == 0)[0]
    counts[empty] = [3.0, 0.0]
    with np.errstate(divide="ignore"):
        logc = np.log(counts)
    c = _csr_case(rng, G, sizes, np.concatenate([[0], np.cumsum(lens)]), grp, cnt, counts, logc)
    c["lens"] = lens
    return c


def set_csr(core, c):
    core.set_csr(c["rowptr"], c["grp"], c["cnt"], c["lut"], LOGZI, c["G"])


def csr_oracle(oracle, c, iters, **kw):
    return oracle.rcg_optl_csr(c["rowptr"], c["grp"], c["lutidx"], c["lut"], LOGZI, c["G"], c["logc"], c["alpha0"], tol=-1.0,
                               max_iters=iters, **kw)


def dense_of(c):
    """the dense G x E matrix of a CSR case"""
    L = np.full((c["G"], c["E"]), LOGZI)
    cols = np.repeat(np.arange(c["E"]), np.diff(c["rowptr"].astype(np.int64)))
    L[c["grp"], cols] = c["lut"][c["grp"], c["cnt"]]
    return L


# ---- index records: which cells are cold, worked out from the frequencies -------------------------------------------

def cold_cells(c, n_hot=HYBRID_HOT):
    """Per cell: is its table entry NOT among the LDS-resident ones?  Restated from set_csr_impl and plan_slot_area
    (host_likelihood.inc): groups of equal size share a table row (numbered by first appearance), a cell's slot is
    row * width + hit count, the used slots are ordered by descending use -- ties by ascending slot -- and the first
    n_hot of them live in LDS, or as many whole sixteens as there are (choose_hybrid_layout, host_layout.inc: the table's
    image is cut in units of 16 entries -- an area of fewer than 16 entries stays in memory as a whole)."""
    sizes = c["sizes"]
    _, first, inv = np.unique(sizes, return_index=True, return_inverse=True)
    row = np.argsort(np.argsort(first))[inv]
    slot = row[c["grp"]].astype(np.int64) * c["lut"].shape[1] + c["cnt"]
    used, freq = np.unique(slot, return_counts=True)
    hot = used[np.argsort(-freq, kind="stable")[:min(n_hot, len(used) // 16 * 16)]]
    return ~np.isin(slot, hot)


def cold_class(n_cold):
    """pack_kernels.hpp cold_class"""
    return 0 if n_cold == 0 else (1 if n_cold <= 2 else (2 if n_cold <= COLD_ROWS else 3))


def index_rows_from_memory(c, n_hot=HYBRID_HOT):
    """rows_from_memory of layout_info for a uniform case under index records (upload_sell): the ECs of equal length are
    ordered by cold class (ECs of up to 16 cells; stable), cut into slices of `per`; a slice's cold segment has as many
    rows as its lane with the most cold cells -- lane t of an EC holds its cells t, t + m, .. -- and a slice with more
    than kColdRows of them takes every row from memory (nhot = 0).  Long ECs are in no slice."""
    L, n = c["L"], c["E"]
    if L > LONG_ROW:
        return 0
    cold = cold_cells(c, n_hot).reshape(n, L)
    m = lanes(L)
    rows, per = -(-L // m), 64 // m
    cls = [cold_class(int(x)) if L <= 16 else 0 for x in cold.sum(1)]
    perm = np.argsort(cls, kind="stable")
    total = 0
    for s0 in range(0, n, per):
        mc = max(int(cold[j, t::m].sum()) for j in perm[s0:s0 + per] for t in range(m))
        total += rows if mc > COLD_ROWS else mc
    return total


COLD_HOT_SIZES, COLD_HOT_COUNTS, COLD_HOT_GROUPS = (4, 5, 6, 7), (1, 2, 3, 4), 32


def cold_case(L, k, n_ecs):
    """n_ecs ECs of L cells with exactly k cold cells each under MSWEEP_HYBRID_HOT=16: 32 groups of the sizes 4..7 hit
    1..4 times -- 16 heavily used (size, count) pairs, the LDS-resident entries -- and a pool of groups of distinct sizes
    from 100 on, each used once with its own (size, count) pair.  L - k cells of an EC come from the first, k from the pool.

    k = L: the 16 LDS-resident entries are the 16 most used ones whatever the input, so some cell has to use them: 16
    further ECs of hot cells alone carry them (they sort in front and share the first slice, which still has ECs of k
    cold cells: nhot = 0 there as in every other slice).  The test asserts what cold_cells() finds per EC."""
    rng = np.random.default_rng(7919 * L + 31 * k + n_ecs)
    n_carry = 16 if k == L else 0
    n_pool = k * n_ecs
    G = COLD_HOT_GROUPS + n_pool
    sizes = np.concatenate([np.repeat(COLD_HOT_SIZES, COLD_HOT_GROUPS // 4), 100 + np.arange(n_pool)]).astype(np.uint64)
    grp, cnt = [], []
    pool = COLD_HOT_GROUPS + rng.permutation(n_pool)
    for j in range(n_ecs):
        g = np.concatenate([rng.choice(COLD_HOT_GROUPS, L - k, replace=False), pool[j * k:(j + 1) * k]]).astype(np.int64)
        g.sort()
        grp.append(g)
        cnt.append(np.where(g < COLD_HOT_GROUPS, rng.integers(1, 5, L), rng.integers(1, sizes[g].astype(np.int64) + 1)))
    for j in range(n_carry):         # cell i of carrier j: pair (j L + i) mod 16, each pair L times; distinct groups (L <= 8)
        pair = (j * L + np.arange(L)) % 16
        g = (pair // 4) * (COLD_HOT_GROUPS // 4) + (j + np.arange(L)) % (COLD_HOT_GROUPS // 4)
        order = np.argsort(g)
        grp.append(g[order])
        cnt.append((1 + pair % 4)[order])
    E = n_ecs + n_carry
    counts, logc = multiplicities(rng, E)
    c = _csr_case(rng, G, sizes, np.arange(E + 1) * L, np.concatenate(grp), np.concatenate(cnt), counts, logc)
    c.update(L=L, k=k, n_carry=n_carry)
    return c


# ---- value records ------------------------------------------------------------------------------------------------

def value_case(L):
    """A dense logl with L continuous values per column over the background, E = ceil(65600 / L) columns -- more than
    kCompressShared = 65536 distinct listed values, where value records engage -- and G = 4 L + 3 groups, so that
    4 nnz <= G E and the matrix is re-expressed at all (host_compress.inc)."""
    rng = np.random.default_rng(5003 * L)
    E, G = -(-65600 // L), 4 * L + 3
    rows = distinct_groups(rng, E, G, L)
    vals = rng.uniform(-12.0, -0.1, (E, L))
    assert len(np.unique(vals)) == E * L > VALUE_RECORDS_ABOVE and 4 * E * L <= G * E
    logl = np.full((G, E), LOGZI)
    logl[rows, np.arange(E)[:, None]] = vals
    counts, logc = multiplicities(rng, E)
    return dict(L=L, G=G, E=E, logl=logl, counts=counts, logc=logc, alpha0=rng.uniform(0.5, 2.0, G))
