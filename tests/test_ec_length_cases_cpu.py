"""CPU: what the cases of tests/test_gpu_ec_length_boundaries.py presuppose of their inputs and of the oracle alone -- held
here, so that none of it is first found out on a GPU."""
import numpy as np
import pytest

import ec_length_cases as ec
from test_gpu_group_boundaries import conditioned_iters

ITERS = 8


@pytest.mark.parametrize("multilane,lengths", [(True, sorted(set(ec.PART_A + ec.PART_B + ec.PART_C + ec.PART_E))),
                                               (False, ec.PART_D)], ids=["multilane", "one_lane"])
def test_uniform_cases_and_the_iterations_the_oracle_allows(oracle, multilane, lengths):
    assert set(ec.PART_B + ec.PART_C + ec.PART_E + ec.PART_E_INDEX) <= set(ec.PART_A)
    for L, n in ec.case_ids(lengths, multilane):
        c = ec.uniform_case(L, n)
        cells = c["grp"].reshape(n, L).astype(np.int64)
        assert c["E"] == n and np.all(np.diff(cells, axis=1) > 0) and cells.max() < c["G"] == ec.G_UNIFORM
        assert np.all((c["cnt"] >= 1) & (c["cnt"] <= c["sizes"][c["grp"]]))
        counts = c["counts"]
        assert np.sum(counts == 0) == n // 5 and np.isneginf(c["logc"]).sum() == n // 5
        if n >= 5:
            assert np.sum(counts != np.rint(counts)) == 1 and np.sum(counts >= 255) == 1
        small = counts[(counts > 0) & (counts < 255) & (counts == np.rint(counts))]
        assert small.size == 0 or (small.min() >= 1 and small.max() <= 15)
        assert c["alpha0"].min() >= 0.5 and c["alpha0"].max() <= 2.0
        k = conditioned_iters(ec.csr_oracle(oracle, c, ITERS, trace=ITERS)["trace"], ITERS)
        assert k >= ec.min_held(n, ec.per_slice(L, multilane)), f"L = {L}, {n} ECs: {k} iterations"


def test_geometry_restated():
    assert [ec.lanes(L) for L in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert ec.lanes(256, multilane=False) == 1 and ec.per_slice(257, multilane=False) == 1 and ec.per_slice(1025) == 1
    assert ec.ec_counts_of(1) == [1, 64, 65, 323] and ec.ec_counts_of(17) == [1, 32, 33, 163]
    assert ec.ec_counts_of(1025) == [1, 2, 8] and ec.ec_counts_of(33) == [17, 83]
    geo = ec.expected_layout([0, 0, 1, 16, 17, 17, 1024, 1025])
    assert geo == dict(slices_by_lanes=[1, 0, 0, 0, 0, 1, 1], max_rows=16, n_long_ecs=1, n_slices=3)
    assert ec.long_row(env=16) == 16 and ec.long_row(multilane=False, env=4000) == 256
    assert ec.passB_wavefronts(0, 10**6, 256) == 256 * 12 and ec.passB_wavefronts(40, 0, 256) == 3 * 12


@pytest.mark.parametrize("n_ecs", [65, 323])
@pytest.mark.parametrize("L,k", ec.PART_C_COLD)
def test_cold_cases_have_k_cold_cells_per_ec(L, k, n_ecs):
    """the 16 heavily used (size, count) pairs are the LDS-resident entries, every pool cell is cold, nothing else"""
    c = ec.cold_case(L, k, n_ecs)
    cold = ec.cold_cells(c).reshape(c["E"], L)
    assert np.all(cold[:n_ecs].sum(1) == k) and not cold[n_ecs:].any() and c["E"] == n_ecs + c["n_carry"]
    assert c["n_carry"] == (16 if k == L else 0)
    assert np.array_equal(cold.ravel(), c["grp"] >= ec.COLD_HOT_GROUPS)
    assert np.all(np.diff(c["grp"].reshape(c["E"], L).astype(np.int64), axis=1) > 0)
    if not c["n_carry"]:
        want = k * ec.expected_layout([L] * n_ecs)["n_slices"] if k <= ec.COLD_ROWS else L * ec.expected_layout([L] * n_ecs)["n_slices"]
        assert ec.index_rows_from_memory(c) == want


def test_fewer_than_sixteen_used_entries_stay_in_memory():
    c = ec.uniform_case(1, 1)
    assert ec.cold_cells(c).all() and ec.index_rows_from_memory(c) == 1


@pytest.mark.parametrize("L", ec.PART_C_VALUE)
def test_value_cases_list_more_values_than_slots_are_shared(L):
    c = ec.value_case(L)
    listed = c["logl"] != ec.LOGZI
    assert np.all(listed.sum(0) == L) and len(np.unique(c["logl"][listed])) == L * c["E"] > ec.VALUE_RECORDS_ABOVE
    assert 4 * listed.sum() <= c["G"] * c["E"]


def test_mixture_case():
    c = ec.mixture_case()
    lens = np.diff(c["rowptr"].astype(np.int64))
    assert sorted(set(lens.tolist())) == [0, 1, 16, 17, 1025] and np.array_equal(lens, c["lens"])
    assert sorted(c["counts"][lens == 0].tolist()) == [0.0, 3.0]
