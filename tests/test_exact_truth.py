"""No GPU: the planted data of tests/test_gpu_exact_truth.py held to their cap (≥ 80 % of the queries decided, every tile / partition
edge row a decided query's neighbour), and the checker of tests/exact_truth.py shown to pass a faithful f32 result and to refuse the
ways a tiled kernel can be subtly wrong — a row dropped at an edge, the tie rule forgotten, a distance a little off."""
import numpy as np
import pytest

from tests import exact_truth
from tests import test_gpu_exact_truth as gpu


@pytest.mark.parametrize("metric,dtype,ndim", gpu.PAIRS, ids=[f"{m}-{d}-{n}" for m, d, n in gpu.PAIRS])
def test_every_pair_is_decided(metric, dtype, ndim):
    case, _, _ = gpu.planted_case(metric, dtype, ndim)
    case.assert_decides(10, cap=ndim >= 64)
    assert len(case.edges) >= 30 and {0, gpu.ROWS - 1, 1279, 1280, 639, 640} <= set(case.edges)


def test_the_other_fixtures_are_decided():
    gpu.planted_case("cos", "f16", 64, rows=8192)[0].assert_decides(10)
    for metric, dtype, ndim in gpu.COUNTED:
        for k in (1, 10, 11, 16, 17, 64):
            gpu.planted_case(metric, dtype, ndim, queries=100, rungs=64)[0].assert_decides(k)
    for count in (512, 520):
        gpu.planted_case("l2sq", "f16", 96, copies=220)[0].assert_decides(10, count=count)
    for metric, dtype in (("cos", "f16"), ("l2sq", "i8")):
        case, removed, half = gpu.planted_case(metric, dtype, 96, rungs=11, removals=True)
        case.assert_decides(10, allowed=~removed)
        case.assert_decides(10, allowed=~removed & half)


@pytest.mark.parametrize("metric,dtype", [("cos", "f16"), ("l2sq", "i8")])
def test_a_large_batch_of_copies_is_decided(metric, dtype):
    case, _, _ = gpu.planted_case(metric, dtype, 64, copies=2049 - gpu.QUERIES)
    for count in (1793, 2049):
        case.assert_decides(10, count=count)


def faithful(truth, k):
    """What a correct kernel may return: the truth's order, its distances rounded to f32."""
    first = truth.order(k)
    distances = truth.distances[np.arange(len(first))[:, None], first].astype(np.float32)
    return first, distances, np.full(len(first), first.shape[1])


@pytest.mark.parametrize("metric,dtype,ndim", [("cos", "f16", 64), ("ip", "bf16", 192), ("l2sq", "f16", 192), ("l2sq", "i8", 192), ("cos", "i8", 128)])
def test_the_checker_passes_the_truth_and_refuses_a_dropped_edge_row(metric, dtype, ndim):
    case, _, _ = gpu.planted_case(metric, dtype, ndim)
    truth = case.truth()
    slots, distances, counts = faithful(truth, 10)
    assert truth.check(slots, distances, counts, 10)["decided"] >= exact_truth.DECIDED_SHARE
    # a kernel that takes row 1 279 — the last of a partition — for dead: whoever had it gets the next best instead
    wider, wider_distances, _ = faithful(truth, 11)
    holders = np.argwhere(wider[:, :10] == 1279)
    assert len(holders)
    query, rank = holders[0]
    slots[query, rank:] = wider[query, rank + 1:]
    distances[query, rank:] = wider_distances[query, rank + 1:]
    with pytest.raises(AssertionError, match="not among its keys|differ from the lexsort"):
        truth.check(slots, distances, counts, 10)


def test_the_checker_refuses_a_distance_off_by_two_bounds_and_a_forgotten_tie_rule():
    case, _, _ = gpu.planted_case("l2sq", "f16", 192)
    truth = case.truth()
    slots, distances, counts = faithful(truth, 10)
    distances[3, 9] += np.float32(2.5 * truth.bound[3, slots[3, 9]])
    with pytest.raises(AssertionError, match="bounds from its row's f64 distance"):
        truth.check(slots, distances, counts, 10)
    rows = np.random.default_rng(1).integers(-60, 61, (600, 32)).astype(np.int8)
    rows[100:140] = rows[100]
    truth = exact_truth.Truth("l2sq", "i8", rows, rows[100:101])
    slots, distances, counts = faithful(truth, 16)
    assert np.array_equal(slots[0], np.arange(139, 123, -1))
    with pytest.raises(AssertionError, match="differ from the lexsort"):
        truth.check(slots[:, ::-1].copy(), distances, counts, 16)


@pytest.mark.parametrize("dtype,ndim", [("bf16", 64), ("i8", 96), ("f16", 64)])
def test_near_ties_are_near_and_still_more_than_two_bounds_apart(dtype, ndim):
    """The cluster of tests/test_gpu_exact_truth.py: nearly every neighbouring pair among a query's eleven nearest lies within 1e-3 (a
    pruning margin that wrong would cut into them) and most of them more than two bounds apart (dropping one then fails
    completeness). bf16 and i8 round the planted rows by more than the spacing: their clusters are as dense, not as regular."""
    truth = gpu.near_ties_case(dtype, ndim).truth()
    first = truth.order(11)
    d = truth.distances[np.arange(len(first))[:, None], first]
    gaps = np.diff(d, axis=1)
    assert (gaps < 1e-3).mean() > 0.9
    assert (gaps > 2 * truth.bound.max()).mean() > 0.5
