"""No GPU: the planted f32 data of tests/test_gpu_exact_f32.py held to the cap of tests/exact_truth.py (≥ 80 % of the queries decided,
every tile / partition edge row a decided query's neighbour — `DECIDED_SHARE`, `DECIDED_GAP_IN_BOUNDS`, no new number), the f32 truth
shown to differ from the existing one in the one assertion only, and its checker shown to refuse what the bound is there to refuse: a
kernel that narrows its operands to 16 bits on the way."""
import numpy as np
import pytest

from tests import exact_truth, exact_truth_f32, util
from tests import test_gpu_exact_f32 as gpu


@pytest.mark.parametrize("metric,ndim", gpu.PAIRS, ids=[f"{m}-{n}" for m, n in gpu.PAIRS])
def test_every_pair_is_decided(metric, ndim):
    case, _, _ = gpu.planted_case(metric, ndim)
    assert isinstance(case, exact_truth_f32.Case) and isinstance(case.truth(), exact_truth_f32.Truth) and case.rows.dtype == np.float32
    share = case.assert_decides(10, cap=ndim > 4)
    assert ndim > 4 or share < exact_truth.DECIDED_SHARE  # (4-d: exempt because it cannot meet the cap, not for convenience)
    assert len(case.edges) >= 30 and {0, gpu.ROWS - 1, 1279, 1280, 639, 640} <= set(case.edges)


def test_the_other_fixtures_are_decided():
    gpu.scaled_case().assert_decides(10)
    for k in (1, 10, 11, 16, 17, 64):
        gpu.planted_case("ip", 96, queries=100, rungs=64)[0].assert_decides(k)
    for count in (512, 520):
        gpu.planted_case("cos", 96, copies=220)[0].assert_decides(10, count=count)
    case, removed, half = gpu.planted_case("cos", 96, rungs=11, removals=True)
    case.assert_decides(10, allowed=~removed)
    case.assert_decides(10, allowed=~removed & half)


def test_a_large_batch_of_copies_is_decided():
    case, _, _ = gpu.planted_case("cos", 64, copies=2049 - gpu.QUERIES)
    for count in (1793, 2049):
        case.assert_decides(10, count=count)


def test_scaling_by_powers_of_two_changes_the_values_and_not_the_truth():
    plain, scaled = gpu.planted_case("cos", 64)[0], gpu.scaled_case()
    assert np.array_equal(scaled.rows * np.float32(2.0 ** -20), plain.rows) and np.array_equal(scaled.queries * np.float32(2.0 ** 20), plain.queries)
    assert np.array_equal(plain.truth().order(11), scaled.truth().order(11))
    assert np.abs(scaled.rows).max() > float(np.finfo(np.float16).max)  # f16 cannot carry the rows …
    assert np.abs(scaled.queries).max() < 2.0 ** -14                 # … nor the queries, short of its subnormals


def test_near_ties_are_near_and_decide_nothing():
    """The cluster at 64-d: gaps of 8e-5 — a few bounds, fewer than the eight that decide — so the conditions for all queries carry it."""
    truth = gpu.near_ties_case().truth()
    first = truth.order(11)
    gaps = np.diff(truth.distances[np.arange(len(first))[:, None], first], axis=1)
    assert (gaps < 1e-3).mean() > 0.9 and (gaps > 2 * truth.bound.max()).mean() > 0.9
    assert np.median(gaps) < exact_truth.DECIDED_GAP_IN_BOUNDS * truth.bound.max()
    assert truth.decided(10).mean() < 0.05


@pytest.mark.parametrize("metric,ndim", [("cos", 64), ("ip", 50)])
def test_the_bound_exceeds_the_suites_tolerance_which_is_why_this_truth_exists(metric, ndim):
    case, _, _ = gpu.planted_case(metric, ndim)
    with pytest.raises(AssertionError, match="the bound exceeds the suite's tolerance"):
        exact_truth.Truth(metric, "f32", case.rows, case.queries)
    truth = case.truth()
    excess = (truth.bound / (util.tolerance("f32") * np.maximum(1.0, np.abs(truth.exact)))).max()
    print(f"\n[exact f32] {metric} {ndim}-d: the worst-case bound is {excess:.1f} × 1e-5·max(1, |d|)")
    assert 1.0 < excess < 8.0


def test_the_same_fields_as_the_existing_truth_where_that_one_can_be_built():
    """4-d: the bound (3·20·2⁻²⁴ = 3.6e-6) is below 1e-5, the one case where `exact_truth.Truth` accepts f32 rows — field for field."""
    case, _, _ = gpu.planted_case("cos", 4)
    ours, theirs = case.truth(), exact_truth.Truth("cos", "f32", case.rows, case.queries)
    for field in ("exact", "bound", "distances", "allowed"):
        assert np.array_equal(getattr(ours, field), getattr(theirs, field)), field
    assert (ours.allowed_count, ours.ndim, ours.metric, ours.dtype) == (theirs.allowed_count, theirs.ndim, theirs.metric, theirs.dtype)


def faithful(truth, k):
    """What a correct kernel may return: the truth's order, its distances rounded to f32."""
    first = truth.order(k)
    distances = truth.distances[np.arange(len(first))[:, None], first].astype(np.float32)
    return first, distances, np.full(len(first), first.shape[1])


@pytest.mark.parametrize("metric,ndim", [("cos", 32), ("ip", 33), ("ip", 50)])
def test_the_checker_passes_the_truth_and_refuses_operands_narrowed_to_16_bits(metric, ndim):
    case, _, _ = gpu.planted_case(metric, ndim)
    truth = case.truth()
    slots, distances, counts = faithful(truth, 10)
    assert truth.check(slots, distances, counts, 10)["decided"] >= exact_truth.DECIDED_SHARE
    # the same rows in the same order, their distances computed from rows and queries that went through f16 on the way
    narrowed = exact_truth_f32.Truth(metric, "f32", case.rows.astype(np.float16).astype(np.float32), case.queries.astype(np.float16).astype(np.float32))
    # (a result that far off may already fail to ascend, which `check` looks at first: refused either way)
    with pytest.raises(AssertionError, match="bounds from its row's f64 distance|distances must ascend"):
        truth.check(slots, narrowed.exact[np.arange(len(slots))[:, None], slots].astype(np.float32), counts, 10)
