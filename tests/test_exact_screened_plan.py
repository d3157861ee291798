"""The screened exact search's table and launch planner (csrc/exact_plan.hpp: `exact_screened_pair`, `plan_exact_screened`) through
their test hooks, no GPU in the loop: which pairs the route takes, that its grid covers every row once, and that a buffer holds what
its rule says."""
import math

import pytest

REFUSAL = "No screened exact-search kernel for this metric / scalar kind / result count"


@pytest.mark.parametrize("metric", ["cos", "ip", "l2sq"])
def test_the_three_metrics_over_f32_are_in_for_1_to_64_results(metric):
    from usearch_amd.index import test_exact_screened_pair
    assert all(test_exact_screened_pair(metric, "f32", wanted) for wanted in range(1, 65))
    assert not any(test_exact_screened_pair(metric, "f32", wanted) for wanted in (0, 65, 2 ** 40))
    assert not any(test_exact_screened_pair(metric, dtype, 10) for dtype in ("b1", "bf16", "f64", "f16", "f8", "i8"))


@pytest.mark.parametrize("metric", ["pearson", "haversine", "divergence", "hamming", "jaccard", "tanimoto", "sorensen"])
def test_no_other_metric_is_in(metric):
    from usearch_amd.index import test_exact_screened_pair
    assert not any(test_exact_screened_pair(metric, dtype, 10) for dtype in ("b1", "bf16", "f64", "f32", "f16", "f8", "i8"))


@pytest.mark.parametrize("rows,count,wanted,partitions,capacity", [
    (130, 65, 10, 1, 100),         # one partition; 10 · (2 + 2 · ⌈log₂ 13⌉)
    (130, 1, 64, 1, 130),          # never more than the partition has rows: it cannot overflow
    (600, 70, 10, 1, 140),         # 10 · (2 + 2 · ⌈log₂ 60⌉): 600 equal rows overflow it
    (1100, 300, 1, 2, 32),         # two partitions of 640 and 460 rows; at least 32
    (10 ** 6, 10 ** 4, 10, 14, 280)])  # the headline: 157 query tiles, 14 partitions of 71 552 rows
def test_plans(rows, count, wanted, partitions, capacity):
    from usearch_amd.index import test_plan_exact, test_plan_exact_screened
    p = test_plan_exact_screened(rows, 3072, 3072, count, wanted)
    tiles = test_plan_exact(rows, 3072, 3072, count, wanted, forced_tile=64, global_lists=False)
    assert (p["query_tiles"], p["partitions"], p["rows_per_partition"]) == (tiles["query_tiles"], tiles["partitions"], tiles["rows_per_partition"])
    assert p["query_tiles"] == -(-count // 64) and p["partitions"] == partitions and p["rows_per_partition"] % 128 == 0
    assert (p["partitions"] - 1) * p["rows_per_partition"] < rows <= p["partitions"] * p["rows_per_partition"]
    longest = min(rows, p["rows_per_partition"])
    assert p["capacity"] == capacity == min(longest, max(32, wanted * (2 + 2 * math.ceil(math.log2(-(-longest // wanted))))))
    cells = count * p["partitions"]
    assert p["scratch_bytes"] == rows * 4 + count * 4 + cells * capacity * 8 + cells * 8 + count * 4
    with pytest.raises(RuntimeError, match="Not enough device memory"):
        test_plan_exact_screened(rows, 3072, 3072, count, wanted, scratch_limit=p["scratch_bytes"] - 1)


def test_refusals():
    from usearch_amd.index import test_plan_exact_screened
    for wanted in (0, 65):
        with pytest.raises(RuntimeError, match=REFUSAL):
            test_plan_exact_screened(1000, 64, 64, 10, wanted)
    assert test_plan_exact_screened(1000, 64, 64, 0, 10)["partitions"] == 0  # an empty batch: nothing to plan, nothing refused
