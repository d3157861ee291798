"""No GPU: the table of (metric, scalar kind, result count) triples that have a tiled exact-search kernel (`exact_tiled_pair` of
csrc/exact_plan.hpp, what `exact_tiled_available` answers with and every tiled route is refused by), through its test hook."""
import pytest

from usearch_amd.index import test_exact_tiled_pair as tiled_pair

METRICS = ("cos", "ip", "l2sq")


@pytest.mark.parametrize("metric", ["cos", "ip"])
def test_f32_has_a_tiled_kernel_for_every_result_count_a_list_holds(metric):
    assert all(tiled_pair(metric, "f32", wanted) for wanted in range(1, 65))
    assert not tiled_pair(metric, "f32", 0) and not tiled_pair(metric, "f32", 65)


def test_l2sq_over_f32_stays_without_one():
    """`exact="tiled"` over an l2sq f32 index is refused, and tests/test_gpu_exact.py pins that: the pair stays out of the table."""
    assert not any(tiled_pair("l2sq", "f32", wanted) for wanted in range(0, 66))


@pytest.mark.parametrize("dtype", ["f16", "bf16", "i8"])
@pytest.mark.parametrize("metric", METRICS)
def test_the_nine_earlier_pairs_are_unchanged(metric, dtype):
    assert all(tiled_pair(metric, dtype, wanted) for wanted in range(1, 65))
    assert not tiled_pair(metric, dtype, 0) and not tiled_pair(metric, dtype, 65) and not tiled_pair(metric, dtype, 1 << 40)


def test_other_metrics_and_kinds_have_none():
    for metric in ("pearson", "divergence", "haversine"):
        for dtype in ("f32", "f16", "bf16", "i8", "f64"):
            assert not tiled_pair(metric, dtype, 10), (metric, dtype)
    for metric in METRICS:
        assert not tiled_pair(metric, "f64", 10) and not tiled_pair(metric, "b1", 10)
    for metric in ("hamming", "tanimoto", "sorensen", "jaccard"):
        assert not tiled_pair(metric, "b1", 10)
