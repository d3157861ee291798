"""The bit tile's table and launch planner (csrc/exact_plan.hpp: `exact_bits_pair`, `plan_exact_bits`) through their test hooks, no GPU
in the loop: which pairs the tile takes, and that the grid it launches covers every (query tile, row partition) pair and every row
exactly once. A partition nobody takes would lose its rows for 256 queries, silently: the merge takes whatever lists it finds."""
import itertools

import pytest

METRICS = ["hamming", "tanimoto", "jaccard", "sorensen"]
ROWS = [1, 63, 64, 65, 255, 256, 257, 5003, 9000, 2 ** 20 + 1, 125 * 10 ** 6]
BYTES = [1, 9, 16, 17, 128, 257]
COUNTS = [1, 63, 64, 65, 300, 600, 10000]
WANTED = [1, 10, 16, 17, 64]
REFUSAL = "No tiled exact-search kernel for this metric / scalar kind / result count"
TILE_QUERIES, WAVE_QUERIES, STEP_ROWS = 256, 64, 64  # four waves of 64 queries; a wave steps through 64 rows at a time


def stride_of(nbytes):
    return -(-nbytes // 16) * 16


def plan(rows, nbytes, count, wanted, stride=None):
    from usearch_amd.index import test_plan_exact_bits
    return test_plan_exact_bits(rows, nbytes, stride_of(nbytes) if stride is None else stride, count, wanted)


@pytest.mark.parametrize("metric", METRICS)
def test_the_four_bit_metrics_over_b1_are_in_for_1_to_64_results(metric):
    from usearch_amd.index import test_exact_bits_pair
    assert all(test_exact_bits_pair(metric, "b1", wanted) for wanted in range(1, 65))
    assert not any(test_exact_bits_pair(metric, "b1", wanted) for wanted in (0, 65, 2 ** 40))
    assert not any(test_exact_bits_pair(metric, dtype, 10) for dtype in ("f32", "f16", "bf16", "i8", "f64"))


@pytest.mark.parametrize("metric", ["cos", "ip", "l2sq", "pearson", "haversine", "divergence"])
def test_no_other_metric_is_in(metric):
    from usearch_amd.index import test_exact_bits_pair
    assert not any(test_exact_bits_pair(metric, dtype, 10) for dtype in ("b1", "f32", "f16", "bf16", "i8", "f64"))


def test_the_table_of_matrix_unit_pairs_is_what_it_was():
    from usearch_amd.index import test_exact_tiled_pair
    assert not any(test_exact_tiled_pair(metric, "b1", 10) for metric in METRICS + ["cos", "ip", "l2sq"])
    assert all(test_exact_tiled_pair(metric, "f16", wanted) for metric in ("cos", "ip", "l2sq") for wanted in (1, 10, 64))
    assert not test_exact_tiled_pair("cos", "f16", 65) and not test_exact_tiled_pair("l2sq", "f32", 10)


@pytest.mark.parametrize("rows", ROWS)
def test_every_plan_covers_the_rows_and_every_pair_once(rows):
    for nbytes, count, wanted in itertools.product(BYTES, COUNTS, WANTED):
        p = plan(rows, nbytes, count, wanted)
        what = (rows, nbytes, count, wanted, p)
        # the partitions' row ranges [y · rows_per_partition, min(rows, (y + 1) · rows_per_partition)) tile [0, rows): the last one
        # is not empty and ends at or past the last row
        assert p["rows_per_partition"] > 0 and p["rows_per_partition"] % STEP_ROWS == 0, what
        assert p["partitions"] >= 1 and (p["partitions"] - 1) * p["rows_per_partition"] < rows <= p["partitions"] * p["rows_per_partition"], what
        # workgroup (x, y) of the 2-D grid takes query tile x and partition y: every pair once, and every query in a tile
        assert p["query_tiles"] == -(-count // TILE_QUERIES), what
        assert (p["query_tiles"] - 1) * TILE_QUERIES < count <= p["query_tiles"] * TILE_QUERIES, what
        # the merge folds partitions · wanted candidates per query with one wave, and the grid has its limits
        assert p["partitions"] * wanted <= 8192, what
        assert p["partitions"] <= 65535 and p["query_tiles"] < 2 ** 31, what
        # the padded copy of the batch: whole waves of queries, whole 16-byte pieces, no more of either than that takes
        assert p["padded_queries"] % WAVE_QUERIES == 0 and count <= p["padded_queries"] < count + WAVE_QUERIES, what
        assert p["padded_query_bytes"] % 16 == 0 and nbytes <= p["padded_query_bytes"] < nbytes + 16, what
        # a wave's lists: [64 queries][wanted] candidates of 8 bytes, four waves; inside the 160 KB of a compute unit
        assert p["lds_bytes"] == TILE_QUERIES * wanted * 8 <= 160 * 1024, what


def test_the_shapes_the_gpu_tests_lean_on():
    """5003 and 9000 rows: several partitions, the last one ragged; 100 and 40 rows: one partition, less than two steps."""
    p = plan(5003, 16, 300, 10)
    assert (p["query_tiles"], p["partitions"], p["rows_per_partition"]) == (2, 16, 320) and 5003 % 320 and 5003 % 64
    p = plan(9000, 16, 300, 10)
    assert (p["partitions"], p["rows_per_partition"]) == (29, 320) and 9000 % 320
    for rows in (40, 100):
        p = plan(rows, 16, 65, 64)
        assert (p["query_tiles"], p["partitions"], p["padded_queries"]) == (1, 1, 128)
    assert plan(5003, 16, 600, 10)["query_tiles"] == 3 and plan(5003, 257, 1, 10)["padded_query_bytes"] == 272


def test_the_flagship_shard_fills_the_chip():
    p = plan(125 * 10 ** 6, 16, 10000, 10)
    assert p["query_tiles"] == 40 and p["query_tiles"] * p["partitions"] >= 2048


def test_the_pitch_does_not_move_the_split():
    assert plan(5003, 16, 300, 10, stride=64) == plan(5003, 16, 300, 10)
    with pytest.raises(RuntimeError, match="Row pitch"):
        plan(5003, 17, 300, 10, stride=16)


@pytest.mark.parametrize("wanted", [0, 65])
def test_result_counts_without_a_kernel_are_refused(wanted):
    with pytest.raises(RuntimeError, match=REFUSAL):
        plan(5003, 16, 300, wanted)


def test_an_empty_batch_plans_nothing_and_an_empty_index_is_refused():
    assert not any(plan(5003, 16, 0, 10).values())
    with pytest.raises(RuntimeError, match="Nothing to scan"):
        plan(0, 16, 300, 10)


def test_nothing_depends_on_the_environment(monkeypatch):
    before = plan(9000, 16, 600, 10)
    for name, value in (("USEARCH_AMD_EXACT_TILE", "64"), ("USEARCH_AMD_EXACT_GLOBAL_LISTS", "1"), ("USEARCH_AMD_NO_TILED_EXACT", "1")):
        monkeypatch.setenv(name, value)
    assert plan(9000, 16, 600, 10) == before
