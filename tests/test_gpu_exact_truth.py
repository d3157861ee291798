"""GPU: the matrix-unit exact search (csrc/exact_tiled.hip — the 64-query tile and the wide tile of 256 × 256) against an f64
ground truth over ALL rows (tests/exact_truth.py), on every route the launch planner (csrc/exact_plan.hpp) can send a batch down.

Every case first asserts, through the planner's test hook, that it takes the route it is there for; then, on the CPU, that its
planted data decide what they are meant to (≥ 80 % of the queries decided, every tile / partition edge row a decided query's
neighbour); then it searches once and holds the result to the truth: counts, ascending distances, no repeated or rejected key,
soundness (a distance within the derived bound of its row's f64 distance), completeness (nobody closer than the last result by
more than the two bounds is missing — what a dropped row fails), the truth's very keys in order for the decided queries; for ip and
l2sq over i8 the numpy lexsort of the exact integers and their bits for EVERY query; for cos over i8 the wave-per-query kernel's
bits as well. Shapes are the smallest that reach a route: 8 200 rows are eight wide partitions of 1 280, the seventh ragged, the
eighth empty, and thirteen 64-tile partitions of 640 (the last ragged).

The 16-byte-row case (f16, 8-d) carries the conditions for all queries only: below 64 dimensions the background is too close for
planting to decide much, and it is exempt from the cap. So are the filters that let fewer than k rows through.

Observed on an MI355X, the largest |distance − f64 distance of the row named| ÷ bound over a case's results (the bound is derived
in tests/exact_truth.py, not fitted to these; both kernels gave the same figure in every case):
    cos f16 64-d 0.021 · ip f16 100-d 0.029 · l2sq f16 192-d 0.013 · cos bf16 100-d 0.017 · ip bf16 192-d 0.024 · l2sq bf16 64-d 0.023
    cos f16 8-d 0.049 · ip f16 96-d (k = 1 … 64) 0.031 · l2sq f16 96-d 0.019 · cos f16 96-d under filters 0.013
    cos i8 128-d 0.30 and 96-d 0.30 of its own bound of 8·2⁻²⁴ (the sums are exact) · ip / l2sq over i8: bits equal, no bound
Decided queries: 100 % in every capped float case but ip f16 at k = 64 (93 %) and cos i8 128-d (84 %); 8-d: 95 %, exempt.
Times on the GPU: the slowest of these tests takes 0.5 s (it builds the first image), most take under 0.2 s, the file 6 s.
"""
import functools

import numpy as np
import pytest

from tests import exact_truth, util

pytestmark = pytest.mark.gpu
ROWS, QUERIES, RUNGS, KEY_BASE = 8200, 300, 16, 1000
SCALAR_BYTES = {"f16": 2, "bf16": 2, "i8": 1}


def stored_bytes(dtype, ndim):
    """(bytes per vector, a row pitch for the planner: whole 16-byte chunks — the plan only looks at it for the 2³¹ limit)."""
    nbytes = SCALAR_BYTES[dtype] * ndim
    return nbytes, (nbytes + 15) // 16 * 16


def route(dtype, ndim, count, k, rows=ROWS, tile=None, global_lists=None):
    """The plan of a search as the engine makes it (`tile` / `global_lists` None: from the environment, like the engine)."""
    from usearch_amd.index import test_plan_exact
    return test_plan_exact(rows, *stored_bytes(dtype, ndim), count, k, forced_tile=tile, global_lists=global_lists)


def edges_of(dtype, ndim, count, k, rows=ROWS):
    """The real edges: the partitions of both kernels for this batch, from the planner."""
    return exact_truth.edge_slots(rows, [route(dtype, ndim, count, k, rows, tile=64), route(dtype, ndim, count, k, rows, tile=256)])


@functools.lru_cache(maxsize=None)
def planted_case(metric, dtype, ndim, rows=ROWS, queries=QUERIES, rungs=RUNGS, copies=0, removals=False, seed=11):
    """→ (case, removed slots, half filter), no GPU involved (tests/test_exact_truth.py holds every one of them to the cap on the CPU).
    `removals`: every 13th member is removed and a seeded half of the slots is what the 'half' filter allows; planted rows sit
    where both leave them."""
    removed, half = np.zeros(rows, dtype=bool), np.ones(rows, dtype=bool)
    if removals:
        removed[5::13] = True
        half = np.random.default_rng(seed + 1).random(rows) < 0.5
    case = exact_truth.plant(metric, dtype, ndim, rows, queries, rungs, seed, edges=edges_of(dtype, ndim, queries + copies, 10, rows),
                             usable=~removed & half, copies=copies)
    return case, removed, half


@functools.lru_cache(maxsize=None)
def planted(*shape, **options):
    """→ (case, index, removed slots, half filter): one image per case, shared by the tests that use it."""
    from usearch_amd import Index
    case, removed, half = planted_case(*shape, **options)
    image, _, _ = util.build_image(len(case.rows), case.rows.shape[1] // (1 if case.dtype != "b1" else 8), case.metric, case.dtype,
                                   vectors=case.rows, connectivity=4, expansion_add=16, remove=np.flatnonzero(removed) + KEY_BASE)
    return case, Index.restore(image), removed, half


def hold_to_truth(case, index, k, what, count=None, allowed=None, filter=None, cap=True):
    case.assert_decides(k, allowed, count, cap)  # on the CPU, before any GPU call
    queries = case.queries[:count]
    got = index.search(queries, k, exact="tiled", dtype=case.dtype, filter=filter)
    report = case.truth(allowed, count).check(got.keys.astype(np.int64) - KEY_BASE, got.distances, got.counts, k, padding=got.keys)
    print(f"\n[exact truth] {what}: largest error {report['error_in_bounds']:.3f} bounds, {report['decided']:.1%} of {len(queries)} queries decided")
    if case.metric == "cos" and case.dtype == "i8" and filter is None:  # exact sums, the same closing arithmetic: the wave kernel's bits
        exact = index.search(queries, k, exact=True, dtype=case.dtype)
        assert np.array_equal(exact.counts, got.counts) and np.array_equal(exact.keys, got.keys)
        assert util.same_float_bits(exact.distances, got.distances)
    return got


# row bytes: 128 (one chunk), 200 → 208 (two chunks, ragged), 384 (three: the staging buffers swap parity from tile to tile),
# 130 → 144 and 192 for i8, and one row of 16 bytes
PAIRS = [("cos", "f16", 64), ("ip", "f16", 100), ("l2sq", "f16", 192), ("cos", "bf16", 100), ("ip", "bf16", 192), ("l2sq", "bf16", 64),
         ("cos", "i8", 128), ("ip", "i8", 130), ("l2sq", "i8", 192), ("cos", "f16", 8)]


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric,dtype,ndim", PAIRS, ids=[f"{m}-{d}-{n}" for m, d, n in PAIRS])
def test_every_pair_on_both_kernels(reference, monkeypatch, metric, dtype, ndim, tile):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    plan = route(dtype, ndim, QUERIES, 10)
    assert plan["wide"] == (tile == 256) and (plan["partitions"], plan["rows_per_partition"]) == ((8, 1280) if tile == 256 else (13, 640))
    assert tile == 64 or (plan["lds_lists"] == 1 and 7 * plan["rows_per_partition"] > ROWS)  # an empty last partition
    case, index, _, _ = planted(metric, dtype, ndim)
    hold_to_truth(case, index, 10, f"{metric} {dtype} {ndim}-d, tile {tile}", cap=ndim >= 64)  # (8-d: exempt, see the module's docstring)


def test_a_row_count_without_a_ragged_partition(reference, monkeypatch):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "256")
    plan = route("f16", 64, QUERIES, 10, rows=8192)
    assert plan["wide"] and plan["partitions"] * plan["rows_per_partition"] == 8192
    case, index, _, _ = planted("cos", "f16", 64, rows=8192)
    hold_to_truth(case, index, 10, "cos f16 64-d, 8 192 rows, tile 256")


# ---- result counts: 1 | 10 | 11 (lists in LDS | in the output arrays) | 16 | 17 (the wide tile | the 64 tile) | 64 | 65 (refused).
#      ip keeps a ladder of any length apart (64 rungs: 100 queries fill 6 400 of the 8 200 rows)
COUNTED = [("ip", "f16", 96), ("l2sq", "i8", 96)]


@pytest.mark.parametrize("k,tile,global_lists,wide,lds_lists", [(1, 256, 0, 1, 1), (10, 256, 0, 1, 1), (10, 256, 1, 1, 0), (11, 256, 0, 1, 0),
                                                                (16, 256, 0, 1, 0), (17, 256, 0, 0, 0), (64, 64, 0, 0, 0)],
                         ids=["1-wide-lds", "10-wide-lds", "10-wide-global-forced", "11-wide-global", "16-wide-global", "17-forced-256-takes-64",
                              "64-tile-64"])
@pytest.mark.parametrize("metric,dtype,ndim", COUNTED, ids=[f"{m}-{d}-{n}" for m, d, n in COUNTED])
def test_result_counts_at_every_boundary(reference, monkeypatch, metric, dtype, ndim, k, tile, global_lists, wide, lds_lists):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    if global_lists:
        monkeypatch.setenv("USEARCH_AMD_EXACT_GLOBAL_LISTS", "1")
    plan = route(dtype, ndim, 100, k)
    assert (plan["wide"], plan["lds_lists"]) == (wide, lds_lists)
    case, index, _, _ = planted(metric, dtype, ndim, queries=100, rungs=64)
    hold_to_truth(case, index, k, f"{metric} {dtype} {ndim}-d, k = {k}, tile {tile}{', global lists' if global_lists else ''}")


@pytest.mark.parametrize("metric,dtype,ndim", COUNTED, ids=[f"{m}-{d}-{n}" for m, d, n in COUNTED])
def test_more_results_than_a_lane_per_entry_are_refused(reference, metric, dtype, ndim):
    case, index, _, _ = planted(metric, dtype, ndim, queries=100, rungs=64)
    with pytest.raises(RuntimeError, match="No tiled exact-search kernel for this metric / scalar kind / result count"):
        index.search(case.queries, 65, exact="tiled", dtype=dtype)


# ---- the default route: nobody forces a tile; more than 512 queries over at least 8 192 rows take the wide one
@pytest.mark.parametrize("count,wide", [(520, 1), (512, 0)])
def test_the_default_route_of_an_index(reference, monkeypatch, count, wide):
    monkeypatch.delenv("USEARCH_AMD_EXACT_TILE", raising=False)
    monkeypatch.delenv("USEARCH_AMD_EXACT_GLOBAL_LISTS", raising=False)
    assert route("f16", 96, count, 10)["wide"] == wide
    case, index, _, _ = planted("l2sq", "f16", 96, copies=220)
    hold_to_truth(case, index, 10, f"l2sq f16 96-d, {count} queries, nothing forced", count=count)


@pytest.mark.parametrize("count,wide", [(520, 1), (512, 0)])
def test_the_default_route_of_a_raw_i8_dataset(monkeypatch, count, wide):
    """`usearch_amd.exact_search` over i8 rows goes to the matrix units on its own; keys are row offsets."""
    import usearch_amd
    for name in ("USEARCH_AMD_EXACT_TILE", "USEARCH_AMD_EXACT_GLOBAL_LISTS", "USEARCH_AMD_NO_TILED_EXACT"):
        monkeypatch.delenv(name, raising=False)
    assert route("i8", 96, count, 10)["wide"] == wide
    case = exact_truth.plant("ip", "i8", 96, ROWS, QUERIES, RUNGS, 13, edges=edges_of("i8", 96, 520, 10), copies=220)
    keys, distances = usearch_amd.exact_search(case.rows, case.queries[:count], 10, metric="ip")
    case.truth(count=count).check(keys.astype(np.int64), distances, np.full(count, 10), 10)


# ---- eight query tiles and more: tiles dealt over the XCDs; nine leave a short last round of workgroups that return early
@pytest.mark.parametrize("count,tiles,per_xcd", [(1793, 8, 1), (2049, 9, 2)])
@pytest.mark.parametrize("metric,dtype", [("cos", "f16"), ("l2sq", "i8")])
def test_query_tiles_dealt_over_the_xcds(reference, monkeypatch, metric, dtype, count, tiles, per_xcd):
    monkeypatch.delenv("USEARCH_AMD_EXACT_TILE", raising=False)
    monkeypatch.delenv("USEARCH_AMD_EXACT_GLOBAL_LISTS", raising=False)
    plan = route(dtype, 64, count, 10)
    assert (plan["wide"], plan["query_tiles"], plan["tiles_per_xcd"]) == (1, tiles, per_xcd)
    assert plan["workgroups"] == 8 * per_xcd * plan["partitions"] >= tiles * plan["partitions"]
    # the first 300 queries have ladders, the rest are copies of them under a permutation: the cap still holds
    case, index, _, _ = planted(metric, dtype, 64, copies=2049 - QUERIES)
    hold_to_truth(case, index, 10, f"{metric} {dtype} 64-d, {count} queries ({tiles} query tiles)", count=count)


# ---- tombstones and the caller's bitmap through the wide kernel's `allow_bits` (tests/test_gpu_filtered.py stops at the 64 tile)
@pytest.mark.parametrize("filtered", ["tombstones-only", "half", "five-rows", "nothing"])
@pytest.mark.parametrize("metric,dtype", [("cos", "f16"), ("l2sq", "i8")])
def test_filters_and_tombstones_through_the_wide_tile(reference, monkeypatch, metric, dtype, filtered):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "256")
    assert route(dtype, 96, QUERIES, 10)["wide"] == 1
    case, index, removed, half = planted(metric, dtype, 96, rungs=11, removals=True)  # (11 rungs: 3 300 planted rows fit the 3 780 slots left)
    bits = {"tombstones-only": None, "half": half, "nothing": np.zeros(ROWS, dtype=bool)}.get(filtered)
    if filtered == "five-rows":  # the first and the last member, three between them, and a removed one, which stays out
        bits = np.zeros(ROWS, dtype=bool)
        bits[np.flatnonzero(~removed)[[0, 100, 2000, 5000, -1]]] = True
        bits[5] = True
        assert removed[5] and int((bits & ~removed).sum()) == 5
    allowed = ~removed if bits is None else bits & ~removed
    got = hold_to_truth(case, index, 10, f"{metric} {dtype} 96-d, {filtered}", allowed=allowed,
                        filter=None if bits is None else index.filter_bits(bits), cap=filtered in ("tombstones-only", "half"))
    assert int(got.counts[0]) == {"five-rows": 5, "nothing": 0}.get(filtered, 10)


# ---- ties: the order is total for i8 (distance ↑, slot ↓), whatever partition or tile an equal row falls in
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric", ["l2sq", "ip", "cos"])
def test_equal_rows_across_a_partition_edge_come_back_by_slot(reference, monkeypatch, metric, tile):
    from usearch_amd import Index
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    plan = route("i8", 96, QUERIES, 16)
    assert plan["wide"] == (tile == 256) and 1280 % plan["rows_per_partition"] == 0  # row 1 280 begins a partition on either route
    rng = np.random.default_rng(17)
    rows = rng.integers(-60, 61, (ROWS, 96)).astype(np.int8)
    queries = rng.integers(-60, 61, (QUERIES, 96)).astype(np.int8)
    rows[1260:1300] = rows[1260]  # forty equal rows, twenty on either side of the edge
    queries[::50] = rows[1260] if metric != "ip" else np.sign(rows[1260]) * 127  # (ip: the query they all serve best, equally)
    image, _, _ = util.build_image(ROWS, 96, metric, "i8", vectors=rows, connectivity=4, expansion_add=16)
    index = Index.restore(image)
    got = index.search(queries, 16, exact="tiled")
    truth = exact_truth.Truth(metric, "i8", rows, queries)
    assert np.array_equal(truth.order(16)[0], np.arange(1299, 1283, -1)), "the fixture: sixteen of the forty, the latest slots first"
    if metric == "cos":  # not an integer pair: equal rows have equal bits all the same, and the wave kernel's order is the reference's
        exact = index.search(queries, 16, exact=True)
        assert np.array_equal(exact.keys, got.keys) and util.same_float_bits(exact.distances, got.distances)
        assert np.array_equal(got.keys[0].astype(np.int64) - KEY_BASE, truth.order(16)[0])
    truth.check(got.keys.astype(np.int64) - KEY_BASE, got.distances, got.counts, 16, padding=got.keys)


# ---- near-ties that arrive AFTER a query's bound is set: where the wide tile's pruning test (a bound shared by the partitions, a margin
#      of 1e-5) would drop a neighbour if it were not conservative. bf16 and i8 take the general fold, f16 the fused one.
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("dtype,ndim", [("bf16", 64), ("i8", 96), ("f16", 64)])
def test_near_ties_that_arrive_after_the_bound_is_set(reference, monkeypatch, dtype, ndim, tile):
    from usearch_amd import Index
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    assert route(dtype, ndim, QUERIES, 10)["wide"] == (tile == 256)
    case = near_ties_case(dtype, ndim)
    image, _, _ = util.build_image(ROWS, ndim, "cos", dtype, vectors=case.rows, connectivity=4, expansion_add=16)
    hold_to_truth(case, Index.restore(image), 10, f"cos {dtype} {ndim}-d near-ties, tile {tile}", cap=False)


@functools.lru_cache(maxsize=None)
def near_ties_case(dtype, ndim):
    partition = route(dtype, ndim, QUERIES, 10, tile=256)["rows_per_partition"]  # a cluster lies inside one wide partition
    return exact_truth.plant("cos", dtype, ndim, ROWS, QUERIES, 14, 19, near_ties=partition)
