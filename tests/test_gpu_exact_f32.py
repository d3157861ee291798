"""GPU: exact search of f32 rows on the matrix units (`v_mfma_f32_32x32x2_f32`, csrc/exact_tiled.hip — the 64-query tile and the wide
tile of 256 × 256) against an f64 ground truth over ALL rows (tests/exact_truth_f32.py), on every route the launch planner
(csrc/exact_plan.hpp) can send a batch down. The mirror of tests/test_gpu_exact_truth.py for the kind it does not cover.

Every case first asserts, through the planner's test hook, that it takes the route it is there for; then, on the CPU, that its
planted data decide what they are meant to (≥ 80 % of the queries decided, every tile / partition edge row a decided query's
neighbour); then it searches once and holds the result to the truth: counts, ascending distances, no repeated or rejected key,
soundness (a distance within the derived bound of its row's f64 distance), completeness (nobody closer than the last result by more
than the two bounds is missing), the truth's very keys in order for the decided queries. 8 200 rows are eight wide partitions of
1 280, the seventh ragged, the eighth empty, and thirteen 64-tile partitions of 640 (the last ragged).

cos and ip only: l2sq over f32 stays refused (tests/test_gpu_exact.py pins that refusal; `test_l2sq_over_f32_is_still_refused`).

The contract is the bound, not 1e-5 and not the wave kernel's bits (tests/exact_truth_f32.py says why). The 16-byte-row case (4-d)
carries the conditions for all queries only and is exempt from the cap, like the 16-byte row of tests/test_gpu_exact_truth.py; so are
the filters that let fewer than k rows through, and the near-ties.

Observed on an MI355X — the largest |distance − f64 distance of the row named| over a case's results as a share of the BOUND
(derived in tests/exact_truth_f32.py, not fitted to these) | as a share of 1e-5·max(1, |d|), the suite's f32 tolerance, which this
route is not promised within; both kernels gave the same figures in every case:
    cos 32-d 0.044 | 0.038 · ip 33-d 0.126 | 0.048 · ip 50-d 0.103 | 0.047 · cos 96-d 0.030 | 0.061 · cos 4-d 0.072 | 0.026
    cos 64-d, rows × 2²⁰ and queries × 2⁻²⁰ 0.035 | 0.050 · the same case in 1 793 and 2 049 queries 0.035 | 0.050
    ip 96-d: k = 1 0.046 | 0.032 · k = 10 (lists in LDS, and forced global) 0.071 | 0.049 · k = 11, 16, 17 0.073 | 0.051 · k = 64 0.077 | 0.059
    cos 96-d at 520 and 512 queries, nothing forced, through an index and as a raw matrix 0.030 | 0.061
    cos 96-d under tombstones, the half filter and five rows 0.027 | 0.055 · cos 64-d near-ties 0.032 | 0.045
    against the wave kernel, distances of decided queries as a share of the two bounds: cos 0.016 · ip 0.042, with 21.4 % and
    20.7 % of all distances bit-equal
Decided queries: 100 % in every capped case but cos 32-d (99.7 %), ip at k = 64 (91 %) and the five-row filter (99.3 %, exempt); 4-d:
73 %, exempt; the near-ties: 0 %, as intended. Times on the GPU: the slowest of these tests takes 0.5 s (it builds the first image),
most take under 0.2 s, the file 4 s.
"""
import functools

import numpy as np
import pytest

from tests import exact_truth_f32, util

pytestmark = pytest.mark.gpu
ROWS, QUERIES, RUNGS, KEY_BASE = 8200, 300, 16, 1000
REFUSAL = "No tiled exact-search kernel for this metric / scalar kind / result count"


def stored_bytes(ndim, scalar_bytes=4):
    """(bytes per vector, a row pitch for the planner: whole 16-byte pieces — the plan only looks at it for the 2³¹ limit)."""
    nbytes = scalar_bytes * ndim
    return nbytes, (nbytes + 15) // 16 * 16


def route(ndim, count, k, rows=ROWS, tile=None, global_lists=None, scalar_bytes=4):
    """The plan of a search as the engine makes it (`tile` / `global_lists` None: from the environment, like the engine)."""
    from usearch_amd.index import test_plan_exact
    return test_plan_exact(rows, *stored_bytes(ndim, scalar_bytes), count, k, forced_tile=tile, global_lists=global_lists)


def edges_of(ndim, count, k, rows=ROWS):
    """The real edges: the partitions of both kernels for this batch, from the planner."""
    return exact_truth_f32.edge_slots(rows, [route(ndim, count, k, rows, tile=64), route(ndim, count, k, rows, tile=256)])


@functools.lru_cache(maxsize=None)
def planted_case(metric, ndim, rows=ROWS, queries=QUERIES, rungs=RUNGS, copies=0, removals=False, seed=11):
    """→ (case, removed slots, half filter), no GPU involved (tests/test_exact_truth_f32.py holds every one of them to the cap on the
    CPU). `removals`: every 13th member is removed and a seeded half of the slots is what the 'half' filter allows; planted rows sit
    where both leave them."""
    removed, half = np.zeros(rows, dtype=bool), np.ones(rows, dtype=bool)
    if removals:
        removed[5::13] = True
        half = np.random.default_rng(seed + 1).random(rows) < 0.5
    case = exact_truth_f32.plant(metric, ndim, rows, queries, rungs, seed, edges=edges_of(ndim, queries + copies, 10, rows),
                                 usable=~removed & half, copies=copies)
    return case, removed, half


@functools.lru_cache(maxsize=None)
def scaled_case():
    """cos 64-d with the rows × 2²⁰ and the queries × 2⁻²⁰ — exact in f32, out of reach of any 16-bit kind (f16 ends at 65 504, bf16
    keeps eight bits of a scalar) — and the truth of the scaled data: the cos distances, and with them what is decided, are those of
    the unscaled case; the norms and the sums the kernel meets are not."""
    case, _, _ = planted_case("cos", 64)
    return exact_truth_f32.Case(case.metric, case.dtype, case.rows * np.float32(2.0 ** 20), case.queries * np.float32(2.0 ** -20),
                                case.ladders, case.edges, case.usable)


@functools.lru_cache(maxsize=None)
def near_ties_case(ndim=64):
    partition = route(ndim, QUERIES, 10, tile=256)["rows_per_partition"]  # a cluster lies inside one wide partition
    return exact_truth_f32.plant("cos", ndim, ROWS, QUERIES, 14, 19, near_ties=partition)


@functools.lru_cache(maxsize=None)
def image_of(case, removed=None):
    """One index per case, shared by the tests that use it."""
    from usearch_amd import Index
    remove = () if removed is None else np.flatnonzero(np.frombuffer(removed, dtype=bool)) + KEY_BASE
    image, _, _ = util.build_image(len(case.rows), case.rows.shape[1], case.metric, case.dtype, vectors=case.rows, connectivity=4,
                                   expansion_add=16, remove=remove)
    return Index.restore(image)


def planted(*shape, **options):
    """→ (case, index, removed slots, half filter)."""
    case, removed, half = planted_case(*shape, **options)
    return case, image_of(case, removed.tobytes() if removed.any() else None), removed, half


def hold_to_truth(case, index, k, what, count=None, allowed=None, filter=None, cap=True):
    case.assert_decides(k, allowed, count, cap)  # on the CPU, before any GPU call
    queries = case.queries[:count]
    got = index.search(queries, k, exact="tiled", dtype=case.dtype, filter=filter)
    truth = case.truth(allowed, count)
    report = truth.check(got.keys.astype(np.int64) - KEY_BASE, got.distances, got.counts, k, padding=got.keys)
    print(f"\n[exact f32] {what}: largest error {report['error_in_bounds']:.3f} bounds, {of_the_tolerance(truth, got, KEY_BASE):.3f} of "
          f"1e-5·max(1, |d|), {report['decided']:.1%} of {len(queries)} queries decided")
    return got


def of_the_tolerance(truth, got, key_base=0):
    """The largest |distance − f64 distance of the row named| as a share of the suite's f32 tolerance, 1e-5·max(1, |d|): recorded,
    not asserted — the contract is the bound."""
    found = int(got.counts.min()) if len(got.counts) else 0
    if not found:
        return 0.0
    slots = got.keys[:, :found].astype(np.int64) - key_base
    exact = truth.exact[np.arange(len(slots))[:, None], slots]
    return float((np.abs(got.distances[:, :found].astype(np.float64) - exact) / (util.tolerance("f32") * np.maximum(1.0, np.abs(exact)))).max())


# ---- 1. every pair on both kernels. Row bytes: 128 (one chunk), 132 (one scalar alone in the second chunk; stored pitch 144, the
#         query pitch no multiple of 16), 200 (a 16-byte piece half filled), 384 (three chunks: the staging buffers swap parity from
#         tile to tile), and one row of 16 bytes
PAIRS = [("cos", 32), ("ip", 33), ("ip", 50), ("cos", 96), ("cos", 4)]


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric,ndim", PAIRS, ids=[f"{m}-{n}" for m, n in PAIRS])
def test_every_pair_on_both_kernels(reference, monkeypatch, metric, ndim, tile):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    plan = route(ndim, QUERIES, 10)
    assert plan["wide"] == (tile == 256) and (plan["partitions"], plan["rows_per_partition"]) == ((8, 1280) if tile == 256 else (13, 640))
    assert tile == 64 or (plan["lds_lists"] == 1 and 7 * plan["rows_per_partition"] > ROWS)  # an empty last partition
    case, index, _, _ = planted(metric, ndim)
    hold_to_truth(case, index, 10, f"{metric} {ndim}-d, tile {tile}", cap=ndim > 4)  # (4-d: exempt, see the module's docstring)


# ---- 2. values no 16-bit kind can carry
@pytest.mark.parametrize("tile", [64, 256])
def test_rows_and_queries_forty_binary_orders_apart(reference, monkeypatch, tile):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    assert route(64, QUERIES, 10)["wide"] == (tile == 256)
    case = scaled_case()
    assert np.abs(case.rows).max() > 65504 and 0 < np.abs(case.queries).max() < 2.0 ** -14
    hold_to_truth(case, image_of(case), 10, f"cos 64-d, rows × 2^20, queries × 2^-20, tile {tile}")


# ---- 3. result counts: 1 | 10 | 11 (lists in LDS | in the output arrays) | 16 | 17 (the wide tile | the 64 tile) | 64 | 65 (refused):
#         the route expectations of tests/test_gpu_exact_truth.py. ip keeps a ladder of any length apart (64 rungs: 100 queries fill
#         6 400 of the 8 200 rows)
@pytest.mark.parametrize("k,tile,global_lists,wide,lds_lists", [(1, 256, 0, 1, 1), (10, 256, 0, 1, 1), (10, 256, 1, 1, 0), (11, 256, 0, 1, 0),
                                                                (16, 256, 0, 1, 0), (17, 256, 0, 0, 0), (64, 64, 0, 0, 0)],
                         ids=["1-wide-lds", "10-wide-lds", "10-wide-global-forced", "11-wide-global", "16-wide-global", "17-forced-256-takes-64",
                              "64-tile-64"])
def test_result_counts_at_every_boundary(reference, monkeypatch, k, tile, global_lists, wide, lds_lists):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    if global_lists:
        monkeypatch.setenv("USEARCH_AMD_EXACT_GLOBAL_LISTS", "1")
    plan = route(96, 100, k)
    assert (plan["wide"], plan["lds_lists"]) == (wide, lds_lists)
    case, index, _, _ = planted("ip", 96, queries=100, rungs=64)
    hold_to_truth(case, index, k, f"ip 96-d, k = {k}, tile {tile}{', global lists' if global_lists else ''}")


def test_more_results_than_a_lane_per_entry_are_refused(reference):
    case, index, _, _ = planted("ip", 96, queries=100, rungs=64)
    with pytest.raises(RuntimeError, match=REFUSAL):
        index.search(case.queries, 65, exact="tiled", dtype="f32")


# ---- 4. the default route: nobody forces a tile; more than 512 queries over at least 8 192 rows take the wide one
def nothing_forced(monkeypatch):
    for name in ("USEARCH_AMD_EXACT_TILE", "USEARCH_AMD_EXACT_GLOBAL_LISTS", "USEARCH_AMD_NO_TILED_EXACT"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("count,wide", [(520, 1), (512, 0)])
def test_the_default_route_of_an_index(reference, monkeypatch, count, wide):
    nothing_forced(monkeypatch)
    assert route(96, count, 10)["wide"] == wide
    case, index, _, _ = planted("cos", 96, copies=220)
    hold_to_truth(case, index, 10, f"cos 96-d, {count} queries, nothing forced", count=count)


@pytest.mark.parametrize("count,wide", [(520, 1), (512, 0)])
def test_the_default_route_of_a_raw_f32_matrix(monkeypatch, count, wide):
    """`usearch_amd.exact_search(…, tiled=True)` over a plain f32 matrix: the matrix units on request; keys are row offsets."""
    import usearch_amd
    nothing_forced(monkeypatch)
    assert route(96, count, 10)["wide"] == wide
    case, _, _ = planted_case("cos", 96, copies=220)
    case.assert_decides(10, count=count)
    keys, distances = usearch_amd.exact_search(case.rows, case.queries[:count], 10, metric="cos", tiled=True)
    report = case.truth(count=count).check(keys.astype(np.int64), distances, np.full(count, 10), 10)
    print(f"\n[exact f32] raw cos 96-d, {count} queries: largest error {report['error_in_bounds']:.3f} bounds")


@pytest.mark.parametrize("count,wide", [(520, 1), (512, 0)])
def test_the_same_raw_call_for_f16(monkeypatch, count, wide):
    """The raw-matrix entry is new for the 16-bit kinds too: f16 under ITS truth (tests/exact_truth.py), untouched."""
    import usearch_amd
    from tests import exact_truth
    nothing_forced(monkeypatch)
    plans = [route(96, 520, 10, tile=tile, scalar_bytes=2) for tile in (64, 256)]
    assert route(96, count, 10, scalar_bytes=2)["wide"] == wide
    case = exact_truth.plant("cos", "f16", 96, ROWS, QUERIES, RUNGS, 13, edges=exact_truth.edge_slots(ROWS, plans), copies=220)
    case.assert_decides(10, count=count)
    keys, distances = usearch_amd.exact_search(case.rows, case.queries[:count], 10, metric="cos", tiled=True)
    case.truth(count=count).check(keys.astype(np.int64), distances, np.full(count, 10), 10)


def test_the_raw_call_refuses_a_pair_without_a_tiled_kernel():
    import usearch_amd
    rows = np.random.default_rng(3).standard_normal((64, 8))
    with pytest.raises(RuntimeError, match=REFUSAL):
        usearch_amd.exact_search(rows, rows[:4], 3, metric="cos", tiled=True)  # f64
    with pytest.raises(RuntimeError, match=REFUSAL):
        usearch_amd.exact_search(rows.astype(np.float32), rows[:4].astype(np.float32), 3, metric="pearson", tiled=True)
    with pytest.raises(RuntimeError, match=REFUSAL):
        usearch_amd.exact_search(rows.astype(np.float32), rows[:4].astype(np.float32), 65, metric="cos", tiled=True)
    with pytest.raises(RuntimeError, match=REFUSAL):  # l2sq over f32: see `test_l2sq_over_f32_is_still_refused`
        usearch_amd.exact_search(rows.astype(np.float32), rows[:4].astype(np.float32), 3, metric="l2sq", tiled=True)


# ---- 5. eight query tiles and more: tiles dealt over the XCDs; nine leave a short last round of workgroups that return early
@pytest.mark.parametrize("count,tiles,per_xcd", [(1793, 8, 1), (2049, 9, 2)])
def test_query_tiles_dealt_over_the_xcds(reference, monkeypatch, count, tiles, per_xcd):
    nothing_forced(monkeypatch)
    plan = route(64, count, 10)
    assert (plan["wide"], plan["query_tiles"], plan["tiles_per_xcd"]) == (1, tiles, per_xcd)
    assert plan["workgroups"] == 8 * per_xcd * plan["partitions"] >= tiles * plan["partitions"]
    # the first 300 queries have ladders, the rest are copies of them under a permutation: the cap still holds
    case, index, _, _ = planted("cos", 64, copies=2049 - QUERIES)
    hold_to_truth(case, index, 10, f"cos 64-d, {count} queries ({tiles} query tiles)", count=count)


# ---- 6. tombstones and the caller's bitmap through the wide kernel's `allow_bits`
@pytest.mark.parametrize("filtered", ["tombstones-only", "half", "five-rows", "nothing"])
def test_filters_and_tombstones_through_the_wide_tile(reference, monkeypatch, filtered):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "256")
    assert route(96, QUERIES, 10)["wide"] == 1
    case, index, removed, half = planted("cos", 96, rungs=11, removals=True)  # (11 rungs: 3 300 planted rows fit the 3 780 slots left)
    bits = {"tombstones-only": None, "half": half, "nothing": np.zeros(ROWS, dtype=bool)}.get(filtered)
    if filtered == "five-rows":  # the first and the last member, three between them, and a removed one, which stays out
        bits = np.zeros(ROWS, dtype=bool)
        bits[np.flatnonzero(~removed)[[0, 100, 2000, 5000, -1]]] = True
        bits[5] = True
        assert removed[5] and int((bits & ~removed).sum()) == 5
    allowed = ~removed if bits is None else bits & ~removed
    got = hold_to_truth(case, index, 10, f"cos 96-d, {filtered}", allowed=allowed,
                        filter=None if bits is None else index.filter_bits(bits), cap=filtered in ("tombstones-only", "half"))
    assert int(got.counts[0]) == {"five-rows": 5, "nothing": 0}.get(filtered, 10)


# ---- 7. near-ties that arrive AFTER a query's bound is set: where the wide tile's pruning test (a bound shared by the partitions, a
#         margin of 1e-5) would drop a neighbour if it were not conservative. f32 takes the general fold.
@pytest.mark.parametrize("tile", [64, 256])
def test_near_ties_that_arrive_after_the_bound_is_set(reference, monkeypatch, tile):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    assert route(64, QUERIES, 10)["wide"] == (tile == 256)
    case = near_ties_case()
    hold_to_truth(case, image_of(case), 10, f"cos 64-d near-ties, tile {tile}", cap=False)


# ---- 8. ties: equal rows give equal bits — the same scalars through the same chain, whatever tile or partition they fall in — and
#         come back by slot, the later first
@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric", ["cos"])
def test_equal_rows_across_a_partition_edge_come_back_by_slot(reference, monkeypatch, metric, tile):
    from usearch_amd import Index
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    plan = route(96, QUERIES, 16)
    assert plan["wide"] == (tile == 256) and 1280 % plan["rows_per_partition"] == 0  # row 1 280 begins a partition on either route
    rng = np.random.default_rng(17)
    rows = (rng.standard_normal((ROWS, 96)) * 0.2).astype(np.float32)
    queries = (rng.standard_normal((QUERIES, 96)) * 0.2).astype(np.float32)
    rows[1260:1300] = rows[1260]  # forty equal rows, twenty on either side of the edge
    queries[::50] = rows[1260]
    image, _, _ = util.build_image(ROWS, 96, metric, "f32", vectors=rows, connectivity=4, expansion_add=16)
    got = Index.restore(image).search(queries, 16, exact="tiled")
    truth = exact_truth_f32.Truth(metric, "f32", rows, queries)
    assert np.array_equal(truth.order(16)[0], np.arange(1299, 1283, -1)), "the fixture: sixteen of the forty, the latest slots first"
    for query in range(0, QUERIES, 50):
        assert np.array_equal(got.keys[query].astype(np.int64) - KEY_BASE, np.arange(1299, 1283, -1))
        assert len(set(got.distances[query].view(np.uint32).tolist())) == 1, "equal rows, different bits"
    truth.check(got.keys.astype(np.int64) - KEY_BASE, got.distances, got.counts, 16, padding=got.keys)


# ---- 9. against the wave-per-query kernel, the bit-exact path: f32 fmaf chains per lane and a tree of adds — fewer than ndim
#         roundings on any path and the same closing arithmetic, so the same bound holds for it — the two kernels' distances for one
#         row are at most the two bounds apart, and where the truth decides, they name the same rows
@pytest.mark.parametrize("metric,ndim", [("cos", 96), ("ip", 96)])
def test_against_the_wave_kernel(reference, monkeypatch, metric, ndim):
    nothing_forced(monkeypatch)
    options = dict(queries=100, rungs=64) if metric == "ip" else dict(rungs=11, removals=True)
    case, index, removed, _ = planted(metric, ndim, **options)
    queries = case.queries[:QUERIES]
    truth = case.truth(~removed if removed.any() else None, len(queries))
    tiled = index.search(queries, 10, exact="tiled", dtype="f32")
    wave = index.search(queries, 10, exact=True, dtype="f32")
    assert np.array_equal(tiled.counts, wave.counts)
    decided = truth.decided(10)
    assert decided.mean() >= exact_truth_f32.DECIDED_SHARE
    assert np.array_equal(tiled.keys[decided], wave.keys[decided])
    slots = tiled.keys[decided].astype(np.int64) - KEY_BASE
    bound = truth.bound[np.flatnonzero(decided)[:, None], slots]
    apart = np.abs(tiled.distances[decided].astype(np.float64) - wave.distances[decided].astype(np.float64))
    print(f"\n[exact f32] {metric} {ndim}-d against the wave kernel: at most {(apart / (2 * bound)).max():.3f} of the two bounds apart, "
          f"{(tiled.distances.view(np.uint32) == wave.distances.view(np.uint32)).mean():.1%} of the distances bit-equal")
    assert np.all(apart <= 2 * bound)


# ---- l2sq over f32 is NOT part of this: tests/test_gpu_exact.py asserts that `exact="tiled"` over an l2sq f32 index is refused,
#      and that assertion stands. The refusal, with its message, on every tiled entry; the wave kernel goes on serving the pair.
def test_l2sq_over_f32_is_still_refused(reference):
    import usearch_amd
    from usearch_amd import Index
    rows = util.make_vectors(600, 16, "f32", seed=1)
    image, _, _ = util.build_image(600, 16, "l2sq", "f32", vectors=rows, connectivity=4, expansion_add=16)
    index = Index.restore(image)
    with pytest.raises(RuntimeError, match=REFUSAL):
        index.search(rows[:4], 3, exact="tiled")
    with pytest.raises(RuntimeError, match=REFUSAL):
        usearch_amd.exact_search(rows, rows[:4], 3, metric="l2sq", tiled=True)
    got = index.search(rows[:4], 3, exact=True)
    assert np.array_equal(got.keys[:, 0], np.arange(4) + KEY_BASE)
