"""GPU: the distance kernels at the edges of the value domain (tests/distance_edges.py) — bit-exact against the oracle in the
kernels' summation layout, exact or within tolerance against its reference loop order, the same result class (finite, ±inf,
NaN) as the real reference on every case, at the lane count the engine picks and at every other one it can be forced to —
and exact search where such distances still have a well-defined order.

No NaN distance reaches a search here and no graph is walked over non-finite data: `sorted_insert` ranks by counting `<`, the
reference by binary search, and under NaN the two need not agree (open points)."""
import functools

import numpy as np
import pytest

from tests import distance_edges as edges
from tests import util

pytestmark = pytest.mark.gpu


def _groups(metric, dtype):
    """The table's cases of one pair by ndim → [(ndim, names, queries [Q, cols], rows [N ≤ 64, cols], slot of each case's row)]."""
    by_ndim = {}
    for name, _, _, ndim, a, b in edges.cases(metric, dtype):
        by_ndim.setdefault(ndim, []).append((name, a, b))
    for ndim, found in by_ndim.items():
        rows, slot_of, slots = [], {}, []
        for _, _, b in found:
            key = b.tobytes()
            if key not in slot_of:
                slot_of[key] = len(rows)
                rows.append(b)
            slots.append(slot_of[key])
        ordinary = util.make_vectors(6, ndim, dtype, seed=50 + ndim, clustered=False, metric=metric)  # something for the builder to link
        rows = np.concatenate([np.stack(rows), ordinary])
        assert len(rows) <= 64
        yield ndim, [name for name, _, _ in found], np.stack([a for _, a, _ in found]), rows, np.array(slots, dtype=np.uint32)


def _forced_lanes(metric, dtype, nbytes):
    """The lane counts USEARCH_AMD_LANES can force for such rows besides the one the engine picks: the other one of 1 and 2 and, where
    the row has the chunks for it, 4 (built for the common pairs only) and 8 on rows of ≤ 128 bytes; 2 and 4 on longer rows."""
    picked, _ = edges.row_geometry(nbytes)
    out = []
    for forced in (1, 2, 4, 8) if picked <= 2 else (2, 4):
        lanes, _ = edges.row_geometry(nbytes, forced)
        if lanes == forced and lanes != picked and (forced != 4 or (metric, dtype) in edges.G4_PAIRS):
            out.append(forced)
    return out


def measure_pair(metric, dtype, setenv, delenv):
    """Runs `Index.distances` over every case of the pair, at the picked lane count and at every forced one.
    → records (name, ndim, lanes, gpu, oracle in that layout, oracle in loop order, reference), all np.float32."""
    from oracle import oraclebind, refbind
    from usearch_amd import Index
    records = []
    for ndim, names, queries, rows, slots in _groups(metric, dtype):
        image, _, _ = util.build_image(len(rows), ndim, metric, dtype, vectors=rows, connectivity=4, expansion_add=16)
        loop = [np.float32(oraclebind.distance(queries[i], rows[slots[i]], metric, dtype, ndim, 0)) for i in range(len(names))]
        real = [np.float32(refbind.distance(queries[i], rows[slots[i]], metric, dtype, ndim)) for i in range(len(names))]
        nbytes = edges.bytes_per_vector(dtype, ndim)
        for forced in [0] + _forced_lanes(metric, dtype, nbytes):
            if forced:
                setenv("USEARCH_AMD_LANES", str(forced))
            try:
                index = Index.restore(image)  # the geometry is fixed when the image is uploaded
            finally:
                if forced:
                    delenv("USEARCH_AMD_LANES")
            lanes = index.lanes_per_row
            assert lanes == edges.row_geometry(nbytes, forced)[0], "tests/distance_edges.py no longer restates row_geometry"
            got = index.distances(queries, slots[:, None])[:, 0]
            for i, name in enumerate(names):
                layout = np.float32(oraclebind.distance(queries[i], rows[slots[i]], metric, dtype, ndim, lanes))
                records.append((name, ndim, lanes, np.float32(got[i]), layout, loop[i], real[i]))
    return records


def same_bits_or_both_nan(a, b) -> bool:
    return bool((np.isnan(a) and np.isnan(b)) or np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32))


def within(got, want, tolerance) -> bool:
    """Same class, and a finite pair within tolerance · max(1, |want|)."""
    if edges.result_class(got) != edges.result_class(want):
        return False
    return not np.isfinite(want) or abs(float(got) - float(want)) <= tolerance * max(1.0, abs(float(want)))


def judge(metric, dtype, records):
    """The asserts of tests/test_gpu_distances.py, case by case → the records that miss one, with which one."""
    tolerance = util.tolerance(dtype)
    wrong = []
    for record in records:
        name, ndim, lanes, got, layout, loop, real = record
        what = []
        if util.layout_exact(metric) and not same_bits_or_both_nan(got, layout):
            what.append("layout")
        if dtype in ("i8", "b1") and metric != "pearson":
            if not same_bits_or_both_nan(got, loop):
                what.append("loop")
        elif not within(got, loop, tolerance):
            what.append("tolerance")
        if edges.result_class(got) != edges.result_class(real):
            what.append("class")
        if what:
            wrong.append((name, ndim, lanes, what, float(got), float(layout), float(loop), float(real)))
    return wrong


@pytest.mark.parametrize("metric,dtype", edges.PAIRS)
def test_distances_over_the_edge_table(reference, monkeypatch, metric, dtype):
    records = measure_pair(metric, dtype, monkeypatch.setenv, monkeypatch.delenv)
    assert {lanes for _, _, lanes, *_ in records} >= ({1} if metric == "haversine" else {1, 2, 8})
    wrong = judge(metric, dtype, records)
    assert not wrong, (f"{len(wrong)} of {len(records)} (name, ndim, lanes, missed, gpu, oracle layout, oracle loop, reference): "
                       f"{wrong[:10]}")


@pytest.mark.parametrize("metric,dtype", [("pearson", "f32"), ("divergence", "f16"), ("cos", "f64"), ("tanimoto", "b1")])
def test_a_forced_lane_count_without_a_build_is_refused(reference, monkeypatch, metric, dtype):
    """G = 4 is built for the common pairs only: forcing it elsewhere is an error by name, not another kernel."""
    from usearch_amd import Index
    image, vectors, _ = util.build_image(20, 1024, metric, dtype, seed=3, connectivity=4, expansion_add=16)
    monkeypatch.setenv("USEARCH_AMD_LANES", "4")
    index = Index.restore(image)
    monkeypatch.delenv("USEARCH_AMD_LANES")
    assert index.lanes_per_row == 4
    with pytest.raises(RuntimeError):
        index.distances(vectors[:2], np.zeros((2, 1), dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
#  Exact search where the order is still well defined
# ---------------------------------------------------------------------------------------------------------------------

def _assert_exact_matches_oracle(image, queries, k, dtype):
    from usearch_amd import Index
    index = Index.restore(image)
    got = index.search(queries, k, exact=True, dtype=dtype)
    keys, distances, counts, *_ = util.oracle_search(image, queries, k, dtype, lanes=index.lanes_per_row, exact=True)
    assert not np.isnan(distances).any(), "this test must stay clear of NaN distances"
    assert np.array_equal(got.counts, counts)
    assert np.array_equal(got.keys, keys), "ties must resolve like lower_bound insertion in slot order"
    assert util.same_float_bits(got.distances, distances)
    return got


def test_exact_search_ranks_plus_infinity_last_and_its_ties_in_slot_order(reference):
    """l2sq / f16, 60 rows of which 52 carry one +inf component: every query finds its 8 finite rows, then +inf ties."""
    n, ndim, k = 60, 40, 10
    rows = util.make_vectors(n, ndim, "f16", seed=61, clustered=False)
    finite = np.array([3, 11, 17, 18, 30, 41, 42, 59])
    for slot in np.setdiff1d(np.arange(n), finite):
        rows[slot, (7 * slot) % ndim] = np.inf if slot % 3 else -np.inf
    image, _, _ = util.build_image(n, ndim, "l2sq", "f16", vectors=rows, connectivity=4, expansion_add=16)
    queries = util.make_vectors(12, ndim, "f16", seed=62, clustered=False)
    got = _assert_exact_matches_oracle(image, queries, k, "f16")
    assert np.isposinf(got.distances[:, 8:]).all() and np.isfinite(got.distances[:, :8]).all()
    assert np.array_equal(np.sort(got.keys[:, :8], axis=1), np.tile(finite + 1000, (12, 1)))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_exact_search_ranks_minus_infinity_first_and_finite_values_of_both_signs(reference, dtype):
    """ip: 1 - Σab is -inf for rows whose one infinite component has the sign of the query's, +inf for the others, and finite of
    either sign for ordinary rows."""
    n, ndim, k = 200, 33, 10
    rows = util.make_vectors(n, ndim, dtype, seed=63, clustered=False)
    rows[rows == 0] = 1
    rows[5:190:37, 4] = np.inf     # 5 rows
    rows[9:190:23, 4] = -np.inf    # 8 rows
    image, _, _ = util.build_image(n, ndim, "ip", dtype, vectors=rows, connectivity=4, expansion_add=16)
    queries = util.make_vectors(16, ndim, dtype, seed=64, clustered=False)
    queries[queries == 0] = 1      # 0 · inf would be NaN
    got = _assert_exact_matches_oracle(image, queries, k, dtype)
    assert np.isneginf(got.distances[:, :5]).all() and np.isfinite(got.distances[:, 8:]).all()
    assert (got.distances[:, 8:] < 0).any() and not np.isposinf(got.distances).any()
    # the other end of the order: with more results than finite rows the +inf rows close the list
    wide = _assert_exact_matches_oracle(image, queries[:4], n, dtype)
    assert np.isinf(wide.distances[:, -5:]).all() and (wide.distances[:, -5:] > 0).all()
    assert (wide.distances > 0).any() and (wide.distances < 0).any()


def test_exact_search_orders_the_negative_cosine_of_i8_before_zero(reference):
    """cos / i8 at d = 1041: a row of 127s against itself or against a row of 64s is -1.19e-7, a zero row is 0 by the reference's
    `ab == 0 → 0`."""
    n, ndim, k = 120, 1041, 10
    rows = edges.full_range_i8(n, ndim, 65)
    rows[10:16] = 127
    rows[30:34] = 0
    rows[50:53] = 64
    rows[70:73] = -128
    image, _, _ = util.build_image(n, ndim, "cos", "i8", vectors=rows, connectivity=4, expansion_add=16)
    queries = np.concatenate([np.full((1, ndim), 127, dtype=np.int8), np.full((1, ndim), -128, dtype=np.int8),
                              np.zeros((1, ndim), dtype=np.int8), edges.full_range_i8(9, ndim, 66)])
    got = _assert_exact_matches_oracle(image, queries, k, "i8")
    assert got.distances[0, 0] == -np.float32(2.0 ** -23) and (got.distances[0] == 0).any()
    # nine rows at -1.19e-7 (slots 50-52 and 10-15), then the zero rows: among equal distances the later slot first, like lower_bound
    assert np.array_equal(got.keys[0], np.array([52, 51, 50, 15, 14, 13, 12, 11, 10, 33]) + 1000)
    assert np.array_equal(got.distances[0], np.array([-2.0 ** -23] * 9 + [0.0], dtype=np.float32))


@functools.lru_cache(maxsize=None)
def _full_range_i8_image(metric, ndim, n):
    rows = edges.full_range_i8(n, ndim, 67 + ndim)
    rows[::97] = -128  # whole rows at the end of the range, and their mirror
    rows[1::97] = 127
    removed = tuple(int(key) for key in np.arange(5, n, 13)[:100] + 1000)
    image, _, _ = util.build_image(n, ndim, metric, "i8", vectors=rows, remove=removed, connectivity=4, expansion_add=16)
    return image, rows, removed


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric,ndim,n", [(metric, ndim, 5003) for metric in ("l2sq", "cos", "ip") for ndim in (96, 1024)])
def test_tiled_exact_search_is_bit_identical_over_the_full_i8_range(reference, monkeypatch, metric, ndim, n, tile):
    """The matrix-unit kernels over rows that reach -128 and 127, at d = 96 and at d = 1 024: the same keys, distance bits and counts
    as the wave-per-query kernel."""
    from usearch_amd import Index
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    image, rows, removed = _full_range_i8_image(metric, ndim, n)
    queries = edges.full_range_i8(131 if tile == 64 else 700, ndim, 68)
    queries[:20] = rows[:20]
    queries[20], queries[21] = -128, 127
    index = Index.restore(image)
    exact = index.search(queries, 10, exact=True)
    tiled = index.search(queries, 10, exact="tiled")
    assert np.array_equal(exact.counts, tiled.counts)
    assert np.array_equal(exact.keys, tiled.keys)
    assert util.same_float_bits(exact.distances, tiled.distances)
    assert not np.isin(tiled.keys, removed).any()
