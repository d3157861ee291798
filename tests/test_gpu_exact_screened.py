"""GPU: the screened exact search (`exact="screened"`, csrc/exact_screened.hip) — the matrix units rule rows out, the wave kernel
measures the rest — against what tests/test_gpu_exact.py holds `exact=True` to: the oracle's restatement of `search_exact_` in the
kernels' summation layout, bit for bit (keys, distance bits, counts)."""
import functools

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def indexed(metric, ndim, rows, remove=()):
    """Seeded normal rows behind a reference-built image, keys = slots → (image, vectors)."""
    image, vectors, _ = util.build_image(rows, ndim, metric, "f32", seed=181, clustered=False, connectivity=4, expansion_add=16,
                                         keys=np.arange(rows, dtype=np.uint64), remove=remove)
    return image, vectors


def assert_oracle_bits(index, image, queries, wanted, got):
    """Counts, keys and distance bits against the oracle, for every query no NaN distance reaches: where one does, `exact=True` and
    the oracle differ ("Open: the order of NaN distances in `top`") and the route is held to `exact=True` instead."""
    keys, distances, counts, *_ = util.oracle_search(image, queries, wanted, "f32", lanes=index.lanes_per_row, exact=True)
    numbers = ~(np.isnan(got.distances).any(axis=1) | np.isnan(distances).any(axis=1))
    assert np.array_equal(got.counts[numbers], counts[numbers])
    assert np.array_equal(got.keys[numbers], keys[numbers])
    assert util.same_float_bits(got.distances[numbers], distances[numbers])
    return numbers


# every metric, row length (below one staged chunk of 32 scalars, whole 16-byte pieces, a ragged tail, the headline), row count (a row
# tile and two rows; two partitions with a short last one), batch (one query, a tile and one, several tiles) and result count once
@pytest.mark.parametrize("metric,ndim,rows,count,wanted", [
    ("cos", 3, 130, 1, 1), ("ip", 3, 1100, 65, 10), ("l2sq", 24, 130, 300, 10), ("cos", 24, 1100, 65, 64),
    ("ip", 100, 130, 65, 64), ("l2sq", 100, 1100, 300, 1), ("cos", 768, 1100, 300, 10), ("l2sq", 768, 1100, 65, 10),
    ("ip", 768, 130, 1, 10), ("l2sq", 3, 1100, 1, 64), ("cos", 100, 1100, 1, 10), ("ip", 24, 1100, 300, 1)])
def test_screened_exact_search_has_the_oracles_bits_and_measures_few_rows(reference, metric, ndim, rows, count, wanted):
    import usearch_amd
    from usearch_amd import Index
    image, vectors = indexed(metric, ndim, rows)
    queries = util.make_vectors(count, ndim, "f32", seed=182, clustered=False)
    queries[0] = vectors[min(7, rows - 1)]  # a query that is a stored row
    index = Index.restore(image)
    got = index.search(queries, wanted, exact="screened")
    assert assert_oracle_bits(index, image, queries, wanted, got).all()
    # the screen ran: at least the results were measured, never the whole index (what `exact=True` reports, and what an unknown
    # value of `exact` used to fall through to)
    measured = got.computed_per_query
    print(f"measured per query: min {measured.min()} mean {measured.mean():.1f} max {measured.max()} of {rows}")
    assert measured.min() >= min(wanted, rows) and measured.max() < rows
    raw_keys, raw_distances = usearch_amd.exact_search(vectors, queries, wanted, metric=metric, tiled="screened")
    assert np.array_equal(raw_keys, got.keys) and util.same_float_bits(raw_distances, got.distances)


def edge_case(name):
    """→ (metric, rows as vectors, removed keys, queries)"""
    rng = np.random.default_rng(183)
    vectors = rng.standard_normal((600, 40)).astype(np.float32)
    queries = rng.standard_normal((70, 40)).astype(np.float32)
    if name == "equal-rows":  # every pair of a query ties: the buffers overflow, the query goes to the wave kernel whole
        vectors[:] = vectors[0]
        return "l2sq", vectors, (), queries
    if name == "zero-query":
        queries[3] = 0
        vectors[11] = 0
        return "cos", vectors, (), queries
    if name.startswith(("nan-and-huge", "huge")):
        if name.startswith("nan"):
            vectors[17, 5] = np.nan
        vectors[400, 2] = 1e30
        queries[5, 1] = 1e30
        return name.rsplit("-", 1)[1], vectors, (), queries
    assert name == "removed"
    return "ip", vectors, tuple(range(4, 600, 9)), queries


@pytest.mark.parametrize("name", ["equal-rows", "zero-query", "nan-and-huge-l2sq", "nan-and-huge-cos", "huge-l2sq", "huge-cos", "removed"])
def test_screened_exact_search_hands_over_what_it_cannot_decide(reference, name):
    """Every case bit for bit against `exact=True` on the same index — the route's promise, NaN cells included: both come from the
    GPU — and against the oracle for every query no NaN reaches. In the two `nan-and-huge` cases that is no query at all: every query
    meets the NaN row, the wave kernel's `top` keeps a NaN in front of every number even when it is full, the reference's `lower_bound`
    insertion moves it along and drops it (l2sq, query 0: keys 17, 41, 45, 568, … here and from `exact=True`, 41, 45, 568, 317, … from
    the oracle). Those two cases cannot be bit-equal to the oracle while `exact=True` is not; the `huge` cases — the same data without
    the NaN — are."""
    from usearch_amd import Index
    metric, vectors, removed, queries = edge_case(name)
    image, _, _ = util.build_image(len(vectors), vectors.shape[1], metric, "f32", vectors=vectors, connectivity=4, expansion_add=16,
                                   keys=np.arange(len(vectors), dtype=np.uint64), remove=removed)
    index = Index.restore(image)
    got = index.search(queries, 10, exact="screened")
    wave = index.search(queries, 10, exact=True)
    assert np.array_equal(got.counts, wave.counts) and np.array_equal(got.keys, wave.keys)
    assert util.same_float_bits(got.distances, wave.distances)
    numbers = assert_oracle_bits(index, image, queries, 10, got)
    assert numbers.all() or name.startswith("nan")
    assert not np.isin(got.keys, removed).any()
    if name == "equal-rows":
        assert np.all(got.computed_per_query == len(vectors))


def test_screened_exact_search_under_a_filter(reference):
    from oracle import oraclebind
    from usearch_amd import Index
    image, vectors = indexed("l2sq", 40, 1100, remove=(5, 17, 300))
    queries = util.make_vectors(70, 40, "f32", seed=184, clustered=False)
    index = Index.restore(image)
    oracle = oraclebind.OracleIndex(image)
    got = index.search(queries, 7, exact="screened", filter=index.filter_key_range(100, 899))  # tiled = 2 of the filtered entry
    for q, query in enumerate(queries):
        found, keys, distances = oracle.filtered_search(query, 7, lambda key: 100 <= key <= 899, dtype="f32", lanes=index.lanes_per_row,
                                                        exact=True)
        assert int(got.counts[q]) == found
        assert np.array_equal(got.keys[q], keys) and util.same_float_bits(got.distances[q], distances), q


@pytest.mark.parametrize("metric,dtype,wanted", [("cos", "f16", 10), ("pearson", "f32", 10), ("cos", "f32", 65)])
def test_screened_exact_search_refuses_other_pairs_by_name(reference, metric, dtype, wanted):
    import usearch_amd
    image, _, _ = util.build_image(300, 16, metric, dtype, seed=185)
    queries = util.make_vectors(3, 16, dtype, seed=186)
    with pytest.raises(RuntimeError, match="No screened exact-search kernel for this metric / scalar kind / result count"):
        usearch_amd.Index.restore(image).search(queries, wanted, exact="screened")
    with pytest.raises(RuntimeError, match="No screened exact-search kernel for this metric / scalar kind / result count"):
        usearch_amd.exact_search(queries, queries, wanted, metric=metric, tiled="screened")
