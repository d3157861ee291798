"""GPU: whole walks and exact searches over an index in which a few rows hold a NaN component — real data's way of putting NaN
distances next to finite ones in `top`, in the frontier and in the merge. 1 500 × 32 f32 rows under l2sq, built by the reference;
rows 7, 104, 201, … (step 97, sixteen of them) carry one NaN; 40 queries, k = 10.

Keys are NOT compared with the oracle here. The oracle restates the reference, whose `top` places a newcomer by a binary search with
`<` over an array that is not partitioned once it holds a NaN beside numbers: where the newcomer lands, and with it which member a
full buffer drops and what the radius becomes, depends on the search's path. The device cannot follow a path-dependent order from a
register layout; it keeps its own rule in every layout — NaN first, then ascending — so from the first NaN on the two
walks may keep different members. What is pinned instead is everything that does not depend on that choice: the counts, that every
result is a distinct member, that a distance is NaN exactly for the sixteen rows, that every finite distance is the exact wave
kernel's for that pair bit for bit, and the order of each list.
"""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

ROWS, NDIM, WANTED, QUERIES = 1500, 32, 10, 40
NAN_ROWS = np.arange(7, ROWS, 97)[:16]
KEY_BASE = 1000  # `util.build_image` keys row r as r + 1000


@pytest.fixture(scope="module")
def nan_index(reference):
    from usearch_amd import Index
    vectors = util.make_vectors(ROWS, NDIM, "f32", seed=5)
    for row in NAN_ROWS:
        vectors[row, row % NDIM] = np.nan
    image, _, _ = util.build_image(ROWS, NDIM, "l2sq", "f32", vectors=vectors)
    queries = util.make_vectors(QUERIES, NDIM, "f32", seed=6)
    index = Index.restore(image)
    # the exact wave kernel's distance for every (query, row): an exact search that returns every row
    everything = index.search(queries, ROWS, exact=True)
    assert (everything.counts == ROWS).all()
    table = np.zeros((QUERIES, ROWS), dtype=np.uint32)
    rows = (everything.keys - KEY_BASE).astype(np.int64)
    assert all(np.array_equal(np.sort(rows[q]), np.arange(ROWS)) for q in range(QUERIES)), "an exact search of every row lost one"
    np.put_along_axis(table, rows, everything.distances.view(np.uint32), axis=1)
    assert np.array_equal(np.isnan(table.view(np.float32)), np.isin(np.arange(ROWS), NAN_ROWS)[None, :].repeat(QUERIES, 0))
    check_lists(everything.keys, everything.distances, everything.counts, np.full(QUERIES, ROWS), table, "every row")
    return image, index, queries, table


def check_lists(keys, distances, counts, want_counts, table, what):
    assert np.array_equal(np.asarray(counts, dtype=np.int64), np.asarray(want_counts, dtype=np.int64)), f"{what}: counts differ from the oracle's"
    bits = distances.view(np.uint32)
    for q in range(len(keys)):
        n = int(counts[q])
        rows = keys[q, :n].astype(np.int64) - KEY_BASE
        assert len(set(rows.tolist())) == n and ((rows >= 0) & (rows < ROWS)).all(), f"{what}: query {q} returns {keys[q, :n]}"
        is_nan = np.isnan(distances[q, :n])
        assert np.array_equal(is_nan, np.isin(rows, NAN_ROWS)), f"{what}: query {q}: NaN distances {distances[q, :n]} for rows {rows}"
        assert np.array_equal(bits[q, :n][~is_nan], table[q % len(table), rows][~is_nan]), f"{what}: query {q}: not the exact kernel's bits"
        nans = int(is_nan.sum())
        assert is_nan[:nans].all(), f"{what}: query {q}: NaNs are not first: {distances[q, :n]}"
        assert (np.diff(distances[q, nans:n]) >= 0).all(), f"{what}: query {q}: the finite part does not ascend: {distances[q, :n]}"


@pytest.mark.parametrize("frontier", [0, 1])
@pytest.mark.parametrize("expansion", [16, 64, 300])
def test_walks_over_nan_rows(nan_index, expansion, frontier):
    from usearch_amd.index import Tuning
    image, index, queries, table = nan_index
    got = index.search(queries, WANTED, expansion=expansion, tuning=Tuning(frontier=frontier) if frontier else None)
    want = util.oracle_search(image, queries, WANTED, "f32", expansion, lanes=index.lanes_per_row, frontier_in_top=got.stats.frontier == 2)
    if frontier:
        assert got.stats.frontier == 1
    check_lists(got.keys, got.distances, got.counts, want[2], table, f"ef {expansion}, frontier {got.stats.frontier}")
    assert np.isnan(got.distances[np.arange(WANTED)[None, :] < got.counts[:, None]]).any(), "no NaN reached a result: the case is empty"


def test_exact_search_over_nan_rows(nan_index):
    """1 500 rows and 40 queries split into 5 partitions of 300 rows, folded with the earlier position first; 8 200 queries leave one
    partition, where only the buffer orders."""
    image, index, queries, table = nan_index
    want = util.oracle_search(image, queries, WANTED, "f32", exact=True)
    got = index.search(queries, WANTED, exact=True)
    check_lists(got.keys, got.distances, got.counts, want[2], table, "exact, 5 partitions")
    many = np.tile(queries, (205, 1))
    one = index.search(many, WANTED, exact=True)
    check_lists(one.keys, one.distances, one.counts, np.tile(want[2], 205), table, "exact, 1 partition")
    # an exact search has one answer under the rule — the NaN rows first, the later slot in front (new before equal inside a
    # partition, the later partition in front in the fold), then the nearest — and the two splits agree on it
    assert np.array_equal(one.keys[:QUERIES], got.keys) and util.same_float_bits(one.distances[:QUERIES], got.distances)
