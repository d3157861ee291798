"""`Index.clustering` (usearch_amd/csrc/clustering.hip) against the model of tests/cluster_model.py fed by device code that was there
before it — `Index.cluster(vectors, level)` and `Index.distances`, both pinned to the oracle by older tests — and against what the
reference recorded (tests/golden/cluster/). Keys, distance bits and every number of the statistics have to agree."""
import functools
import glob
import os

import numpy as np
import pytest

import usearch_amd
from oracle import refbind
from tests import cluster_model, util
from tests.cluster_feeds import DeviceFeed

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")
STATS = ("clusters", "unique_before_merge", "merge_cycles", "mapping_passes", "visited_members", "computed_distances", "level")
PAIRS = [("l2sq", "i8", 33, 2000), ("hamming", "b1", 72, 1500), ("cos", "f16", 40, 2500), ("cos", "f32", 24, 3000), ("ip", "bf16", 64, 2000)]


@functools.lru_cache(maxsize=None)
def device_index(metric, dtype, ndim, n, seed=11, duplicates=False, remove=()):
    """→ (Index, DeviceFeed, vectors): connectivity 4, so that a few thousand members stack up to `max_level` ≥ 3."""
    assert refbind.available(), "oracle/_ref/libusearch_ref.so is missing: build() makes it where the reference is mounted"
    vectors = util.make_vectors(n, ndim, dtype, seed, metric=metric)
    if duplicates:  # every row twice: equal merge distances
        vectors = np.ascontiguousarray(np.repeat(vectors[: n // 2], 2, axis=0))
    image, vectors, _ = util.build_image(n, ndim, metric, dtype, seed=seed, connectivity=4, vectors=vectors, remove=remove)
    index = usearch_amd.Index.restore(image, device=0)
    feed = DeviceFeed(index, image, vectors, dtype)
    assert feed.facts.max_level >= 3
    return index, feed, vectors


def assert_same(got: usearch_amd.Clustering, model: dict, what: str = ""):
    assert np.array_equal(got.matches.keys[:, 0], model["keys"]), f"{what}: keys differ from the model's"
    assert util.same_float_bits(got.matches.distances[:, 0], model["distances"]), f"{what}: distance bits differ from the model's"
    for name in STATS:
        assert got.stats[name] == model[name], f"{what}: {name} is {got.stats[name]}, the model says {model[name]}"


@pytest.mark.parametrize("count", [1, 63, 64, 65, 2000])
@pytest.mark.parametrize("metric,dtype,ndim,n", PAIRS)
def test_device_equals_model(metric, dtype, ndim, n, count):
    index, feed, _ = device_index(metric, dtype, ndim, n)
    queries = util.make_vectors(count, ndim, dtype, seed=12 + count, metric=metric)
    model = feed.run(queries, 6, 5)
    got = index.clustering(vectors=queries, min_count=6, max_count=5, dtype=dtype)
    assert_same(got, model, f"{metric}/{dtype} × {count}")
    assert got.matches.visited_members == model["visited_members"] and len(got.matches) == count


def test_every_query_its_own_centroid_many_popularity_ties():
    index, feed, vectors = device_index("l2sq", "i8", 33, 2000)
    members = np.flatnonzero(feed.facts.levels >= 2)
    queries = np.ascontiguousarray(vectors[members])  # a member of level ≥ 2 reaches itself on level 2
    model = feed.run(queries, 100, 7)
    assert model["popularity_ties"] and model["unique_before_merge"] > 60 and model["merge_cycles"] > 50
    assert_same(index.clustering(vectors=queries, min_count=100, max_count=7), model)


def test_equal_merge_distances_go_to_the_lowest_position():
    """Hamming distances over 72 bits are small integers: several candidates of a cycle are equally near, duplicated rows included."""
    index, feed, _ = device_index("hamming", "b1", 72, 1500, duplicates=True)
    queries = util.make_vectors(500, 72, "b1", seed=31)
    model = feed.run(queries, 20, 4)
    assert model["merge_cycles"] >= 4
    assert any(runner_up is not None and runner_up == winner for winner, runner_up in model["margins"]), "no equal merge distances met"
    assert_same(index.clustering(vectors=queries, min_count=20, max_count=4), model)


@pytest.mark.parametrize("metric,dtype,ndim,n", [PAIRS[0], PAIRS[3]])
def test_one_cluster_one_cycle_and_a_long_chain(metric, dtype, ndim, n):
    index, feed, _ = device_index(metric, dtype, ndim, n)
    queries = util.make_vectors(700, ndim, dtype, seed=41, metric=metric)
    model = feed.run(queries, 20, 1)  # max_count = 1: everything ends in one centroid
    assert model["clusters"] == 1 and model["merge_cycles"] == model["unique_before_merge"] - 1
    longest = max(cluster_model.chain_length(slot, model["merged_into"]) for slot in model["merged_into"])
    assert longest >= 3, f"the longest trace chain has {longest} hops"
    got = index.clustering(vectors=queries, min_count=20, max_count=1, dtype=dtype)
    assert_same(got, model)
    assert len(np.unique(got.matches.keys)) == 1
    unique = model["unique_before_merge"]
    model = feed.run(queries, 20, unique - 1)  # U − max_count = 1
    assert model["merge_cycles"] == 1
    assert_same(index.clustering(vectors=queries, min_count=20, max_count=unique - 1, dtype=dtype), model)


def test_refine_down_to_level_one_and_min_count_above_every_level():
    index, feed, vectors = device_index("cos", "f32", 24, 3000)
    queries = np.ascontiguousarray(np.repeat(vectors[5:6], 40, axis=0))  # co-located: one centroid on every level
    model = feed.run(queries, 3, 3)
    assert model["level"] == 1 and model["mapping_passes"] >= 3
    assert_same(index.clustering(vectors=queries, min_count=3, max_count=3), model)
    queries = util.make_vectors(300, 24, "f32", seed=51)
    model = feed.run(queries, 10 ** 6, 9)  # no level has that many nodes: level 1, then merges down to 9
    assert model["level"] == 1 and model["clusters"] == 9
    assert_same(index.clustering(vectors=queries, min_count=10 ** 6, max_count=9), model)


def test_min_count_zero_is_the_level_one_descent():
    index, feed, _ = device_index("hamming", "b1", 72, 1500)
    queries = util.make_vectors(200, 72, "b1", seed=61)
    model = feed.run(queries)
    assert model["level"] == 1 and model["merge_cycles"] == 0
    got = index.clustering(vectors=queries)
    assert_same(got, model)
    keys, distances, _, _ = index.cluster(queries, 1)
    assert np.array_equal(got.matches.keys[:, 0], keys) and util.same_float_bits(got.matches.distances[:, 0], distances)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))), ids=os.path.basename)
def test_device_equals_the_reference_recorded(path):
    fixture = np.load(path)
    dtype = str(fixture["dtype"])
    index = usearch_amd.Index.restore(fixture["image"], device=0)
    config = dict(min_count=int(fixture["min_count"]) or None, max_count=int(fixture["max_count"]) or None)
    if int(fixture["by_keys"]):
        got = index.clustering(keys=fixture["queries"], **config)
    else:
        got = index.clustering(vectors=fixture["queries"], dtype=dtype, **config)
    assert got.stats["clusters"] == int(fixture["clusters"])
    assert got.stats["visited_members"] == int(fixture["visited_members"])
    assert got.stats["computed_distances"] == int(fixture["computed_distances"])
    if dtype in ("i8", "b1"):
        assert np.array_equal(got.matches.keys[:, 0], fixture["cluster_keys"])
        assert util.same_float_bits(got.matches.distances[:, 0], fixture["cluster_distances"])
    else:
        recorded = lambda queries, k: (fixture["cluster_keys"][:, None], fixture["cluster_distances"][:, None],  # noqa: E731
                                       np.ones(len(queries), dtype=np.uint64))
        util.assert_float_parity(got.matches.keys, got.matches.distances, got.matches.counts, recorded, fixture["queries"], 1, dtype, path)


def test_members_as_queries():
    index, feed, vectors = device_index("hamming", "b1", 72, 1500)
    some = feed.facts.keys[np.random.default_rng(71).choice(1500, 333, replace=False)]
    assert_same(index.clustering(keys=some, min_count=6, max_count=4), feed.run_members(some, 6, 4), "explicit keys")
    everybody = index.clustering(min_count=6, max_count=4)
    assert np.array_equal(everybody.queries, feed.facts.keys)
    assert_same(everybody, feed.run_members(feed.facts.keys, 6, 4), "all members")
    with pytest.raises(RuntimeError, match="Key missing!"):
        index.clustering(keys=np.array([1000, 7], dtype=np.uint64), min_count=6, max_count=4)


def test_removed_members_are_neither_queries_nor_centroids():
    """Members of level 0 are removed: no descent to a level above ends on one (the descent itself, like the reference's, does not
    ask the predicate: index.hpp:3123), and the all-members form leaves them out of the queries."""
    _, whole, _ = device_index("l2sq", "i8", 33, 2000)
    ground = np.flatnonzero(whole.facts.levels == 0)
    removed = tuple(int(key) for key in whole.facts.keys[np.random.default_rng(81).choice(ground, 300, replace=False)])
    index, feed, _ = device_index("l2sq", "i8", 33, 2000, remove=removed)
    live = feed.facts.keys[feed.facts.keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    assert len(live) == 1700
    got = index.clustering(min_count=6, max_count=5)
    assert np.array_equal(got.queries, live)
    assert not np.isin(got.matches.keys, np.array(removed + (0xFFFFFFFFFFFFFFFF,), dtype=np.uint64)).any()
    assert_same(got, feed.run_members(live, 6, 5))
    with pytest.raises(RuntimeError, match="Key missing!"):
        index.clustering(keys=np.array([removed[0]], dtype=np.uint64), min_count=6, max_count=5)


def test_a_removed_member_of_the_level_stays_a_centroid_under_the_free_key():
    """The descent, like the reference's (index.hpp:3123), does not ask whether a member was removed. Two members of level 2 are
    removed and queried with their own rows: each is an entry of its own (the reference would fold them into one under the free
    key), told apart by slot, reported under the free key while it survives, merged like any other entry when it does not."""
    free = 0xFFFFFFFFFFFFFFFF
    _, whole, vectors = device_index("l2sq", "i8", 33, 2000)
    a, b = (int(slot) for slot in np.flatnonzero(whole.facts.levels == 2)[[3, 17]])
    removed = (int(whole.facts.keys[a]), int(whole.facts.keys[b]))
    index, feed, _ = device_index("l2sq", "i8", 33, 2000, remove=removed)
    assert feed.facts.keys[a] == free and feed.facts.keys[b] == free
    queries = np.ascontiguousarray(np.concatenate([util.make_vectors(300, 33, "i8", seed=83), np.repeat(vectors[a:a + 1], 7, axis=0),
                                                   np.repeat(vectors[b:b + 1], 4, axis=0)]))
    model = feed.run(queries, 100, 10 ** 6)  # level 2 (118 nodes) gives fewer than 100 centroids: level 1, where the two exist too
    assert model["level"] == 1 and model["mapping_passes"] == 2 and model["merge_cycles"] == 0 and {a, b} <= set(model["merged_into"])
    got = index.clustering(vectors=queries, min_count=100, max_count=10 ** 6)
    assert_same(got, model, "removed centroids, no merges")
    assert (got.matches.keys[300:, 0] == np.uint64(free)).all() and (got.matches.distances[300:, 0] == 0).all()
    model = feed.run(queries, 100, 12)
    assert model["merge_cycles"] > 10
    assert_same(index.clustering(vectors=queries, min_count=100, max_count=12), model, "removed centroids, merged")
    everybody = index.clustering(min_count=100, max_count=12)  # the two are no queries, and may still be centroids
    live = feed.facts.keys[feed.facts.keys != np.uint64(free)]
    assert np.array_equal(everybody.queries, live)
    assert_same(everybody, feed.run_members(live, 100, 12), "all live members")


def test_errors_by_name_and_the_empty_batch():
    index, _, _ = device_index("l2sq", "i8", 33, 2000)
    queries = util.make_vectors(10, 33, "i8", seed=91)
    with pytest.raises(RuntimeError, match="max_clusters"):
        index.clustering(vectors=queries, min_count=5)
    with pytest.raises(ValueError, match="not both"):
        index.clustering(vectors=queries, keys=np.array([1000], dtype=np.uint64), min_count=5, max_count=5)
    empty = index.clustering(vectors=queries[:0], min_count=5, max_count=5, dtype="i8")
    assert len(empty.matches) == 0 and empty.matches.keys.shape == (0, 1) and empty.stats["clusters"] == 0
    image, _, _ = util.build_image(12, 33, "l2sq", "i8", seed=92, connectivity=16)  # a dozen members: one level at most
    small = usearch_amd.Index.restore(image, device=0)
    assert small.max_level < 2
    with pytest.raises(RuntimeError, match="Index too small to cluster!"):
        small.clustering(vectors=queries, min_count=2, max_count=3)


def test_two_runs_give_identical_bytes_and_cluster_is_left_alone():
    index, _, _ = device_index("cos", "f16", 40, 2500)
    queries = util.make_vectors(1000, 40, "f16", seed=95)
    before = index.cluster(queries, 2)
    first = index.clustering(vectors=queries, min_count=20, max_count=3)
    second = index.clustering(vectors=queries, min_count=20, max_count=3)
    assert first.matches.keys.tobytes() == second.matches.keys.tobytes()
    assert first.matches.distances.tobytes() == second.matches.distances.tobytes()
    assert {name: first.stats[name] for name in STATS} == {name: second.stats[name] for name in STATS}
    after = index.cluster(queries, 2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


def test_members_of_and_subcluster():
    index, feed, _ = device_index("l2sq", "i8", 33, 2000)
    queries = util.make_vectors(600, 33, "i8", seed=97)
    got = index.clustering(vectors=queries, min_count=6, max_count=3)
    centroids, popularity = got.centroids_popularity
    assert len(centroids) == got.stats["clusters"] == 3 and int(popularity.sum()) == 600
    biggest = int(centroids[np.argmax(popularity)])
    members = got.members_of(biggest)
    assert len(members) == int(popularity.max())
    assert np.array_equal(members, queries[got.members_of(biggest, queries_only=True)])
    again = got.subcluster(biggest, min_count=6, max_count=2)
    assert len(again.matches) == len(members)
    assert_same(again, feed.run(members, 6, 2), "subcluster")


def test_an_index_built_on_the_device_clusters_its_members():
    """`BuiltIndex.clustering`: the builder's snapshot, keys given at build time; the model runs over the image it saves."""
    vectors = util.make_vectors(1200, 33, "i8", seed=101)
    keys = 7000 + np.arange(1200, dtype=np.uint64)
    built = usearch_amd.build(vectors, metric="l2sq", dtype="i8", keys=keys, connectivity=4)
    got = built.clustering(min_count=5, max_count=3)
    image = built.save_buffer()
    feed = DeviceFeed(usearch_amd.Index.restore(image, device=0), image, vectors, "i8")
    assert feed.facts.max_level >= 2 and np.array_equal(feed.facts.keys, keys) and np.array_equal(got.queries, keys)
    assert_same(got, feed.run_members(keys, 5, 3), "all members of a built index")
    queries = util.make_vectors(300, 33, "i8", seed=102)
    assert_same(built.clustering(vectors=queries, min_count=5, max_count=3), feed.run(queries, 5, 3), "vectors over a built index")
