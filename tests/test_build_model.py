"""Is tests/build_model.py the reference's? (CPU only.) The model is the yardstick of the device builder
(tests/test_gpu_build_model.py compares GPU-built graphs with it list for list), so its own rules are pinned here first:

- `refine` and the reverse-link rule against the COMPILED reference: one `add` of the real `index_gt` (include/usearch/index.hpp
  2759-2879) must change the graph exactly as the model says — the new member's list, every touched neighbour's list, nothing else;
- a graph the model builds on its own is a well-formed HNSW graph, as good as the reference's under the same search;
- the corner cases of `refine` that the kernels' shortcuts make interesting, on points one can check by hand.
"""
import numpy as np
import pytest

from oracle import oraclebind
from tests import build_model, util


# ---- refine, by hand: squared Euclidean distance between points of the plane; the centre is the origin

def plane(points):
    def dist(a, b):
        return (points[a][0] - points[b][0]) ** 2 + (points[a][1] - points[b][1]) ** 2
    return dist


def from_origin(points):
    return sorted((x * x + y * y, slot) for slot, (x, y) in enumerate(points))


def test_refine_takes_a_small_set_whole():
    points = [(1.0, 0.0), (1.5, 0.0), (2.2, 0.0)]  # on one ray: the first would strike both others
    candidates = from_origin(points)
    assert build_model.refine(candidates, 4, plane(points)) == candidates  # fewer than needed: index.hpp:4284-4285


def test_refine_prunes_a_set_of_exactly_the_needed_size():
    points = [(1.0, 0.0), (1.5, 0.0), (2.2, 0.0)]
    candidates = from_origin(points)
    assert build_model.refine(candidates, 3, plane(points)) == candidates[:1]  # `<`, not `<=`: three candidates ARE refined


def test_refine_strikes_everything_behind_the_first():
    points = [(1.0, 0.0), (1.5, 0.0), (2.2, 0.0), (3.0, 0.1), (4.0, -0.1)]
    candidates = from_origin(points)
    assert build_model.refine(candidates, 3, plane(points)) == candidates[:1]


def test_refine_asks_every_kept_node_not_only_the_first():
    # 0 and 1 keep each other (1 is closer to the origin than to 0); 2 is far from 0 but next to 1; 3 is far from all of them
    points = [(1.0, 0.0), (0.0, 1.5), (0.2, 2.5), (-3.0, -0.5)]
    candidates = from_origin(points)
    dist = plane(points)
    assert dist(0, 2) > candidates[2][0] > dist(1, 2)  # struck by the second kept node, not by the first
    assert [slot for _, slot in build_model.refine(candidates, 4, dist)] == [0, 1, 3]
    assert [slot for _, slot in build_model.refine(candidates, 2, dist)] == [0, 1]  # stops at `needed`


def test_the_model_refuses_to_settle_a_tie():
    points = [(1.0, 0.0), (0.0, 1.0), (5.0, 5.0)]  # 0 and 1 are equally far from the origin
    with pytest.raises(build_model.Tie):
        build_model.refine(from_origin(points), 2, plane(points))
    points = [(1.0, 0.0), (0.5, 1.0), (9.0, 9.0)]  # 1 is 1.25 from the origin and 1.25 from kept 0: struck or not?
    with pytest.raises(build_model.Tie):
        build_model.refine(from_origin(points), 2, plane(points))
    # two members on either side of the query (slot 2, no member): the descent cannot say which of them is closer
    sides = plane([(1.0, 0.0), (-1.0, 0.0), (0.0, 0.0)])
    graph = [[[1], [1]], [[0], [0]]]
    with pytest.raises(build_model.Tie):
        build_model.beam(graph, [1, 1], 0, 1, 2, 0, 4, 2, sides)


# ---- against the compiled reference: what ONE `add` does to the graph

PIN_SIZES = [500, 509, 517, 526, 534, 543, 551, 560, 568, 577, 585, 594]
PIN_CASES = [
    # metric, ndim, connectivity, expansion_add
    ("l2sq", 16, 4, 40), ("l2sq", 16, 8, 100), ("l2sq", 16, 3, 100),
    ("cos", 24, 3, 100), ("cos", 24, 4, 100), ("cos", 24, 8, 40),
]


def lists_of(oracle: oraclebind.OracleIndex, slot: int):
    return [oracle.neighbors(slot, level).tolist() for level in range(oracle.level(slot) + 1)]


@pytest.mark.parametrize("metric,ndim,connectivity,expansion_add", PIN_CASES)
def test_one_reference_add_changes_the_graph_as_the_model_says(reference, metric, ndim, connectivity, expansion_add):
    """Members 0 … n - 2 are added by the real reference on one thread (image A), then member n - 1 (image B). With the
    candidates of the oracle's search of A (k = expansion = expansion_add — the insertion search of a level-0 member is that
    search), B's list of the new member must be `refine(candidates, M)`; every picked neighbour's list must be old + [new]
    while it has room, else `refine` of old ∪ {new} sorted by distance, to M0; and no other list may differ from A's.
    New members above level 0 are left out (their insertion searches every level); so is a size where a tie decides."""
    m, m0 = connectivity, 2 * connectivity
    vectors = util.make_vectors(PIN_SIZES[-1], ndim, "f32", seed=31, clustered=False)
    keys = np.arange(len(vectors), dtype=np.uint64)  # key = slot
    dist = util.slot_distance(vectors, metric, "f32", ndim, lanes=0)
    index = reference.RefIndex(ndim, metric, "f32", connectivity=connectivity, expansion_add=expansion_add)
    added, checked, compared_lists, repruned = 0, [], 0, 0
    for n in PIN_SIZES:
        new = n - 1
        assert index.add(keys[added:new], vectors[added:new], threads=1) == new - added
        before = oraclebind.OracleIndex(index.save_buffer())
        assert index.add(keys[new:n], vectors[new:n], threads=1) == 1
        after = oraclebind.OracleIndex(index.save_buffer())
        added = n
        assert len(before) == new and len(after) == n
        if after.level(new) != 0:
            continue
        found_keys, found_distances, counts, *_ = before.search(vectors[new:n], expansion_add, dtype="f32",
                                                                expansion=expansion_add, lanes=0)
        candidates = [(float(d), int(k)) for d, k in zip(found_distances[0, :counts[0]], found_keys[0, :counts[0]])]
        try:
            picks = build_model.refine(candidates, m, dist)
            expected = {}
            for filed, target in picks:
                old = before.neighbors(target, 0).tolist()
                if len(old) < m0:  # index.hpp:3874-3877
                    expected[target] = old + [new]
                    continue
                pool = sorted([(dist(target, other), other) for other in old] + [(filed, new)])
                expected[target] = [slot for _, slot in build_model.refine(pool, m0, dist)]
                repruned += 1
        except build_model.Tie:
            continue
        assert after.neighbors(new, 0).tolist() == [slot for _, slot in picks], f"n = {n}: the new member's list"
        for slot in range(new):
            now, then = lists_of(after, slot), lists_of(before, slot)
            if slot in expected:
                assert now[0] == expected[slot], f"n = {n}: the list of picked neighbour {slot}"
                then[0] = now[0]
            assert now == then, f"n = {n}: member {slot} was not picked and changed"
            compared_lists += len(now)
        checked.append(n)
    print(f"{metric} M={m} ef={expansion_add}: checked n = {checked}, {compared_lists} lists, {repruned} re-pruned")
    assert compared_lists > 0 and 2 * len(checked) >= len(PIN_SIZES), f"only {checked} of {PIN_SIZES} could be checked"


# ---- a graph the model builds by itself

def draw_levels(n: int, connectivity: int, seed: int) -> np.ndarray:
    """The reference's distribution (index.hpp:3895-3899) from a seeded generator of the test's own."""
    uniform = 1.0 - np.random.default_rng(seed).random(n)  # (0, 1]
    return np.floor(-np.log(uniform) / np.log(connectivity)).astype(np.int64)


def check_model_structure(graph, levels, connectivity: int, connectivity_base: int) -> int:
    """tests/test_gpu_build.py `check_structure`, on the model's lists."""
    n, linked = len(graph), 0
    for slot in range(n):
        assert len(graph[slot]) == levels[slot] + 1
        for level, neighbours in enumerate(graph[slot]):
            assert len(neighbours) <= (connectivity_base if level == 0 else connectivity)
            assert slot not in neighbours
            assert len(set(neighbours)) == len(neighbours)
            assert all(other < n and levels[other] >= level for other in neighbours)
            linked += len(neighbours)
    return linked


def test_a_model_built_graph_is_well_formed_and_as_good_as_the_references(reference):
    n, ndim, metric, connectivity, expansion_add, queries_count, k = 400, 16, "l2sq", 8, 64, 100, 10
    everything = util.make_vectors(n + queries_count, ndim, "f32", seed=41, clustered=False)  # rows n … are the queries
    vectors = everything[:n]
    dist = util.slot_distance(everything, metric, "f32", ndim, lanes=0)
    levels = draw_levels(n, connectivity, seed=42)
    assert levels.max() >= 1
    built = build_model.build(vectors, levels, dist, connectivity, 0, expansion_add, max_batch=16, batch_divisor=16)
    assert check_model_structure(built.graph, levels, connectivity, 2 * connectivity) > n
    assert built.max_level == levels.max() and levels[built.entry] == built.max_level
    assert built.batches > 0 and built.passes >= built.batches and built.repruned_lists > 0

    image, _, _ = util.build_image(n, ndim, metric, "f32", connectivity=connectivity, expansion_add=expansion_add,
                                   vectors=vectors, keys=np.arange(n, dtype=np.uint64))
    theirs = oraclebind.OracleIndex(image)
    their_levels = [theirs.level(slot) for slot in range(n)]
    their_graph = [lists_of(theirs, slot) for slot in range(n)]

    truth = [sorted(range(n), key=lambda slot, q=q: dist(q, slot))[:k] for q in range(n, n + queries_count)]

    def recall(graph, graph_levels, entry, max_level) -> float:
        hits = 0
        for q, expected in zip(range(n, n + queries_count), truth):
            found = build_model.beam(graph, graph_levels, entry, max_level, q, 0, 16, n, dist)[:k]
            hits += len(set(slot for _, slot in found) & set(expected))
        return hits / (k * queries_count)

    ours = recall(built.graph, levels, built.entry, built.max_level)
    own = recall(their_graph, their_levels, int(theirs.ix.entry_slot), int(theirs.ix.max_level))
    print(f"recall@{k}: model-built {ours:.4f}, reference-built {own:.4f}")
    assert ours >= own - 0.03, (ours, own)  # the margin of tests/test_gpu_build.py
