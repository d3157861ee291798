"""Is tests/build_model.py the reference's? (CPU only.) The model is the yardstick of the device builder
(tests/test_gpu_build_model.py compares GPU-built graphs with it list for list), so its own rules are pinned here first:

- `refine` and the reverse-link rule against the COMPILED reference: one `add` of the real `index_gt` (include/usearch/index.hpp
  2759-2879) must change the graph exactly as the model says — the new member's list, every touched neighbour's list, nothing else;
- the relink rules (`exclude_own`, the replaced list, the kept inbound links) against one `update` of it: a removed slot recycled;
- `extend` resumes a build where a batch ended, `update` relinks in place: the model against itself;
- a graph the model builds on its own is a well-formed HNSW graph, as good as the reference's under the same search;
- the corner cases of `refine` that the kernels' shortcuts make interesting, on points one can check by hand.
"""
import numpy as np
import pytest

from oracle import oraclebind
from tests import build_model, compact_model, util


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


def test_the_walk_of_an_update_routes_through_the_member_and_never_names_it():
    # a chain 0 – 1 – 2 on a line; member 1 is searched for from 0: it is the only way to 2, and no candidate of its own
    chain = plane([(0.0, 0.0), (1.0, 0.0), (2.5, 0.0)])
    graph = [[[1]], [[0, 2]], [[1]]]
    routed = []
    found = build_model.beam(graph, [0, 0, 0], 0, 0, 1, 0, 4, 3, chain, exclude_own=True, routed=routed)
    assert found == [(1.0, 0), (2.25, 2)] and routed == [1]
    assert build_model.beam(graph, [0, 0, 0], 0, 0, 1, 0, 4, 3, chain) == [(0.0, 1), (1.0, 0), (2.25, 2)]
    # the entry point itself: nothing to descend from, the walk starts at the member and `top` starts empty
    routed = []
    assert build_model.beam(graph, [0, 0, 0], 1, 0, 1, 0, 4, 3, chain, exclude_own=True, routed=routed) == [(1.0, 0), (2.25, 2)]
    assert routed == [1]


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


# ---- against the compiled reference: what ONE `update` (a recycled slot) does to the graph

RELINK_MEMBERS = 500
RELINK_TRIALS = ["most_inbound", "across", "nudged", "fresh", "fresh", "most_inbound", "across", "fresh", "nudged", "fresh"]


def relink_trial(kind: str, trial: int, lists, levels, vectors, spare):
    """→ (u, new row) by rule from the graph as it stands: a level-0 member with the most inbound links on level 0; a member whose
    new row lies across the space from its old one (all its inbound links go stale); one moved by a hair (its picks mostly name
    it already); one that gets an unrelated row."""
    n = len(lists)
    ground = [slot for slot in range(n) if levels[slot] == 0]
    if kind == "most_inbound":
        inbound = [0] * n
        for slot in range(n):
            for other in lists[slot][0]:
                inbound[other] += 1
        u = max(ground, key=lambda slot: (inbound[slot], -slot))
        return u, spare[trial]
    u = ground[(trial * 7919 + 13) % len(ground)]
    if kind == "across":
        return u, (-vectors[u]).astype(vectors.dtype)
    if kind == "nudged":
        return u, (vectors[u] * np.float32(1.001) + np.float32(0.001) * spare[trial]).astype(vectors.dtype)
    return u, spare[trial]


@pytest.mark.parametrize("metric,ndim,connectivity,expansion_add", PIN_CASES)
def test_one_reference_update_relinks_the_graph_as_the_model_says(reference, metric, ndim, connectivity, expansion_add):
    """The real reference adds RELINK_MEMBERS members on one thread (key = slot). Per trial: `remove(key of u)` (image A), then
    `add(new key, new row)`, which recycles slot u through `index_gt::update` (image B). With the model's
    `beam(…, exclude_own=True)` over A's graph and the NEW row at u, B's list of u must be exactly `refine(candidates, M)` — that
    pins `exclude_own` and the emptied-then-refilled list; every picked target whose list did not name u must be old + [u] while
    it has room, else `refine` of old ∪ {u} to M0; nothing else may differ; u keeps its level and B names the new key at slot u.
    Targets whose list names u already are the stated deviation: the reference appends or re-prunes with a duplicate,
    the builder does not file twice. They are left out of the equality, counted and printed. Trials go on from each other's
    graphs. A trial is set aside where a tie decides (u is chosen on level 0).

    What is measured. The reference stores the new row only AFTER `update` has returned (the `on_success` callback,
    index_dense.hpp:2029-2048), so during its update slot u still holds the OLD row: the walk measures the new value against stored
    rows (u's own routing priority is d(new, old), not 0), and a re-prune that has u in its pool asks u's old row about the others
    while u's distance to the centre is the one filed with the new value. The builder overwrites every row first. The
    RULES are what is pinned here, so the model gets the reference's measure: `from_value` for the walk, stored rows elsewhere."""
    m, m0 = connectivity, 2 * connectivity
    n = RELINK_MEMBERS
    assert expansion_add > m0  # the walk's limit is the expansion itself (index.hpp:2973), the model's max(M0 + 1, expansion)
    everything = util.make_vectors(n + len(RELINK_TRIALS), ndim, "f32", seed=37, clustered=False)
    # rows 0 … n - 1 are the STORED rows, row n is the value being written; `slot_distance` reads them in place
    vectors, spare = np.ascontiguousarray(np.concatenate([everything[:n], everything[:1]])), everything[n:]
    dist = util.slot_distance(vectors, metric, "f32", ndim, lanes=0)

    def from_value(_, slot):  # what the walk measures: the new value against a stored row
        return dist(n, slot)
    index = reference.RefIndex(ndim, metric, "f32", connectivity=connectivity, expansion_add=expansion_add)
    assert index.add(np.arange(n, dtype=np.uint64), vectors[:n], threads=1) == n
    checked, compared_lists, repruned, appended, named, routed_walks = [], 0, 0, 0, [0, 0], 0
    for trial, kind in enumerate(RELINK_TRIALS):
        lists, levels, keys, entry, max_level = compact_model.read_image(index.save_buffer())
        u, row = relink_trial(kind, trial, lists, levels, vectors, spare)
        assert levels[u] == 0 and u != entry
        assert index.remove(keys[u]) == 1
        before = compact_model.read_image(index.save_buffer())
        assert before[:2] == (lists, levels) and before[2][u] == compact_model.FREE_KEY  # `remove` leaves the graph alone
        vectors[n] = row
        new_key = n + trial
        assert index.add(np.array([new_key], dtype=np.uint64), row[None, :], threads=1) == 1
        after_lists, after_levels, after_keys, after_entry, after_max_level = compact_model.read_image(index.save_buffer())
        assert len(after_lists) == n and after_keys[u] == new_key and after_levels == levels
        assert (after_entry, after_max_level) == (entry, max_level)
        try:
            routed = []
            found = build_model.beam(lists, levels, entry, max_level, u, 0, expansion_add, n, from_value, True, routed)
            picks = build_model.refine(found, m, dist)
            expected, already = {}, set()
            for filed, target in picks:
                old = lists[target][0]
                if u in old:
                    already.add(target)
                    named[len(old) == m0] += 1
                elif len(old) < m0:  # index.hpp:3874-3877
                    expected[target] = old + [u]
                    appended += 1
                else:
                    pool = sorted([(dist(target, other), other) for other in old] + [(filed, u)])
                    expected[target] = [slot for _, slot in build_model.refine(pool, m0, dist)]
                    repruned += 1
        except build_model.Tie:
            continue
        finally:
            vectors[u] = row  # stored from here on
        assert u not in [slot for _, slot in found]
        assert after_lists[u] == [[slot for _, slot in picks]], f"trial {trial} ({kind}): the list of updated member {u}"
        for slot in range(n):
            if slot == u:
                continue
            now, then = after_lists[slot], [list(cells) for cells in lists[slot]]
            if slot in expected:
                assert now[0] == expected[slot], f"trial {trial} ({kind}): the list of picked neighbour {slot}"
                then[0] = now[0]
            elif slot in already:
                then[0] = now[0]
            assert now == then, f"trial {trial} ({kind}): member {slot} was not picked and changed"
            compared_lists += len(now)
        routed_walks += len(routed)
        checked.append(trial)
    print(f"update {metric} M={m} ef={expansion_add}: checked trials {checked}, {compared_lists} lists, {appended} appended, "
          f"{repruned} re-pruned; left out, the target named u already: {named[0]} with room, {named[1]} full; "
          f"{routed_walks} walks routed through u")
    assert compared_lists > 0 and 2 * len(checked) >= len(RELINK_TRIALS), f"only {checked} of {len(RELINK_TRIALS)} trials"
    assert repruned > 0 and appended > 0


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


# ---- `extend` and `update` of the model itself

def test_extend_resumes_a_build_where_a_batch_ended():
    """With divisor 1 a build of 300 ends batches at 160 and 224: a build to either edge and `extend`s to the end go through the
    same batches against the same graphs — the same lists and the same counts, summed over the operations."""
    n, ndim, m = 300, 16, 4
    vectors = util.make_vectors(n, ndim, "f32", seed=51, clustered=False)
    dist = util.slot_distance(vectors, "l2sq", "f32", ndim, lanes=0)
    levels = draw_levels(n, m, seed=52)
    whole = build_model.build(vectors, levels, dist, m, 0, 40, max_batch=16, batch_divisor=1)
    parts = build_model.build(vectors[:160], levels[:160], dist, m, 0, 40, max_batch=16, batch_divisor=1)
    build_model.extend(parts, levels, dist, 160, 224, m, 0, 40, max_batch=16, batch_divisor=1)
    build_model.extend(parts, levels, dist, 224, n, m, 0, 40, max_batch=16, batch_divisor=1)
    assert parts.graph == whole.graph and (parts.entry, parts.max_level) == (whole.entry, whole.max_level)
    assert [operation.kind for operation in parts.operations] == ["build", "extend", "extend"]
    for count in ("batches", "passes", "repruned_lists"):
        assert sum(getattr(operation, count) for operation in parts.operations) == getattr(parts, count) == getattr(whole, count)
    # off an edge the first batch of the extension is a full one where the build's was the rest of one: another graph
    ragged = build_model.build(vectors[:150], levels[:150], dist, m, 0, 40, max_batch=16, batch_divisor=1)
    build_model.extend(ragged, levels, dist, 150, n, m, 0, 40, max_batch=16, batch_divisor=1)
    assert ragged.batches == whole.batches + 1 and ragged.graph != whole.graph
    check_model_structure(ragged.graph, levels, m, 2 * m)


def test_update_relinks_in_place_and_keeps_the_inbound_links():
    n, ndim, m = 300, 16, 4
    everything = util.make_vectors(n + 40, ndim, "f32", seed=53, clustered=False)
    vectors = np.ascontiguousarray(everything[:n])
    dist = util.slot_distance(vectors, "l2sq", "f32", ndim, lanes=0)  # reads the rows in place
    levels = draw_levels(n, m, seed=54)
    built = build_model.build(vectors, levels, dist, m, 0, 40, max_batch=16, batch_divisor=1)
    entry, max_level, batches = built.entry, built.max_level, built.batches
    # a member overwritten with its own row picks again what it had found before the lists around it filled up; what names it stays
    same = next(slot for slot in range(n) if levels[slot] == 0 and slot != entry)
    inbound = [slot for slot in range(n) if same in built.graph[slot][0]]
    build_model.update(built, [same], levels, dist, m, 0, 40, max_batch=16)
    assert all(same in built.graph[slot][0] for slot in inbound) and built.named_requests
    # 40 members get other rows, in descending order, the entry point among them: batches of 16, 16 and 8
    slots = sorted(set(range(100, 139)) | {entry}, reverse=True)[:40]
    assert len(slots) == 40 and entry in slots
    vectors[slots] = everything[n:]
    with pytest.raises(AssertionError):
        build_model.update(built, slots + slots[:1], levels, dist, m, 0, 40, max_batch=16)  # the same slot twice is no case
    build_model.update(built, slots, levels, dist, m, 0, 40, max_batch=16)
    assert (built.entry, built.max_level) == (entry, max_level) and built.entry_point_updated
    assert built.operations[-1].kind == "update" and built.operations[-1].batches == 3 and built.batches == batches + 4
    assert built.own_slot_routed > 0
    check_model_structure(built.graph, levels, m, 2 * m)
    # the memo dropped every pair that names an updated slot: what it holds is what `dist` says now
    assert all(value == dist(a, b) for (a, b), value in built.memo.items())
