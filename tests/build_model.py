"""A plain restatement of batched HNSW construction as the device builder states it (usearch_amd/csrc/build.hip,
build_kernels.hpp), one node, one candidate and one comparison at a time. It is the yardstick of the link kernels: the builder
is deterministic by design, so this model predicts every neighbour list of a GPU-built graph exactly, in order
(tests/test_gpu_build_model.py), and its pruning rule is pinned to the compiled reference on the CPU (tests/test_build_model.py).

The rules, and where they come from:
- `refine`: the reference's `refine_` (include/usearch/index.hpp:4276-4318) as the SEQUENTIAL loop it is — a candidate is
  kept unless a node kept before it is strictly closer to it than the centre is. The kernels reach the same lists by "forward
  elimination" (an accepted node strikes out the later candidates it would reject); that the two agree is what is tested, so
  this file deliberately does not eliminate forward.
- `beam`: the insertion search the builder runs (`search_extras_t::beam_level`, `reference_frontier`, `query_ids`): the greedy
  descent of oracle/usearch_oracle.c `search_for_one` down to the level above the one being linked, then the best-first beam
  of `search_to_find_in_base` on THAT level with `top` limited to `ef`. The frontier is the reference's binary heap restated
  move for move (`_heap_insert` / `_heap_pop`), because equal keys leave a heap in an order that depends on its layout.
- `build`: `builder_t::build` / `link_range`: slot 0 is the first entry point; a batch holds
  max(1, min(max_batch, begin // batch_divisor)) nodes and is linked level by level, bottom-up, every search of a pass against
  the graph as it stood before the batch; `build_select_kernel` = `refine` to M plus one reverse-link request per pick;
  `build_reverse_kernel` = append in ascending requester order while the list has room, else old ∪ requesters sorted by
  (distance, slot) and refined to the capacity.
- `extend`: `builder_t::extend`: the same batch rule from `max(first, 1)` on a graph that exists; `build` is "member 0 is the entry
  point, then `extend` from 1".
- `update`: `builder_t::update` (`index_gt::update`, index.hpp:2916-2999): the slots of a call, `max_batch` at a time in the order
  given, are linked anew against the whole index: the walk never names the member itself (`exclude_own`), select REPLACES the
  member's list, its inbound links stay, and a requester the target's list names already files nothing ("not new" in both
  branches of `build_reverse_kernel`). The reference pin of these rules and the two stated deviations: tests/test_build_model.py.

Ties. Wherever two DIFFERENT members meet at the same distance and a strict `<` or an order between them decides something —
the descent's `d < closest`, the beam's `d < radius`, which of two equally far members stays in the final `top`, two equally far
candidates of `refine` that both pass everything kept before them, a struck-or-kept test — the outcome hangs on details this
model does not claim, and it raises `Tie` instead of guessing. An equality that cannot change the outcome (two equally far members
of which `top` drops one and later the other; an equally far candidate that `refine` strikes anyway) is let pass: among a few
hundred f32 distances per search such pairs are common.

`dist(a, b)` → the distance with member `a` staged as the query and member `b` as the stored row (the kernels' operand order);
`build` memoises it per ordered pair. Written for clarity, not speed: graphs of a few hundred members take seconds.
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Sequence, Tuple

Candidate = Tuple[float, int]           # (distance, slot)
Distance = Callable[[int, int], float]  # (query slot, row slot) → distance
Graph = List[List[List[int]]]           # graph[slot][level] → ordered neighbour list


class Tie(Exception):
    """Two different members at the same distance where the order between them decides the outcome."""


def _check_number(d: float) -> float:
    if d != d:
        raise Tie("a NaN distance orders against nothing")
    return d


def refine(candidates: Sequence[Candidate], needed: int, dist: Distance) -> List[Candidate]:
    """index.hpp:4276-4318. `candidates`: [(distance to the centre, slot)] ascending. → the kept ones, in order."""
    candidates = list(candidates)
    if len(candidates) < needed:  # 4284-4285: a small set is taken whole, unsorted and unpruned
        return candidates
    kept = [candidates[0]]  # 4290: the closest is always submitted
    for consumed in range(1, len(candidates)):
        if len(kept) >= needed:  # 4292
            break
        distance, slot = candidates[consumed]
        before = candidates[consumed - 1][0]
        if distance < candidates[consumed - 1][0]:
            raise ValueError("refine: the candidates are not in ascending order")
        good = True
        for kept_distance, submitted in kept:  # 4296-4306, in the order they were kept; stops at the first that strikes
            if kept_distance == distance:
                # both passed everything kept before them: which of the two comes first — and is asked about the other — is open.
                # (An equally far candidate that was struck, or this one struck before it gets here, changes nothing.)
                raise Tie(f"refine: candidates {submitted} and {slot} are equally far from the centre and both in the running")
            between = _check_number(dist(submitted, slot))
            if between == distance:
                raise Tie(f"refine: {slot} is as far from kept {submitted} as from the centre")
            if between < distance:  # 4302, strict
                good = False
                break
        if good:
            kept.append((distance, slot))
    return kept


def _heap_insert(heap: List[Candidate], item: Candidate) -> None:
    """max_heap_gt::insert_reserved + shift_up on the negated distance (index.hpp:765-770, 808-811), written on plain
    distances: an element rises while its parent is strictly FARTHER."""
    heap.append(item)
    i = len(heap) - 1
    while i and heap[(i - 1) // 2][0] > heap[i][0]:
        heap[(i - 1) // 2], heap[i] = heap[i], heap[(i - 1) // 2]
        i = (i - 1) // 2


def _heap_pop(heap: List[Candidate]) -> Candidate:
    """pop + shift_down (index.hpp:786-794, 819-834): the last element replaces the root and sinks towards the closer child; the
    left child unless the right one is strictly closer still."""
    root = heap[0]
    last = heap.pop()
    if heap:
        heap[0] = last
        i = 0
        while True:
            best, left, right = i, 2 * i + 1, 2 * i + 2
            if left < len(heap) and heap[best][0] > heap[left][0]:
                best = left
            if right < len(heap) and heap[best][0] > heap[right][0]:
                best = right
            if best == i:
                break
            heap[i], heap[best] = heap[best], heap[i]
            i = best
    return root


def beam(graph: Graph, levels: Sequence[int], entry: int, max_level: int, query_slot: int, level: int, ef: int,
         frontier: int, dist: Distance, exclude_own: bool = False, routed: List[int] = None) -> List[Candidate]:
    """The insertion search of one node on one level → ≤ `ef` (distance, slot), ascending. Only members below `frontier` exist:
    a list that names another one is a broken graph, not something to skip. `exclude_own`: the query's own slot routes but never
    becomes a candidate (`search_to_update_`, index.hpp:4087-4168: it enters the frontier and the visited set, not `top`, and
    leaves the radius alone). `routed`: a list that receives `query_slot` when the walk expanded the query's own slot."""
    def neighbours(slot: int, on: int) -> List[int]:
        assert levels[slot] >= on, f"member {slot} is not on level {on}"
        found = graph[slot][on]
        for other in found:
            assert other < frontier, f"the list of {slot} on level {on} names {other}, beyond the frontier {frontier}"
        return found

    def measure(slot: int) -> float:
        return _check_number(dist(query_slot, slot))

    # search_for_one: every neighbour of the closest member so far, in list order, strict `<`, again while something changed
    assert entry < frontier
    closest, closest_distance = entry, measure(entry)
    for above in range(max_level, level, -1):
        changed = True
        while changed:
            changed = False
            for other in list(neighbours(closest, above)):
                d = measure(other)
                if d == closest_distance and other != closest:
                    raise Tie(f"descent of {query_slot}: {other} and {closest} are equally close")
                if d < closest_distance:
                    closest_distance, closest, changed = d, other, True

    # search_to_find_in_base on `level`
    radius = measure(closest)
    nearest: List[Candidate] = []
    _heap_insert(nearest, (radius, closest))
    visited = {closest}
    top: List[Candidate] = []

    dropped_twins: Dict[float, int] = {}  # distance → a member `top` dropped while an equally far one stayed

    def admit(d: float, slot: int) -> None:
        nonlocal radius
        if exclude_own and slot == query_slot:
            return
        at = bisect.bisect_left(top, (d, -1))
        top.insert(at, (d, slot))
        if len(top) > ef:
            dropped = top.pop()
            if top[-1][0] == dropped[0]:
                # which of the two goes is open, and changes nothing yet: both are in the frontier already and the radius is the
                # same number either way. It matters only if the one that stayed is still there at the end (checked below).
                dropped_twins[dropped[0]] = dropped[1]
        radius = top[-1][0]

    admit(radius, closest)
    while nearest:
        d, candidate = nearest[0]
        if d > radius and len(top) == ef:  # index.hpp:4210, strict
            break
        _heap_pop(nearest)
        if routed is not None and candidate == query_slot:
            routed.append(query_slot)
        for successor in neighbours(candidate, level):
            if successor in visited:
                continue
            visited.add(successor)
            ds = measure(successor)
            if len(top) == ef and ds == radius:
                raise Tie(f"beam of {query_slot}: {successor} is exactly as far as the radius")
            if len(top) < ef or ds < radius:  # index.hpp:4233, strict
                _heap_insert(nearest, (ds, successor))
                admit(ds, successor)
    if top and top[-1][0] in dropped_twins:
        raise Tie(f"beam of {query_slot}: {top[-1][1]} stayed and {dropped_twins[top[-1][0]]} went, equally far")
    return top


@dataclass
class Operation:
    """What one call (`build`, `extend` or `update`) added to the builder's life-long counts."""
    kind: str
    batches: int = 0
    passes: int = 0
    repruned_lists: int = 0


@dataclass
class BuildResult:
    graph: Graph                    # graph[slot][level] → ordered neighbour list
    entry: int
    max_level: int
    batches: int = 0                # these three count over the result's life, like `usearch_amd_build_stats_t`
    passes: int = 0
    repruned_lists: int = 0
    # what the build went through, for tests that must know a case reached the branch it is named for
    most_candidates: int = 0        # the longest candidate list a select step received
    widest_upper_pass: int = 0      # most nodes linked in one pass on a level above 0
    most_requesters: int = 0        # most requests one target received in one pass
    most_requesters_repruned: int = 0  # … among the targets that were re-pruned
    widest_reprune: int = 0         # most candidates (old neighbours + requesters) one re-prune sorted
    candidate_counts: List[int] = field(default_factory=list)  # every select step's candidate count
    # requests whose requester the target's list already named (only a relink files such), by (list capacity, had the list room?)
    named_requests: Dict[Tuple[int, bool], int] = field(default_factory=dict)
    own_slot_routed: int = 0        # walks of `update` that expanded the member's own slot as a route (`exclude_own` did something)
    entry_point_updated: bool = False  # an `update` named the entry point
    operations: List[Operation] = field(default_factory=list)  # one per call, in order
    memo: Dict[Tuple[int, int], float] = field(default_factory=dict)  # (query slot, row slot) → distance

    @property
    def named_with_room(self) -> int:
        return sum(count for (_, room), count in self.named_requests.items() if room)

    @property
    def named_when_full(self) -> int:
        return sum(count for (_, room), count in self.named_requests.items() if not room)


def _link_pass(result: BuildResult, operation: Operation, nodes: Sequence[int], level: int, frontier: int, relink: bool,
               levels: Sequence[int], distance: Distance, m: int, m0: int, ef: int) -> None:
    """One pass of `link_batch`: the searches of all `nodes` on `level`, then select for all of them, then the reverse step."""
    graph = result.graph
    routed: List[int] = []
    # every search of the pass sees the graph as it stood before the pass
    found = {i: beam(graph, levels, result.entry, result.max_level, i, level, ef, frontier, distance, relink, routed)
             for i in nodes}
    result.own_slot_routed += len(routed)
    inboxes: Dict[int, List[Candidate]] = {}
    for i in nodes:  # select: the node's list BECOMES the picks (a relinked node's old list is gone), and one request per pick
        result.candidate_counts.append(len(found[i]))
        result.most_candidates = max(result.most_candidates, len(found[i]))
        picks = refine(found[i], m, distance)
        graph[i][level] = [slot for _, slot in picks]
        for d, slot in picks:
            inboxes.setdefault(slot, []).append((d, i))
    capacity = m0 if level == 0 else m
    for target, requests in inboxes.items():  # reverse: targets are independent of each other
        existing = graph[target][level]  # as select left it: a relinked target's list is its new one
        fresh = [(d, requester) for d, requester in requests if requester not in existing]
        if len(fresh) != len(requests):  # a relinked member keeps its inbound links: it does not file twice
            key = (capacity, len(existing) < capacity)
            result.named_requests[key] = result.named_requests.get(key, 0) + len(requests) - len(fresh)
        result.most_requesters = max(result.most_requesters, len(fresh))
        if len(existing) + len(fresh) <= capacity:
            existing.extend(sorted(requester for _, requester in fresh))  # ascending requester
            continue
        # old neighbours measured from the target, requesters with the distance they filed
        pool = [(_check_number(distance(target, other)), other) for other in existing] + fresh
        pool.sort()  # (distance, slot)
        graph[target][level] = [slot for _, slot in refine(pool, capacity, distance)]
        result.repruned_lists += 1
        operation.repruned_lists += 1
        result.most_requesters_repruned = max(result.most_requesters_repruned, len(fresh))
        result.widest_reprune = max(result.widest_reprune, len(pool))
    if level:
        result.widest_upper_pass = max(result.widest_upper_pass, len(nodes))
    result.passes += 1
    operation.passes += 1


def _memoised(result: BuildResult, dist: Distance) -> Distance:
    memo = result.memo

    def distance(a: int, b: int) -> float:
        key = (a, b)
        if key not in memo:
            memo[key] = dist(a, b)
        return memo[key]
    return distance


def extend(result: BuildResult, levels: Sequence[int], dist: Distance, first: int, total: int, connectivity: int,
           connectivity_base: int = 0, expansion_add: int = 128, max_batch: int = 65536, batch_divisor: int = 16,
           kind: str = "extend") -> BuildResult:
    """`builder_t::extend` → `link_range(max(first, 1), total)`: continues `result` (members 0 … first − 1) with members
    first … total − 1, in place. `levels` covers all `total` members. The distance memo lives on `result` and is carried on."""
    assert len(result.graph) == first <= total <= len(levels) and first >= 1
    m = connectivity
    m0 = connectivity_base or 2 * m
    ef = max(max(m, m0) + 1, expansion_add)  # index.hpp:2799-2800
    batch_divisor, max_batch = max(1, batch_divisor), max(1, min(max_batch, total))
    distance = _memoised(result, dist)
    graph = result.graph
    graph.extend([[] for _ in range(int(levels[slot]) + 1)] for slot in range(first, total))
    operation = Operation(kind)
    result.operations.append(operation)
    begin = max(first, 1)
    while begin < total:
        limit = max(1, min(max_batch, begin // batch_divisor))
        end = min(total, begin + limit)
        batch = list(range(begin, end))
        batch_top = max(int(levels[i]) for i in batch)
        for level in range(min(batch_top, result.max_level) + 1):  # bottom-up; the levels above were not touched yet
            nodes = [i for i in batch if levels[i] >= level]
            if nodes:
                _link_pass(result, operation, nodes, level, begin, False, levels, distance, m, m0, ef)
        if batch_top > result.max_level:  # index.hpp:2874-2877: a taller node becomes the entry point
            result.entry = next(i for i in batch if levels[i] == batch_top)
            result.max_level = batch_top
        result.batches += 1
        operation.batches += 1
        begin = end
    return result


def update(result: BuildResult, slots: Sequence[int], levels: Sequence[int], dist: Distance, connectivity: int,
           connectivity_base: int = 0, expansion_add: int = 128, max_batch: int = 65536) -> BuildResult:
    """`builder_t::update` → `link_range(size, size, slots)`: the members in `slots` have new rows and are linked anew, in place
    (`index_gt::update`, index.hpp:2916-2999). Every row of the call is overwritten before the first batch is linked, so `dist`
    is the distance over the NEW rows for the whole call; the pairs of the memo that name an updated slot are dropped here, on
    entry, and the memo is carried on otherwise. `slots` is taken in the order given, `max_batch` at a time (no divisor rule);
    the frontier is the whole index; levels, the entry point and the max level stay. The same slot twice is refused by the
    builder, so it is no case of the model."""
    slots = [int(slot) for slot in slots]
    n = len(result.graph)
    assert all(0 <= slot < n for slot in slots) and len(set(slots)) == len(slots)
    m = connectivity
    m0 = connectivity_base or 2 * m
    ef = max(max(m, m0) + 1, expansion_add)
    max_batch = max(1, min(max_batch, n))
    updated = set(slots)
    for pair in [pair for pair in result.memo if pair[0] in updated or pair[1] in updated]:
        del result.memo[pair]
    distance = _memoised(result, dist)
    result.entry_point_updated = result.entry_point_updated or result.entry in updated
    operation = Operation("update")
    result.operations.append(operation)
    for offset in range(0, len(slots), max_batch):
        batch = slots[offset:offset + max_batch]
        batch_top = max(int(levels[i]) for i in batch)
        for level in range(min(batch_top, result.max_level) + 1):
            nodes = [i for i in batch if levels[i] >= level]
            if nodes:
                _link_pass(result, operation, nodes, level, n, True, levels, distance, m, m0, ef)
        result.batches += 1
        operation.batches += 1
    return result


def build(vectors, levels: Sequence[int], dist: Distance, connectivity: int, connectivity_base: int = 0,
          expansion_add: int = 128, max_batch: int = 65536, batch_divisor: int = 16) -> BuildResult:
    """`builder_t::build` for `len(vectors)` members whose levels are given (the level draw is not modelled): member 0 is the
    entry point, the rest is an `extend` from 1."""
    n = len(vectors)
    assert n == len(levels) and n >= 1
    result = BuildResult(graph=[[[] for _ in range(int(levels[0]) + 1)]], entry=0, max_level=int(levels[0]))
    if n == 1:
        result.operations.append(Operation("build"))
        return result
    return extend(result, levels, dist, 1, n, connectivity, connectivity_base, expansion_add, max_batch, batch_divisor, "build")


def from_lists(lists: Graph, entry: int, max_level: int) -> BuildResult:
    """A graph read from an image (tests/compact_model.py `read_image`) as the state `extend` and `update` continue."""
    return BuildResult(graph=[[list(cells) for cells in per_level] for per_level in lists], entry=entry, max_level=max_level)


