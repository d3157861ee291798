"""`extend` and `update` of the device builder (usearch_amd/csrc/build.hip `builder_t::extend`, `update`, `link_range`,
`grow_for_build`, `overwrite_member`; the link kernels of build_kernels.hpp with `relinked` members; the walk's `exclude_own`)
held to the model list for list, as tests/test_gpu_build_model.py holds the one-shot build.

A case is a sequence of operations run on the device and on tests/build_model.py side by side (`Pair`). After EVERY operation:
every list of every member on every level equals the model's, in order, and so do the entry slot and the max level; the
operation's own `batches`, `passes` and `repruned_lists` — the differences of `BuiltIndex.stats` across it — equal the model's, and
the cumulative ones equal the sums over the builder's life; `dropped_requests == refiled_requests == 0`; the keys in the image
are what was given; the built index answers a few dozen queries as the oracle does over the saved image, bit for bit (keys,
distance bits, both counters — this is what sees a stale row next to a list); and the compiled reference loads the image.

All cases link with `max_batch = 16` (no inbox overflows: test_gpu_build_model.py), on continuous rows (`case_vectors`); a
`build_model.Tie` fails a case. Levels are read from the saved image. Slots to update are chosen by rule from the model's state.

Times observed (GPU part: every operation with its save; model: every operation) are in each case's docstring, and every
operation prints both; the whole file takes 3 s. No case costs the model more than 0.31 s — `lds_three_per_lane`, the slowest case
of test_gpu_build_model.py, links 900 members with lists of 128 and an expansion of 160: many times the comparisons of any case here.
"""
import time

import numpy as np
import pytest

import usearch_amd
from oracle import oraclebind, refbind
from tests import build_model, compact_model, util
from tests import test_gpu_build_model as build_cases
from tests import test_gpu_search_parity as parity

pytestmark = pytest.mark.gpu

MAX_BATCH = build_cases.MAX_BATCH
QUERIES, K, EXPANSION = 32, 10, 64
FREE_KEY = compact_model.FREE_KEY


def batch_edges(total: int, divisor: int, max_batch: int = MAX_BATCH):
    """Where `link_range(1, total)` ends its batches."""
    edges, begin = [], 1
    while begin < total:
        begin = min(total, begin + max(1, min(max_batch, begin // divisor)))
        edges.append(begin)
    return edges


class Pair:
    """One index on the device and in the model. `pool` holds every row the case will ever use; `store[slot]` is the row of member
    `slot` as it stands (the model's distances read it in place)."""

    def __init__(self, name, metric, dtype, ndim, m, m0, expansion_add, divisor, rows_seed, pool_size, build_seed=0, clusters=0):
        assert MAX_BATCH <= (min(32, 64 - max(m, m0)) if max(m, m0) < 64 else 32), "an inbox could overflow: not deterministic"
        self.name, self.metric, self.dtype, self.ndim = name, metric, dtype, ndim
        self.m, self.m0, self.expansion_add, self.divisor, self.build_seed = m, m0, expansion_add, divisor, build_seed
        self.pool = build_cases.case_vectors(metric, dtype, ndim, pool_size, rows_seed, clusters)
        self.store = np.zeros_like(self.pool)
        self.queries = build_cases.case_vectors(metric, dtype, ndim, QUERIES, rows_seed + 7000)
        self.taken, self.size = 0, 0
        self.keys, self.levels = [], []
        self.built, self.model, self.dist = None, None, None
        self.totals = [0, 0, 0]  # batches, passes, re-pruned lists over the builder's life
        self.seen = (0, 0, 0)
        self.gpu_seconds = self.model_seconds = 0.0
        self.image = None

    # ---- the device side

    def device_build(self, rows, keys):
        self.built = usearch_amd.build(rows, self.metric, self.dtype, keys=keys, connectivity=self.m, connectivity_base=self.m0,
                                       expansion_add=self.expansion_add, max_batch=MAX_BATCH, batch_divisor=self.divisor,
                                       seed=self.build_seed)
        return self.built.index.lanes_per_row

    def device_extend(self, rows, keys):
        self.built.extend(rows, keys)

    def device_update(self, slots, rows, keys):
        self.built.update(slots, rows, keys)

    def device_remove(self, slots):
        assert self.built.remove(slots) == len(slots)

    def device_compact(self):
        return self.built.compact(slot_map=True).tolist()

    def observe(self):
        """→ the saved image and the levels in it."""
        image = self.built.save_buffer()
        oracle = oraclebind.OracleIndex(image)
        assert len(oracle) == self.size and oracle.ix.connectivity == self.m and oracle.ix.connectivity_base == self.m0
        return image, [oracle.level(slot) for slot in range(self.size)]

    def read_image(self, image):
        return compact_model.read_image(image)

    # ---- operations

    def take(self, count):
        rows = self.pool[self.taken:self.taken + count]
        assert len(rows) == count, "the case's pool of rows is too small"
        self.taken += count
        return rows

    def timed_device(self, call, *args):
        started = time.perf_counter()
        result = call(*args)
        image, levels = self.observe()
        self.gpu_seconds += time.perf_counter() - started
        return result, image, levels

    def timed_model(self, call, *args):
        started = time.perf_counter()
        call(*args)
        self.model_seconds += time.perf_counter() - started

    def shape(self):
        return self.m, self.m0, self.expansion_add, MAX_BATCH

    def build(self, count, keys=None):
        rows = self.take(count)
        self.store[:count] = rows
        self.size = count
        self.keys = list(range(count)) if keys is None else [int(key) for key in keys]
        lanes, image, levels = self.timed_device(self.device_build, rows, keys)
        self.dist = util.slot_distance(self.store, self.metric, self.dtype, self.ndim, lanes=lanes)
        self.levels = levels
        started = time.perf_counter()
        self.model = build_model.build(self.store[:count], levels, self.dist, *self.shape(), self.divisor or build_cases.DEFAULT_DIVISOR)
        self.model_seconds += time.perf_counter() - started
        self.check(image, f"build {count}")

    def extend(self, count, keys=None):
        rows = self.take(count)
        first, total = self.size, self.size + count
        self.store[first:total] = rows
        self.size = total
        self.keys += list(range(first, total)) if keys is None else [int(key) for key in keys]
        _, image, levels = self.timed_device(self.device_extend, rows, keys)
        assert levels[:first] == self.levels, "an extension changed the level of an earlier member"
        self.levels = levels
        self.timed_model(build_model.extend, self.model, levels, self.dist, first, total, *self.shape(),
                         self.divisor or build_cases.DEFAULT_DIVISOR)
        self.check(image, f"extend {first} → {total}")

    def update(self, slots, rows, keys):
        slots = [int(slot) for slot in slots]
        rows = np.ascontiguousarray(rows)
        _, image, levels = self.timed_device(self.device_update, np.array(slots, dtype=np.uint32), rows,
                                             np.array(keys, dtype=np.uint64))
        assert levels == self.levels, "an update changed a level"
        for slot, row, key in zip(slots, rows, keys):
            self.store[slot] = row
            self.keys[slot] = int(key)
        self.timed_model(build_model.update, self.model, slots, levels, self.dist, *self.shape())
        self.check(image, f"update of {len(slots)}")

    def remove(self, slots):
        slots = [int(slot) for slot in slots]
        _, image, levels = self.timed_device(self.device_remove, np.array(slots, dtype=np.uint32))
        assert levels == self.levels
        for slot in slots:
            self.keys[slot] = FREE_KEY
        self.check(image, f"remove of {len(slots)}", linked=False)

    def compact(self):
        """`compact` renumbers the survivors. The model goes on from the graph of the image saved right after it, which must be
        what tests/compact_model.py makes of the model's graph before."""
        expected = compact_model.compact(self.model.graph, self.levels, self.keys, self.model.entry)
        survivors = [slot for slot, key in enumerate(self.keys) if key != FREE_KEY]
        self.size = len(survivors)
        slot_map, image, levels = self.timed_device(self.device_compact)
        assert slot_map == expected["slot_map"]
        lists, image_levels, keys, entry, max_level = self.read_image(image)
        assert (lists, image_levels, keys, entry, max_level) == (expected["lists"], expected["levels"], expected["keys"],
                                                                 expected["entry"], expected["max_level"])
        store = np.zeros_like(self.store)
        store[:self.size] = self.store[survivors]
        self.store = store
        self.dist = util.slot_distance(self.store, self.metric, self.dtype, self.ndim, lanes=self.built.index.lanes_per_row)
        self.keys, self.levels = keys, levels
        reach = self.model
        self.model = build_model.from_lists(lists, entry, max_level)  # a new memo: the slots have other rows now
        self.model.named_requests, self.model.own_slot_routed = reach.named_requests, reach.own_slot_routed
        self.check(image, "compact", linked=False)

    # ---- what must hold after every operation

    def check(self, image, what, linked=True):
        self.image = image
        stats = self.built.stats
        oracle = oraclebind.OracleIndex(image)
        for slot in range(self.size):
            for level in range(self.levels[slot] + 1):
                got, expected = oracle.neighbors(slot, level).tolist(), self.model.graph[slot][level]
                assert got == expected, (f"{self.name}, {what}: first difference at slot {slot}, level {level}: the GPU wrote {got}, "
                                         f"the model says {expected}")
        assert (int(oracle.ix.entry_slot), int(oracle.ix.max_level)) == (self.model.entry, self.model.max_level), what
        assert stats.max_level == self.model.max_level
        operation = self.model.operations[-1] if linked else build_model.Operation("none")
        done = (operation.batches, operation.passes, operation.repruned_lists)
        now = (stats.batches, stats.passes, stats.repruned_lists)
        assert tuple(a - b for a, b in zip(now, self.seen)) == done, f"{what}: the operation's own statistics {now} - {self.seen} ≠ {done}"
        self.totals = [a + b for a, b in zip(self.totals, done)]
        assert list(now) == self.totals, f"{what}: the cumulative statistics {now} ≠ {self.totals}"
        self.seen = now
        assert stats.dropped_requests == 0 and stats.refiled_requests == 0, what
        assert [oracle.key(slot) for slot in range(self.size)] == self.keys, f"{what}: the keys in the image"
        parity.check_against_oracle(self.built.index, image, self.queries, K, self.dtype, EXPANSION)
        present = sum(key != FREE_KEY for key in self.keys)
        assert len(refbind.RefIndex.from_buffer(image, dtype=self.dtype)) == present, f"{what}: the reference's size of the image"
        print(f"{self.name}, {what}: {done[0]} batches, {done[1]} passes, {done[2]} re-pruned; max level {self.model.max_level}, "
              f"entry {self.model.entry}; GPU {self.gpu_seconds:.2f} s, model {self.model_seconds:.2f} s so far")

    # ---- slots by rule

    def ground(self):
        return [slot for slot in range(self.size) if self.levels[slot] == 0 and self.keys[slot] != FREE_KEY]

    def inbound(self):
        counts = [0] * self.size
        for slot in range(self.size):
            for other in self.model.graph[slot][0]:
                counts[other] += 1
        return counts

    def nudged(self, slot):
        """The member's own row moved by a hair: its picks are mostly the members that name it already."""
        row = self.store[slot].astype(np.float64)
        return (row * 1.001 + 0.001 * self.take(1)[0].astype(np.float64)).astype(self.store.dtype)


def fresh_reach(pair):
    """Forget the widths reached so far, so that the next operation's reach is its own."""
    pair.model.widest_upper_pass = pair.model.most_requesters_repruned = pair.model.most_requesters = 0


# ---- extend

def test_extend_off_a_batch_boundary_twice():
    """Build 150, extend by 140 (the arrays grow to 1024, a workspace is made), extend by 210 (fits, the workspace is reused);
    290 is no multiple of 16. Cumulative statistics across growth and no growth, then an update on top.
    Observed: GPU 0.24 s (the process's first build), model 0.16 s."""
    pair = Pair("off_boundary", "l2sq", "f32", 16, 4, 8, 40, 1, 301, 600)
    pair.build(150)
    for count in (140, 210):
        fresh_reach(pair)
        level0 = pair.built.index.arrays.level0
        pair.extend(count)
        assert (pair.built.index.arrays.level0 != level0) == (count == 140), "the first extension grows the arrays, the second fits"
        assert pair.model.operations[-1].repruned_lists > 0
        assert pair.model.widest_upper_pass >= 2 and pair.model.most_requesters_repruned >= 2
    assert pair.size % MAX_BATCH and 290 % MAX_BATCH
    slots = pair.ground()[:20]
    pair.update(slots, pair.take(len(slots)), [9000 + slot for slot in slots])
    assert [operation.kind for operation in pair.model.operations] == ["build", "extend", "extend", "update"]
    assert all(operation.repruned_lists > 0 for operation in pair.model.operations), "the cumulative count has four parts"


def test_extend_moves_the_entry_point():
    """An appended member is taller than everything before it. Observed: GPU 0.01 s, model 0.06 s."""
    pair = Pair("entry_moves", "l2sq", "f32", 16, 4, 8, 40, 1, 302, 300, build_seed=2)
    pair.build(150)
    entry, top = pair.model.entry, pair.model.max_level
    pair.extend(140)
    assert max(pair.levels[150:]) > max(pair.levels[:150]), "the level seed no longer makes an appended member the tallest"
    assert pair.model.max_level > top and pair.model.entry >= 150 and pair.model.entry != entry
    assert pair.model.max_level == max(pair.levels)


def test_extend_through_a_second_growth():
    """Build 40 (exact arrays), extend to 1000 (capacity 1024), extend by 100 (capacity 2048): `nbr0`, `upper_ref`, the upper lists
    and the inboxes move twice. Observed: GPU 0.03 s, model 0.10 s."""
    m = 3
    pair = Pair("second_growth", "l2sq", "f32", 16, m, 6, 8, 1, 303, 1100)
    pair.build(40)
    capacities = []
    for count, capacity in ((960, 1024), (100, 2048)):
        level0 = pair.built.index.arrays.level0
        pair.extend(count)
        assert pair.built.index.arrays.level0 != level0, "the arrays did not move"
        # builder_t::extend's room for upper lists once the member capacity grows
        capacities.append(sum(pair.levels) + (capacity - pair.size) // (m - 1) * 3 // 2 + 1024)
    assert capacities[1] > capacities[0] > sum(pair.levels[:40]), "the upper-list array grows as well as nbr0"
    assert pair.model.max_level >= 2


def test_extend_long_rows_with_late_keys():
    """cos f16 768-d: 8 lanes per row. Built without keys, extended with keys: the image's keys are the row numbers followed by
    the given ones. Observed: GPU 0.04 s, model 0.31 s."""
    pair = Pair("long_rows_late_keys", "cos", "f16", 768, 8, 16, 64, 0, 304, 260)
    pair.build(150)
    assert pair.built.index.lanes_per_row == 8
    keys = np.arange(110, dtype=np.uint64) * 3 + 70000
    pair.extend(110, keys)
    assert pair.keys == list(range(150)) + keys.tolist()


def test_inline_rows_build_extend_update():
    """l2sq f32 4-d: 16-byte rows live next to the lists and must be rewritten after the lists and rows change.
    Observed: GPU 0.02 s, model 0.06 s."""
    pair = Pair("inline_rows", "l2sq", "f32", 4, 4, 8, 40, 1, 305, 500)
    pair.build(200)
    assert pair.built.index.inline_rows
    pair.extend(150)
    assert pair.built.index.inline_rows
    slots = pair.ground()[5:25] + [pair.model.entry]
    pair.update(slots, pair.take(len(slots)), [5000 + slot for slot in slots])
    assert pair.built.index.inline_rows and pair.model.entry_point_updated


def test_build_to_an_edge_then_extend_equals_a_one_shot_build_byte_for_byte():
    """With divisor 1 the batches of a one-shot build end at multiples of 16 from 16 on: a build to such an edge and an extension
    to the end link the same batches against the same graphs. Also: the levels do not depend on how the members arrived.
    Observed: GPU 0.03 s, model 0.18 s, the three indexes together."""
    total, edge, second_edge = 300, 160, 224
    assert edge in batch_edges(total, 1) and second_edge in batch_edges(total, 1)
    whole = Pair("one_shot", "l2sq", "f32", 16, 4, 8, 40, 1, 306, total)
    whole.build(total)
    parts = Pair("edge_then_extend", "l2sq", "f32", 16, 4, 8, 40, 1, 306, total)
    parts.build(edge)
    parts.extend(total - edge)
    assert parts.levels == whole.levels
    assert parts.model.graph == whole.model.graph
    assert parts.totals == whole.totals, "the same batches, passes and re-prunes, however the members arrived"
    assert parts.image.tobytes() == whole.image.tobytes(), "build + extend wrote another image than the one-shot build"
    thirds = Pair("edge_extend_extend", "l2sq", "f32", 16, 4, 8, 40, 1, 306, total)
    thirds.build(edge)
    thirds.extend(second_edge - edge)
    thirds.extend(total - second_edge)
    assert thirds.levels == whole.levels and thirds.image.tobytes() == whole.image.tobytes()


# ---- update

def built_pair(name, rows_seed, n=400, spare=120, metric="l2sq", dtype="f32", ndim=16, m=4, m0=8, expansion_add=40, clusters=0):
    pair = Pair(name, metric, dtype, ndim, m, m0, expansion_add, 1, rows_seed, n + spare, clusters=clusters)
    pair.build(n)
    return pair


def test_update_one_at_a_time():
    """Three calls: a level-0 member, a member above level 0, the entry point (index.hpp:2962-2969: no descent, the walk starts
    at the member itself). Observed: GPU 0.02 s, model 0.10 s."""
    pair = built_pair("one_at_a_time", 311)
    ground = pair.ground()[0]
    upper = next(slot for slot in range(pair.size) if 0 < pair.levels[slot] < pair.model.max_level)
    for slot in (ground, upper, pair.model.entry):
        assert not pair.model.entry_point_updated  # until the last call
        pair.update([slot], pair.take(1), [8000 + slot])
        assert pair.model.operations[-1].batches == 1 and pair.model.operations[-1].passes == min(pair.levels[slot], pair.model.max_level) + 1
    assert pair.model.entry_point_updated and pair.model.own_slot_routed > 0


def test_update_one_batch_of_16():
    """One pass holds a member and its first neighbour, the member with the most inbound links, two members that move next to each
    other and pick each other, and members moved by a hair (their targets name them already, in lists with room and in full ones).
    Observed: GPU 0.01 s, model 0.10 s."""
    pair = built_pair("one_batch", 312)
    graph, ground = pair.model.graph, pair.ground()
    member = next(slot for slot in ground if graph[slot][0])
    inbound = pair.inbound()
    hub = max(ground, key=lambda slot: (inbound[slot], -slot))
    slots = [member, graph[member][0][0], hub]
    mutual = next((a, b) for a in ground for b in graph[a][0] if a in graph[b][0] and not {a, b} & set(slots))
    slots += list(mutual)
    named_in_full = [slot for slot in ground if slot not in slots and
                     any(len(graph[other][0]) == pair.m0 and slot in graph[other][0] for other in graph[slot][0])]
    named_with_room = [slot for slot in ground if slot not in slots and slot not in named_in_full[:6] and
                       any(len(graph[other][0]) < pair.m0 and slot in graph[other][0] for other in graph[slot][0])]
    hair = named_in_full[:5] + named_with_room[:4]
    slots += hair
    # … and two that move next to one member whose list is full and names neither: one re-prune with two requesters
    crowded = next(slot for slot in ground if slot not in slots and len(graph[slot][0]) == pair.m0)
    movers = [slot for slot in ground if slot not in slots and slot != crowded and slot not in graph[crowded][0]][:2]
    slots += movers
    assert len(slots) == MAX_BATCH == len(set(slots))
    rows = pair.take(len(slots)).copy()
    rows[0] = pair.nudged(slots[0])          # the member stays where its first neighbour knows it …
    rows[1] = pair.nudged(slots[1])          # … and so does the neighbour
    near = pair.take(1)[0].astype(np.float64)
    rows[3] = (near * 1.0005).astype(rows.dtype)   # the two land next to each other, away from where they were
    rows[4] = (near * 0.9996 + 0.0002 * pair.take(1)[0]).astype(rows.dtype)
    for position in range(5, 5 + len(hair)):
        rows[position] = pair.nudged(slots[position])
    centre = pair.store[crowded].astype(np.float64)
    rows[14] = (centre * 1.002 + 0.001 * pair.take(1)[0]).astype(rows.dtype)
    rows[15] = (centre * 0.997 + 0.001 * pair.take(1)[0]).astype(rows.dtype)
    fresh_reach(pair)
    pair.update(slots, rows, [8000 + slot for slot in slots])
    a, b = mutual
    assert graph[a][0][0] == b and graph[b][0][0] == a, "the two moved members did not pick each other first"
    model = pair.model
    print(f"one_batch: named with room {model.named_with_room}, when full {model.named_when_full}, own slot routed "
          f"{model.own_slot_routed}, requesters re-pruned ≤ {model.most_requesters_repruned}")
    assert model.operations[-1].batches == 1
    assert model.named_with_room > 0 and model.named_when_full > 0 and model.own_slot_routed > 0
    assert model.most_requesters_repruned >= 2


def test_update_40_slots_in_one_call():
    """Batches of 16, 16 and 8; later batches walk the lists earlier ones wrote. The slots come in descending order, and the order
    given is what is linked. Observed: GPU 0.01 s, model 0.10 s."""
    pair = built_pair("forty", 313)
    slots = sorted(pair.ground()[10:50], reverse=True)
    pair.update(slots, pair.take(40), [8000 + slot for slot in slots])
    assert pair.model.operations[-1].batches == 3 and pair.model.operations[-1].repruned_lists > 0


def test_update_far_and_near():
    """One member moves across the space: all its inbound links are stale. One is overwritten with its own row.
    Observed: GPU 0.01 s, model 0.09 s."""
    pair = built_pair("far_and_near", 314)
    inbound = pair.inbound()
    far = max(pair.ground(), key=lambda slot: (inbound[slot], -slot))
    same = next(slot for slot in pair.ground() if slot != far and pair.model.graph[slot][0])
    rows = np.stack([(-3.0 * pair.store[far].astype(np.float64)).astype(pair.store.dtype), pair.store[same].copy()])
    before = [list(pair.model.graph[slot][0]) for slot in (far, same)]
    pair.update([far, same], rows, [8000 + far, 8000 + same])
    assert inbound[far] >= 8 and not set(pair.model.graph[far][0]) & set(before[0]), "the far member kept an old neighbour"
    assert pair.model.named_requests, "the member that stayed picked nobody that names it"


def test_update_wide_lists_meet_a_named_requester_in_lds():
    """M 32 / M0 64 on the clustered rows of `lds_two_per_lane`: capacity + inbox > 64 on level 0, so the reverse kernel's LDS
    branch is the one that finds requesters the list already names (lists with room: a re-prune leaves a wide list well below its
    capacity, so a full one that names an updated member does not come up at this size). Observed: GPU 0.02 s, model 0.30 s."""
    pair = built_pair("wide_lists", 108, n=700, spare=40, m=32, m0=64, expansion_add=80, clusters=4)
    assert pair.m0 + min(32, 64) > 64
    graph = pair.model.graph
    longest = sorted(range(pair.size), key=lambda slot: (-len(graph[slot][0]), slot))[:4]  # the cluster centres' lists, 33 cells or more
    assert all(len(graph[slot][0]) > 32 for slot in longest)
    named_by_them = [slot for slot in pair.ground() if slot not in longest and any(slot in graph[other][0] for other in longest)]
    slots = named_by_them[:10] + [slot for slot in pair.ground() if slot not in longest and slot not in named_by_them][:6]
    assert len(slots) == MAX_BATCH
    rows = np.stack([pair.nudged(slot) for slot in slots])
    pair.update(slots, rows, [8000 + slot for slot in slots])
    named = pair.model.named_requests
    print(f"wide_lists: already-named requests by (capacity, room): {named}")
    assert sum(count for (capacity, _), count in named.items() if capacity == 64) > 0, "the LDS branch met no named requester"
    assert any(target in longest and set(slots) & set(graph[target][0]) for target in longest)


def test_recycle_as_the_drop_in_does():
    """`remove` slots, `update` them with new keys and rows (ascending, deduplicated), then `extend`. The tombstones are gone from
    the image; the one slot left removed keeps routing, never matches, and stays flagged.
    Observed: GPU 0.02 s, model 0.10 s."""
    pair = built_pair("recycle", 315, n=300, spare=200)
    removed = sorted(pair.ground()[3:33:2] + [pair.model.entry])
    pair.remove(removed)
    recycled, left = removed[:-2] + removed[-1:], removed[-2]
    pair.update(recycled, pair.take(len(recycled)), [6000 + slot for slot in recycled])
    pair.extend(100, np.arange(100, dtype=np.uint64) + 7000)
    assert [slot for slot, key in enumerate(pair.keys) if key == FREE_KEY] == [left]
    assert any(left in per_level[0] for per_level in pair.model.graph), "the removed member no longer routes"
    got = pair.built.index.search(pair.store[left:left + 1], K, expansion=EXPANSION)
    assert FREE_KEY not in got.keys[0, :got.counts[0]].tolist() and got.counts[0] == K
    assert pair.model.entry_point_updated


def test_extend_and_update_after_compact():
    """`remove`, `compact`, then `extend` and `update` over the renumbered survivors; the statistics go on counting although
    `compact` gave the arrays a new shape. Observed: GPU 0.02 s, model 0.11 s."""
    pair = built_pair("after_compact", 316, n=300, spare=200)
    pair.extend(60)  # a workspace exists when `compact` comes
    pair.remove(pair.ground()[2:60:3] + [0])
    pair.compact()
    assert pair.size == 360 - 21
    pair.extend(90, np.arange(90, dtype=np.uint64) + 7000)
    slots = pair.ground()[1:30]
    pair.update(slots, pair.take(len(slots)), [8000 + slot for slot in slots])
    assert pair.totals[2] > 0 and all(operation.repruned_lists > 0 for operation in pair.model.operations)
