"""Plain-Python models of the ordering containers every search result passes through: the result buffer `top`, the frontier heap
`next` and the fold of per-shard lists. No GPU: distances are Python floats (an f32 converts exactly), so every
comparison below is the IEEE one, NaN included.

Two inserts are kept apart on purpose:

* `lower_bound_insert` is the reference's `sorted_buffer_gt::insert` as oracle/usearch_oracle.c restates it: a binary search by `<`.
  Over an array that holds NaN beside numbers that search's answer depends on its path; it is the truth on NaN-free and on NaN-only
  scripts.
* `nan_first_insert` is the device's own rule for every layout: a NaN newcomer lands in cell 0, a number lands behind
  all NaNs at its lower bound among the numbers, a full buffer drops its last cell. On NaN-free and NaN-only scripts the two agree.

An entry is a list `[distance, slot, closed]`; `closed` is the frontier flag that rides with a member of `top` when the frontier lives
in `top` (bit 31 of the slot word on the device).
"""
import math

import numpy as np


def accepts(buf, d, limit):
    """The traversal's acceptance rule: the buffer is not full, or `d` is smaller than its last (worst) distance."""
    return len(buf) < limit or d < buf[-1][0]


def _place(buf, position, d, slot, closed, limit):
    if position == limit:
        return False
    if len(buf) == limit:
        buf.pop()
    buf.insert(position, [d, slot, closed])
    return True


def lower_bound_insert(buf, d, slot, limit, closed=False):
    """sorted_buffer_gt::insert: position = std::lower_bound by `<` (binary, the oracle's midpoint), new before equal; a position of
    `limit` is refused, a full buffer drops its last."""
    lo, hi = 0, len(buf)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if buf[mid][0] < d:
            lo = mid + 1
        else:
            hi = mid
    return _place(buf, lo, d, slot, closed, limit)


def nan_first_insert(buf, d, slot, limit, closed=False):
    """The device's rule: NaN first (a NaN newcomer in front of the NaNs already there), then distance ascending, new before equal."""
    position = 0
    if not math.isnan(d):
        while position < len(buf) and (math.isnan(buf[position][0]) or buf[position][0] < d):
            position += 1
    return _place(buf, position, d, slot, closed, limit)


def first_open(buf):
    """Index of the first member that is not closed, or None: what the heap-less frontier expands next."""
    for index, entry in enumerate(buf):
        if not entry[2]:
            return index
    return None


class RefHeap:  # max-heap on key, reference sift rules (max_heap_gt, index.hpp:664-835)
    def __init__(self):
        self.e = []

    def push(self, key, slot):
        self.e.append((key, slot))
        i = len(self.e) - 1
        while i and self.e[(i - 1) // 2][0] < self.e[i][0]:
            self.e[(i - 1) // 2], self.e[i] = self.e[i], self.e[(i - 1) // 2]
            i = (i - 1) // 2

    def pop(self):
        top = self.e[0]
        self.e[0] = self.e[-1]
        self.e.pop()
        i, n = 0, len(self.e)
        while True:
            best, left, right = i, 2 * i + 1, 2 * i + 2
            if left < n and self.e[best][0] < self.e[left][0]:
                best = left
            if right < n and self.e[best][0] < self.e[right][0]:
                best = right
            if best == i:
                break
            self.e[i], self.e[best] = self.e[best], self.e[i]
            i = best
        return top


def merge_model(lists, wanted, later_position_first=True, insert=nan_first_insert):
    """The fold of per-shard lists (`lists[shard]` = [(distance, key), …] as the rule leaves a list: NaNs, then ascending) into one
    of at most `wanted`: the lists are inserted one after the other in shard order, each newcomer in front of its equals. Inside a
    shard the elements go in by position (`later_position_first`, the reference's `merge_into`: the later position ends up in front of
    its equals) or from the last position to the first (the earlier position ends up in front). → [(distance, key), …]."""
    merged = []
    for entries in lists:
        for d, key in (entries if later_position_first else reversed(entries)):
            insert(merged, d, key, wanted)
    return [(entry[0], entry[1]) for entry in merged]


class TopModel:
    """`top` under the traversal: inserts pass the acceptance rule first; the radius is the last distance once the buffer is full
    (+inf before that, as the kernels initialise it). Every operation returns what the device's hook records for it."""

    def __init__(self, limit, insert):
        self.limit, self.insert_rule, self.buf, self.radius, self.accepted = limit, insert, [], math.inf, 0

    def insert(self, d, slot, closed=False):
        accepted = accepts(self.buf, d, self.limit)
        if accepted:
            landed = self.insert_rule(self.buf, d, slot, self.limit, closed)
            assert landed, "the acceptance rule let through what the insert refuses"
            self.accepted += 1
            if len(self.buf) == self.limit:
                self.radius = self.buf[-1][0]
        return accepted

    def pop_open(self):
        """first_open + close → (cell, distance, slot) or None."""
        cell = first_open(self.buf)
        if cell is None:
            return None
        self.buf[cell][2] = True
        return cell, self.buf[cell][0], self.buf[cell][1]


SIGNALING_NAN_BITS = 0x7FA00000  # the padding of a result list beyond its count (index.hpp:2707-2722), beside key 0


def nan_first_lists(rng, shards, queries, wanted, nan_share, levels=4):
    """Per-shard result lists in the shape the rule leaves them — NaNs first, then ascending, tie-heavy — for the merge tests:
    → distances [shards, queries, wanted] f32, keys (distinct), counts [shards, queries] with 0 and `wanted` among them. Cells beyond a
    list's count hold numbers SMALLER than everything kept, so a merge that reads them shows."""
    distances = rng.integers(0, levels, size=(shards, queries, wanted)).astype(np.float32) * 0.25
    distances[rng.random(distances.shape) < nan_share] = np.nan
    counts = rng.integers(0, wanted + 1, size=(shards, queries)).astype(np.uint64)
    counts[:, :3], counts[:, 3:6] = 0, wanted
    counts[0, 6], counts[1:, 6] = wanted, 0
    for shard in range(shards):
        for q in range(queries):
            n = int(counts[shard, q])
            kept = distances[shard, q, :n]
            nans = np.isnan(kept)
            distances[shard, q, :n] = np.concatenate([kept[nans], np.sort(kept[~nans])])
            distances[shard, q, n:] = -7.0
    keys = (rng.permutation(shards * queries * wanted).astype(np.uint64) + np.uint64(1)).reshape(shards, queries, wanted)
    return distances, keys, counts


def assert_merge_follows_model(got, distances, keys, counts, later_position_first, key_sentinel):
    """(keys, distances, counts) of a merge against `merge_model`, bit for bit: every cell below the count written (no sentinel left),
    no key twice, the padding beyond."""
    got_k, got_d, got_c = got
    shards, queries, wanted = distances.shape
    bits, got_bits = distances.view(np.uint32), got_d.view(np.uint32)
    for q in range(queries):
        lists = [[(float(distances[s, q, i]), (s, i)) for i in range(int(counts[s, q]))] for s in range(shards)]
        want = merge_model(lists, wanted, later_position_first)
        n = len(want)
        assert int(got_c[q]) == n == min(int(counts[:, q].sum()), wanted), q
        assert got_k[q, :n].tolist() == [int(keys[s, q, i]) for _, (s, i) in want], (q, got_k[q], got_d[q])
        assert got_bits[q, :n].tolist() == [int(bits[s, q, i]) for _, (s, i) in want], q
        assert key_sentinel not in got_k[q].tolist() and len(set(got_k[q, :n].tolist())) == n, q
        assert (got_k[q, n:] == 0).all() and (got_bits[q, n:] == SIGNALING_NAN_BITS).all(), q
