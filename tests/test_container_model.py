"""CPU: the plain-Python container models of tests/container_model.py against each other, against the linear insert the GPU container
test has always used, and against the oracle's `merge_into` — where all of them must agree: scripts without NaN and scripts of NaN
only. (Where NaN meets numbers the reference's binary search has no path-independent answer; the device's own rule there is
`nan_first_insert`, DESIGN.md §3.1a, and the GPU tests hold every layout to it.)"""
import math

import numpy as np
import pytest

from tests import container_model as model

LIMITS = (1, 3, 4, 5, 16, 63, 64, 65, 100)
SPECIALS = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0], dtype=np.float32)


def script(seed, count, kind):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        return rng.integers(0, 2 + seed % 7, size=count).astype(np.float32) * 0.5 - 1.0
    if kind == "specials":
        return SPECIALS[rng.integers(0, len(SPECIALS), size=count)]
    return np.full(count, np.nan, dtype=np.float32)


def replay(insert, values, limit):
    """`values` through `insert` under the traversal's acceptance rule → the buffer, and per operation (accepted, size)."""
    buf, trace = [], []
    for slot, d in enumerate(values):
        d = float(d)
        accepted = model.accepts(buf, d, limit)
        if accepted:
            insert(buf, d, slot, limit)
        trace.append((accepted, len(buf)))
    return buf, trace


def same(a, b):
    """Equal entry by entry, a NaN equal to a NaN and −0.0 apart from +0.0."""
    return len(a) == len(b) and all(x[1:] == y[1:] and (x[0] == y[0] and math.copysign(1.0, x[0]) == math.copysign(1.0, y[0]) or
                                                        (math.isnan(x[0]) and math.isnan(y[0]))) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["ties", "specials", "nan"])
def test_the_two_inserts_agree_without_nan_and_on_nan_only(kind):
    for seed in range(60):
        limit = LIMITS[seed % len(LIMITS)]
        values = script(seed, 400, kind)
        binary, binary_trace = replay(model.lower_bound_insert, values, limit)
        first, first_trace = replay(model.nan_first_insert, values, limit)
        assert same(binary, first), (seed, limit)
        assert [t[:2] for t in binary_trace] == [t[:2] for t in first_trace], (seed, limit)


def test_raw_inserts_agree_without_the_acceptance_rule():
    """`sorted_buffer_gt::insert` on its own refuses only a position of `limit`: a NaN into a full buffer of numbers lands in cell 0 and
    drops the last — in both models."""
    for insert in (model.lower_bound_insert, model.nan_first_insert):
        buf = []
        for slot, d in enumerate([1.0, 2.0, 3.0]):
            assert insert(buf, d, slot, 3)
        assert not insert(buf, 4.0, 9, 3) and [e[1] for e in buf] == [0, 1, 2]
        assert insert(buf, math.nan, 7, 3)
        assert [e[1] for e in buf] == [7, 0, 1]


def test_nan_first_keeps_what_the_cell_rule_lost():
    """[NaN, 1, 2] and the newcomer 1.5: `d[i-1] < nd` per cell makes cells 0 and 2 both take it and the NaN vanish."""
    buf = []
    for slot, d in enumerate([1.0, 2.0, math.nan]):
        model.nan_first_insert(buf, d, slot, 8)
    assert [e[1] for e in buf] == [2, 0, 1]
    model.nan_first_insert(buf, 1.5, 3, 8)
    assert [e[1] for e in buf] == [2, 0, 3, 1]
    model.nan_first_insert(buf, math.nan, 4, 4)  # full: the last cell falls off
    assert [e[1] for e in buf] == [4, 2, 0, 3]


def test_binary_model_equals_the_linear_insert_without_nan():
    """The NaN-free row of the issue's table: 300 tie-heavy scripts of 400 operations under the acceptance rule."""
    from tests.test_gpu_containers import ref_sorted_insert
    for seed in range(300):
        limit = LIMITS[seed % len(LIMITS)]
        values = script(seed, 400, "ties")
        binary, _ = replay(model.lower_bound_insert, values, limit)
        linear = []
        for slot, d in enumerate(values):
            if model.accepts(linear, float(d), limit):
                ref_sorted_insert(linear, float(d), slot, limit)
        assert [(e[0], e[1]) for e in binary] == linear, (seed, limit)


def test_first_open_and_the_closed_flag():
    top = model.TopModel(4, model.nan_first_insert)
    assert top.pop_open() is None
    top.insert(2.0, 10)
    top.insert(1.0, 11, closed=True)
    top.insert(3.0, 12)
    assert top.pop_open() == (1, 2.0, 10)  # the closed member in cell 0 is never handed out
    top.insert(0.5, 13)
    assert top.radius == 3.0 and top.pop_open() == (0, 0.5, 13)
    assert top.pop_open() == (3, 3.0, 12) and top.pop_open() is None
    assert not top.insert(3.0, 14) and top.insert(2.5, 15) and top.accepted == 5
    assert [e[1] for e in top.buf] == [13, 11, 10, 15] and top.radius == 2.5


def lists_for_merge(rng, shards, queries, k, levels):
    distances = np.sort(rng.integers(0, levels, size=(shards, queries, k)).astype(np.float32) * 0.25, axis=2)
    keys = rng.integers(1, 1 << 40, size=(shards, queries, k)).astype(np.uint64)
    counts = rng.integers(0, k + 1, size=(shards, queries)).astype(np.uint64)
    counts[:, 0], counts[:, 1] = 0, k
    return distances, keys, counts


@pytest.mark.parametrize("shards,k,levels", [(2, 10, 3), (8, 1, 2), (3, 100, 50), (5, 7, 4)])
def test_merge_model_equals_merge_into_without_nan(shards, k, levels):
    from oracle import oraclebind
    rng = np.random.default_rng(shards * 100 + k)
    queries = 24
    distances, keys, counts = lists_for_merge(rng, shards, queries, k, levels)
    for q in range(queries):
        out_k, out_d, merged = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.float32), 0
        lists = []
        for shard in range(shards):
            n = int(counts[shard, q])
            merged = oraclebind.merge_into(out_k, out_d, merged, keys[shard, q, :n], distances[shard, q, :n], n)
            lists.append([(float(d), int(key)) for d, key in zip(distances[shard, q, :n], keys[shard, q, :n])])
        got = model.merge_model(lists, k, later_position_first=True)
        assert got == [(float(d), int(key)) for d, key in zip(out_d[:merged], out_k[:merged])], q
        # the binary insert gives the same fold, and the other order inside a shard differs only among equal distances of one shard
        assert got == model.merge_model(lists, k, True, insert=model.lower_bound_insert)
        other = model.merge_model(lists, k, later_position_first=False)
        assert [d for d, _ in other] == [d for d, _ in got]


@pytest.mark.parametrize("later_position_first", [True, False])
@pytest.mark.parametrize("nan_share", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("shards,k", [(3, 1), (3, 7), (8, 7), (8, 100)])
def test_host_merge_rank_follows_the_model(shards, k, nan_share, later_position_first):
    """`merge_rank` (csrc/merge_core.hpp) walked on the host as the sharded step walks it without a device, over lists kept under the
    rule: NaN first, then distance ↑, then shard ↓ and the order inside a shard — equal to inserting the lists one after the other.
    The same lists go through the merge kernel in tests/test_gpu_merge.py."""
    from usearch_amd import index as ua
    rng = np.random.default_rng(shards * 1000 + k)
    distances, keys, counts = model.nan_first_lists(rng, shards, 64, k, nan_share)
    sentinel = 0xABABABABABABABAB
    got = ua.test_merge(distances, keys, counts, later_position_first, on_host=True, key_sentinel=sentinel)
    model.assert_merge_follows_model(got, distances, keys, counts, later_position_first, sentinel)
