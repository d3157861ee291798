"""A plain model of clustering a batch by the index's own levels (usearch_amd/csrc/clustering.hpp, rules 1 - 8), restated from
`index_dense_gt::cluster` (index_dense.hpp:1819-1981) on Python lists.

The model knows nothing about graphs or metrics; it is fed by callables:
    descend(queries, level)   → (keys, slots, distances, visited, computed), one cell per query: the greedy descent to `level`
    pair_distance(a, b)       → metric(stored row of slot a as the query, stored row of slot b)
    query_distance(q, slot)   → metric(query number q, stored row of `slot`)
    nodes_at_or_above(level)  → members whose level is at least `level`, removed ones included (`stats(level).nodes`)

tests/test_cluster_model.py pins it to the compiled reference (oracle descent, oracle distances, recorded fixtures);
tests/test_gpu_clustering.py pins the device code to it (fed by `Index.cluster` and `Index.distances`).
"""
from __future__ import annotations

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


class ClusteringError(RuntimeError):
    pass


def choose_level(max_level: int, nodes_at_or_above, min_clusters: int, max_clusters: int):
    """Rule 1 (and the refusal of rule 8). → (level, min_clusters, max_clusters)."""
    if min_clusters and not max_clusters:
        raise ClusteringError("Clustering needs max_clusters when min_clusters is set")
    level = max_level
    if min_clusters:
        while level > 1:
            if nodes_at_or_above(level) > min_clusters:
                break
            level -= 1
    else:
        level, max_clusters, min_clusters = 1, (nodes_at_or_above(1) if max_level >= 1 else 0), 2
    if max_level < 2:
        raise ClusteringError("Index too small to cluster!")
    return level, min_clusters, max_clusters


def order_entries(entries):
    """Rule 5: popularity descending, then centroid key ascending, then slot. `entries`: dicts with slot, key, popularity.
    → (ordered list, whether two entries had the same popularity)."""
    popularities = [e["popularity"] for e in entries]
    ties = len(set(popularities)) != len(popularities)
    return sorted(entries, key=lambda e: (-e["popularity"], e["key"], e["slot"])), ties


def merge(entries, max_clusters: int, pair_distance):
    """Rule 6 on an ordered list of entries (modified in place: `merged_into` = the slot an entry went into, or None).
    → (live entries in their final order, merge cycles, per cycle (winner distance, runner-up distance or None))."""
    for e in entries:
        e.setdefault("merged_into", None)
    order = list(entries)
    live, cycles, margins = len(order), 0, []
    while live > max_clusters:
        source = order[live - 1]
        target_position, merge_distance, measured = 0, FLT_MAX, []
        for position in range(live - 1):
            d = float(np.float32(pair_distance(source["slot"], order[position]["slot"])))
            measured.append(d)
            if d < merge_distance:  # strict: the first of equals stays; NaN, +inf and FLT_MAX never win
                merge_distance, target_position = d, position
        others = [d for position, d in enumerate(measured) if position != target_position and d == d]
        runner_up = min(others) if others else None
        margins.append((merge_distance, runner_up))
        target = order[target_position]
        source["merged_into"] = target["slot"]
        target["popularity"] += source["popularity"]
        source["popularity"] = 0
        while target_position and order[target_position - 1]["popularity"] < order[target_position]["popularity"]:
            order[target_position - 1], order[target_position] = order[target_position], order[target_position - 1]
            target_position -= 1
        live -= 1
        cycles += 1
    return order[:live], cycles, margins


def trace(slot: int, merged_into: dict) -> int:
    """Rule 7: the slot of the centroid that survived."""
    hops = 0
    while merged_into.get(slot) is not None:
        slot = merged_into[slot]
        hops += 1
        assert hops <= len(merged_into), "a cycle in merged_into"
    return slot


def chain_length(slot: int, merged_into: dict) -> int:
    hops = 0
    while merged_into.get(slot) is not None:
        slot, hops = merged_into[slot], hops + 1
    return hops


def cluster(queries, max_level: int, nodes_at_or_above, descend, pair_distance, query_distance, min_clusters: int = 0,
            max_clusters: int = 0) -> dict:
    """The whole of it. → dict(keys, distances, clusters, unique_before_merge, merge_cycles, mapping_passes, visited_members,
    computed_distances, level, popularity_ties, merged_into (slot → slot), margins, final_order (slots))."""
    level, min_clusters, max_clusters = choose_level(max_level, nodes_at_or_above, min_clusters, max_clusters)
    count = len(queries)
    result = dict(keys=np.zeros(count, dtype=np.uint64), distances=np.zeros(count, dtype=np.float32), clusters=0, unique_before_merge=0,
                  merge_cycles=0, mapping_passes=0, visited_members=0, computed_distances=0, level=level, popularity_ties=False,
                  merged_into={}, margins=[], final_order=[])
    if not count:
        return result
    while True:
        keys, slots, distances, visited, computed = descend(queries, level)
        result["mapping_passes"] += 1
        result["visited_members"] += int(np.sum(visited))
        result["computed_distances"] += int(np.sum(computed))
        by_slot = {}
        for key, slot in zip(keys.tolist(), slots.tolist()):
            entry = by_slot.setdefault(slot, dict(slot=slot, key=key, popularity=0))
            entry["popularity"] += 1
        if len(by_slot) < min_clusters and level > 1:
            level -= 1
            continue
        break
    entries, ties = order_entries(list(by_slot.values()))
    unique = len(entries)
    survivors, cycles, margins = merge(entries, max_clusters, pair_distance)
    merged_into = {e["slot"]: e["merged_into"] for e in entries}
    out_keys, out_distances = np.array(keys, dtype=np.uint64), np.array(distances, dtype=np.float32)
    if cycles:
        key_of = {e["slot"]: e["key"] for e in entries}
        for q, slot in enumerate(slots.tolist()):
            final = trace(slot, merged_into)
            out_keys[q] = key_of[final]
            out_distances[q] = np.float32(query_distance(q, final))
    result.update(keys=out_keys, distances=out_distances, clusters=unique - cycles, unique_before_merge=unique, merge_cycles=cycles,
                  level=level, popularity_ties=ties, merged_into=merged_into, margins=margins,
                  final_order=[e["slot"] for e in survivors])
    return result
