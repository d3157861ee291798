"""What feeds tests/cluster_model.py: the descent and the distances, from the oracle (CPU) or from device code that was there before
`clustering` (`Index.cluster(vectors, level)` and `Index.distances`, both pinned to the oracle by older tests)."""
from __future__ import annotations

import numpy as np

from oracle import oraclebind
from tests import cluster_model, util


FREE_KEY = 0xFFFFFFFFFFFFFFFF  # index_dense.hpp:513


class ImageFacts:
    """Keys, levels and the level counts of a serialized index, read through the oracle's parser."""

    def __init__(self, image: np.ndarray):
        self.oracle = oraclebind.OracleIndex(image)
        n = len(self.oracle)
        self.keys = np.array([self.oracle.key(slot) for slot in range(n)], dtype=np.uint64)
        self.levels = np.array([self.oracle.level(slot) for slot in range(n)], dtype=np.int64)
        self.max_level = int(self.levels.max()) if n else 0
        self.slot_of = {int(key): slot for slot, key in enumerate(self.keys.tolist()) if key != FREE_KEY}

    def nodes_at_or_above(self, level: int) -> int:
        return int(np.sum(self.levels >= level))

    def slots_of(self, keys: np.ndarray) -> np.ndarray:
        return np.array([self.slot_of[int(key)] for key in keys], dtype=np.uint32)

    def reached_slots(self, keys: np.ndarray, distances: np.ndarray, level: int, distance_to) -> np.ndarray:
        """The slots behind a descent's keys. A removed member answers under the free key, which names nobody: it is the removed
        member of that level or above whose distance to the query has the bits the descent returned (`distance_to(q, slot)`);
        two of them at equal distance would be ambiguous, and that is an error of the test's data."""
        slots = np.zeros(len(keys), dtype=np.uint32)
        removed = [slot for slot in np.flatnonzero(self.keys == np.uint64(FREE_KEY)).tolist() if self.levels[slot] >= max(1, level)]
        for q, key in enumerate(keys.tolist()):
            if key != FREE_KEY:
                slots[q] = self.slot_of[key]
                continue
            wanted = np.float32(distances[q]).view(np.uint32)
            fits = [slot for slot in removed if np.float32(distance_to(q, slot)).view(np.uint32) == wanted]
            assert len(fits) == 1, f"query {q}: {len(fits)} removed members fit the free key the descent returned"
            slots[q] = fits[0]
        return slots


class OracleFeed:
    """The oracle's descent and distances in the summation layout of `lanes` lanes per row (0 = the reference's serial loops)."""

    def __init__(self, image, vectors, metric: str, dtype: str, ndim: int, lanes: int = 0):
        self.facts = ImageFacts(image)
        self.vectors, self.metric, self.dtype, self.ndim, self.lanes = np.ascontiguousarray(vectors), metric, dtype, ndim, lanes
        self.pair_distance = util.slot_distance(self.vectors, metric, dtype, ndim, lanes)
        self.queries = None

    def descend(self, queries, level: int):
        self.queries = np.ascontiguousarray(queries)
        keys, distances, visited, computed = self.facts.oracle.cluster(self.queries, level, dtype=self.dtype, lanes=self.lanes)
        return keys, self.facts.reached_slots(keys, distances, level, self.query_distance), distances, visited, computed

    def query_distance(self, q: int, slot: int) -> float:
        return oraclebind.distance(self.queries[q], self.vectors[slot], self.metric, self.dtype, self.ndim, self.lanes)

    def run(self, queries, min_clusters: int = 0, max_clusters: int = 0) -> dict:
        return cluster_model.cluster(queries, self.facts.max_level, self.facts.nodes_at_or_above, self.descend, self.pair_distance,
                                     self.query_distance, min_clusters, max_clusters)

    def run_members(self, keys, min_clusters: int = 0, max_clusters: int = 0) -> dict:
        return self.run(self.vectors[self.facts.slots_of(keys)], min_clusters, max_clusters)


class DeviceFeed:
    """`Index.cluster(vectors, level)` and `Index.distances`; the distance tables are made in one launch each, when first asked."""

    def __init__(self, index, image, vectors, dtype: str):
        self.index, self.facts, self.vectors, self.dtype = index, ImageFacts(image), np.ascontiguousarray(vectors), dtype
        self.pairs = None
        self.queries = self.to_queries = None

    def all_slots(self, rows: int) -> np.ndarray:
        return np.ascontiguousarray(np.broadcast_to(np.arange(len(self.vectors), dtype=np.uint32), (rows, len(self.vectors))))

    def descend(self, queries, level: int):
        if self.queries is not queries:
            self.queries, self.to_queries = queries, None
        keys, distances, visited, computed = self.index.cluster(queries, level, dtype=self.dtype)
        return keys, self.facts.reached_slots(keys, distances, level, self.query_distance), distances, visited, computed

    def pair_distance(self, a: int, b: int) -> float:
        if self.pairs is None:
            self.pairs = self.index.distances(self.vectors, self.all_slots(len(self.vectors)))
        return float(self.pairs[a, b])

    def query_distance(self, q: int, slot: int) -> float:
        if self.to_queries is None:
            self.to_queries = self.index.distances(np.ascontiguousarray(self.queries), self.all_slots(len(self.queries)))
        return float(self.to_queries[q, slot])

    def run(self, queries, min_clusters: int = 0, max_clusters: int = 0) -> dict:
        return cluster_model.cluster(queries, self.facts.max_level, self.facts.nodes_at_or_above, self.descend, self.pair_distance,
                                     self.query_distance, min_clusters, max_clusters)

    def run_members(self, keys, min_clusters: int = 0, max_clusters: int = 0) -> dict:
        return self.run(np.ascontiguousarray(self.vectors[self.facts.slots_of(keys)]), min_clusters, max_clusters)
