"""A ground truth for exact search over bit vectors that does not come from a kernel: plain numpy, no GPU.

Rows and queries are unpacked to 0 / 1, the intersections |a∧b| of every (query, row) pair are one int32 matrix product, |a| and |b|
are row sums, and everything else follows in integers: |a⊕b| = |a| + |b| − 2|a∧b|, |a∨b| = |a| + |b| − |a∧b|. The distances close
in `np.float32`, in the order of `finalize_distance` (csrc/kernels.hpp) and `closing_distance` (csrc/device_math.hpp):

    hamming    (float)|a⊕b|
    tanimoto   1 − (float)|a∧b| / (float)|a∨b|          (jaccard is tanimoto)
    sorensen   1 − 2·(float)|a∧b| / (float)(|a| + |b|)

— one IEEE division of exact integers, so a kernel's distances must carry these very bits. 0 / 0 (two empty sets) is a NaN, as the
reference returns it; which NaN is the divider's business, so NaN cells are compared by `isnan`. The order is `search_exact_`'s:
NaN first, then distance ↑, then the later slot first among equals, over the rows `allowed` lets through.

`data` is what every test of the bit tile runs on, and `tie_share` says why it is worth running: how many queries have EQUAL distances
at ranks k and k + 1, where only the tie rule decides who is returned."""
from __future__ import annotations

import functools

import numpy as np

from tests import util

METRICS = ("hamming", "tanimoto", "jaccard", "sorensen")
ROWS, QUERIES, K = 5003, 300, 10  # the shape the tie shares below are stated for


class BitsTruth:
    def __init__(self, metric: str, rows: np.ndarray, queries: np.ndarray, allowed=None):
        assert metric in METRICS and rows.dtype == np.uint8 and queries.dtype == np.uint8
        self.metric = metric
        r, q = np.unpackbits(rows, axis=1).astype(np.int32), np.unpackbits(queries, axis=1).astype(np.int32)
        both = q @ r.T  # |a∧b|, exact
        r1, q1 = r.sum(1, dtype=np.int32), q.sum(1, dtype=np.int32)
        total = q1[:, None] + r1[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            if metric == "hamming":
                d = (total - 2 * both).astype(np.float32)
            elif metric == "sorensen":
                d = np.float32(1) - np.float32(2) * both.astype(np.float32) / total.astype(np.float32)
            else:
                d = np.float32(1) - both.astype(np.float32) / (total - both).astype(np.float32)
        assert d.dtype == np.float32
        self.exact = d
        self.allowed = np.ones(len(rows), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
        self.allowed_count = int(self.allowed.sum())

    def restricted(self, count=None, allowed=None) -> "BitsTruth":
        """The same distances for the first `count` queries (None: all) over the rows `allowed` lets through (None: as before)."""
        other = object.__new__(BitsTruth)
        other.metric, other.exact = self.metric, self.exact[:count]
        other.allowed = self.allowed if allowed is None else np.asarray(allowed, dtype=bool)
        other.allowed_count = int(other.allowed.sum())
        return other

    def order(self, width: int) -> np.ndarray:
        """→ slots [Q, min(width, allowed rows)]: the first `width` of every query under (NaN first, distance ↑, slot ↓)."""
        width = min(width, self.allowed_count)
        slots = np.flatnonzero(self.allowed)
        out = np.zeros((len(self.exact), width), dtype=np.int64)
        for i, row in enumerate(self.exact):
            d = row[slots]
            rank = np.where(np.isnan(d), -np.inf, d.astype(np.float64))
            out[i] = slots[np.lexsort((-slots, rank))][:width]
        return out

    def check(self, slots: np.ndarray, distances: np.ndarray, counts: np.ndarray, k: int, padding=None) -> None:
        """Holds a result — `slots` [Q, k] (keys mapped back to slots), `distances`, `counts` — to the truth for EVERY query: counts,
        keys in order, distance bits (NaN cells by `isnan`). `padding` [Q, k]: the raw keys, whose cells past a query's count must be
        0; the distances there must be the signalling NaN."""
        slots, counts = np.asarray(slots, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        distances = np.asarray(distances, dtype=np.float32)
        queries = len(self.exact)
        assert slots.shape == distances.shape == (queries, k) and counts.shape == (queries,)
        expected_count = min(k, self.allowed_count)
        assert np.all(counts == expected_count), f"counts: {np.unique(counts)} where {expected_count} rows are due"
        if padding is not None:
            assert np.all(np.asarray(padding)[:, expected_count:] == 0), "cells past a query's count must carry key 0"
        assert np.all(distances[:, expected_count:].view(np.uint32) == 0x7FA00000), "cells past a query's count: the signalling NaN"
        if not expected_count:
            return
        first = self.order(k)
        got = slots[:, :expected_count]
        wrong = np.argwhere(got != first)
        assert not len(wrong), f"{len(wrong)} keys differ from the truth's order; first at (query, rank) {wrong[0]}: slot " \
                               f"{got[tuple(wrong[0])]} for {first[tuple(wrong[0])]}"
        want = self.exact[np.arange(queries)[:, None], first]
        have = distances[:, :expected_count]
        assert np.array_equal(np.isnan(have), np.isnan(want)), "NaN distances in other cells than the truth's"
        numbers = ~np.isnan(want)
        assert np.array_equal(have[numbers].view(np.uint32), want[numbers].view(np.uint32)), "distance bits differ from the truth's"

    def tie_share(self, k: int) -> float:
        """The share of queries whose distances at ranks k and k + 1 are equal (two NaNs count as equal)."""
        first = self.order(k + 1)
        d = self.exact[np.arange(len(first))[:, None], first[:, k - 1:k + 1]]
        return float(((d[:, 0] == d[:, 1]) | (np.isnan(d[:, 0]) & np.isnan(d[:, 1]))).mean())


@functools.lru_cache(maxsize=None)
def data(ndim: int, rows: int = ROWS, queries: int = QUERIES):
    """→ (rows, queries): `util.make_vectors` with seed 1 and seed 2. At 8 dimensions the rows are random bits, all-zero rows among
    them; the LAST query is then made all zero too, so that tanimoto and sorensen meet 0 / 0."""
    r, q = util.make_vectors(rows, ndim, "b1", 1), util.make_vectors(queries, ndim, "b1", 2)
    if ndim == 8:
        q[-1] = 0
    r.setflags(write=False), q.setflags(write=False)
    return r, q


@functools.lru_cache(maxsize=None)
def truth(metric: str, ndim: int, rows: int = ROWS, queries: int = QUERIES) -> BitsTruth:
    """The truth over `data(ndim, rows, queries)`, every row allowed; computed once and shared."""
    return BitsTruth(metric, *data(ndim, rows, queries))
