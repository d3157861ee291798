"""A ground truth for exact search that does not come from a kernel, and data on which it decides: plain numpy, no GPU.

THE TRUTH. Rows and queries are widened exactly to f64 (f16, bf16 = bits << 16 and i8 are all exact there), the whole distance
matrix is computed in f64 — cos, ip, l2sq, with the reference's answers for zero norms in cos (metric_cos_gt: 0 for two zero
vectors, 1 for one) — and ordered as `search_exact_` orders: distance ↑, slot ↓.

THE BOUND, per (query a, row b): what a distance from f32 accumulation of EXACT products (f16 × f16 and bf16 × bf16 fit an f32
mantissa, i8 sums are integers) plus the closing arithmetic may differ from the f64 value by. u = 2⁻²⁴, γ = (ndim + 16)·u.
  · Σab summed in f32 in any order: |error| ≤ (ndim − 1)·u·Σ|aᵢbᵢ| (first order; the matrix unit's order is its own).
  · Σa², Σb² (`row_norms_kernel`: a lane takes every 64th element by fmaf, then six shuffle-adds): ≤ (ndim/64 + 6)·u·Σx² each.
  · ip (`closing_distance`: 1 − Σab): one more rounding, u·|1 − Σab| ≤ u·(1 + Σ|aᵢbᵢ|), which the 16 spare units of γ cover while
    Σ|aᵢbᵢ| ≥ 1/15 — `Truth` asserts that for ip.                                                     bound = γ·Σ|aᵢbᵢ|
  · l2sq (Σa² + Σb² − 2Σab, two roundings of at most u·(Σa² + Σb²) and u·d): (ndim/64 + 8)·u·(Σa² + Σb²) + 2(ndim − 1)·u·Σ|aᵢbᵢ|
                                                                                       bound = γ·(Σa² + Σb² + 2Σ|aᵢbᵢ|)
  · cos (1 − Σab / (√Σa²·√Σb²)): Σ|aᵢbᵢ| ≤ √Σa²·√Σb² (Cauchy-Schwarz), so the sum's error is ≤ (ndim − 1)·u of the quotient's scale;
    the norms add (ndim/64 + 6)·u (half of it per root, two roots), the two roots, their product, the division and the subtraction
    a rounding each (quotient ≤ 1): (ndim + ndim/64 + 10)·u < 2γ.
  · cos over i8: the three sums are exact integers below 2²⁴, so only the closing arithmetic rounds — two roots (u each, both in the
    product), the product, the division (quotient ≤ 1: ≤ 4u so far) and the subtraction (≤ 2u): 6u, stated as 8u. (3γ would exceed
    the suite's tolerance for i8, 1e-5, from 40 dimensions on; the exact sums do not need it.)             bound(cos, i8) = 8u
  · the wide kernel's fused fold (f16 cos / ip) rounds the accumulator once more with −threshold·√Σb² in it and takes that out again by
    one fmaf: 2u·(|Σab| + |threshold·√Σb²|) more. cos: the threshold is (1 − bound)·√Σa² with a distance bound in [0, 2]: ≤ 4u of the
    quotient's scale, inside the third γ. ip: the threshold is the query's k-th best Σab so far, which a row that passes the test
    reaches (Σab ≥ threshold) — for thresholds ≥ 0 that is ≤ 4u·Σ|aᵢbᵢ|, inside the 16 spare units; the fixtures' ip queries all
    have positive k-th best sums (their planted rows).                                                          bound(cos) = 3γ
The bound is derived, not measured; the GPU tests record the largest observed error ÷ bound (tests/test_gpu_exact_truth.py). It must
stay below the suite's float tolerance, `util.tolerance(dtype)·max(1, |d|)`: `Truth` asserts that over the whole matrix.
For ip and l2sq over i8 the distances are integers below 2²⁴: exact in f32, no bound at all.

THE DATA (`plant`): a random background and, for every query, a ladder of planted rows at distances that grow by a fixed factor
(cos / l2sq: q + σⱼ·u with |u| fixed and σⱼ = 0.03·1.22ʲ; ip: q·(1 + 0.1(rungs − j)) + 0.01·u), so that the first k + 1 distances of
most queries lie many bounds apart. A query is DECIDED for k when each of its first k gaps in f64 (ranks 1 … k + 1) is at least 8
bounds wide: then no summation order can change its result, and a kernel's keys must equal the truth's, in order. Rung 0 of decided
queries is moved onto a list of EDGE slots (row 0, row n − 1, the first and last row of every partition of either kernel — taken
from the launch planner — and of a tile, the rows around the 32- and 64-row marks of a tile), so that every edge row is a neighbour
somebody is certain of. `Case.assert_decides` holds the construction to its cap: ≥ 80 % of the queries decided, every edge covered.
"""
from __future__ import annotations

import numpy as np

from tests import util

UNIT = 2.0 ** -24
DECIDED_GAP_IN_BOUNDS = 8.0
DECIDED_SHARE = 0.8


def widen(x: np.ndarray, dtype: str) -> np.ndarray:
    """Storage scalars → f64, exactly."""
    if dtype == "bf16":
        return (np.ascontiguousarray(x, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert x.dtype == util.NP_DTYPE[dtype]
    return x.astype(np.float64)


def narrow(x: np.ndarray, dtype: str) -> np.ndarray:
    """f64 → storage scalars (round to nearest; bf16 by truncation, like `util.to_bf16`; i8 clipped to ±127)."""
    if dtype == "bf16":
        return util.to_bf16(x)
    if dtype == "i8":
        return np.clip(np.rint(x), -127, 127).astype(np.int8)
    return x.astype(util.NP_DTYPE[dtype])


def integer_pair(metric: str, dtype: str) -> bool:
    return dtype == "i8" and metric in ("ip", "l2sq")


class Truth:
    """Distances of `queries` to `rows` in f64, their bounds, and the order (distance ↑, slot ↓) over the rows `allowed` lets through."""

    def __init__(self, metric: str, dtype: str, rows: np.ndarray, queries: np.ndarray, allowed=None):
        self.metric, self.dtype = metric, dtype
        r, q = widen(rows, dtype), widen(queries, dtype)
        self.ndim = ndim = r.shape[1]
        self.allowed = np.ones(len(r), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
        ab, r2, q2 = q @ r.T, (r * r).sum(1), (q * q).sum(1)
        gamma = (ndim + 16) * UNIT
        if metric == "ip":
            d = 1.0 - ab
            absolute = np.abs(q) @ np.abs(r).T
            bound = gamma * absolute
            assert integer_pair(metric, dtype) or absolute.min() >= 1.0 / 15, "γ's spare units must cover the closing subtraction"
        elif metric == "l2sq":
            d = np.maximum(q2[:, None] + r2[None, :] - 2.0 * ab, 0.0)
            bound = gamma * (q2[:, None] + r2[None, :] + 2.0 * (np.abs(q) @ np.abs(r).T))
        else:
            assert metric == "cos"
            with np.errstate(divide="ignore", invalid="ignore"):
                d = 1.0 - ab / (np.sqrt(q2)[:, None] * np.sqrt(r2)[None, :])
            zero_q, zero_r = (q2 == 0)[:, None], (r2 == 0)[None, :]
            d = np.where(zero_q & zero_r, 0.0, np.where(zero_q | zero_r, 1.0, d))
            if dtype == "i8":  # metric_cos_i8_t: a zero sum closes to 0 whatever the norms
                d = np.where(ab == 0, 0.0, d)
            bound = np.full_like(d, 8.0 * UNIT if dtype == "i8" else 3.0 * gamma)
        if integer_pair(metric, dtype):
            assert np.abs(d).max() < 2 ** 24, "integer distances must be exact in f32"
            bound = np.zeros_like(d)
        else:
            assert np.all(bound <= util.tolerance(dtype) * np.maximum(1.0, np.abs(d))), "the bound exceeds the suite's tolerance"
        self.exact = d  # of every row, allowed or not (soundness is checked against the row a key names)
        self.bound = bound
        self.distances = np.where(self.allowed[None, :], d, np.inf)
        self.allowed_count = int(self.allowed.sum())

    def order(self, width: int) -> np.ndarray:
        """→ slots [Q, min(width, allowed rows)]: the first `width` of every query under (distance ↑, slot ↓)."""
        width = min(width, self.allowed_count)
        out = np.zeros((len(self.distances), width), dtype=np.int64)
        slots = np.arange(self.distances.shape[1])
        for i, row in enumerate(self.distances):
            # every row that could be among the first `width`: at most as far as the width-th smallest distance
            near = slots[row <= np.partition(row, width - 1)[width - 1]] if width else slots[:0]
            out[i] = near[np.lexsort((-near, row[near]))][:width]
        return out

    def decided(self, k: int) -> np.ndarray:
        """→ bool [Q]: each of the first k gaps (ranks 1 … k + 1, as far as rows exist) is ≥ 8 bounds wide."""
        first = self.order(k + 1)
        at = np.arange(len(first))[:, None]
        d, b = self.distances[at, first], self.bound[at, first]
        if integer_pair(self.metric, self.dtype):
            return np.ones(len(first), dtype=bool)  # the order is total and the sums exact: every query is decided
        return np.all(d[:, 1:] - d[:, :-1] >= DECIDED_GAP_IN_BOUNDS * np.maximum(b[:, 1:], b[:, :-1]), axis=1)

    def check(self, slots: np.ndarray, distances: np.ndarray, counts: np.ndarray, k: int, padding=None) -> dict:
        """Holds a result — `slots` [Q, k] (keys mapped back to slots), `distances`, `counts` — to the conditions for ALL queries
        (counts, ascending distances, no repeats, nobody the filter rejects, soundness, completeness) and, for the decided ones, to
        the truth's keys in order; integer pairs to the truth's keys and distance bits for every query. `padding` [Q, k]: the raw
        keys, whose cells past a query's count must be 0. → what was observed: the largest error ÷ bound, the decided share."""
        slots, counts = np.asarray(slots, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        distances = np.asarray(distances, dtype=np.float32)
        queries, rows = self.distances.shape
        assert slots.shape == distances.shape == (queries, k) and counts.shape == (queries,)
        expected_count = min(k, self.allowed_count)
        got = distances[:, :expected_count].astype(np.float64)  # (the cells past a count are signalling NaNs: not looked at)
        assert np.all(counts == expected_count), f"counts: {np.unique(counts)} where {expected_count} rows are due"
        found = np.arange(k)[None, :] < counts[:, None]
        if padding is not None:
            assert np.all(np.asarray(padding)[~found] == 0), "cells past a query's count must carry key 0"
        slots = slots[:, :expected_count]
        first = self.order(k)
        report = dict(error_in_bounds=0.0, decided=1.0)
        if not expected_count:
            return report
        assert np.all((slots >= 0) & (slots < rows)), "a key that names no row"
        assert np.all(self.allowed[slots]), "a row the filter rejects, or a removed one"
        ordered = np.sort(slots, axis=1)
        assert np.all(ordered[:, 1:] != ordered[:, :-1]), "a key is repeated"
        assert np.all(np.diff(got, axis=1) >= 0), "distances must ascend"
        at = np.arange(queries)[:, None]
        if integer_pair(self.metric, self.dtype):
            wrong = np.argwhere(slots != first)
            assert not len(wrong), f"{len(wrong)} keys differ from the lexsort of the exact integers; first at (query, rank) {wrong[0]}: " \
                                   f"slot {slots[tuple(wrong[0])]} for {first[tuple(wrong[0])]}"
            assert np.array_equal(got.astype(np.float32).view(np.uint32), self.distances[at, first].astype(np.float32).view(np.uint32))
            return report
        # soundness: every distance within the bound of the f64 distance of the row it names
        error, bound = np.abs(got - self.exact[at, slots]), self.bound[at, slots]
        report["error_in_bounds"] = float((error / bound).max())
        worst = np.unravel_index(np.argmax(error / bound), error.shape)
        assert np.all(error <= bound), f"a distance is {error[worst] / bound[worst]:.2f} bounds from its row's f64 distance " \
                                       f"(query {worst[0]}, rank {worst[1]}, slot {slots[worst]}: {got[worst]!r} for {self.exact[worst[0], slots[worst]]!r})"
        # completeness: whoever is closer than the last returned distance by more than the two bounds is among the keys
        returned = np.zeros((queries, rows), dtype=bool)
        returned[at, slots] = True
        if expected_count < k:
            missing = self.allowed[None, :] & ~returned
        else:
            last, last_bound = got[:, -1:], self.bound[at, slots][:, -1:]
            missing = (self.distances < last - (self.bound + last_bound)) & ~returned
        dropped = np.argwhere(missing)
        assert not len(dropped), f"{len(dropped)} rows closer than a query's last result are not among its keys; first: query " \
                                 f"{dropped[0][0]} lacks slot {dropped[0][1]} at {self.distances[tuple(dropped[0])]!r}, its last is {got[dropped[0][0], -1]!r}"
        decided = self.decided(k)
        report["decided"] = float(decided.mean())
        wrong = np.argwhere((slots != first) & decided[:, None])
        assert not len(wrong), f"{len(wrong)} keys of decided queries differ from the truth's; first at (query, rank) {wrong[0]}: slot " \
                               f"{slots[tuple(wrong[0])]} for {first[tuple(wrong[0])]}"
        return report


def edge_slots(rows: int, plans) -> list:
    """The rows where a tile or a partition begins or ends, for every plan in `plans` (dicts of `test_plan_exact`): row 0, row n − 1,
    the first and last row of every partition, of the second 256-row and the second 128-row tile, and the rows around the 32- and
    64-row marks of the third 256-row tile."""
    edges = {0, rows - 1, 128, 255, 256, 511, 512 + 31, 512 + 32, 512 + 63, 512 + 64}
    for plan in plans:
        for partition in range(plan["partitions"]):
            first = partition * plan["rows_per_partition"]
            if first < rows:  # (the wide kernel may be left with an empty last partition)
                edges |= {first, min(first + plan["rows_per_partition"], rows) - 1}
    return sorted(edge for edge in edges if 0 <= edge < rows)


class Case:
    """Planted data: `rows` [n], `queries` [Q], `ladders` [Q, rungs] the slots of every query's planted rows, nearest first, the
    `edges` that hold rung 0 of a decided query, and `usable` [n] — where planted rows may sit (the members a filter or a removal will
    leave)."""

    def __init__(self, metric, dtype, rows, queries, ladders, edges, usable):
        self.metric, self.dtype, self.rows, self.queries, self.ladders, self.edges, self.usable = metric, dtype, rows, queries, ladders, edges, usable
        self._truths = {}

    def truth(self, allowed=None, count=None) -> Truth:
        """The truth over the members `allowed` lets through (None: all), for the first `count` queries (None: all)."""
        key = (None if allowed is None else np.asarray(allowed, dtype=bool).tobytes(), count)
        if key not in self._truths:
            self._truths[key] = Truth(self.metric, self.dtype, self.rows, self.queries[:count], allowed)
        return self._truths[key]

    def assert_decides(self, k: int, allowed=None, count=None, cap: bool = True):
        """The construction's cap, checked before any GPU call: ≥ 80 % of the queries decided for k, and every edge row among the
        first k of a decided query. (Integer pairs are decided everywhere; the edges still have to be somebody's neighbours.)"""
        truth = self.truth(allowed, count)
        decided, first = truth.decided(k), truth.order(k)
        if cap:
            assert decided.mean() >= DECIDED_SHARE, f"only {decided.mean():.1%} of the queries are decided for k = {k}"
            covered = set(first[decided].reshape(-1).tolist())
            lost = [edge for edge in self.edges if edge not in covered and truth.allowed[edge]]
            assert not lost, f"edge rows {lost} are no decided query's neighbour for k = {k}"
        return float(decided.mean())


def plant(metric: str, dtype: str, ndim: int, rows: int, queries: int, rungs: int, seed: int, edges=(), usable=None, copies: int = 0,
          near_ties: int = 0) -> Case:
    """Background rows and queries of norm ≈ 2 (i8: entries within ±60, N(0, 20²) clipped at three deviations), a ladder of `rungs` planted rows per query at seeded random
    usable slots, then rung 0 of decided queries moved onto the usable `edges`. `copies` more queries repeat the first `queries`
    under a seeded permutation (a large batch whose truth costs no more to decide).
    `near_ties` (cos; the rows of a wide partition): the planted rows of a query form a cluster instead, cos distances
    0.01 + 8e-5·j — more than two bounds and far less than 1e-3 apart — all inside ONE partition (a partition's list then fills with
    them, where a cluster dealt over the partitions would leave every partition's k-th best out in the background), in slots that
    run from the farthest to the nearest: the last of them arrive when their query's k-th best stands a hair above them, which is
    where a pruning test that is not conservative drops a neighbour. Little is decided there; the conditions for all queries are
    what such data are for."""
    rng = np.random.default_rng(seed)
    usable = np.ones(rows, dtype=bool) if usable is None else np.asarray(usable, dtype=bool)
    scale = 60.0 / 3.0 if dtype == "i8" else 2.0 / np.sqrt(ndim)
    background = narrow(np.clip(rng.standard_normal((rows, ndim)), -3, 3) * scale, dtype)
    # (ip over i8: queries within ±40, so that the ladder's multiples of a query, up to 2.6 of it, stay inside int8)
    q = narrow(np.clip(rng.standard_normal((queries, ndim)), -3, 3) * (40.0 / 3.0 if (metric, dtype) == ("ip", "i8") else scale), dtype)
    wide_q = widen(q, dtype)
    free = np.flatnonzero(usable)
    assert queries * rungs <= len(free), "more planted rows than usable slots"
    ladders = rng.permutation(free)[:queries * rungs].reshape(queries, rungs)
    u = rng.standard_normal((queries, rungs, ndim))
    u *= 2.0 * np.linalg.norm(wide_q, axis=1)[:, None, None] / np.linalg.norm(u, axis=2, keepdims=True)  # |u| = 2·|q|
    j = np.arange(rungs)[None, :, None]
    if near_ties:
        assert metric == "cos" and not len(edges)
        full = rows // near_ties  # whole partitions
        assert -(-queries // full) * rungs <= near_ties and usable.all()
        dealt = [rng.permutation(near_ties)[:-(-queries // full) * rungs].reshape(-1, rungs) + p * near_ties for p in range(full)]
        ladders = np.stack([dealt[i % full][i // full] for i in range(queries)])
        ladders = -np.sort(-ladders, axis=1)  # rung 0, the nearest, in the last slot
        u -= (u * wide_q[:, None, :]).sum(2, keepdims=True) / (wide_q * wide_q).sum(1)[:, None, None] * wide_q[:, None, :]  # u ⟂ q,
        u *= 2.0 * np.linalg.norm(wide_q, axis=1)[:, None, None] / np.linalg.norm(u, axis=2, keepdims=True)            # |u| = 2·|q|:
        planted = wide_q[:, None, :] + 0.5 * np.sqrt((1.0 - (0.01 + 8e-5 * j)) ** -2 - 1.0) * u  # cos distance 0.01 + 8e-5·j before rounding
    elif metric == "ip":
        assert dtype != "i8" or rungs <= 16
        planted = wide_q[:, None, :] * (1.0 + 0.1 * (rungs - j)) + 0.01 * u
    else:
        planted = wide_q[:, None, :] + 0.03 * 1.22 ** j * u
    background[ladders.reshape(-1)] = narrow(planted.reshape(-1, ndim), dtype)
    case = Case(metric, dtype, background, q, ladders, [], usable)
    # rung 0 of decided queries onto the edges: swapping the contents of two usable slots changes nobody's distances
    decided = np.flatnonzero(case.truth(usable).decided(rungs - 1))
    edges = [edge for edge in edges if usable[edge]]
    assert len(edges) <= len(decided), "more edge rows than decided queries to lend them a neighbour"
    owner = {int(slot): (i, r) for i in range(queries) for r, slot in enumerate(ladders[i])}
    for edge, i in zip(edges, decided):
        here = int(ladders[i, 0])
        if here == edge:
            continue
        background[[edge, here]] = background[[here, edge]]
        displaced = owner.pop(edge, None)
        owner[edge] = (int(i), 0)
        ladders[i, 0] = edge
        if displaced is not None:
            owner[here] = displaced
            ladders[displaced] = here
        else:
            owner.pop(here)
    if copies:
        q = np.concatenate([q, q[rng.integers(0, queries, copies)]])
    return Case(metric, dtype, background, q, ladders, edges, usable)
