"""The sketch's lower bound (usearch_amd/csrc/sketch.hpp) against the cos distance computed the kernel's way: for every
(query, row) pair the bound must not exceed the oracle's distance in the eight-lane summation layout — the layout of every
kernel build that carries the sketch path — and a row or a query that must never be pruned has to give −inf. CPU only: the host
twins of the record builder and of the bound, through the test-hook library."""
from __future__ import annotations

import numpy as np
import pytest

import usearch_amd.index as ua_index
from tests import util

ROWS, QUERIES = 2000, 64
F16_LARGEST, F16_SMALLEST_NORMAL = 65504.0, 2.0 ** -14
# rows of the low-rank set that are replaced by the edge cases
ZERO_ROWS = (5, 1500)
NAN_ROW, INF_ROW = 77, 1234
LARGE_ROW, SMALL_ROW = 300, 301
# magnitudes at which the kernel's f32 sums of squares underflow or overflow (f16 stores them as zeros and infinities)
UNDERFLOWING_ROW, OVERFLOWING_ROW = 302, 303
DUPLICATES = ((400, 10), (401, 10), (1999, 1998))
ZERO_QUERY, UNDERFLOWING_QUERY, OVERFLOWING_QUERY = 3, 4, 5


def _store(x: np.ndarray, dtype: str) -> np.ndarray:
    return util.to_bf16(x) if dtype == "bf16" else x.astype(util.NP_DTYPE[dtype])


def _dataset(kind: str, ndim: int, dtype: str):
    """→ (rows, queries, rows that are never pruned, queries that never prune)."""
    rng = np.random.default_rng(1000 + ndim)
    if kind == "gaussian":
        rows, queries = rng.standard_normal((ROWS, ndim)), rng.standard_normal((QUERIES, ndim))
        return _store(rows, dtype), _store(queries, dtype), (), ()
    # the benchmark's data: a seeded rank-32 latent plus 0.05 noise, out-of-sample queries
    rank = min(32, max(2, ndim // 4))
    basis = rng.standard_normal((rank, ndim))
    rows = rng.standard_normal((ROWS, rank)) @ basis + 0.05 * rng.standard_normal((ROWS, ndim))
    queries = rng.standard_normal((QUERIES, rank)) @ basis + 0.05 * rng.standard_normal((QUERIES, ndim))
    rows[LARGE_ROW] *= F16_LARGEST / np.abs(rows[LARGE_ROW]).max()
    rows[SMALL_ROW] *= F16_SMALLEST_NORMAL / np.abs(rows[SMALL_ROW]).max()
    rows[UNDERFLOWING_ROW] *= 1e-20 / np.abs(rows[UNDERFLOWING_ROW]).max()
    rows[OVERFLOWING_ROW] *= 1e18 / np.abs(rows[OVERFLOWING_ROW]).max()
    for copy, original in DUPLICATES:
        rows[copy] = rows[original]
    for row in ZERO_ROWS:
        rows[row] = 0.0
    rows[NAN_ROW, ndim // 2] = np.nan
    rows[INF_ROW, 1] = np.inf
    queries[ZERO_QUERY] = 0.0
    queries[UNDERFLOWING_QUERY] *= 1e-20 / np.abs(queries[UNDERFLOWING_QUERY]).max()
    queries[OVERFLOWING_QUERY] *= 1e18 / np.abs(queries[OVERFLOWING_QUERY]).max()
    with np.errstate(invalid="ignore", over="ignore"):
        return _store(rows, dtype), _store(queries, dtype), ZERO_ROWS + (NAN_ROW, INF_ROW, UNDERFLOWING_ROW, OVERFLOWING_ROW), (ZERO_QUERY, UNDERFLOWING_QUERY, OVERFLOWING_QUERY)


@pytest.mark.parametrize("kind", ["lowrank", "gaussian"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("ndim", [768, 100, 24])
def test_bound_never_exceeds_the_kernels_distance(ndim, dtype, kind):
    rows, queries, never_rows, never_queries = _dataset(kind, ndim, dtype)
    bounds, rank = ua_index.test_sketch_bounds(rows, queries, dtype)
    assert 0 < rank <= min(62, ndim), f"{rank} directions for {ndim} dimensions"
    both = np.ascontiguousarray(np.concatenate([queries, rows]))
    measure = util.slot_distance(both, "cos", dtype, ndim, lanes=8)
    distances = np.array([[measure(q, QUERIES + r) for r in range(ROWS)] for q in range(QUERIES)], dtype=np.float32)

    for row in never_rows:
        assert np.all(np.isneginf(bounds[:, row])), f"row {row} must never be pruned"
    for query in never_queries:
        assert np.all(np.isneginf(bounds[query])), f"query {query} must never prune"
    assert not np.isnan(bounds).any()
    comparable = ~np.isnan(distances)  # a NaN distance orders against nothing; its bound is −inf (checked above)
    assert np.all(np.isneginf(bounds[~comparable]))
    excess = np.where(comparable, bounds.astype(np.float64) - distances.astype(np.float64), -np.inf)
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    print(f"{kind} {ndim} {dtype}: {rank} directions, largest bound − distance {excess.max():.3g}")
    assert np.all(bounds[comparable] <= distances[comparable]), \
        f"bound {bounds[worst]} above the distance {distances[worst]} at query {worst[0]}, row {worst[1]}"

    for copy, original in (DUPLICATES if kind == "lowrank" else ()):
        assert np.array_equal(bounds[:, copy], bounds[:, original]), "equal rows, equal records"
    if kind == "lowrank":
        # the bound has to be of use on data with low-rank structure: tighter than the distances are spread
        finite = comparable & np.isfinite(bounds)
        slack = np.median(distances[finite].astype(np.float64) - bounds[finite])
        low, high = np.percentile(distances[finite], [10, 90])
        print(f"  median distance − bound {slack:.4g}, 10th … 90th percentile of the distances {low:.4g} … {high:.4g}")
        assert slack < high - low
