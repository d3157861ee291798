"""The k-means assignment on the 256 × 256 LDS-DMA tile (`assign_wide_kernel`, csrc/kmeans.hip), forced with
USEARCH_AMD_KMEANS_TILE=256 at the smallest shapes at which it can go wrong — a short point tile, two tiles and one point, a second
centroid tile holding one row, rows below / of exactly / beyond a 128-byte chunk — against the model (tests/kmeans_model.py): the
reference's casts and serial distance loops, the lowest index among equals. Every case asserts its route through the plan hook."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import usearch_amd
from tests import kmeans_model, util

pytestmark = pytest.mark.gpu

DECIDED_SHARE = 0.8  # the suite's convention (tests/exact_truth.py): at most 20 % of a case's points may be left out as undecided
ITEM_BYTES = {"f16": 2, "bf16": 2, "i8": 1}


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8)


def force(monkeypatch, tile: int, count: int, k: int, ndim: int, dtype: str) -> None:
    """Sets the switch and asserts that this shape then takes that tile."""
    from usearch_amd.index import test_plan_kmeans_assign
    monkeypatch.setenv("USEARCH_AMD_KMEANS_TILE", str(tile))
    plan = test_plan_kmeans_assign(count, k, (ITEM_BYTES[dtype] * ndim + 15) // 16 * 16)
    assert plan["wide"] == (1 if tile == 256 else 0)
    if tile == 256:
        assert plan["point_tiles"] == (count + 255) // 256 and plan["centroid_tiles"] == (k + 255) // 256


@functools.lru_cache(maxsize=None)
def float_case(count: int, k: int, ndim: int, dtype: str, metric: str):
    """`count` points around `k` centres (f32), and the model's distance matrix of their quantised rows, computed once."""
    X, centres = kmeans_model.blobs(count, ndim, k, seed=7 + 1000 * ndim + k, with_centres=True)
    want = kmeans_model.distance_matrix(kmeans_model.quantize(X, "f32", dtype), kmeans_model.quantize(centres, "f32", dtype), metric,
                                        dtype, ndim)
    want.setflags(write=False)
    return X, centres, want


def integer_case(count: int, k: int, ndim: int):
    rng = np.random.default_rng(count + k + ndim)
    return rng.integers(-60, 61, (count, ndim)).astype(np.int8), rng.integers(-60, 61, (k, ndim)).astype(np.int8)


# row bytes: 80 (below a chunk), 128 (one chunk), 400 (three chunks and a 16-byte piece), 192
FLOAT_CASES = [(200, 2, 40, "f16", "l2sq"), (256, 256, 64, "f16", "cos"), (513, 257, 200, "f16", "ip"), (513, 300, 96, "bf16", "l2sq"),
               (200, 257, 96, "bf16", "cos")]


@pytest.mark.parametrize("count,k,ndim,dtype,metric", FLOAT_CASES)
def test_float_kinds_against_the_model(monkeypatch, count, k, ndim, dtype, metric):
    X, centres, want = float_case(count, k, ndim, dtype, metric)
    tolerance = util.tolerance(dtype)
    separated = kmeans_model.separation(want, tolerance)
    assert separated.mean() >= DECIDED_SHARE, "the case must not pass by leaving points out"  # on the CPU, before any GPU call
    force(monkeypatch, 256, count, k, ndim, dtype)
    index, distance = usearch_amd.kmeans_assign(X, centres, metric=metric, dtype=dtype)
    want_index, want_distance = kmeans_model.nearest(want)
    error = np.abs(distance.astype(np.float64) - want_distance)
    print(f"\n[wide] {dtype} {metric} {count} x {k} x {ndim}: max error {error.max():.3g}, undecided {int((~separated).sum())}")
    assert np.all(error <= tolerance * np.maximum(1.0, np.abs(want_distance)))
    assert np.array_equal(index[separated], want_index[separated])


# row bytes: 33 (a ragged piece), 96
@pytest.mark.parametrize("count,k,ndim,metric", [(200, 300, 33, "cos"), (513, 257, 96, "l2sq"), (256, 2, 33, "ip")])
def test_i8_is_exact(monkeypatch, count, k, ndim, metric):
    X, centroids = integer_case(count, k, ndim)
    force(monkeypatch, 256, count, k, ndim, "i8")
    index, distance = usearch_amd.kmeans_assign(X, centroids, metric=metric, dtype="i8")
    want_index, want_distance = kmeans_model.nearest(kmeans_model.distance_matrix(bits(X), bits(centroids), metric, "i8", ndim))
    assert np.array_equal(index, want_index)
    assert util.same_float_bits(distance, want_distance)


@pytest.mark.parametrize("dtype", ["i8", "f16"])
def test_a_copy_in_the_second_tile_never_wins(monkeypatch, dtype):
    """Centroid 259 is a byte copy of centroid 3, which is the row of point 10: equal distances, the lower index wins — across the
    two centroid tiles and across the lanes that share a point."""
    X, centroids = integer_case(200, 300, 96)
    if dtype == "f16":
        X, centroids = (X / 8.0).astype(np.float16), (centroids / 8.0).astype(np.float16)
    centroids[3] = centroids[259] = X[10]
    force(monkeypatch, 256, 200, 300, 96, dtype)
    index, distance = usearch_amd.kmeans_assign(X, centroids, metric="l2sq", dtype=dtype)
    assert index[10] == 3 and distance[10] == 0.0
    assert not (index == 259).any()


def test_nan_never_wins(monkeypatch):
    """f16 l2sq: a centroid row holding a NaN is nobody's nearest; the point whose distances are all NaN ends at index 0 with FLT_MAX."""
    X, centres, _ = float_case(200, 2, 40, "f16", "l2sq")
    X, centres = X.copy(), np.concatenate([centres, centres + 1.0, centres - 1.0])
    X[7, 3] = np.nan
    centres[0, 0] = np.nan
    force(monkeypatch, 256, 200, len(centres), 40, "f16")
    index, distance = usearch_amd.kmeans_assign(X, centres, metric="l2sq", dtype="f16")
    assert index[7] == 0 and distance[7] == np.finfo(np.float32).max
    others = np.arange(200) != 7
    assert (index[others] != 0).all() and np.isfinite(distance[others]).all()


def test_i8_trajectory_equals_the_model(monkeypatch):
    """Three iterations over two point tiles: assignments, distances, centroids and the count of shifted points, bit for bit."""
    X = kmeans_model.blobs(300, 33, 5, seed=11)
    arguments = dict(metric="l2sq", dtype="i8", max_iterations=3, inertia_threshold=0.0, min_shifts=0.0, seed=21)
    want = kmeans_model.run(X, "f32", 5, **arguments)
    force(monkeypatch, 256, 300, 5, 33, "i8")
    assignments, distances, centroids, stats = usearch_amd.kmeans(X, 5, max_seconds=0.0, return_stats=True, **arguments)
    assert stats.iterations == want["iterations"]
    assert stats.last_iteration_points_shifted == want["last_iteration_points_shifted"]
    assert np.array_equal(assignments, want["assignments"])
    assert util.same_float_bits(distances, want["distances"])
    assert np.array_equal(bits(centroids), want["centroids"])


@pytest.mark.parametrize("count,k,ndim,dtype,metric", [FLOAT_CASES[2], FLOAT_CASES[3]])
def test_both_tiles_close_to_the_same_bits(monkeypatch, count, k, ndim, dtype, metric):
    X, centres, _ = float_case(count, k, ndim, dtype, metric)
    results = []
    for tile in (64, 256):
        force(monkeypatch, tile, count, k, ndim, dtype)
        results.append(usearch_amd.kmeans_assign(X, centres, metric=metric, dtype=dtype))
    assert np.array_equal(results[0][0], results[1][0])
    assert util.same_float_bits(results[0][1], results[1][1])
