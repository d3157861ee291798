"""`usearch_amd.kmeans` / `kmeans_assign` on the device against the model of tests/kmeans_model.py (which
tests/test_kmeans_model.py pins to the real reference).

Shapes are the smallest that cross every boundary of the kernels (csrc/kmeans.hip: 64 points per tile, 128 centroids per inner
tile, 128-byte chunks, rows padded to 16 bytes): N = 197 is three point tiles and a ragged one; k ∈ {2, 5, 129, 300} is less than
a quarter of a centroid tile, one tile plus one centroid, and two tiles plus a ragged one; ndim ∈ {40, 96, 200} gives 16-bit rows
below one chunk (80 bytes), of 192 bytes, and of 400 bytes with a tail; i8 rows of 33 bytes (padded to 48) and of 96.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import usearch_amd
from tests import kmeans_model, util

pytestmark = pytest.mark.gpu

COUNT = 197
NUMPY = {"f32": np.float32, "f16": np.float16, "i8": np.int8}


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def blob_case(ndim: int, k: int, seed: int = 5):
    """197 points around k centres a few units apart, noise 0.1 → (points f32, the centres f32)."""
    return kmeans_model.blobs(COUNT, ndim, k, seed=seed + 1000 * ndim + k, with_centres=True)


@functools.lru_cache(maxsize=None)
def model_assignment(ndim: int, k: int, metric: str, dtype: str):
    """The model's distance matrix for the blob case, computed once per (shape, metric, kind)."""
    X, centres = blob_case(ndim, k)
    Q, C = kmeans_model.quantize(X, "f32", dtype), kmeans_model.quantize(centres, "f32", dtype)
    distances = kmeans_model.distance_matrix(Q, C, metric, dtype, ndim)
    distances.setflags(write=False)
    return distances


# ---------------------------------------------------------------------------------------------------------------- 1. exact kinds

@pytest.mark.parametrize("ndim", [33, 96])
@pytest.mark.parametrize("metric", ["l2sq", "ip", "cos"])
def test_assign_i8_is_exact_and_ties_go_to_the_lower_index(metric, ndim):
    rng = np.random.default_rng(ndim)
    X = rng.integers(-60, 61, (COUNT, ndim)).astype(np.int8)
    centroids = rng.integers(-60, 61, (300, ndim)).astype(np.int8)
    planted = [(3, 7), (0, 128), (127, 129)]
    for (low, high), point in zip(planted, (10, 90, 170)):  # a point's own row, twice: that point is nearest to the pair
        centroids[low] = centroids[high] = X[point]
    got_index, got_distance = usearch_amd.kmeans_assign(X, centroids, metric=metric, dtype="i8")
    want_index, want_distance = kmeans_model.nearest(kmeans_model.distance_matrix(bits(X), bits(centroids), metric, "i8", ndim))
    assert np.array_equal(got_index, want_index)
    assert util.same_float_bits(got_distance, want_distance)
    assert not np.isin(got_index, [high for _, high in planted]).any()
    if metric != "ip":  # (under ip the nearest centroid is the longest aligned one, not the point's own row)
        for (low, _), point in zip(planted, (10, 90, 170)):
            assert got_index[point] == low


@functools.lru_cache(maxsize=None)
def shared_tile_case(ndim: int, dtype: str):
    """197 points and 300 centroids in `dtype`: the integers −60 … 60 of the test above for i8; for the 16-bit kinds the same
    integers plus a fraction, so that products and partial sums round and the order of the summation shows in the bits."""
    rng = np.random.default_rng(ndim)
    X, centroids = rng.integers(-60, 61, (COUNT, ndim)), rng.integers(-60, 61, (300, ndim))
    if dtype == "i8":
        return X.astype(np.int8), centroids.astype(np.int8)
    X, centroids = (X + rng.random(X.shape)) / 8.0, (centroids + rng.random(centroids.shape)) / 8.0
    narrow = util.to_bf16 if dtype == "bf16" else (lambda a: a.astype(np.float16))
    return narrow(X), narrow(centroids)


@pytest.mark.parametrize("ndim", [33, 96])
@pytest.mark.parametrize("metric", ["l2sq", "ip", "cos"])
@pytest.mark.parametrize("dtype", ["i8", "f16", "bf16"])
def test_assignment_and_exact_search_close_the_same_distance(dtype, metric, ndim):
    """The assignment kernel and the 64-query tile of exact search multiply, take Σx² and close through the same code
    (csrc/device_math.hpp): a point's distance to its nearest centroid has the same float bits either way — i8 also on the
    wave-per-query kernel, whose bits the integer sums carry. Distances only: among equal ones k-means keeps the lower index, exact
    search the later slot. (f16 / bf16: same products in the same order; the bits were equal before the code was shared, too.)"""
    X, centroids = shared_tile_case(ndim, dtype)
    _, assigned = usearch_amd.kmeans_assign(X, centroids, metric=metric, dtype=dtype)
    assert np.isfinite(assigned).all()
    routes = [True, False] if dtype == "i8" else [True]
    for tiled in routes:
        _, nearest = usearch_amd.exact_search(centroids, X, 1, metric=metric, dtype=dtype, tiled=tiled)
        differing = assigned.view(np.uint32) != nearest[:, 0].view(np.uint32)
        print(f"{dtype} {metric} {ndim} tiled={tiled}: {int(differing.sum())} of {COUNT} distances differ in their bits, "
              f"max |difference| {np.abs(assigned.astype(np.float64) - nearest[:, 0]).max():.3g}")
        assert not differing.any()


def test_assign_all_nan_distances_end_at_index_zero():
    """A NaN never wins; a point whose distances are all NaN keeps index 0 and FLT_MAX (index_plugins.hpp:2366-2375)."""
    X = blob_case(40, 5)[0].copy()
    centroids = blob_case(40, 5)[1].copy()
    X[7, 3] = np.nan
    centroids[0, 0] = np.nan  # index 0 is NaN for everybody: nobody may take it except the all-NaN point
    index, distance = usearch_amd.kmeans_assign(X, centroids, metric="l2sq", dtype="f16")
    assert index[7] == 0 and distance[7] == np.finfo(np.float32).max
    others = np.arange(COUNT) != 7
    assert (index[others] != 0).all() and np.isfinite(distance[others]).all()


# ---------------------------------------------------------------------------------------------------------------- 2. float kinds

FLOAT_SHAPES = [(40, 2), (96, 5), (200, 129), (40, 300), (200, 300)]


@pytest.mark.parametrize("ndim,k", FLOAT_SHAPES)
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_assign_float_kinds(dtype, metric, ndim, k):
    X, centres = blob_case(ndim, k)
    want = model_assignment(ndim, k, metric, dtype)
    tolerance = util.tolerance(dtype)
    separated = kmeans_model.separation(want, tolerance)
    assert (~separated).mean() <= 0.01, "the case must not pass by leaving points out"
    index, distance = usearch_amd.kmeans_assign(X, centres, metric=metric, dtype=dtype)
    want_index, want_distance = kmeans_model.nearest(want)
    error = np.abs(distance.astype(np.float64) - want_distance)
    print(f"{dtype} {metric} {ndim}x{k}: max error {error.max():.3g}, unseparated {int((~separated).sum())}")
    assert np.all(error <= tolerance * np.maximum(1.0, np.abs(want_distance)))
    assert np.array_equal(index[separated], want_index[separated])


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_assign_ip(dtype):
    """ip over a few centroids of different lengths (the gaps between 1 − Σab are wide there)."""
    X, centres = blob_case(96, 5)
    want = model_assignment(96, 5, "ip", dtype)
    separated = kmeans_model.separation(want, util.tolerance(dtype))
    assert (~separated).mean() <= 0.01
    index, distance = usearch_amd.kmeans_assign(X, centres, metric="ip", dtype=dtype)
    want_index, want_distance = kmeans_model.nearest(want)
    assert np.all(np.abs(distance - want_distance) <= util.tolerance(dtype) * np.maximum(1.0, np.abs(want_distance)))
    assert np.array_equal(index[separated], want_index[separated])


# ---------------------------------------------------------------------------------------------------------------- 3. one update

def one_step(X, k, metric, dtype, seed):
    return usearch_amd.kmeans(X, k, metric=metric, dtype=dtype, max_iterations=1, inertia_threshold=0.0, max_seconds=0.0,
                              min_shifts=0.0, seed=seed, return_stats=True)


def assert_update_of(X, k, metric, dtype, assignments, centroids):
    """`centroids` (the caller's f32) must be the model's update of the DEVICE's assignments, bit for bit."""
    ndim = X.shape[1]
    Q = kmeans_model.quantize(X, "f32", dtype)
    want = kmeans_model.export(kmeans_model.update(Q, assignments, k, metric, dtype, ndim), dtype, "f32", ndim)
    assert np.array_equal(bits(centroids), want)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("dtype,ndim", [("bf16", 40), ("bf16", 200), ("f16", 96), ("f16", 200), ("i8", 33), ("i8", 96), ("f32", 40)])
def test_one_assign_one_update(dtype, ndim, metric):
    X = blob_case(ndim, 5)[0]
    assignments, _, centroids, stats = one_step(X, 5, metric, dtype, seed=3)
    assert stats.iterations == 1 and stats.computed_distances == COUNT * 5
    assert_update_of(X, 5, metric, dtype, assignments, centroids)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "i8", "f32"])
def test_update_leaves_an_empty_cluster_all_zero(dtype, metric):
    """k = 129 (a centroid tile and one more) with seeds that repeat: of two equal centroids the lower index takes every point, the
    other one stays empty and becomes the all-zero row."""
    k, X = 129, blob_case(40, 5)[0]
    seed = 1
    while len(set(kmeans_model.draw_seeds(COUNT, k, seed)[1])) == k:
        seed += 1
    assignments, _, centroids, _ = one_step(X, k, metric, dtype, seed)
    sizes = np.bincount(assignments.astype(np.int64), minlength=k)
    assert (sizes == 0).any()
    assert not centroids[sizes == 0].any()
    assert_update_of(X, k, metric, dtype, assignments, centroids)


@pytest.mark.parametrize("dtype", ["bf16", "i8"])
def test_update_of_a_cluster_with_most_points(dtype):
    X = kmeans_model.blobs(COUNT, 96, 2, seed=77, shares=[0.8, 0.2])
    assignments, _, centroids, _ = one_step(X, 2, "l2sq", dtype, seed=5)
    assert np.bincount(assignments.astype(np.int64), minlength=2).max() > COUNT // 2
    assert_update_of(X, 2, "l2sq", dtype, assignments, centroids)


# ---------------------------------------------------------------------------------------------------------------- 4. trajectories

@pytest.mark.parametrize("max_iterations", [1, 2, 50])
@pytest.mark.parametrize("metric,ndim", [("l2sq", 33), ("cos", 96)])
def test_i8_trajectory_equals_the_model(metric, ndim, max_iterations):
    X = blob_case(ndim, 5)[0]
    want = kmeans_model.run(X, "f32", 5, metric=metric, dtype="i8", max_iterations=max_iterations, inertia_threshold=0.0,
                            min_shifts=0.0, seed=21)
    assignments, distances, centroids, stats = usearch_amd.kmeans(X, 5, metric=metric, dtype="i8", max_iterations=max_iterations,
                                                                  inertia_threshold=0.0, max_seconds=0.0, min_shifts=0.0, seed=21,
                                                                  return_stats=True)
    assert stats.iterations == want["iterations"]
    assert stats.last_iteration_points_shifted == want["last_iteration_points_shifted"]
    assert np.array_equal(assignments, want["assignments"])
    assert util.same_float_bits(distances, want["distances"])
    assert np.array_equal(bits(centroids), want["centroids"])
    assert stats.last_iteration_inertia == want["last_iteration_inertia"] == 1.0  # the reference's dead inertia test
    assert stats.computed_distances == want["computed_distances"]
    assert abs(stats.aggregate_distance - want["aggregate_distance"]) <= 1e-12 * abs(want["aggregate_distance"])


@pytest.mark.parametrize("dtype,ndim", [("bf16", 40), ("f16", 200)])
def test_float_trajectory_on_blobs(dtype, ndim):
    X = blob_case(ndim, 5)[0]
    arguments = dict(metric="l2sq", dtype=dtype, max_iterations=50, inertia_threshold=0.0, min_shifts=0.0, seed=9)
    want = kmeans_model.run(X, "f32", 5, **arguments)
    assignments, distances, centroids, stats = usearch_amd.kmeans(X, 5, max_seconds=0.0, return_stats=True, **arguments)
    Q = kmeans_model.quantize(X, "f32", dtype)
    separated = kmeans_model.separation(kmeans_model.distance_matrix(Q, want["assigned_against"], "l2sq", dtype, ndim),
                                        util.tolerance(dtype))
    assert (~separated).mean() <= 0.01
    assert np.array_equal(assignments[separated], want["assignments"][separated])
    assert stats.last_iteration_inertia == 1.0
    assert stats.iterations > 1
    # the centroids that come back are the update of the assignment that comes back — whether the run ended after an update or
    # because nothing shifted (then the last two assignments are one)
    assert_update_of(X, 5, "l2sq", dtype, assignments, centroids)
    again = usearch_amd.kmeans(X, 5, max_seconds=0.0, return_stats=True, **arguments)
    assert again[0].tobytes() == assignments.tobytes() and again[1].tobytes() == distances.tobytes()
    assert again[2].tobytes() == centroids.tobytes()
    assert again[3].aggregate_distance == stats.aggregate_distance and again[3].iterations == stats.iterations


def test_seeds_are_the_reference_draws():
    """A run that the clock ends in its first iteration returns the seed rows untouched: `std::mt19937_64(seed)() % N`, draws
    that repeat included."""
    X = blob_case(40, 5)[0]
    Q = kmeans_model.quantize(X, "f32", "bf16")
    drawn = {}
    for seed in (1, 2, 0xFFFFFFFFFFFFFFFF):
        _, _, centroids, stats = usearch_amd.kmeans(X, 24, dtype="bf16", max_seconds=1e-9, seed=seed, return_stats=True)
        assert stats.iterations == 1
        chosen = kmeans_model.draw_seeds(COUNT, 24, seed)[1]
        assert np.array_equal(bits(centroids), kmeans_model.export(Q[chosen], "bf16", "f32", 40))
        drawn[seed] = tuple(chosen)
    assert len(set(drawn.values())) == 3


# ---------------------------------------------------------------------------------------------------------------- 5. refusals

def test_refusals_by_name():
    X = blob_case(40, 5)[0]
    with pytest.raises(ValueError, match="The number of clusters must be at least 2"):
        usearch_amd.kmeans(X, 1)
    with pytest.raises(ValueError, match="The number of clusters must be less than the number of vectors"):
        usearch_amd.kmeans(X, COUNT)
    with pytest.raises(ValueError, match="The number of iterations must be at least 1"):
        usearch_amd.kmeans(X, 5, max_iterations=0)
    with pytest.raises(ValueError, match="f64"):
        usearch_amd.kmeans(X, 5, dtype="f64")
    with pytest.raises(ValueError, match="b1"):
        usearch_amd.kmeans(X, 5, dtype="b1")
    with pytest.raises(ValueError, match="rows must be contiguous"):
        usearch_amd.kmeans(X[:, ::2], 5)
    with pytest.raises(ValueError, match="rank-2"):
        usearch_amd.kmeans(X[0], 5)
    with pytest.raises(ValueError, match="f64"):
        usearch_amd.kmeans_assign(X, X[:5], dtype="f64")


def test_max_seconds_ends_a_run():
    X = blob_case(40, 5)[0]
    _, _, _, stats = usearch_amd.kmeans(X, 5, inertia_threshold=0.0, min_shifts=0.0, max_seconds=1e-9, seed=4, return_stats=True)
    assert stats.iterations == 1 and stats.runtime_seconds >= 1e-9


def test_rows_with_a_stride():
    """Rows that are contiguous but further apart than their length are taken as they lie."""
    wide = np.zeros((COUNT, 64), dtype=np.float32)
    wide[:, :40] = blob_case(40, 5)[0]
    a = usearch_amd.kmeans(wide[:, :40], 5, max_iterations=3, seed=8)
    b = usearch_amd.kmeans(np.ascontiguousarray(wide[:, :40]), 5, max_iterations=3, seed=8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- 6. device casts

def edge_rows(ndim: int) -> np.ndarray:
    rng = np.random.default_rng(ndim)
    X = (rng.standard_normal((COUNT, ndim)) * np.exp(rng.uniform(-12, 12, (COUNT, 1)))).astype(np.float32)
    X[0] = 0.0
    X[1, :4] = [-0.0, 1e-41, 65504.0, 65520.0]         # a denormal, the largest f16 and the first value that rounds past it
    X[2, :4] = [1e30, -1e30, 6.1e-5, 5.96e-8]            # beyond f16, the f16 denormal range
    X[3, :3] = [1.00390625, 1.01171875, -1.00390625]     # ties and near-ties of the bf16 / f16 mantissas
    return X


@pytest.mark.parametrize("ndim", [33, 200])
@pytest.mark.parametrize("source,target", [("f32", "bf16"), ("f32", "f16"), ("f32", "i8"), ("f16", "bf16")])
def test_device_casts_equal_the_host_cast(source, target, ndim):
    X = edge_rows(ndim)
    if source == "f16":
        with np.errstate(over="ignore"):
            X = X.astype(np.float16)
    got = usearch_amd.index.test_kmeans_quantize(X, source, target)
    with np.errstate(all="ignore"):
        want = np.stack([usearch_amd.cast(row, source, target, ndim) for row in X])
    assert np.array_equal(got, want)
