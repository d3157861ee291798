"""A plain model of the k-means loop the product mirrors: the reference's `kmeans_clustering_gt`
(index_plugins.hpp:2244-2499) restated step by step, quirks included. Casts are `oraclebind.cast`, distances are
`oraclebind.distance` (the reference's serial loops), sums are sequential f64. tests/test_kmeans_model.py pins it to the real
reference through recorded fixtures; tests/test_gpu_kmeans.py holds the device to it.

Rows travel as uint8 matrices `[rows, bytes per row]` in the quantised kind.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from oracle import oraclebind

FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
ITEM_BYTES = {"f64": 8, "f32": 4, "f16": 2, "bf16": 2, "i8": 1}


class MT19937_64:
    """`std::mt19937_64` (the standard's constants; seeding by the linear recurrence with 6364136223846793005)."""
    MASK = (1 << 64) - 1

    def __init__(self, seed: int = 5489):
        self.state = [seed & self.MASK]
        for i in range(1, 312):
            previous = self.state[-1]
            self.state.append((6364136223846793005 * (previous ^ (previous >> 62)) + i) & self.MASK)
        self.at = 312

    def _twist(self) -> None:
        s = self.state
        for i in range(312):
            x = (s[i] & 0xFFFFFFFF80000000) | (s[(i + 1) % 312] & 0x7FFFFFFF)
            s[i] = s[(i + 156) % 312] ^ (x >> 1) ^ (0xB5026F5AA96619E9 if x & 1 else 0)
        self.at = 0

    def __call__(self) -> int:
        if self.at == 312:
            self._twist()
        x = self.state[self.at]
        self.at += 1
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000
        x ^= (x << 37) & 0xFFF7EEE000000000
        x ^= x >> 43
        return x & self.MASK


def quantize(X: np.ndarray, kind: str, dtype: str) -> np.ndarray:
    """Rows of the caller's `kind` → rows of `dtype` with the reference's casts (2317-2322; equal kinds are copied)."""
    X = np.ascontiguousarray(X)
    count, ndim = X.shape
    out = np.zeros((count, ITEM_BYTES[dtype] * ndim), dtype=np.uint8)
    for i in range(count):
        cast = oraclebind.cast(X[i], kind, dtype, ndim)
        out[i] = cast if cast is not None else X[i].view(np.uint8)
    return out


def draw_seeds(count: int, k: int, seed: int):
    """2308-2350 → (index per point before the first iteration, the point every centroid starts from). The "uniqueness" test
    compares index[j] — an assignment — for j < i with the drawn point index, as the reference does."""
    index = [k] * count
    engine = MT19937_64(seed)
    chosen = []
    for i in range(k):
        while True:
            random_index = engine() % count
            if all(index[j] != random_index for j in range(i)):
                break
        chosen.append(random_index)
        index[random_index] = i
    return index, chosen


def distance_matrix(Q: np.ndarray, centroids: np.ndarray, metric: str, dtype: str, ndim: int) -> np.ndarray:
    """metric(point, centroid) for every pair → float32 [points, centroids]."""
    measure = oraclebind.lib().uo_distance
    metric_kind, scalar_kind, dimensions = oraclebind.METRIC[metric], oraclebind.SCALAR[dtype], ctypes.c_uint64(ndim)
    Q, centroids = np.ascontiguousarray(Q), np.ascontiguousarray(centroids)
    out = np.zeros((len(Q), len(centroids)), dtype=np.float32)
    for i in range(len(Q)):
        a = Q.ctypes.data + i * Q.strides[0]
        for j in range(len(centroids)):
            out[i, j] = measure(metric_kind, scalar_kind, a, centroids.ctypes.data + j * centroids.strides[0], dimensions, 0)
    return out


def nearest(distances: np.ndarray):
    """2366-2375: an ascending scan with strict `<` from FLT_MAX → (index uint64, distance float32) per point."""
    index = np.zeros(len(distances), dtype=np.uint64)
    best = np.full(len(distances), FLT_MAX, dtype=np.float32)
    for i, row in enumerate(distances):
        closest, at = np.float32(FLT_MAX), 0
        for j, d in enumerate(row):
            if d < closest:
                closest, at = d, j
        index[i], best[i] = at, closest
    return index, best


def decompress(Q: np.ndarray, dtype: str, ndim: int) -> np.ndarray:
    """Quantised rows → f64 (`casts.to.f64`): exact for the float kinds, x / 127.f in f64 for i8."""
    if dtype == "i8":
        return Q.view(np.int8).astype(np.float64) / np.float64(np.float32(127))
    if dtype == "bf16":
        return (Q.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return Q.view({"f16": np.float16, "f32": np.float32}[dtype]).astype(np.float64)


def update(Q: np.ndarray, assignments, k: int, metric: str, dtype: str, ndim: int) -> np.ndarray:
    """2415-2477 on one thread: sequential f64 sums in ascending point order, the metric's normalisation, the cast back."""
    precise = decompress(Q, dtype, ndim)
    sums = np.zeros((k, ndim), dtype=np.float64)
    sizes = [0] * k
    for point, centroid in enumerate(assignments):
        sums[int(centroid)] += precise[point]
        sizes[int(centroid)] += 1
    out = np.zeros((k, Q.shape[1]), dtype=np.uint8)
    for c in range(k):
        row = sums[c]
        if metric == "l2sq":
            if sizes[c] > 0:
                row = row / np.float64(sizes[c])
        elif metric == "cos":
            norm = 0.0
            for x in row:
                norm += float(x) * float(x)
            norm = math.sqrt(norm)
            if norm > 0.0:
                row = row / np.float64(norm)
        with np.errstate(all="ignore"):
            cast = oraclebind.cast(np.ascontiguousarray(row), "f64", dtype, ndim)
        out[c] = cast
    return out


def export(centroids: np.ndarray, dtype: str, kind: str, ndim: int) -> np.ndarray:
    """2491-2496: centroids leave in the caller's kind → uint8 rows."""
    out = np.zeros((len(centroids), ITEM_BYTES[kind] * ndim), dtype=np.uint8)
    for i, row in enumerate(centroids):
        cast = oraclebind.cast(row, dtype, kind, ndim)
        out[i] = cast if cast is not None else row
    return out


def aggregate(distances: np.ndarray) -> float:
    total = 0.0
    for d in distances:
        total += float(d)
    return total


def run(X: np.ndarray, kind: str, k: int, metric: str = "l2sq", dtype: str = "bf16", max_iterations: int = 300,
        inertia_threshold: float = 1e-4, min_shifts: float = 0.01, seed: int = 0, Q: Optional[np.ndarray] = None) -> dict:
    """The whole loop (`max_seconds` never ends a model run). → dict(assignments, distances, centroids (uint8 rows in `kind`),
    quantized_centroids, assigned_against (the quantised centroids the last assignment was measured against), iterations, last_iteration_points_shifted, last_iteration_inertia, aggregate_distance, computed_distances,
    seeds)."""
    count, ndim = X.shape
    assert max_iterations >= 1 and 2 <= k < count
    Q = quantize(X, kind, dtype) if Q is None else Q
    index, chosen = draw_seeds(count, k, seed)
    index = np.array(index, dtype=np.uint64)
    centroids = assigned_against = Q[chosen].copy()
    distances = np.full(count, FLT_MAX, dtype=np.float32)
    iterations, shifted, inertia = 0, 0, 0.0
    minimum = int(min_shifts * count)
    last_aggregate = DBL_MAX  # never assigned again: 2355
    while iterations < max_iterations:
        iterations += 1
        assigned_against = centroids
        new_index, distances = nearest(distance_matrix(Q, centroids, metric, dtype, ndim))
        shifted = int((new_index != index).sum())
        index = new_index
        total = aggregate(distances)
        inertia = abs(total - last_aggregate) / last_aggregate
        if last_aggregate != 0.0 and inertia_threshold != 0.0 and inertia <= inertia_threshold:
            break
        if (minimum != 0 or shifted == 0) and shifted <= minimum:
            break
        centroids = update(Q, index, k, metric, dtype, ndim)
    return dict(assignments=index, distances=distances, centroids=export(centroids, dtype, kind, ndim), quantized_centroids=centroids,
                assigned_against=assigned_against, iterations=iterations, last_iteration_points_shifted=shifted, last_iteration_inertia=inertia,
                aggregate_distance=aggregate(distances), computed_distances=count * k * iterations, seeds=chosen)


def blobs(count: int, ndim: int, centres: int, seed: int, noise: float = 0.1, spread: float = 1.0, with_centres: bool = False,
          shares=None):
    """`centres` blobs a few units apart (centre coordinates uniform in ±spread), Gaussian noise around them → float32 points
    (and the centres with `with_centres`). `shares`: the probability of every blob, uniform when None."""
    rng = np.random.default_rng(seed)
    middle = rng.uniform(-spread, spread, (centres, ndim))
    member = rng.choice(centres, count, p=shares) if shares is not None else rng.integers(0, centres, count)
    points = (middle[member] + noise * rng.standard_normal((count, ndim))).astype(np.float32)
    return (points, middle.astype(np.float32)) if with_centres else points


def separation(distances: np.ndarray, tolerance: float) -> np.ndarray:
    """Per point: do the best and the second-best distance differ by more than twice the tolerance (scaled like
    `util.tolerance`: · max(1, |d|))? Both sides' rounding together cannot swap such a pair."""
    ordered = np.sort(np.asarray(distances, dtype=np.float64), axis=1)
    gap = ordered[:, 1] - ordered[:, 0]
    return gap > 2.0 * tolerance * np.maximum(1.0, np.maximum(np.abs(ordered[:, 0]), np.abs(ordered[:, 1])))
