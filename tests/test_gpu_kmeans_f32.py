"""The k-means assignment of f32 rows on the screened matrix-unit tile (`assign_screened_kernel`, csrc/kmeans.hip): the tile's sums
only choose the few centroids that can win, the wave kernel's arithmetic measures them — so USEARCH_AMD_KMEANS_TILE=64 (the tile)
and =1 (the wave kernel alone) must agree to the bit, and the hook `test_kmeans_screen` shows what the screen left to re-measure."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import usearch_amd
from tests import kmeans_model, util

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
TOLERANCE = util.tolerance("f32")


def f64_distances(X: np.ndarray, C: np.ndarray, metric: str) -> np.ndarray:
    x, c = X.astype(np.float64), C.astype(np.float64)
    ab, a, b = x @ c.T, np.sqrt((x * x).sum(1))[:, None], np.sqrt((c * c).sum(1))[None, :]
    return {"l2sq": a * a + b * b - 2.0 * ab, "ip": 1.0 - ab, "cos": 1.0 - ab / (a * b)}[metric]


@functools.lru_cache(maxsize=None)
def case(count: int, k: int, ndim: int, metric: str):
    X, centres = kmeans_model.blobs(count, ndim, k, seed=3 + 1000 * ndim + k, with_centres=True)
    want = f64_distances(X, centres, metric)
    for array in (X, centres, want):
        array.setflags(write=False)
    return X, centres, want


def both_routes(monkeypatch, X, C, metric):
    results = []
    for tile in ("64", "1"):
        monkeypatch.setenv("USEARCH_AMD_KMEANS_TILE", tile)
        results.append(usearch_amd.kmeans_assign(X, C, metric=metric, dtype="f32"))
    return results


def assert_same(screened, wave):
    assert np.array_equal(screened[0], wave[0])
    assert util.same_float_bits(screened[1], wave[1])


@pytest.mark.parametrize("count,k", [(64, 128), (65, 129), (197, 300)])
@pytest.mark.parametrize("ndim", [33, 96, 200])
@pytest.mark.parametrize("metric", ["l2sq", "cos", "ip"])
def test_same_bits_as_the_wave_kernel(monkeypatch, metric, ndim, count, k):
    X, centres, want = case(count, k, ndim, metric)
    separated = kmeans_model.separation(want, TOLERANCE)
    assert separated.mean() >= 0.8, "the case must not pass by leaving points out"  # on the CPU, before any GPU call
    screened, wave = both_routes(monkeypatch, X, centres, metric)
    assert_same(screened, wave)
    nearest = want.min(1)
    assert np.array_equal(screened[0][separated], want.argmin(1)[separated])
    assert np.all(np.abs(screened[1] - nearest)[separated] <= (TOLERANCE * np.maximum(1.0, np.abs(nearest)))[separated])


@pytest.mark.parametrize("metric", ["l2sq", "cos", "ip"])
def test_blobs_leave_one_contender(metric):
    """DESIGN.md §9's e per (point, centroid), in f64: a point whose f64 gaps to every other centroid exceed 2·(e + e of the
    nearest) cannot keep a second contender. The data decides the share, the device has to show it."""
    from usearch_amd.index import test_kmeans_screen
    count, k, ndim = 197, 300, 96
    X, centres, want = case(count, k, ndim, metric)
    g = 2.0 * (ndim + 16) * 2.0**-24
    a = np.sqrt((X.astype(np.float64)**2).sum(1))[:, None]
    b = np.sqrt((centres.astype(np.float64)**2).sum(1))[None, :]
    e = {"l2sq": g * (a + b)**2, "ip": g * a * b + 2.0**-23, "cos": g * a + 0.0 * b}[metric]
    score = want * a if metric == "cos" else want
    rows, best = np.arange(count), want.argmin(1)
    gap = score - score[rows, best][:, None] - 2.0 * (e + e[rows, best][:, None])
    gap[rows, best] = np.inf
    assert ((gap > 0).all(1)).mean() > 0.9  # on the CPU, before any GPU call
    index, distance, contenders = test_kmeans_screen(X, centres, metric)
    print(f"\n[screen] {metric}: one contender at {np.mean(contenders == 1):.3f} of the points, handed over {int((contenders == 0).sum())}")
    assert np.mean(contenders == 1) > 0.9
    assert np.array_equal(index, best)


def test_a_copy_one_ulp_away_in_the_next_tile(monkeypatch):
    from usearch_amd.index import test_kmeans_screen
    X, centres, _ = case(197, 128, 96, "l2sq")
    copies = centres.copy()
    copies[:, 0] = np.nextafter(copies[:, 0], np.float32(np.inf))
    C = np.concatenate([centres, copies])  # centroid j + 128 lies in the second centroid tile
    index, distance, contenders = test_kmeans_screen(X, C, "l2sq")
    assert (contenders >= 2).all()
    assert_same((index, distance), both_routes(monkeypatch, X, C, "l2sq")[1])


def test_six_equal_centroids_go_to_the_wave_kernel():
    from usearch_amd.index import test_kmeans_screen
    X, centres, want = case(197, 300, 96, "l2sq")
    C, nearest = centres.copy(), int(want[0].argmin())
    six = (nearest + 37 * np.arange(6)) % 300  # over all three centroid tiles
    C[six] = centres[nearest]
    theirs = want.argmin(1) == nearest
    index, distance, contenders = test_kmeans_screen(X, C, "l2sq")
    assert (contenders[theirs] == 0).all() and (index[theirs] == six.min()).all()


def test_nan_goes_to_the_wave_kernel(monkeypatch):
    from usearch_amd.index import test_kmeans_screen
    X, centres, _ = case(197, 300, 96, "l2sq")
    X = X.copy()
    X[7, 3] = np.nan
    index, distance, contenders = test_kmeans_screen(X, centres, "l2sq")
    assert contenders[7] == 0 and (contenders[np.arange(197) != 7] > 0).all()
    assert_same((index, distance), both_routes(monkeypatch, X, centres, "l2sq")[1])
    index, distance, contenders = test_kmeans_screen(X, np.full_like(centres, np.nan), "l2sq")
    assert (contenders == 0).all() and (index == 0).all() and (distance == FLT_MAX).all()


def test_zero_rows_under_cos(monkeypatch):
    X, centres, _ = case(197, 300, 96, "cos")
    X, C = X.copy(), centres.copy()
    X[5] = 0.0
    C[2] = 0.0
    assert_same(*both_routes(monkeypatch, X, C, "cos"))


def test_a_whole_run(monkeypatch):
    X = kmeans_model.blobs(300, 33, 5, seed=11)
    runs = []
    for tile in ("64", "1"):
        monkeypatch.setenv("USEARCH_AMD_KMEANS_TILE", tile)
        runs.append(usearch_amd.kmeans(X, 5, dtype="f32", max_iterations=5, seed=9))
    assert_same(runs[0][:2], runs[1][:2])
    assert util.same_float_bits(runs[0][2], runs[1][2])
