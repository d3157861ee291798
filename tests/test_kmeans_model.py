"""The k-means model (tests/kmeans_model.py) against the REAL reference: tests/golden/kmeans/*.npz hold what
`kmeans_clustering_t` returned on one thread (recorded by make_kmeans_golden.{cpp,py} next to them) and the model has to
reproduce every one of them bit for bit — the dead inertia test and seeds that repeat included."""
from __future__ import annotations

import glob
import os

import numpy as np
import pytest

from tests import kmeans_model

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans", "*.npz")))


def test_mersenne_twister_known_value():
    """[rand.predef]: the 10 000th consecutive invocation of a default-constructed mt19937_64 produces 9981545732273789042."""
    engine = kmeans_model.MT19937_64()
    for _ in range(9999):
        engine()
    assert engine() == 9981545732273789042


def test_fixtures_cover_the_cases():
    cases = {(str(f["dtype"]), str(f["metric"])) for f in map(np.load, GOLDEN)}
    assert {("bf16", "l2sq"), ("f16", "l2sq"), ("i8", "l2sq"), ("f32", "l2sq"), ("bf16", "cos"), ("i8", "cos")} <= cases
    assert any(int(np.load(path)["k"]) == 2 for path in GOLDEN)
    repeated = [path for path in GOLDEN if "repeated_seed" in path]
    assert repeated
    for path in repeated:
        fixture = np.load(path)
        chosen = kmeans_model.draw_seeds(len(fixture["X"]), int(fixture["k"]), int(fixture["seed"]))[1]
        assert len(set(chosen)) < len(chosen), "this fixture's seed was picked because a draw repeats"


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(path)[:-4] for path in GOLDEN])
def test_model_reproduces_the_reference(path):
    fixture = np.load(path)
    X = fixture["X"]
    assert X.shape == (197, 40) and X.dtype == np.float32
    got = kmeans_model.run(X, "f32", int(fixture["k"]), metric=str(fixture["metric"]), dtype=str(fixture["dtype"]),
                           max_iterations=int(fixture["max_iterations"]), inertia_threshold=float(fixture["inertia_threshold"]),
                           min_shifts=float(fixture["min_shifts"]), seed=int(fixture["seed"]))
    assert got["iterations"] == int(fixture["iterations"])
    assert got["last_iteration_points_shifted"] == int(fixture["last_iteration_points_shifted"])
    assert got["computed_distances"] == int(fixture["computed_distances"])
    assert np.array_equal(got["assignments"], fixture["assignments"])
    assert np.array_equal(got["distances"].view(np.uint32), fixture["distance_bits"])
    assert np.array_equal(got["centroids"].view(np.uint32), fixture["centroid_bits"])
    assert np.float64(got["last_iteration_inertia"]).tobytes() == np.float64(fixture["last_iteration_inertia"]).tobytes()
    assert np.float64(got["aggregate_distance"]).tobytes() == np.float64(fixture["aggregate_distance"]).tobytes()


def test_inertia_is_the_dead_value():
    """`last_aggregate_distance` stays DBL_MAX (index_plugins.hpp:2355), so the reported inertia is |Σ − DBL_MAX| / DBL_MAX = 1."""
    for path in GOLDEN:
        assert float(np.load(path)["last_iteration_inertia"]) == 1.0
