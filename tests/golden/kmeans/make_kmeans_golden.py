"""One-off: records tests/golden/kmeans/*.npz with the driver of make_kmeans_golden.cpp (compile it as its header says).

    python tests/golden/kmeans/make_kmeans_golden.py <path of the compiled driver>

Every fixture holds the input (X float32 [197, 40], five blobs), k, seed, metric, dtype and the three thresholds, and what the
reference returned for them: assignments, the bits of the distances and of the centroids, and the stats. Not run by any test.
(The fixtures have a folder of their own: tests/fuzz/ takes every .npz directly under tests/golden/ for an index image.)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from tests import kmeans_model  # noqa: E402

COUNT, NDIM = 197, 40


def repeating_seed(k: int) -> int:
    """The first seed whose draws name one point twice (the reference's uniqueness test lets it through)."""
    seed = 1
    while len(set(kmeans_model.draw_seeds(COUNT, k, seed)[1])) == k:
        seed += 1
    return seed


# name → (k, metric, dtype, max_iterations, inertia_threshold, max_seconds, min_shifts, seed)
CASES = {
    "bf16_l2sq": (5, "l2sq", "bf16", 300, 1e-4, 60.0, 0.01, 11),
    "f16_l2sq": (5, "l2sq", "f16", 300, 1e-4, 60.0, 0.01, 12),
    "i8_l2sq": (5, "l2sq", "i8", 300, 1e-4, 60.0, 0.01, 13),
    "f32_l2sq": (5, "l2sq", "f32", 300, 1e-4, 60.0, 0.01, 14),
    "bf16_cos": (5, "cos", "bf16", 300, 1e-4, 60.0, 0.01, 15),
    "i8_cos": (5, "cos", "i8", 4, 0.0, 0.0, 0.0, 16),            # ends at max_iterations or with nothing shifted
    "bf16_l2sq_repeated_seed": (24, "l2sq", "bf16", 3, 0.0, 0.0, 0.0, repeating_seed(24)),  # ends with an update
    "bf16_l2sq_k2": (2, "l2sq", "bf16", 300, 1e-4, 60.0, 0.0, 18),
}


def main(driver: str) -> None:
    X = kmeans_model.blobs(COUNT, NDIM, 5, seed=2024)
    with tempfile.TemporaryDirectory() as scratch:
        X.tofile(os.path.join(scratch, "X.bin"))
        for name, (k, metric, dtype, max_iterations, inertia_threshold, max_seconds, min_shifts, seed) in CASES.items():
            out = os.path.join(scratch, "out.bin")
            subprocess.check_call([driver, os.path.join(scratch, "X.bin"), str(COUNT), str(NDIM), str(k), metric, dtype,
                                   str(max_iterations), repr(inertia_threshold), repr(max_seconds), repr(min_shifts), str(seed), out])
            raw = open(out, "rb").read()
            at = 0

            def take(dtype_, n):
                nonlocal at
                part = np.frombuffer(raw, dtype=dtype_, count=n, offset=at).copy()
                at += part.nbytes
                return part
            assignments, distance_bits = take(np.uint64, COUNT), take(np.uint32, COUNT)
            centroid_bits = take(np.uint32, k * NDIM).reshape(k, NDIM)
            iterations, shifted, computed = (int(v) for v in take(np.uint64, 3))
            inertia, total = (float(v) for v in take(np.float64, 2))
            assert at == len(raw)
            np.savez_compressed(os.path.join(HERE, f"{name}.npz"), X=X, k=k, seed=np.uint64(seed), metric=metric, dtype=dtype,
                                max_iterations=max_iterations, inertia_threshold=inertia_threshold, max_seconds=max_seconds,
                                min_shifts=min_shifts, assignments=assignments, distance_bits=distance_bits,
                                centroid_bits=centroid_bits, iterations=iterations, last_iteration_points_shifted=shifted,
                                computed_distances=computed, last_iteration_inertia=inertia, aggregate_distance=total)


if __name__ == "__main__":
    main(sys.argv[1])
