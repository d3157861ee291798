"""One-off: records tests/golden/cluster/*.npz with the driver of make_cluster_golden.cpp (compile it as its header says).

    python tests/golden/cluster/make_cluster_golden.py <path of the compiled driver>

Every fixture holds the image of one small index the reference built on one thread (key = 1000 + row), the queries (rows in the
storage kind, or member keys), the configuration, and what the reference's own `cluster` returned: `cluster_keys`,
`cluster_distances`, `clusters`, `visited_members`, `computed_distances`. Not run by any test.

A case is recorded only where the reference and this project are comparable (usearch_amd/csrc/clustering.hpp, rule 5): the model of
tests/cluster_model.py, fed by the oracle, must meet NO equal popularities, and for the float case the runner-up of every merge
cycle must be further from the winner than the project's float tolerance (tests/util.py). Seeds are tried until both hold.
(The fixtures have a folder of their own: tests/fuzz/ takes every .npz directly under tests/golden/ for an index image.)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from tests import util  # noqa: E402
from tests.cluster_feeds import OracleFeed  # noqa: E402

LARGEST_FIXTURE = 83758  # tests/golden/cos_f16_96.npz


def reference(driver, scratch, metric, dtype, X, ndim, connectivity, queries, by_keys, min_count, max_count):
    X.tofile(os.path.join(scratch, "X.bin"))
    queries.tofile(os.path.join(scratch, "Q.bin"))
    image, results = os.path.join(scratch, "image.usearch"), os.path.join(scratch, "results.bin")
    subprocess.check_call([driver, metric, dtype, os.path.join(scratch, "X.bin"), str(len(X)), str(ndim), str(connectivity),
                           "keys" if by_keys else "vectors", os.path.join(scratch, "Q.bin"), str(len(queries)), str(min_count),
                           str(max_count), image, results])
    raw, q = np.fromfile(results, dtype=np.uint8), len(queries)
    keys = raw[:8 * q].view(np.uint64).copy()
    distances = raw[8 * q:12 * q].view(np.float32).copy()
    clusters, visited, computed = raw[12 * q:].view(np.uint64).tolist()
    return np.fromfile(image, dtype=np.uint8), keys, distances, clusters, visited, computed


def comparable(model: dict, dtype: str) -> bool:
    if model["popularity_ties"]:
        return False
    if dtype in ("i8", "b1"):
        return True
    for winner, runner_up in model["margins"]:
        if runner_up is not None and abs(runner_up - winner) <= 2.0 * util.tolerance(dtype) * max(1.0, abs(winner)):
            return False
    return True


def make_queries(kind: str, X, ndim, dtype, metric, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return util.make_vectors(400, ndim, dtype, seed=seed + 1, metric=metric)
    if kind == "colocated":  # two spots: fewer centroids than `min_count` on every level
        a, b = rng.choice(len(X), 2, replace=False)
        return np.ascontiguousarray(np.concatenate([np.repeat(X[a:a + 1], 50, axis=0), np.repeat(X[b:b + 1], 30, axis=0)]))
    if kind == "few":  # three spots of 5, 3 and 1 queries
        a, b, c = rng.choice(len(X), 3, replace=False)
        return np.ascontiguousarray(np.concatenate([np.repeat(X[a:a + 1], 5, axis=0), np.repeat(X[b:b + 1], 3, axis=0), X[c:c + 1]]))
    raise ValueError(kind)


CASES = {
    # name: metric, dtype, ndim, members, connectivity, queries, min_count, max_count, what the model must show
    "l2sq_i8_merges": ("l2sq", "i8", 16, 800, 4, "random", 6, 4, lambda m: m["merge_cycles"] >= 3),
    "hamming_b1_72_keys": ("hamming", "b1", 72, 800, 4, "keys", 6, 5, lambda m: m["merge_cycles"] >= 2),
    "cos_f32_merges": ("cos", "f32", 8, 600, 4, "random", 6, 4, lambda m: m["merge_cycles"] >= 3),
    "refine_colocated": ("l2sq", "i8", 16, 800, 4, "colocated", 3, 3, lambda m: m["mapping_passes"] >= 2 and m["level"] == 1),
    "min_count_zero": ("l2sq", "i8", 16, 800, 4, "few", 0, 0, lambda m: m["merge_cycles"] == 0 and m["unique_before_merge"] == 3),
}


def main(driver: str) -> None:
    with tempfile.TemporaryDirectory() as scratch:
        for name, (metric, dtype, ndim, n, connectivity, kind, min_count, max_count, shows) in CASES.items():
            for seed in range(100, 400):
                X = util.make_vectors(n, ndim, dtype, seed=seed, metric=metric)
                by_keys = kind == "keys"
                queries = 1000 + np.arange(n, dtype=np.uint64) if by_keys else make_queries(kind, X, ndim, dtype, metric, seed)
                image, keys, distances, clusters, visited, computed = reference(driver, scratch, metric, dtype, X, ndim, connectivity,
                                                                                queries, by_keys, min_count, max_count)
                feed = OracleFeed(image, X, metric, dtype, ndim)
                model = feed.run_members(queries, min_count, max_count) if by_keys else feed.run(queries, min_count, max_count)
                if comparable(model, dtype) and shows(model):
                    break
            else:
                raise SystemExit(f"{name}: no seed gives a comparable case")
            path = os.path.join(HERE, name + ".npz")
            np.savez_compressed(path, image=image, vectors=X, queries=queries, by_keys=np.uint8(by_keys), metric=np.array(metric),
                                dtype=np.array(dtype), ndim=np.uint64(ndim), min_count=np.uint64(min_count),
                                max_count=np.uint64(max_count), cluster_keys=keys, cluster_distances=distances,
                                clusters=np.uint64(clusters), visited_members=np.uint64(visited), computed_distances=np.uint64(computed))
            assert os.path.getsize(path) <= LARGEST_FIXTURE, (name, os.path.getsize(path))
            print(name, "seed", seed, "level", model["level"], "U", model["unique_before_merge"], "cycles", model["merge_cycles"],
                  "clusters", clusters, os.path.getsize(path), "bytes; model == reference keys:", np.array_equal(model["keys"], keys))


if __name__ == "__main__":
    main(sys.argv[1])
