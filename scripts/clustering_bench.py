"""Clustering by the index's own levels at scale: N × dims i8 rows (l2sq) built on the device, every member clustered.
Prints one JSON line: the seconds of the three phases (map: descents, popularity count and ranking; merge; trace and closing
distances), the level, the distinct centroids before the merges, the cycles, and the wall seconds of the call.

    python scripts/clustering_bench.py --n 1000000 --dim 96 --min-count 1000 --max-count 1024

The yardstick is the reference's own `cluster` over the same kind of index on the host's cores: the driver of
tests/golden/cluster/make_cluster_golden.cpp with a `repeats` argument (profiles/r10_clustering/README.md).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n: int, dim: int, seed: int) -> np.ndarray:
    """Low-rank latent + noise, i8 rows; generated in slabs."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((16, dim)).astype(np.float32)
    out = np.empty((n, dim), dtype=np.int8)
    for first in range(0, n, 65536):
        last = min(n, first + 65536)
        x = rng.standard_normal((last - first, 16), dtype=np.float32) @ basis + 0.3 * rng.standard_normal((last - first, dim), dtype=np.float32)
        out[first:last] = np.clip(np.rint(x * (100.0 / 16.0)), -127, 127).astype(np.int8)
    return out


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=96)
    parser.add_argument("--min-count", type=int, default=1000)
    parser.add_argument("--max-count", type=int, default=1024)
    parser.add_argument("--connectivity", type=int, default=16)
    parser.add_argument("--repeat", type=int, default=3)
    parser.add_argument("--seed", type=int, default=5)
    args = parser.parse_args()

    import usearch_amd
    rows = synthetic(args.n, args.dim, args.seed)
    begin = time.perf_counter()
    built = usearch_amd.build(rows, metric="l2sq", dtype="i8", connectivity=args.connectivity)
    build_seconds = time.perf_counter() - begin
    best = None
    for _ in range(args.repeat):
        begin = time.perf_counter()
        got = built.clustering(min_count=args.min_count, max_count=args.max_count)
        wall = time.perf_counter() - begin
        if best is None or wall < best[0]:
            best = (wall, got.stats)
    wall, stats = best
    print(json.dumps({"bench": "clustering", "n": args.n, "dim": args.dim, "dtype": "i8", "metric": "l2sq", "min_count": args.min_count,
                      "max_count": args.max_count, "build_seconds": round(build_seconds, 3), "seconds": round(wall, 4),
                      "seconds_map": round(stats["seconds_map"], 4), "seconds_merge": round(stats["seconds_merge"], 4),
                      "seconds_trace": round(stats["seconds_trace"], 4), "level": stats["level"],
                      "unique_before_merge": stats["unique_before_merge"], "merge_cycles": stats["merge_cycles"],
                      "clusters": stats["clusters"], "mapping_passes": stats["mapping_passes"]}))


if __name__ == "__main__":
    main()
