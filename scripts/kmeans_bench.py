"""k-means at scale: N × dims f16 rows quantised to bf16, k clusters, a fixed number of iterations (every early exit off).
Prints one JSON line: milliseconds per assignment and per update (HIP events around the kernels), TFLOP/s of the assignment
against the 2.5 PFLOP/s dense peak, GB/s of the update (every quantised row read once) against 8 TB/s, the wall time of the call —
and, with `--reference-driver`, the seconds the reference's `kmeans_clustering_t` takes on the host's cores for the same kind of
input (scripts/kmeans_reference_driver.cpp, compiled outside the repository; `--reference-n` / `--reference-iterations` run it on
fewer points / iterations, its work being proportional to both, and the line says so).

    python scripts/kmeans_bench.py --n 1000000 --dim 768 --k 1024 --iterations 10
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_DENSE_FLOPS = 2.5e15  # MI355X, f16 / bf16 on the matrix units
PEAK_HBM_BYTES = 8.0e12


def synthetic(n: int, dim: int, centres: int, seed: int) -> np.ndarray:
    """`centres` Gaussian blobs, f16 rows; generated in slabs (the f32 intermediate of 1M × 768 would be 3 GB)."""
    rng = np.random.default_rng(seed)
    middle = rng.standard_normal((centres, dim)).astype(np.float32)
    out = np.empty((n, dim), dtype=np.float16)
    for first in range(0, n, 65536):
        last = min(n, first + 65536)
        out[first:last] = middle[rng.integers(0, centres, last - first)] + 0.3 * rng.standard_normal((last - first, dim), dtype=np.float32)
    return out


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--k", type=int, default=1024)
    parser.add_argument("--iterations", type=int, default=10)
    parser.add_argument("--dtype", default="bf16", help="the kind the loop runs in")
    parser.add_argument("--metric", default="l2sq")
    parser.add_argument("--repeat", type=int, default=2, help="runs timed; the last one is reported (the first pays the module load)")
    parser.add_argument("--reference-driver", default="", help="the compiled scripts/kmeans_reference_driver.cpp")
    parser.add_argument("--reference-n", type=int, default=0, help="points the reference clusters (0 = --n)")
    parser.add_argument("--reference-iterations", type=int, default=0, help="iterations the reference runs (0 = --iterations)")
    parser.add_argument("--reference-threads", type=int, default=16)
    args = parser.parse_args()

    import usearch_amd

    X = synthetic(args.n, args.dim, args.k, 42)
    for _ in range(args.repeat):
        begin = time.perf_counter()
        assignments, distances, centroids, stats = usearch_amd.kmeans(
            X, args.k, metric=args.metric, dtype=args.dtype, max_iterations=args.iterations, inertia_threshold=0.0, max_seconds=0.0,
            min_shifts=0.0, seed=42, return_stats=True)
        seconds = time.perf_counter() - begin
    iterations = int(stats.iterations)
    assign_ms, update_ms = stats.assign_ms / iterations, stats.update_ms / iterations
    row_bytes = {"bf16": 2, "f16": 2, "i8": 1, "f32": 4}[args.dtype] * args.dim
    line = {
        "what": "kmeans", "n": args.n, "dims": args.dim, "k": args.k, "source": "f16", "dtype": args.dtype, "metric": args.metric,
        "iterations": iterations, "seconds_total": round(seconds, 4), "seconds_loop": round(stats.runtime_seconds, 4),
        "assign_ms": round(assign_ms, 3), "update_ms": round(update_ms, 3),
        "assign_tflops": round(2.0 * args.n * args.k * args.dim / (assign_ms * 1e-3) / 1e12, 1),
        "assign_share_of_dense_peak": round(2.0 * args.n * args.k * args.dim / (assign_ms * 1e-3) / PEAK_DENSE_FLOPS, 4),
        "update_gbps": round(args.n * row_bytes / (update_ms * 1e-3) / 1e9, 1),
        "update_share_of_hbm_peak": round(args.n * row_bytes / (update_ms * 1e-3) / PEAK_HBM_BYTES, 4),
        "aggregate_distance": stats.aggregate_distance, "clusters_left_empty": int(args.k - len(np.unique(assignments))),
    }
    if args.reference_driver:
        n = args.reference_n or args.n
        rounds = args.reference_iterations or args.iterations
        with tempfile.TemporaryDirectory() as scratch:
            path = os.path.join(scratch, "X.f16")
            X[:n].tofile(path)
            out = subprocess.run([args.reference_driver, path, str(n), str(args.dim), str(args.k), str(rounds), str(args.reference_threads)],
                                 check=True, capture_output=True, text=True).stdout.split()
        reference_seconds = float(out[0])
        scale = (args.n / n) * (iterations / int(out[1]))
        line.update({"reference_threads": args.reference_threads, "reference_n": n, "reference_iterations": int(out[1]),
                     "reference_seconds_measured": round(reference_seconds, 3),
                     "reference_seconds_at_full_size": round(reference_seconds * scale, 1),
                     "reference_scaled_by": round(scale, 2),
                     "speedup_loop": round(reference_seconds * scale / max(1e-9, stats.runtime_seconds), 1)})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
