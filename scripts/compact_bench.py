"""`isolate` and `compact` at scale: N × dims f16 rows (cos) built on the device, a share of the members removed at random.
Prints one JSON line: milliseconds of `isolate`; milliseconds of `compact`, split into scan / lists / rows; the bytes of rows that
moved and bytes ÷ time as a share of the streaming-copy ceiling (a row is read once and written once; 6.29 TB/s is what a float4
copy reaches on an MI355X, 79 % of the 8 TB/s peak); milliseconds per step of `--queries` queries at `--expansion` with
`stats.frontier` / `stats.plain` before the removals, with tombstones and after `compact` — and, with `--reference-driver`, the
seconds the reference's `isolate()` takes on the host's cores over the same image (scripts/compact_reference_driver.cpp, compiled
outside the repository).

    python scripts/compact_bench.py --n 10000000 --dim 768 --removed 0.1 --queries 10000 --expansion 608

`isolate` runs on a second build of the same rows (a build is deterministic), so that `compact` meets lists nobody has isolated.
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

COPY_CEILING_BYTES = 6.29e12  # float4 copy, read + write counted


def synthetic(n: int, dim: int, seed: int) -> np.ndarray:
    """Low-rank latent + noise, f16 rows; generated in slabs."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((32, dim)).astype(np.float32)
    out = np.empty((n, dim), dtype=np.float16)
    for first in range(0, n, 65536):
        last = min(n, first + 65536)
        out[first:last] = rng.standard_normal((last - first, 32), dtype=np.float32) @ basis + 0.3 * rng.standard_normal((last - first, dim), dtype=np.float32)
    return out


def step(index, queries, expansion: int, repeat: int):
    """Best of `repeat` steps: kernel milliseconds of the batch, and the kernels it ran."""
    best, stats = float("inf"), None
    for _ in range(repeat):
        begin = time.perf_counter()
        got = index.search(queries, 10, expansion=expansion)
        wall_ms = (time.perf_counter() - begin) * 1e3
        ms = got.stats.kernel_ms if got.stats.kernel_ms > 0 else wall_ms
        if ms < best:
            best, stats = ms, got.stats
    return {"ms": round(best, 3), "frontier": int(stats.frontier), "plain": int(stats.plain)}


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=10_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--removed", type=float, default=0.1)
    parser.add_argument("--queries", type=int, default=10_000)
    parser.add_argument("--expansion", type=int, default=608)
    parser.add_argument("--repeat", type=int, default=3)
    parser.add_argument("--staging-bytes", type=int, default=0)
    parser.add_argument("--skip-isolate", action="store_true", help="no second build for `isolate` alone")
    parser.add_argument("--reference-driver", default="", help="the compiled scripts/compact_reference_driver.cpp")
    parser.add_argument("--reference-threads", type=int, default=16)
    args = parser.parse_args()

    import usearch_amd

    rows = synthetic(args.n, args.dim, 42)
    queries = synthetic(args.queries, args.dim, 43)
    removed = np.sort(np.random.default_rng(44).choice(args.n, int(args.n * args.removed), replace=False)).astype(np.uint32)
    keys = np.arange(args.n, dtype=np.uint64)
    line = {"what": "compact", "n": args.n, "dims": args.dim, "dtype": "f16", "metric": "cos", "removed": int(len(removed)),
            "queries": args.queries, "expansion": args.expansion}

    if not args.skip_isolate:
        built = usearch_amd.build(rows, "cos", "f16", keys=keys)
        built.remove(removed)
        if args.reference_driver:
            with tempfile.TemporaryDirectory() as scratch:
                path = os.path.join(scratch, "tombstones.usearch")
                built.save(path)
                out = subprocess.run([args.reference_driver, path, str(args.reference_threads)], check=True, capture_output=True,
                                     text=True).stdout.split()
            line.update({"reference_isolate_seconds": float(out[0]), "reference_threads": args.reference_threads})
        begin = time.perf_counter()
        pruned = built.isolate()
        stats = built.index.compact_stats
        line.update({"isolate_ms": round(stats["scan_ms"] + stats["lists_ms"], 3), "isolate_wall_ms": round((time.perf_counter() - begin) * 1e3, 3),
                     "isolate_pruned_edges": int(pruned)})
        built.close()

    built = usearch_amd.build(rows, "cos", "f16", keys=keys)
    line["step_before"] = step(built.index, queries, args.expansion, args.repeat)
    built.remove(removed)
    line["step_tombstones"] = step(built.index, queries, args.expansion, args.repeat)
    begin = time.perf_counter()
    built.compact(staging_bytes=args.staging_bytes)
    wall_ms = (time.perf_counter() - begin) * 1e3
    stats = built.index.compact_stats
    traffic = 2.0 * stats["moved_bytes"]  # every moved row is read once and written once (the staging hop doubles both)
    line.update({"compact_ms": round(stats["scan_ms"] + stats["lists_ms"] + stats["rows_ms"], 3), "compact_wall_ms": round(wall_ms, 3),
                 "scan_ms": round(stats["scan_ms"], 3), "lists_ms": round(stats["lists_ms"], 3), "rows_ms": round(stats["rows_ms"], 3),
                 "moved_bytes": int(stats["moved_bytes"]), "chunks": int(stats["chunks"]), "pruned_edges": int(stats["pruned_edges"]),
                 "rows_share_of_copy_ceiling": round(traffic / max(1e-9, stats["rows_ms"] * 1e-3) / COPY_CEILING_BYTES, 4)})
    line["step_compacted"] = step(built.index, queries, args.expansion, args.repeat)
    if "reference_isolate_seconds" in line and "isolate_ms" in line:
        line["isolate_speedup"] = round(line["reference_isolate_seconds"] * 1e3 / max(1e-9, line["isolate_ms"]), 1)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
