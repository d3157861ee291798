#!/usr/bin/env python3
"""The three exact-search routes of f32 rows on ONE index in ONE process: N × dim f32 rows, Q queries, k results, per metric.

    python scripts/exact_screened_bench.py [--n 1000000] [--dim 768] [--queries 10000] [--k 10] [--repeats 3] [--wave-queries 200]
                                           [--metrics cos,l2sq]

  · wave — `exact=True`'s wave-per-query kernel (`exact_search_device(tiled=False)`) on the first `--wave-queries` queries: it reads
    the whole dataset once per query, so its time is proportional to the queries; ms per query as measured on that sample, the full
    batch's printed as "at this rate", not as a measurement;
  · tiled — the f32 matrix-unit tile (`tiled=True`), cos and ip only (l2sq over f32 is refused): distances within a bound, not the bits;
  · screened — `tiled="screened"` (csrc/exact_screened.hip): the wave kernel's bits.
HIP-event time of the kernels, the steps alternating so that a drift of the clocks meets all of them; seeded data generated on the
device. One more screened search through the host entry reports the rows measured per query (mean, maximum) and the queries handed to
the wave kernel whole (they report every row), and checks its keys against the wave kernel's on the sample. A line per figure and one
JSON line per metric.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--queries", type=int, default=10_000)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--wave-queries", type=int, default=200)
    parser.add_argument("--metrics", default="cos,l2sq")
    args = parser.parse_args()
    import torch

    import bench
    import usearch_amd
    device = torch.device("cuda", 0)
    rows = bench.synthetic_vectors_device(args.n, args.dim, "f32", 42, device)
    queries = bench.synthetic_vectors_device(args.queries, args.dim, "f32", 43, device)
    keys = torch.zeros((args.queries, args.k), dtype=torch.int64, device=device)
    distances = torch.zeros((args.queries, args.k), dtype=torch.float32, device=device)
    counts = torch.zeros(args.queries, dtype=torch.int64, device=device)
    stream = torch.cuda.Stream(device)
    sample = min(args.wave_queries, args.queries)
    host_queries = queries.view(torch.float32).cpu().numpy()

    for metric in args.metrics.split(","):
        built = usearch_amd.build(None, metric, "f32", connectivity=4, expansion_add=16, device=0, device_pointer=rows.data_ptr(),
                                  count=args.n, stride=rows.stride(0), ndim=args.dim)
        index = built.index

        def step(count, tiled) -> float:
            return index.exact_search_device(queries.data_ptr(), count, queries.stride(0), args.k, keys.data_ptr(), distances.data_ptr(),
                                             counts.data_ptr(), stream=stream.cuda_stream, tiled=tiled)

        steps = {"wave": lambda: step(sample, False), "screened": lambda: step(args.queries, "screened")}
        if metric != "l2sq":
            steps["tiled"] = lambda: step(args.queries, True)
        for name in steps:  # warm the shapes up: first launches, the scratch, the clocks
            steps[name]()
        ms = {name: [] for name in steps}
        for _ in range(args.repeats):
            for name in steps:
                ms[name].append(steps[name]())
        got = index.search(host_queries, args.k, exact="screened")
        truth = index.search(host_queries[:sample], args.k, exact=True)
        same = bool(np.array_equal(got.keys[:sample], truth.keys) and
                    np.array_equal(got.distances[:sample].view(np.uint32), truth.distances.view(np.uint32)))
        measured = got.computed_per_query
        handed = int((measured == len(index)).sum())
        screened_rows = measured[measured != len(index)]
        wave_per_query = np.array(ms["wave"]) / sample
        screened = np.array(ms["screened"])
        print(f"{metric} wave (exact=True), {sample} queries measured: {np.median(wave_per_query):.4f} ms per query (min "
              f"{wave_per_query.min():.4f}, max {wave_per_query.max():.4f}); {args.queries} queries at this rate: "
              f"{np.median(wave_per_query) * args.queries:.0f} ms (not measured)", flush=True)
        if "tiled" in ms:
            print(f"{metric} tiled: {np.median(ms['tiled']):.1f} ms (min {min(ms['tiled']):.1f}, max {max(ms['tiled']):.1f})", flush=True)
        print(f"{metric} screened: {np.median(screened):.1f} ms (min {screened.min():.1f}, max {screened.max():.1f}) = "
              f"{np.median(screened) / args.queries:.4f} ms per query, {np.median(wave_per_query) * args.queries / np.median(screened):.1f} × "
              f"less than the wave kernel at its rate; rows measured per screened query: mean "
              f"{screened_rows.mean() if len(screened_rows) else 0:.1f}, max {screened_rows.max() if len(screened_rows) else 0}; handed "
              f"over: {handed} of {args.queries}; same keys and bits as exact=True on the sample: {same}", flush=True)
        print(json.dumps({"bench": "exact_screened", "n": args.n, "dim": args.dim, "queries": args.queries, "k": args.k, "metric": metric,
                          "repeats": args.repeats, "wave_queries": sample, "wave_ms": [round(float(x), 3) for x in ms["wave"]],
                          "wave_ms_per_query": round(float(np.median(wave_per_query)), 4),
                          "tiled_ms": [round(float(x), 3) for x in ms.get("tiled", [])],
                          "screened_ms": [round(float(x), 3) for x in screened],
                          "remeasured_mean": round(float(screened_rows.mean()), 2) if len(screened_rows) else None,
                          "remeasured_max": int(screened_rows.max()) if len(screened_rows) else None, "handed_over": handed,
                          "same_bits_on_sample": same}), flush=True)
        del index, built
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
