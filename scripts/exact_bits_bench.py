#!/usr/bin/env python3
"""Batched exact search over bit vectors (the bit tile, csrc/exact_bits.hip) at the size of one shard of the largest baseline
configuration: N × dim b1 rows, Q queries, k results, through `Index.exact_search_device`. Seeded data generated on the device;
HIP-event time of the kernels (the two popcount passes where the metric needs them, the padded copy of the batch, the tile kernel;
not the merge).

    python scripts/exact_bits_bench.py [--n 125000000] [--dim 128] [--metric hamming] [--queries 10000] [--k 10] [--repeats 5]
                                       [--wave-queries 200]

Two figures from ONE process, the steps alternating so that a drift of the clocks meets both:
  · the bit tile (`tiled=True`) over the full batch — kernel ms per repeat, their spread, and the share of the YARDSTICK it reaches;
  · the wave-per-query kernel (`tiled=False`, what `exact=True` runs: the only b1 route before this one) on the same index for the
    first `--wave-queries` queries — ms per query, as measured on that sample: it reads the whole matrix once per query, so its time
    is proportional to the queries, and the full batch's is printed as "at this rate", not as a measurement.
The yardstick is derived, not measured: two vector instructions (the logic operation and the accumulating popcount) per 32 bits of
every (query, row) pair, at the chip's issue rate of one 64-lane vector instruction per 2 cycles per SIMD — 256 compute units × 4
SIMDs × 32 lanes per cycle × 2.4 GHz = 78.6 · 10¹² lane-operations a second. 10 000 × 125 M × 128 bits are 10¹³ of them: 0.127 s.
Prints a line per figure and one JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LANE_OPERATIONS_PER_SECOND = 256 * 4 * 32 * 2.4e9  # one 64-lane vector instruction per 2 cycles per SIMD


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=125_000_000)
    parser.add_argument("--dim", type=int, default=128)
    parser.add_argument("--metric", default="hamming", choices=["hamming", "tanimoto", "sorensen"])
    parser.add_argument("--queries", type=int, default=10_000)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--wave-queries", type=int, default=200)
    args = parser.parse_args()
    import torch

    import bench
    import usearch_amd
    device = torch.device("cuda", 0)

    rows = bench.synthetic_vectors_device(args.n, args.dim, "b1", 42, device)
    queries = bench.synthetic_vectors_device(args.queries, args.dim, "b1", 43, device)
    # the graph is irrelevant here and kept thin; the index is what owns the rows
    built = usearch_amd.build(None, args.metric, "b1", connectivity=4, expansion_add=16, device=0, device_pointer=rows.data_ptr(),
                              count=args.n, stride=rows.stride(0), ndim=args.dim)
    index = built.index
    print(f"{args.n} x {args.dim} b1 rows generated and indexed on the device", flush=True)
    del rows
    torch.cuda.empty_cache()
    keys = torch.zeros((args.queries, args.k), dtype=torch.int64, device=device)
    distances = torch.zeros((args.queries, args.k), dtype=torch.float32, device=device)
    counts = torch.zeros(args.queries, dtype=torch.int64, device=device)
    stream = torch.cuda.Stream(device)
    sample = min(args.wave_queries, args.queries)

    def step(count, tiled) -> float:
        return index.exact_search_device(queries.data_ptr(), count, queries.stride(0), args.k, keys.data_ptr(), distances.data_ptr(),
                                         counts.data_ptr(), stream=stream.cuda_stream, tiled=tiled)

    steps = {"tile": lambda: step(args.queries, True), "wave": lambda: step(sample, False)}
    # the two kernels must agree before their times mean anything: the sample through both, bit for bit
    step(sample, True)
    torch.cuda.synchronize()
    tile_result = (keys[:sample].clone(), distances[:sample].clone().view(torch.int32), counts[:sample].clone())
    step(sample, False)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(tile_result, (keys[:sample], distances[:sample].view(torch.int32), counts[:sample])))
    print(f"the first {sample} queries through both kernels: {'the same keys, distance bits and counts' if same else 'DIFFERENT RESULTS'}", flush=True)
    for name in steps:  # warm the shapes up: first launches, the scratch, the clocks
        steps[name]()
    ms = {name: [] for name in steps}
    for _ in range(args.repeats):
        for name in steps:
            ms[name].append(steps[name]())

    words = -(-args.dim // 32)
    yardstick_ms = 2.0 * words * 32 * args.queries * args.n / LANE_OPERATIONS_PER_SECOND * 1e3  # 2 instructions × 32-bit words × 64 lanes / 2 cycles
    tile, wave = np.array(ms["tile"]), np.array(ms["wave"])
    per_query = wave / sample
    print(f"bit tile, {args.n} x {args.dim} b1 {args.metric}, {args.queries} queries, k = {args.k}: kernel {np.median(tile):.1f} ms (min "
          f"{tile.min():.1f}, max {tile.max():.1f}, {args.repeats} repeats); the derived yardstick (2 vector instructions per 32 bits per "
          f"pair at the chip's issue rate) is {yardstick_ms:.1f} ms: {yardstick_ms / np.median(tile):.1%} of it reached", flush=True)
    print(f"wave-per-query (exact=True), {sample} queries measured: kernel {np.median(wave):.1f} ms (min {wave.min():.1f}, max "
          f"{wave.max():.1f}) = {np.median(per_query):.3f} ms per query; {args.queries} queries at this rate: "
          f"{np.median(per_query) * args.queries:.0f} ms (not measured) — the tile's {np.median(tile) / args.queries:.4f} ms per query is "
          f"{np.median(per_query) / (np.median(tile) / args.queries):.2f} × less", flush=True)
    print(json.dumps({"bench": "exact_bits", "n": args.n, "dim": args.dim, "queries": args.queries, "k": args.k, "metric": args.metric,
                      "repeats": args.repeats, "same_results_on_sample": same, "tile_ms": [round(float(x), 3) for x in tile],
                      "yardstick_ms": round(yardstick_ms, 3), "tile_share_of_yardstick": round(yardstick_ms / float(np.median(tile)), 4),
                      "wave_queries": sample, "wave_ms": [round(float(x), 3) for x in wave],
                      "wave_ms_per_query": round(float(np.median(per_query)), 4),
                      "wave_over_tile_per_query": round(float(np.median(per_query) / (np.median(tile) / args.queries)), 3)}))
    del built


if __name__ == "__main__":
    main()
