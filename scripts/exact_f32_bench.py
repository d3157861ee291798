#!/usr/bin/env python3
"""Exact search of f32 rows on the matrix units (`v_mfma_f32_32x32x2_f32`, csrc/exact_tiled.hip) at the size of the f32 baseline
configuration: N × dim f32 rows (cos), Q queries, k results, through `Index.exact_search_device(tiled=True)`. Seeded data generated on
the device; HIP-event time of the kernels (norms, the tile kernel; not the merge). Work is 2·Q·N·dim FLOP, the binding limit the f32
matrix peak of 157.3 TFLOP/s (64 FLOP/clk/SIMD), not HBM.

    python scripts/exact_f32_bench.py [--n 1000000] [--dim 768] [--queries 10000] [--k 10] [--repeats 5] [--wave-queries 200]

Three figures from ONE process, the steps alternating so that a drift of the clocks meets all of them:
  · f32 tiled — kernel ms per repeat, their spread, TFLOP/s and the share of the f32 matrix peak;
  · the wave-per-query kernel (`tiled=False`, what `exact=True` runs: the only f32 route before this one) on the same index for the
    first `--wave-queries` queries — ms per query, as measured on that sample: it reads the whole dataset once per query, so its time
    is proportional to the queries, and the full batch's is printed as "at this rate", not as a measurement;
  · f16 tiled on the same values narrowed to f16 — what f32 costs.
Prints a line per figure and one JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

F32_MATRIX_PEAK_TFLOPS = 157.3  # 256 CUs × 4 SIMDs × 64 FLOP/clk × 2.4 GHz


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--queries", type=int, default=10_000)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--wave-queries", type=int, default=200)
    args = parser.parse_args()
    import torch

    import bench
    import usearch_amd
    device = torch.device("cuda", 0)

    def index_of(data, dtype):
        built = usearch_amd.build(None, "cos", dtype, connectivity=4, expansion_add=16, device=0, device_pointer=data.data_ptr(),
                                  count=args.n, stride=data.stride(0), ndim=args.dim)
        return built, built.index

    rows = bench.synthetic_vectors_device(args.n, args.dim, "f32", 42, device)
    queries = bench.synthetic_vectors_device(args.queries, args.dim, "f32", 43, device)
    rows16 = rows.view(torch.float32).to(torch.float16).view(torch.uint8)  # the same values, narrowed
    queries16 = queries.view(torch.float32).to(torch.float16).view(torch.uint8)
    built32, index32 = index_of(rows, "f32")
    built16, index16 = index_of(rows16, "f16")
    del rows, rows16
    torch.cuda.empty_cache()
    keys = torch.zeros((args.queries, args.k), dtype=torch.int64, device=device)
    distances = torch.zeros((args.queries, args.k), dtype=torch.float32, device=device)
    counts = torch.zeros(args.queries, dtype=torch.int64, device=device)
    stream = torch.cuda.Stream(device)
    sample = min(args.wave_queries, args.queries)

    def step(index, batch, count, tiled) -> float:
        return index.exact_search_device(batch.data_ptr(), count, batch.stride(0), args.k, keys.data_ptr(), distances.data_ptr(),
                                         counts.data_ptr(), stream=stream.cuda_stream, tiled=tiled)

    steps = {"f32_tiled": lambda: step(index32, queries, args.queries, True), "f32_wave": lambda: step(index32, queries, sample, False),
             "f16_tiled": lambda: step(index16, queries16, args.queries, True)}
    for name in steps:  # warm the shapes up: first launches, the scratch, the clocks
        steps[name]()
        steps[name]()
    ms = {name: [] for name in steps}
    for _ in range(args.repeats):
        for name in steps:
            ms[name].append(steps[name]())

    def tflops(milliseconds, count):
        return 2.0 * count * args.n * args.dim / (milliseconds / 1e3) / 1e12

    tiled32, wave32, tiled16 = (np.array(ms[name]) for name in ("f32_tiled", "f32_wave", "f16_tiled"))
    print(f"f32 tiled: kernel {np.median(tiled32):.1f} ms (min {tiled32.min():.1f}, max {tiled32.max():.1f}, {args.repeats} repeats) = "
          f"{tflops(np.median(tiled32), args.queries):.1f} TFLOP/s = {tflops(np.median(tiled32), args.queries) / F32_MATRIX_PEAK_TFLOPS:.1%} "
          f"of the f32 matrix peak ({F32_MATRIX_PEAK_TFLOPS} TFLOP/s)", flush=True)
    per_query = wave32 / sample
    print(f"f32 wave-per-query (exact=True), {sample} queries measured: kernel {np.median(wave32):.1f} ms (min {wave32.min():.1f}, max "
          f"{wave32.max():.1f}) = {np.median(per_query):.3f} ms per query; {args.queries} queries at this rate: "
          f"{np.median(per_query) * args.queries:.0f} ms (not measured) — the tiled kernel's {np.median(tiled32) / args.queries:.4f} ms per "
          f"query is {np.median(per_query) / (np.median(tiled32) / args.queries):.1f} × less", flush=True)
    print(f"f16 tiled, the same values narrowed: kernel {np.median(tiled16):.1f} ms (min {tiled16.min():.1f}, max {tiled16.max():.1f}) = "
          f"{tflops(np.median(tiled16), args.queries):.1f} TFLOP/s; f32 costs {np.median(tiled32) / np.median(tiled16):.2f} × the f16 time", flush=True)
    print(json.dumps({"bench": "exact_f32", "n": args.n, "dim": args.dim, "queries": args.queries, "k": args.k, "metric": "cos",
                      "repeats": args.repeats, "f32_tiled_ms": [round(float(x), 3) for x in tiled32],
                      "f32_tiled_tflops": round(tflops(np.median(tiled32), args.queries), 2),
                      "f32_tiled_share_of_peak": round(tflops(np.median(tiled32), args.queries) / F32_MATRIX_PEAK_TFLOPS, 4),
                      "f32_wave_queries": sample, "f32_wave_ms": [round(float(x), 3) for x in wave32],
                      "f32_wave_ms_per_query": round(float(np.median(per_query)), 4),
                      "f16_tiled_ms": [round(float(x), 3) for x in tiled16],
                      "f16_tiled_tflops": round(tflops(np.median(tiled16), args.queries), 2)}))
    del built32, built16


if __name__ == "__main__":
    main()
