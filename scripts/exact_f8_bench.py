#!/usr/bin/env python3
"""Batched exact search of f8 (OCP e4m3) rows against the same values as f16, both on the matrix-unit tiles (csrc/exact_tiled.hip)
through `usearch_amd.exact_search(…, tiled=True)`, at the size of the f32 baseline configuration: Q queries × N × dim, cos, k results.

    python scripts/exact_f8_bench.py [--n 1000000] [--dim 768] [--queries 10000] [--k 10] [--repeats 5]

Seeded f32 values; the f8 codes by `usearch_amd.cast_rows` (csrc/cast_rows.hip, timed on its own), the f16 values by numpy. f8 has no
index to search (only the raw-matrix route takes it), so both kinds go the same way and what is timed is the WHOLE CALL by the host
clock — upload of both matrices, norms, tile kernel, merge, download; the call ends in a device-to-host copy — not the kernel alone:
the upload (N·dim bytes for f8, twice that for f16) is part of either figure and is printed as bytes. Two warm-up calls per kind,
then `--repeats` calls alternating between the kinds, so that a drift of the clocks meets both. Prints a line per kind, how far the
results agree (the keys of the f8 search against an f16 search of the DECODED codes: the same values, so the same neighbours up to
near-ties), and one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--n", type=int, default=1_000_000)
    parser.add_argument("--dim", type=int, default=768)
    parser.add_argument("--queries", type=int, default=10_000)
    parser.add_argument("--k", type=int, default=10)
    parser.add_argument("--repeats", type=int, default=5)
    args = parser.parse_args()
    import usearch_amd

    rng = np.random.default_rng(42)
    rows = rng.standard_normal((args.n, args.dim), dtype=np.float32)
    queries = rng.standard_normal((args.queries, args.dim), dtype=np.float32)
    began = time.perf_counter()
    rows8, queries8 = usearch_amd.cast_rows(rows, "f8"), usearch_amd.cast_rows(queries, "f8")
    cast_ms = (time.perf_counter() - began) * 1e3
    # the f16 side searches the values the codes stand for: every e4m3 value is an f16 value, so both kinds see the same numbers
    decode = usearch_amd.cast(np.arange(256, dtype=np.uint8), "f8", "f16", 256).view(np.float16)
    rows16, queries16 = decode[rows8], decode[queries8]
    del rows, queries

    def call(dataset, batch, dtype):
        began = time.perf_counter()
        keys, distances = usearch_amd.exact_search(dataset, batch, args.k, metric="cos", dtype=dtype, tiled=True)
        return (time.perf_counter() - began) * 1e3, keys

    steps = {"f8": lambda: call(rows8, queries8, "f8"), "f16": lambda: call(rows16, queries16, "f16")}
    keys = {}
    for name in steps:  # warm the shapes up: first launches, the allocator, the clocks
        steps[name]()
        keys[name] = steps[name]()[1]
    ms = {name: [] for name in steps}
    for _ in range(args.repeats):
        for name in steps:
            ms[name].append(steps[name]()[0])
    agree = float((keys["f8"] == keys["f16"]).mean())
    for name, width in (("f8", 1), ("f16", 2)):
        t = np.array(ms[name])
        print(f"{name} tiled, whole call: {np.median(t):.1f} ms (min {t.min():.1f}, max {t.max():.1f}, {args.repeats} repeats), "
              f"{(args.n + args.queries) * args.dim * width / 1e6:.0f} MB uploaded per call", flush=True)
    print(f"f8 takes {np.median(ms['f8']) / np.median(ms['f16']):.2f} × the f16 call; keys equal to the f16 search of the decoded codes: {agree:.4f}; "
          f"cast_rows of both matrices (upload, kernel, download): {cast_ms:.0f} ms", flush=True)
    print(json.dumps({"bench": "exact_f8", "n": args.n, "dim": args.dim, "queries": args.queries, "k": args.k, "metric": "cos",
                      "repeats": args.repeats, "timed": "whole call, host clock", "f8_ms": [round(float(x), 2) for x in ms["f8"]],
                      "f16_ms": [round(float(x), 2) for x in ms["f16"]], "keys_equal": round(agree, 4), "cast_rows_ms": round(cast_ms, 1)}))


if __name__ == "__main__":
    main()
