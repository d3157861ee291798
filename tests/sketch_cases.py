"""The data sets of the sketch's prune-count tests, shared by the GPU test (tests/test_gpu_sketch_counts.py) and by the CPU test that
shows the model has teeth on exactly these data (tests/test_sketch_truth.py): reference-built indexes of 3 000 low-rank rows, their
queries, the oracle's hop traces and the twin bounds the model prunes by."""
from __future__ import annotations

import functools

import numpy as np

import usearch_amd.index as ua_index
from oracle import oraclebind
from tests import sketch_truth, util

ROWS, QUERIES, SINGLES, K, LANES, TILE = 3000, 640, 64, 10, 8, 64
# name → (dimensions, scalar kind, connectivity). 777 × f16 = 1 554 bytes and 389 × f32 = 1 556 bytes: 98 chunks of 16 bytes, 12 whole
# chunks per lane of 8 (the builds that carry the sketch), no multiple of 16 elements, the last chunk ragged.
CASES = {"f16_777_m16": (777, "f16", 16), "bf16_768_m16": (768, "bf16", 16), "f32_389_m16": (389, "f32", 16), "f16_777_m40": (777, "f16", 40)}


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """→ image (reference-built, single-threaded: slot = row number), rows, queries, and the twins' directions and records of the rows."""
    ndim, dtype, connectivity = CASES[name]
    seed = 300 + sorted(CASES).index(name)
    image, rows, _ = util.build_image(ROWS, ndim, "cos", dtype, seed=seed, connectivity=connectivity, keys=np.arange(ROWS, dtype=np.uint64))
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=seed + 50)
    directions, rank, defect = ua_index.test_sketch_directions(rows, dtype)
    records = ua_index.test_sketch_twin_records(rows, dtype, directions, defect)
    sums = np.array([oraclebind.sum_of_squares(q, dtype, ndim, lanes=LANES) for q in queries], dtype=np.float32)
    return {"name": name, "ndim": ndim, "dtype": dtype, "connectivity": connectivity, "image": image, "rows": rows, "queries": queries,
            "directions": directions, "rank": rank, "defect": defect, "records": records, "sums": sums}


@functools.lru_cache(maxsize=None)
def traced(name: str, expansion: int, frontier: int, count: int):
    """The oracle's search of the case's first `count` queries in the kernels' summation layout, with its hop trace →
    ((keys, distances, counts, visited, computed), traces)."""
    from concurrent.futures import ThreadPoolExecutor
    c = case(name)
    oracle = oraclebind.OracleIndex(c["image"])

    def part(first):  # (the trace and the frontier switch are the calling thread's own; the index is read-only)
        return oracle.search_traced(c["queries"][first:min(count, first + SINGLES)], K, dtype=c["dtype"], expansion=expansion, lanes=LANES,
                                    frontier_in_top=frontier == 2, tile_cells=TILE)
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(part, range(0, count, SINGLES)))
    found = tuple(np.concatenate([p[0][field] for p in parts]) for field in range(5))
    return found, [trace for p in parts for trace in p[1]]


def bounds_of(c: dict, queries: np.ndarray, sums: np.ndarray, directions: np.ndarray, records: np.ndarray):
    """Twin bounds of `queries` against `records` → (bounds [queries, records] f32, used [queries])."""
    return ua_index.test_sketch_twin_bounds(queries, sums, c["dtype"], directions, records)


def model_counts(traces, bounds: np.ndarray, used: np.ndarray) -> np.ndarray:
    """→ int64 [queries, 2]: the model's (tested, pruned) of every query."""
    return np.array([sketch_truth.prune_counts(trace, bounds[q] if used[q] else None) for q, trace in enumerate(traces)], dtype=np.int64).reshape(-1, 2)
