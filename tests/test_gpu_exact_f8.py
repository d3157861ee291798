"""GPU: batched exact search over f8 (OCP e4m3) rows on the matrix units (csrc/exact_tiled.hip, both tiles) and the matrix cast that
makes the codes (csrc/cast_rows.hip). The oracle has no arithmetic for f8, so the truth is tests/exact_truth.py's: data planted as
f16, rounded to e4m3 by the codec of tests/test_f8_cast.py and viewed as f16 again (exact) are held to `Truth(metric, "f16", …)`, whose
bound applies unchanged: products exact in f32, an f32 sum in any order, Σx² by the f16 scheme. Every case asserts its route and, on
the CPU, that ≥ 80 % of its queries are decided before it searches.
Observed on an MI355X, largest |distance − f64 distance| ÷ bound: cos 64-d 0.011 (64 tile), 0.010 (wide tile); 0.000 in every ip and
l2sq case (such sums of e4m3 products are exact in f32). The same cases through gfx950's fp8 matrix instructions, before the kernels
decoded to f16: 1.5 … 1.9 bounds (csrc/device_math.hpp has the account). Decided: 92 … 100 % per case. The file takes 2 s on the GPU.
"""
import functools

import numpy as np
import pytest

import usearch_amd
from tests import exact_truth
from tests.test_f8_cast import DECODE, FINITE, encode

pytestmark = pytest.mark.gpu
SIZES = {64: (3000, 70, 0), 256: (8200, 100, 200)}  # tile → rows, planted queries, copies (the wide tile wants ≥ 8 192 rows)


def route(rows, ndim, count, k, tile=None):
    return usearch_amd.index.test_plan_exact(rows, ndim, (ndim + 15) // 16 * 16, count, k, forced_tile=tile)


@functools.lru_cache(maxsize=None)
def planted(metric, ndim, rungs, tile, seed=5):
    # → codes of the rows, of the queries, and the f64 truth of the values they stand for
    rows, queries, copies = SIZES[tile]
    edges = exact_truth.edge_slots(rows, [route(rows, ndim, queries + copies, 10, tile=t) for t in ((64, 256) if tile == 256 else (64,))])
    case = exact_truth.plant(metric, "f16", ndim, rows, queries, rungs, seed, edges=edges, copies=copies)
    r, q = encode(case.rows), encode(case.queries)
    return r, q, exact_truth.Truth(metric, "f16", DECODE[r].astype(np.float16), DECODE[q].astype(np.float16))


def hold_to_truth(monkeypatch, metric, ndim, k, rungs, tile, wide, size=None):
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", str(tile))
    rows, queries, truth = planted(metric, ndim, rungs, size or tile)
    assert route(len(rows), ndim, len(queries), k)["wide"] == wide
    assert truth.decided(k).mean() >= exact_truth.DECIDED_SHARE  # on the CPU, before any GPU call
    keys, distances = usearch_amd.exact_search(rows, queries, k, metric=metric, dtype="f8", tiled=True)
    print(f"\n[exact f8] {metric} {ndim}-d k = {k} tile {tile}:", truth.check(keys.astype(np.int64), distances, np.full(len(queries), k), k))


SHAPES = [("cos", 64, 10, 16), ("l2sq", 96, 10, 16), ("l2sq", 130, 16, 18), ("ip", 200, 10, 16), ("ip", 768, 10, 16)]  # row bytes: below a chunk, 96, two bytes into the second chunk, 200, six chunks


@pytest.mark.parametrize("tile", [64, 256])
@pytest.mark.parametrize("metric,ndim,k,rungs", SHAPES, ids=[f"{m}-{n}-k{k}" for m, n, k, _ in SHAPES])
def test_every_shape_on_both_tiles(monkeypatch, metric, ndim, k, rungs, tile):
    hold_to_truth(monkeypatch, metric, ndim, k, rungs, tile, wide=int(tile == 256))


@pytest.mark.parametrize("k,tile,wide", [(1, 256, 1), (10, 256, 1), (11, 256, 1), (16, 256, 1), (17, 256, 0), (64, 64, 0)])
def test_result_counts_at_every_boundary(monkeypatch, k, tile, wide):
    hold_to_truth(monkeypatch, "ip", 200, k, 64, tile, wide, size=256)  # (the 64 tile too: 100 ladders of 64 rungs want the rows)


def test_more_results_than_a_list_holds_and_the_wave_kernel_are_refused():
    rows = np.full((64, 16), 0x38, dtype=np.uint8)  # 0x38: the code of 1.0
    with pytest.raises(RuntimeError, match="No tiled exact-search kernel for this metric / scalar kind / result count"):
        usearch_amd.exact_search(rows, rows, 65, metric="ip", dtype="f8", tiled=True)
    with pytest.raises(RuntimeError, match="No MI355X kernel for this metric / scalar kind combination"):
        usearch_amd.exact_search(rows, rows, 10, metric="ip", dtype="f8", tiled=False)


@pytest.mark.parametrize("metric", ["ip", "l2sq"])
@pytest.mark.parametrize("part", range(4))
def test_every_code_decodes_exactly_on_the_64_tile(monkeypatch, metric, part):  # ip: 1 − 16·v, every term exact; l2sq: the norms' decode
    monkeypatch.delenv("USEARCH_AMD_EXACT_TILE", raising=False)
    codes = FINITE[64 * part:64 * part + 64]
    rows, query = np.repeat(codes[:, None], 16, axis=1), np.full((1, 16), 0x38, dtype=np.uint8)
    keys, distances = usearch_amd.exact_search(rows, query, len(codes), metric=metric, dtype="f8", tiled=True)
    if metric == "l2sq":
        exact_truth.Truth(metric, "f16", DECODE[rows].astype(np.float16), DECODE[query].astype(np.float16)).check(
            keys.astype(np.int64), distances, np.array([len(codes)]), len(codes))
    else:
        expected = (1.0 - 16.0 * DECODE[codes]).astype(np.float32)
        order = np.lexsort((-np.arange(len(codes)), expected))
        assert np.array_equal(keys[0].astype(np.int64), order) and np.array_equal(distances[0].view(np.uint32), expected[order].view(np.uint32))


def test_every_code_decodes_exactly_on_the_wide_tile(monkeypatch):
    # row j filled with finite code j mod 254, a query per code: its own rows are at l2sq 0 exactly (Σa², Σb², Σab: one exact number)
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "256")
    rows = np.repeat(FINITE[np.arange(8192) % len(FINITE), None], 16, axis=1)
    queries = np.repeat(FINITE[:, None], 16, axis=1)
    assert route(len(rows), 16, len(queries), 16)["wide"] == 1
    keys, distances = usearch_amd.exact_search(rows, queries, 16, metric="l2sq", dtype="f8", tiled=True)
    assert np.array_equal(distances.view(np.uint32), np.zeros_like(keys, dtype=np.uint32))
    assert np.array_equal(DECODE[rows[keys.astype(np.int64), 0]], np.repeat(DECODE[FINITE][:, None], 16, axis=1))


def test_cast_rows_gives_the_codec_bytes_and_they_search_alike(monkeypatch):
    monkeypatch.delenv("USEARCH_AMD_EXACT_TILE", raising=False)
    rng = np.random.default_rng(3)  # magnitudes from below the subnormals to past 448; 130-d: rows of 520 bytes, pieces run over their ends
    x = (rng.standard_normal((1000, 130)) * 2.0 ** rng.integers(-12, 11, (1000, 130))).astype(np.float32)
    x[0, :4] = [np.inf, -np.inf, np.nan, -0.0]
    codes = usearch_amd.cast_rows(x, "f8")
    assert np.array_equal(codes, encode(x)) and np.array_equal(usearch_amd.cast_rows(x[:, :100], "f8"), codes[:, :100])  # (… and a pitch)
    got, same = (usearch_amd.exact_search(c[1:], c[1:71], 10, metric="l2sq", dtype="f8", tiled=True) for c in (codes, encode(x)))
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[1].view(np.uint32), same[1].view(np.uint32))
