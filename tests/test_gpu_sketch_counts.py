"""`stats.sketch_tested` / `stats.sketch_pruned` of the walk against a MODEL of its prune decision (tests/sketch_truth.py
`prune_counts`), query by query: the oracle's hop trace (which candidates each hop found fresh, `top`'s state at the start of each tile
of 64 list cells) and the host twins' bounds computed from the records and directions READ BACK from the snapshot, with the query's Σa²
from the oracle's eight-lane layout. tests/golden/sketch_hop/counters.json pins these counters to what the library counted earlier;
this pins them to what they must be — a ρ that is 1e-3 off either way, a coefficient column read from the wrong lane or a dimension
left out of the query's projection moves the counts (tests/test_sketch_truth.py `test_prune_model_has_teeth` shows by how much, on
these very data).

Indexes of 3 000 low-rank rows, cos, built by the reference: 777 × f16, 768 × bf16 and 389 × f32 at connectivity 16 (lists of 32 cells: the
records are fetched beside the probe) and 777 × f16 at connectivity 40 (80 cells: two tiles, the second tested against the state the
first one's commits left; records behind the probe). 777 × f16 and 389 × f32 are no multiple of 16 elements: the scalar tail of the
projection runs. Their rows pad to 104 chunks of 16 bytes, 13 per lane of 8; the planner gives rows of 12 chunks per lane AND MORE the
builds with twelve loads in flight, which carry the sketch — asserted below through `index.arrays.sketch`, the lanes, the chunks and
the variant the call reports. Both frontiers, expansions 16 and 64; 64 queries one per call with the one-wave build forced (a single
query would else go to the five-wave team, which has no sketch path), and one batch of 640."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import usearch_amd.index as ua_index
from tests import sketch_cases, util

pytestmark = pytest.mark.gpu

K, OFF, ON = sketch_cases.K, 1, 2  # usearch_amd_tuning_t::sketch
ONE_WAVE = {1: 3, 2: 4}  # usearch_amd_tuning_t::variant: twelve loads in flight; for the in-`top` frontier two rows per lane group


@functools.lru_cache(maxsize=None)
def restored(name: str):
    """→ (index, records, directions) with the sketch as the snapshot holds it."""
    from usearch_amd import Index
    c = sketch_cases.case(name)
    index = Index.restore(c["image"])
    assert index.arrays.sketch == 1 and index.lanes_per_row == 8 and index.row_stride // 16 // 8 >= 12, f"{name} is not eligible for a sketch"
    records, directions, defect, rows = ua_index.test_sketch_read_back(index)
    assert np.array_equal(rows, np.ascontiguousarray(c["rows"]).view(np.uint8).reshape(len(rows), -1)), "slot = row number"
    assert np.array_equal(directions, c["directions"]) and defect == c["defect"], "directions other than the twin draws from these rows"
    return index, records, directions


def _search(index, queries, expansion, sketch, frontier, variant=0):
    from usearch_amd import Tuning
    return index.search(queries, K, expansion=expansion, dtype=index.dtype, tuning=Tuning(sketch=sketch, frontier=frontier, variant=variant))


def _same(a, b, what):
    assert np.array_equal(a.keys, b.keys), f"{what}: keys differ"
    assert util.same_float_bits(a.distances, b.distances), f"{what}: distance bits differ"
    assert np.array_equal(a.counts, b.counts), f"{what}: counts differ"
    assert np.array_equal(a.visited_per_query, b.visited_per_query), f"{what}: visited members differ"
    assert np.array_equal(a.computed_per_query, b.computed_per_query), f"{what}: computed distances differ"


@pytest.mark.parametrize("expansion", [16, 64])
@pytest.mark.parametrize("frontier", [1, 2])
@pytest.mark.parametrize("name", list(sketch_cases.CASES))
def test_counters_equal_the_model(name, frontier, expansion):
    c = sketch_cases.case(name)
    index, records, directions = restored(name)
    queries, dtype = c["queries"], c["dtype"]
    what = f"{name}, expansion {expansion}, frontier {frontier}"
    bounds, used = sketch_cases.bounds_of(c, queries, c["sums"], directions, records)
    assert used.all()
    (keys, distances, counts, visited, computed), traces = sketch_cases.traced(name, expansion, frontier, sketch_cases.QUERIES)
    model = sketch_cases.model_counts(traces, bounds, used)

    # soundness on the walk's own pairs: no tested candidate's bound exceeds the distance the kernel computes for it
    singles = sketch_cases.SINGLES
    both = np.ascontiguousarray(np.concatenate([queries[:singles], c["rows"]]))
    measure = util.slot_distance(both, "cos", dtype, c["ndim"], lanes=sketch_cases.LANES)
    pairs, worst = 0, -np.inf
    for q in range(singles):
        for full, _, _, fresh in traces[q]:
            for slot in (fresh if full else ()):
                pairs += 1
                worst = max(worst, float(bounds[q, slot]) - measure(q, singles + int(slot)))
    print(f"{what}: {pairs} tested pairs of {singles} queries, largest bound − distance {worst:.3g}")
    assert pairs and worst <= 0.0

    # one query per call
    device = np.zeros((singles, 2), dtype=np.int64)
    for q in range(singles):
        on = _search(index, queries[q:q + 1], expansion, ON, frontier, ONE_WAVE[frontier])
        assert on.stats.variant != 5 and on.stats.frontier == frontier, "one wave per query, the frontier asked for"
        assert on.stats.sketch_tested > 0, f"{what}, query {q}: the walk did not use the sketch"
        device[q] = on.stats.sketch_tested, on.stats.sketch_pruned
        assert np.array_equal(on.keys[0], keys[q]) and util.same_float_bits(on.distances[0], distances[q]), f"{what}, query {q}: not the oracle's result"
    wrong = np.flatnonzero((device != model[:singles]).any(axis=1))
    print(f"{what}: one query per call, {singles - len(wrong)} of {singles} equal to the model; "
          f"device {device.sum(axis=0).tolist()}, model {model[:singles].sum(axis=0).tolist()} (tested, pruned)")
    assert not len(wrong), f"{what}: queries {wrong[:8]}: device {device[wrong[:8]].tolist()}, model {model[wrong[:8]].tolist()}"

    # the batch: totals, and sketch on against sketch off against the oracle
    on, off = _search(index, queries, expansion, ON, frontier), _search(index, queries, expansion, OFF, frontier)
    assert on.stats.variant != 5 and on.stats.frontier == frontier
    assert off.stats.sketch_tested == 0 and off.stats.sketch_pruned == 0
    _same(on, off, what)
    assert np.array_equal(on.keys, keys) and util.same_float_bits(on.distances, distances) and np.array_equal(on.counts, counts), what
    assert np.array_equal(on.visited_per_query, visited) and np.array_equal(on.computed_per_query, computed), what
    totals = (int(on.stats.sketch_tested), int(on.stats.sketch_pruned))
    print(f"{what}: batch of {len(queries)}, device {list(totals)}, model {model.sum(axis=0).tolist()} (tested, pruned)")
    assert totals == tuple(int(v) for v in model.sum(axis=0)), what


def _unused_queries(dtype: str, ndim: int, like: np.ndarray):
    zero = np.zeros_like(like)
    if dtype != "f32":
        return {"zero": zero}
    shape = like.astype(np.float64) / np.abs(like).max()
    return {"zero": zero, "elements at 1e-20": (shape * 1e-20).astype(np.float32), "elements at 1e18": (shape * 1e18).astype(np.float32)}


@pytest.mark.parametrize("frontier", [1, 2])
@pytest.mark.parametrize("name", ["f32_389_m16", "f16_777_m16"])
def test_queries_out_of_range_walk_without_the_sketch(name, frontier):
    c = sketch_cases.case(name)
    index, _, _ = restored(name)
    for label, query in _unused_queries(c["dtype"], c["ndim"], c["queries"][0]).items():
        query = np.ascontiguousarray(query[None, :])
        a2 = sketch_cases.oraclebind.sum_of_squares(query[0], c["dtype"], c["ndim"], lanes=sketch_cases.LANES)
        assert not (2.0 ** -100 <= float(a2) <= 2.0 ** 100), f"{label}: Σa² = {a2} is in range"
        on = _search(index, query, 64, ON, frontier, ONE_WAVE[frontier])
        off = _search(index, query, 64, OFF, frontier, ONE_WAVE[frontier])
        assert on.stats.variant != 5 and on.stats.variant == off.stats.variant
        print(f"{name}, frontier {frontier}, query {label}: Σa² = {a2}, tested {on.stats.sketch_tested}, visited {int(on.visited_per_query[0])}")
        assert on.stats.sketch_tested == 0 and on.stats.sketch_pruned == 0, f"{label}: the sketch was used"
        _same(on, off, f"{name}, frontier {frontier}, query {label}")
    # … while an ordinary query through the very same call does use it
    assert _search(index, c["queries"][:1], 64, ON, frontier, ONE_WAVE[frontier]).stats.sketch_tested > 0
