"""The sketch's bounds in the shadow of the probe's second round (usearch_amd/csrc/kernels.hpp, `search_one`, the in-`top` builds that
carry the sketch): with the records beside the probe — `top` full, a list of at most 32 cells — the first round of `probe_rest` is
peeled off, the lanes that met a taken home cell issue their second compare-and-swap, and the bounds of all 32 list positions are
computed before that answer is waited for. A change of order, and of which positions get a bound (all of them, fresh or not): not a
bit of a result or a counter may move. Every case against the oracle — keys, distance bits, counts, `visited`, `computed` — and
sketch on against sketch off.

Batches of 640 queries so that the one-wave kernel runs. Low-rank rows of 20 000 × 768 f16 under cos with lists of 16, 32, 48 and 80
cells (the records beside the probe and behind it, a list of two tiles), expansions 16, 64 and 608, both frontiers (the heap frontier
keeps the old order and must behave as before); 768 × f32 (the two-row form), 768 × bf16, 800 × f16 (a ragged tail); and a visited
set forced small, where most lanes meet a taken home cell, many go on past the peeled round, and the query finally overflows and is
run again up the ladder."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_sketch_hop import OFF, ON, _same, _same_as_oracle, _search

pytestmark = pytest.mark.gpu

QUERIES = 640

# name → (dimensions, scalar kind, connectivity, expansions, frontiers (0 = the engine's choice), queries the oracle restates)
CASES = {
    "f16_768_m16": (768, "f16", 16, (16, 64), (1, 2), QUERIES),
    "f16_768_m16_ef608": (768, "f16", 16, (608,), (0,), 64),
    "f16_768_m8": (768, "f16", 8, (16, 64), (1, 2), QUERIES),
    "f16_768_m24": (768, "f16", 24, (16, 64), (1, 2), QUERIES),
    "f16_768_m40": (768, "f16", 40, (16, 64), (1, 2), QUERIES),
    "f32_768_m16": (768, "f32", 16, (64,), (1, 2), QUERIES),
    "bf16_768_m16": (768, "bf16", 16, (64,), (1, 2), QUERIES),
    "f16_800_m16": (800, "f16", 16, (16, 64), (2,), QUERIES),
}
ROWS = 20000


def _build(rows, dtype, seed, connectivity):
    import usearch_amd
    built = usearch_amd.build(rows, "cos", dtype, keys=np.arange(len(rows), dtype=np.uint64), seed=seed, connectivity=connectivity)
    image = built.save_buffer()
    built.close()
    index = usearch_amd.Index.restore(image)
    assert index.arrays.sketch == 1
    return image, index


@pytest.mark.parametrize("name", list(CASES))
def test_walk_equals_the_oracle(name):
    ndim, dtype, connectivity, expansions, frontiers, restated = CASES[name]
    seed = 300 + sorted(CASES).index(name)
    rows = util.make_vectors(ROWS, ndim, dtype, seed=seed)
    image, index = _build(rows, dtype, seed, connectivity)
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=seed + 1)
    queries[:32] = rows[:32]  # stored rows among the queries: distance zero at the first hop that meets them
    for expansion in expansions:
        for frontier in frontiers:
            what = f"{name}, expansion {expansion}, frontier {frontier}"
            off, on = _search(index, queries, expansion, OFF, frontier, dtype=dtype), _search(index, queries, expansion, ON, frontier, dtype=dtype)
            assert on.stats.variant != 5 and (frontier == 0 or on.stats.frontier == frontier), "one wave per query, the frontier asked for"
            assert on.stats.sketch_tested > 0 and off.stats.sketch_tested == 0, what
            _same(on, off, what)
            _same_as_oracle(on, image, queries, dtype, expansion, index.lanes_per_row, what, restated)
            print(f"{what}: frontier {on.stats.frontier}, {int(on.visited_per_query.sum())} hops, {int(on.computed_per_query.sum())} distances")


def test_crowded_visited_set(monkeypatch):
    """A visited set forced small (1 024 cells, 768 usable): towards the end of its room most probes meet a taken home cell and many a
    taken second cell — the peeled round, then `probe_rest` from one cell further on — until a walk at expansion 64 outgrows it, is
    abandoned and run again up the retry ladder with four times the cells. Same results as the launch that was sized well."""
    ndim, dtype = 768, "f16"
    rows = util.make_vectors(ROWS, ndim, dtype, seed=341)
    image, index = _build(rows, dtype, 341, 16)
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=342)
    for frontier in (1, 2):
        monkeypatch.delenv("USEARCH_AMD_HASH_CAP", raising=False)
        roomy = _search(index, queries, 64, ON, frontier)
        assert roomy.stats.passes == 1 and roomy.stats.frontier == frontier and roomy.stats.variant != 5
        assert int(roomy.computed_per_query.max()) > 768, "no walk of this case outgrows 768 cells: the case is empty"
        monkeypatch.setenv("USEARCH_AMD_HASH_CAP", "1024")
        tight = _search(index, queries, 64, ON, frontier)
        monkeypatch.delenv("USEARCH_AMD_HASH_CAP")
        assert tight.stats.passes >= 2, "1 024 cells were expected to overflow"
        _same(tight, roomy, f"a small visited set, frontier {frontier}")
        _same_as_oracle(tight, image, queries, dtype, 64, index.lanes_per_row, f"a small visited set, frontier {frontier}")
