"""The hop of the sketch walk (usearch_amd/csrc/kernels.hpp, `sketch_ak` builds): survivors measured one row per lane group when
they fit one round, records requested beside the visited-set probe when the list has at most 32 cells. Neither may change a
result: sketch on against sketch off against the oracle, bit for bit — keys, distance bits, counts and both traversal counters,
with either frontier — and `stats.sketch_tested` / `stats.sketch_pruned` equal to what the library BEFORE these changes counted
(tests/golden/sketch_hop/counters.json, written by tests/golden/sketch_hop/record.py).

Batches of 640 queries so that the one-wave kernel runs; indexes of 20 000 rows (2 500 where the reference builds them). The
cases: three kinds of data, each asserted to be what it is there for (survivors per hop = (tested − pruned) / Σ visited) — low-rank
rows (under 8: one row per lane group), i.i.d. Gaussian rows with the sketch forced on (over 8: the two-row form, nothing lost when
nothing is pruned), a half-and-half mixture (both, hop by hop); lists on both sides of the 32-cell rule — connectivity 8, 16, 24, 40
= 16, 32, 48, 80 cells; rows of 768 × f16 / bf16 / f32 and 800 × f16 (a ragged tail); expansion 608 (the 16-cell `top`);
tombstones, a filtered search over the heap frontier, and rows stored three times (exact ties at the radius)."""
import json
import os

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

QUERIES, K = 640, 10
OFF, ON = 1, 2  # usearch_amd_tuning_t::sketch
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sketch_hop", "counters.json")

# name → (data kind, rows, dimensions, scalar kind, connectivity, expansions, frontiers (0 = the engine's choice), queries the oracle restates)
CASES = {
    "lowrank_f16_m16": ("lowrank", 20000, 768, "f16", 16, (16, 64), (1, 2), QUERIES),
    "gaussian_f16_m16": ("gaussian", 20000, 768, "f16", 16, (16, 64), (1, 2), QUERIES),
    "mixture_f16_m16": ("mixture", 20000, 768, "f16", 16, (16, 64), (1, 2), QUERIES),
    "lowrank_f16_m16_ef608": ("lowrank", 20000, 768, "f16", 16, (608,), (0,), 64),
    "lowrank_f16_m8": ("lowrank", 20000, 768, "f16", 8, (16, 64), (2,), QUERIES),
    "lowrank_f16_m24": ("lowrank", 20000, 768, "f16", 24, (16, 64), (2,), QUERIES),
    "mixture_f16_m40": ("mixture", 20000, 768, "f16", 40, (16, 64), (2,), QUERIES),
    "lowrank_bf16_m16": ("lowrank", 20000, 768, "bf16", 16, (64,), (1, 2), QUERIES),
    "lowrank_f32_m16": ("lowrank", 20000, 768, "f32", 16, (64,), (1, 2), QUERIES),
    "lowrank_f16_800_m16": ("lowrank", 20000, 800, "f16", 16, (16, 64), (2,), QUERIES),
}


def make_rows(kind, n, ndim, dtype, seed):
    if kind == "lowrank":
        return util.make_vectors(n, ndim, dtype, seed=seed)
    if kind == "gaussian":
        return util.make_vectors(n, ndim, dtype, seed=seed, clustered=False)
    half = n // 2  # the mixture: one half of each, shuffled
    rows = np.concatenate([util.make_vectors(half, ndim, dtype, seed=seed), util.make_vectors(n - half, ndim, dtype, seed=seed + 1000, clustered=False)])
    return np.ascontiguousarray(rows[np.random.default_rng(seed + 2000).permutation(n)])


def _search(index, queries, expansion, sketch, frontier=0, **more):
    from usearch_amd import Tuning
    return index.search(queries, K, expansion=expansion, tuning=Tuning(sketch=sketch, frontier=frontier), **more)


def _same(a, b, what):
    assert np.array_equal(a.keys, b.keys), f"{what}: keys differ"
    assert util.same_float_bits(a.distances, b.distances), f"{what}: distance bits differ"
    assert np.array_equal(a.counts, b.counts), f"{what}: counts differ"
    assert np.array_equal(a.visited_per_query, b.visited_per_query), f"{what}: visited members differ"
    assert np.array_equal(a.computed_per_query, b.computed_per_query), f"{what}: computed distances differ"


def _same_as_oracle(got, image, queries, dtype, expansion, lanes, what, rows=QUERIES):
    keys, distances, counts, visited, computed = util.oracle_search(image, queries[:rows], K, dtype, expansion, lanes=lanes,
                                                                    frontier_in_top=got.stats.frontier == 2, threads=8)
    assert np.array_equal(got.keys[:rows], keys), f"{what}: keys differ from the oracle's"
    assert util.same_float_bits(got.distances[:rows], distances), f"{what}: distance bits differ from the oracle's"
    assert np.array_equal(got.counts[:rows], counts), what
    assert np.array_equal(got.visited_per_query[:rows], visited), f"{what}: visited members differ from the oracle's"
    assert np.array_equal(got.computed_per_query[:rows], computed), f"{what}: computed distances differ from the oracle's"


def _counters(on):
    return {"tested": int(on.stats.sketch_tested), "pruned": int(on.stats.sketch_pruned), "visited": int(on.visited_per_query.sum())}


def run_case(name):
    """One entry of CASES: every sameness check, → {"ef<expansion>_frontier<frontier>": counters}."""
    import usearch_amd
    kind, n, ndim, dtype, connectivity, expansions, frontiers, restated = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    rows = make_rows(kind, n, ndim, dtype, seed)
    built = usearch_amd.build(rows, "cos", dtype, keys=np.arange(n, dtype=np.uint64), seed=seed, connectivity=connectivity)
    image = built.save_buffer()
    built.close()
    index = usearch_amd.Index.restore(image)
    assert index.arrays.sketch == 1
    queries = make_rows(kind, QUERIES, ndim, dtype, seed + 1)
    counters = {}
    for expansion in expansions:
        for frontier in frontiers:
            what = f"{name}, expansion {expansion}, frontier {frontier}"
            off, on = _search(index, queries, expansion, OFF, frontier, dtype=dtype), _search(index, queries, expansion, ON, frontier, dtype=dtype)
            assert on.stats.variant != 5 and (frontier == 0 or on.stats.frontier == frontier), "one wave per query, the frontier asked for"
            assert off.stats.sketch_tested == 0 and off.stats.sketch_pruned == 0
            _same(on, off, what)
            _same_as_oracle(on, image, queries, dtype, expansion, index.lanes_per_row, what, restated)
            counters[f"ef{expansion}_frontier{frontier}"] = _counters(on)
            print(f"{what}: {counters[f'ef{expansion}_frontier{frontier}']}, survivors per hop "
                  f"{(on.stats.sketch_tested - on.stats.sketch_pruned) / max(1, int(on.visited_per_query.sum())):.2f}")
    return counters


def _tombstoned():
    from usearch_amd import Index
    n, ndim = 2500, 768
    removed = np.arange(0, n, 3)
    image, _, _ = util.build_image(n, ndim, "cos", "f16", seed=137, keys=np.arange(n, dtype=np.uint64), remove=removed)
    return Index.restore(image), image, removed, util.make_vectors(QUERIES, ndim, "f16", seed=138)


def run_tombstoned():
    index, image, removed, queries = _tombstoned()
    assert index.arrays.sketch == 1
    counters = {}
    for expansion in (16, 64):
        off, on = _search(index, queries, expansion, OFF), _search(index, queries, expansion, ON)
        _same(on, off, f"tombstones, expansion {expansion}")
        assert not np.isin(on.keys[on.counts > 0, 0], removed).any()
        _same_as_oracle(on, image, queries, "f16", expansion, index.lanes_per_row, f"tombstones, expansion {expansion}")
        counters[f"ef{expansion}"] = _counters(on)
    return counters


def run_filtered():
    """The heap frontier with `allowed`: members below the key bound are walked through and never returned."""
    from oracle import oraclebind
    index, image, _, queries = _tombstoned()
    n = 2500  # members of the image, tombstones included
    allowed = index.filter_key_range(n // 2, 2**64 - 2)
    oracle = oraclebind.OracleIndex(image)
    counters = {}
    for expansion in (16, 64):
        off, on = _search(index, queries, expansion, OFF, filter=allowed), _search(index, queries, expansion, ON, filter=allowed)
        _same(on, off, f"filtered, expansion {expansion}")
        assert on.stats.frontier == 1, "a filtered search walks with the heap frontier"
        for q in range(0, QUERIES, 20):
            found, keys, distances, visited, computed = oracle.filtered_search(
                queries[q], K, lambda key: key >= n // 2, dtype="f16", expansion=expansion, lanes=index.lanes_per_row, counters=True)
            assert int(on.counts[q]) == found and np.array_equal(on.keys[q], keys) and util.same_float_bits(on.distances[q], distances)
            assert int(on.visited_per_query[q]) == visited and int(on.computed_per_query[q]) == computed
        counters[f"ef{expansion}"] = _counters(on)
    return counters


def run_ties():
    """Every vector stored three times (tests/test_gpu_sketch.py: test_exact_ties_at_the_radius), lists of 32 cells."""
    import usearch_amd
    ndim, dtype = 768, "f16"
    unique = util.make_vectors(2000, ndim, dtype, seed=127)
    vectors = np.ascontiguousarray(np.concatenate([unique, unique, unique])[np.random.default_rng(128).permutation(6000)])
    built = usearch_amd.build(vectors, "cos", dtype, keys=np.arange(len(vectors), dtype=np.uint64), seed=127, connectivity=16)
    image = built.save_buffer()
    built.close()
    index = usearch_amd.Index.restore(image)
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=129)
    queries[:64] = unique[:64]
    counters = {}
    for expansion in (16, 64):
        for frontier in (1, 2):
            off, on = _search(index, queries, expansion, OFF, frontier), _search(index, queries, expansion, ON, frontier)
            _same(on, off, f"tripled rows, expansion {expansion}, frontier {frontier}")
            counters[f"ef{expansion}_frontier{frontier}"] = _counters(on)
    # (the oracle restates the heap's order among equal distances, the in-`top` frontier's only where they are distinct)
    _same_as_oracle(_search(index, queries, 64, ON, 1), image, queries, dtype, 64, index.lanes_per_row, "tripled rows, heap")
    return counters


SPECIAL = {"tombstoned_f16_m16": run_tombstoned, "filtered_f16_m16": run_filtered, "ties_f16_m16": run_ties}


def run(name):
    return SPECIAL[name]() if name in SPECIAL else run_case(name)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as file:
        return json.load(file)


def _survivors_per_hop(counters):
    return (counters["tested"] - counters["pruned"]) / counters["visited"]


@pytest.mark.parametrize("name", list(CASES) + list(SPECIAL))
def test_hop_changes_nothing(name, golden):
    counters = run(name)
    assert counters == golden[name], f"{name}: the sketch's counters differ from the ones recorded before the hop changed"
    for run_name, c in counters.items():
        assert 0 < c["tested"] and c["pruned"] <= c["tested"], run_name
        if name.startswith("lowrank"):
            assert c["pruned"] > 0 and _survivors_per_hop(c) < 8, f"{name}, {run_name}: low-rank rows must take the one-row path"
        elif name.startswith("gaussian"):
            assert _survivors_per_hop(c) > 8, f"{name}, {run_name}: Gaussian rows must take the two-row path"
        elif name.startswith("mixture"):
            # neither pure kind: the share pruned lies well away from the Gaussian rows' (recorded: 0.003) and from the low-rank
            # rows' (0.64 … 0.71) — recorded for the mixtures: 0.25 … 0.40 — so hops that prune nearly everything and hops that prune
            # nothing both occur; and the mean number of survivors is over 8 while a quarter and more of the candidates are pruned:
            # hops on either side of the one-round limit
            assert 0.1 < c["pruned"] / c["tested"] < 0.6, f"{name}, {run_name}: a mixture prunes a part, not nearly all or nearly nothing"
            assert _survivors_per_hop(c) > 8, f"{name}, {run_name}"
            if name == "mixture_f16_m16":  # same lists, same expansions as the two pure kinds: strictly between them
                low, high = golden["lowrank_f16_m16"][run_name], golden["gaussian_f16_m16"][run_name]
                assert _survivors_per_hop(low) < _survivors_per_hop(c) < _survivors_per_hop(high), f"{name}, {run_name}"
