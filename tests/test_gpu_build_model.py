"""The link kernels (usearch_amd/csrc/build_kernels.hpp: `build_select_kernel`, `build_reverse_kernel`, `refine_forward`) and the
two search modes only the builder uses (`beam_level` > 0; `reference_frontier` with `query_ids`) against a plain model of the
rules they state (tests/build_model.py, pinned to the compiled reference by tests/test_build_model.py).

The builder is deterministic by design — a batch is linked against the graph as it stood before the batch, appends go in
ascending requester order — so the model predicts EVERY neighbour list of a GPU-built graph exactly, in order, and the image is
compared with it list for list. One condition: no inbox overflows (which request is parked is decided by atomic order). A node
files at most one request per target and pass, so `max_batch` ≤ the inbox capacity (min(32, 64 - max(M, M0)) below 64, 32 from
64 on) rules that out: every case here builds with `max_batch = 16`.

Distances come from the oracle in the kernels' summation layout (`lanes_per_row`; bit-exact, tests/test_gpu_distances.py) with
the kernels' operand order (the staged row is the query). The data is continuous and checked to be free of deciding ties: a
`build_model.Tie` fails the case, it is never skipped.
"""
import time

import numpy as np
import pytest

import usearch_amd
from oracle import oraclebind
from tests import build_model, util

pytestmark = pytest.mark.gpu

MAX_BATCH = 16
DEFAULT_DIVISOR = 16  # build.hpp `build_config_t::batch_divisor`

# `divisor` 1: batches of 16 from the 16th member on, so several members of one pass pick the same targets (append order, re-prunes
# with more than one requester). `candidates`: the longest candidate list a select step must have received (the live-candidate
# bitmap of `refine_forward` has one 64-bit word per 64 of them). `reprune`: how many candidates — old neighbours + requesters —
# the widest re-prune must at least have sorted. `requesters`: … and how many requesters at least met in one re-pruned list.
# `clusters`: the rows are Gaussian clusters whose centres are members themselves (the first rows). A centre is the nearest
# neighbour of most of its cluster, so its list fills up — 64 or 128 cells — within a few hundred members; among unstructured rows
# in 16 dimensions the fullest list holds about 110 neighbours after 900 members.
CASES = {
    # name: (metric, dtype, ndim, n, M, M0, expansion_add, divisor, seed, what the model must have gone through)
    "one_word_ragged": ("l2sq", "f32", 16, 500, 4, 8, 40, 0, 101, dict(candidates=40, upper_pass=2)),
    "one_full_word": ("l2sq", "f32", 16, 500, 4, 8, 64, 1, 102, dict(candidates=64, upper_pass=2, requesters=2)),
    "two_words_ragged": ("l2sq", "f32", 16, 500, 4, 8, 100, 0, 103, dict(candidates=100, upper_pass=2)),
    "two_full_words": ("l2sq", "f32", 16, 400, 4, 8, 128, 1, 104, dict(candidates=128, upper_pass=2, requesters=2)),
    "five_words": ("l2sq", "f32", 16, 400, 8, 16, 300, 0, 105, dict(candidates=300, upper_pass=2)),
    "list_and_inbox_fill_a_wave": ("cos", "f32", 24, 600, 16, 32, 64, 1, 106, dict(candidates=64, reprune=34, requesters=2)),
    "inbox_of_16": ("cos", "f32", 24, 600, 24, 48, 64, 1, 107, dict(candidates=64, reprune=50, requesters=2)),
    "lds_two_per_lane": ("l2sq", "f32", 16, 700, 32, 64, 80, 1, 108, dict(candidates=80, reprune=66, requesters=2, clusters=4)),
    "lds_three_per_lane": ("l2sq", "f32", 16, 900, 64, 128, 160, 1, 2, dict(candidates=160, reprune=130, requesters=2, clusters=4)),
    "long_rows": ("cos", "f16", 768, 300, 8, 16, 64, 0, 110, dict(candidates=64, upper_pass=2)),
    "ragged_dimension": ("cos", "f32", 97, 400, 8, 16, 48, 1, 211, dict(candidates=48, upper_pass=2, requesters=2)),
    "connectivity_base": ("ip", "f32", 40, 500, 16, 20, 64, 1, 112, dict(candidates=64, requesters=2)),
}


def case_vectors(metric: str, dtype: str, ndim: int, n: int, seed: int, clusters: int = 0) -> np.ndarray:
    if clusters:
        rng = np.random.default_rng(seed)
        centres = 4.0 * rng.standard_normal((clusters, ndim))
        vectors = centres[rng.integers(0, clusters, n)] + rng.standard_normal((n, ndim))
        vectors[:clusters] = centres
        return np.ascontiguousarray(vectors.astype(util.NP_DTYPE[dtype]))
    vectors = util.make_vectors(n, ndim, dtype, seed=seed, clustered=False)
    if metric == "ip":  # unit rows
        vectors = (vectors / np.linalg.norm(vectors, axis=1, keepdims=True)).astype(vectors.dtype)
    return np.ascontiguousarray(vectors)


def check_reach(model: build_model.BuildResult, reach: dict):
    """A case must go through the branch it is named for — seen from the model's side, whose steps are the kernels'."""
    assert model.repruned_lists > 0
    assert model.most_candidates == reach["candidates"], (model.most_candidates, reach)
    assert model.widest_upper_pass >= reach.get("upper_pass", 0), (model.widest_upper_pass, reach)
    assert model.widest_reprune >= reach.get("reprune", 0), (model.widest_reprune, reach)
    assert model.most_requesters_repruned >= reach.get("requesters", 0), (model.most_requesters_repruned, reach)
    if reach.get("requesters", 0) >= 2:  # appends of more than one requester as well
        assert model.most_requesters >= 2


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_built_graph_equals_the_model_list_for_list(name):
    metric, dtype, ndim, n, m, m0, expansion_add, divisor, seed, reach = CASES[name]
    assert MAX_BATCH <= (min(32, 64 - max(m, m0)) if max(m, m0) < 64 else 32), "an inbox could overflow: not deterministic"
    vectors = case_vectors(metric, dtype, ndim, n, seed, reach.get("clusters", 0))

    started = time.perf_counter()
    built = usearch_amd.build(vectors, metric, dtype, connectivity=m, connectivity_base=m0, expansion_add=expansion_add,
                              max_batch=MAX_BATCH, batch_divisor=divisor)
    stats = built.stats
    image = built.save_buffer()
    gpu_seconds = time.perf_counter() - started

    oracle = oraclebind.OracleIndex(image)
    assert len(oracle) == n and oracle.ix.connectivity == m and oracle.ix.connectivity_base == m0
    levels = [oracle.level(slot) for slot in range(n)]
    dist = util.slot_distance(vectors, metric, dtype, ndim, lanes=built.index.lanes_per_row)
    started = time.perf_counter()
    model = build_model.build(vectors, levels, dist, m, m0, expansion_add, MAX_BATCH, divisor or DEFAULT_DIVISOR)
    model_seconds = time.perf_counter() - started
    print(f"{name}: GPU build + save {gpu_seconds:.3f} s, model {model_seconds:.2f} s; max level {model.max_level}, "
          f"{model.batches} batches, {model.passes} passes, {model.repruned_lists} re-pruned lists, "
          f"candidates ≤ {model.most_candidates}, widest re-prune {model.widest_reprune}, "
          f"requesters ≤ {model.most_requesters} ({model.most_requesters_repruned} re-pruned)")
    check_reach(model, reach)

    for slot in range(n):
        for level in range(levels[slot] + 1):
            got, expected = oracle.neighbors(slot, level).tolist(), model.graph[slot][level]
            assert got == expected, (f"{name}: first difference at slot {slot}, level {level}: the GPU wrote {got}, "
                                     f"the model says {expected}")
    assert (int(oracle.ix.entry_slot), int(oracle.ix.max_level)) == (model.entry, model.max_level)
    assert (stats.batches, stats.passes, stats.repruned_lists) == (model.batches, model.passes, model.repruned_lists)
    assert stats.max_level == model.max_level
    assert stats.dropped_requests == 0 and stats.refiled_requests == 0
