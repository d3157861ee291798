"""The sketch of long cos rows (usearch_amd/csrc/sketch.hpp) on the device: a walk that skips the rows of candidates the sketch
proves too far must give, bit for bit, what the walk without it gives — keys, distances, counts and both traversal counters —
and what the oracle gives, with either frontier. Batches of 640 queries, so that the one-wave kernel runs and not the team
build; expansions 16 and 64, so that `top` fills within the first hops and nearly every later hop takes the new path."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

QUERIES, K = 640, 10
OFF, ON = 1, 2  # usearch_amd_tuning_t::sketch


def _search(index, queries, expansion, sketch, frontier=0, **more):
    from usearch_amd import Tuning
    return index.search(queries, K, expansion=expansion, tuning=Tuning(sketch=sketch, frontier=frontier), **more)


def _same(a, b, what):
    assert np.array_equal(a.keys, b.keys), f"{what}: keys differ"
    assert util.same_float_bits(a.distances, b.distances), f"{what}: distance bits differ"
    assert np.array_equal(a.counts, b.counts), f"{what}: counts differ"
    assert np.array_equal(a.visited_per_query, b.visited_per_query), f"{what}: visited members differ"
    assert np.array_equal(a.computed_per_query, b.computed_per_query), f"{what}: computed distances differ"


def _same_as_oracle(got, image, queries, dtype, expansion, lanes, what):
    keys, distances, counts, visited, computed = util.oracle_search(image, queries, K, dtype, expansion, lanes=lanes,
                                                                    frontier_in_top=got.stats.frontier == 2, threads=8)
    assert np.array_equal(got.keys, keys), f"{what}: keys differ from the oracle's"
    assert util.same_float_bits(got.distances, distances), f"{what}: distance bits differ from the oracle's"
    assert np.array_equal(got.counts, counts), what
    assert np.array_equal(got.visited_per_query, visited), f"{what}: visited members differ from the oracle's"
    assert np.array_equal(got.computed_per_query, computed), f"{what}: computed distances differ from the oracle's"


def _built(n, ndim, dtype, seed, clustered=True, vectors=None):
    """An index built on the device and loaded afresh from its serialized image → (index, image)."""
    import usearch_amd
    if vectors is None:
        vectors = util.make_vectors(n, ndim, dtype, seed=seed, clustered=clustered)
    built = usearch_amd.build(vectors, "cos", dtype, keys=np.arange(len(vectors), dtype=np.uint64), seed=seed)
    image = built.save_buffer()
    built.close()
    return usearch_amd.Index.restore(image), image


@pytest.mark.parametrize("n,ndim,dtype,eligible", [(20000, 768, "f16", True), (20000, 768, "f32", True), (8000, 256, "f32", False)])
def test_sketch_changes_nothing_but_the_rows_fetched(n, ndim, dtype, eligible):
    index, image = _built(n, ndim, dtype, seed=7)
    assert bool(index.arrays.sketch) == eligible
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=8)
    for expansion in (16, 64):
        for frontier in (1, 2):
            off = _search(index, queries, expansion, OFF, frontier)
            on = _search(index, queries, expansion, ON, frontier)
            what = f"{n} x {ndim} {dtype}, expansion {expansion}, frontier {frontier}"
            assert off.stats.variant != 5 and on.stats.frontier == frontier, "one wave per query, the frontier asked for"
            assert off.stats.sketch_tested == 0 and off.stats.sketch_pruned == 0
            _same(on, off, what)
            _same_as_oracle(on, image, queries, dtype, expansion, index.lanes_per_row, what)
            print(f"{what}: {on.stats.sketch_pruned} of {on.stats.sketch_tested} tested candidates pruned, "
                  f"{int(on.computed_per_query.sum())} computed")
            if eligible:
                assert on.stats.sketch_pruned > 0, "low-rank data: the sketch must prune"
                assert on.stats.sketch_pruned <= on.stats.sketch_tested <= int(on.computed_per_query.sum())
            else:
                assert on.stats.sketch_tested == 0, "rows under 1 536 bytes carry no sketch"


def test_auto_mode_gives_up_on_gaussian_rows():
    """i.i.d. Gaussian rows leave 0.96 of their norm outside any 62 directions: nothing can be pruned, and after the first batch
    of at least 1 024 queries the snapshot walks without its sketch."""
    n, ndim, dtype, queries_count = 8000, 768, "f16", 1024
    index, image = _built(n, ndim, dtype, seed=17, clustered=False)
    assert index.arrays.sketch == 1
    queries = util.make_vectors(queries_count, ndim, dtype, seed=18, clustered=False)
    off = _search(index, queries, 64, OFF)
    forced = _search(index, queries, 64, ON)
    assert forced.stats.sketch_tested > 0 and forced.stats.sketch_pruned * 4 < forced.stats.sketch_tested
    assert index.arrays.sketch == 1, "a forced call is not judged"
    auto = _search(index, queries, 64, 0)
    assert auto.stats.sketch_tested > 0
    _same(forced, off, "gaussian, forced")
    _same(auto, off, "gaussian, auto")
    _same_as_oracle(auto, image, queries, dtype, 64, index.lanes_per_row, "gaussian, auto")
    assert index.arrays.sketch == 0, "auto mode must have switched the sketch off after the first batch"
    after = _search(index, queries, 64, 0)
    assert after.stats.sketch_tested == 0
    _same(after, off, "gaussian, after the sketch was dropped")


def test_exact_ties_at_the_radius():
    """Every vector stored three times: the radius is met exactly by the copies of what `top` holds."""
    ndim, dtype = 768, "f16"
    unique = util.make_vectors(2000, ndim, dtype, seed=27)
    vectors = np.ascontiguousarray(np.concatenate([unique, unique, unique])[np.random.default_rng(28).permutation(6000)])
    index, image = _built(len(vectors), ndim, dtype, seed=27, vectors=vectors)
    queries = util.make_vectors(QUERIES, ndim, dtype, seed=29)
    queries[:64] = unique[:64]
    for expansion in (16, 64):
        for frontier in (1, 2):
            off, on = _search(index, queries, expansion, OFF, frontier), _search(index, queries, expansion, ON, frontier)
            _same(on, off, f"tripled rows, expansion {expansion}, frontier {frontier}")
            assert on.stats.sketch_pruned > 0
    # (the oracle restates the heap's order among equal distances, the in-`top` frontier's only where they are distinct)
    _same_as_oracle(_search(index, queries, 64, ON, 1), image, queries, dtype, 64, index.lanes_per_row, "tripled rows, heap")


@pytest.fixture(scope="module")
def tombstoned():
    from usearch_amd import Index
    n, ndim = 2500, 768
    removed = np.arange(0, n, 3)
    image, vectors, _ = util.build_image(n, ndim, "cos", "f16", seed=37, keys=np.arange(n, dtype=np.uint64), remove=removed)
    return Index.restore(image), image, removed, util.make_vectors(QUERIES, ndim, "f16", seed=38)


def test_tombstoned_index(tombstoned):
    index, image, removed, queries = tombstoned
    assert index.arrays.sketch == 1
    for expansion in (16, 64):
        off, on = _search(index, queries, expansion, OFF), _search(index, queries, expansion, ON)
        _same(on, off, f"tombstones, expansion {expansion}")
        assert on.stats.sketch_pruned > 0 and not np.isin(on.keys[on.counts > 0, 0], removed).any()
        _same_as_oracle(on, image, queries, "f16", expansion, index.lanes_per_row, f"tombstones, expansion {expansion}")


def test_filtered_search(tombstoned):
    from oracle import oraclebind
    index, image, _, queries = tombstoned
    n = 2500  # members of the fixture's image, tombstones included
    allowed = index.filter_key_range(n // 2, 2**64 - 2)
    oracle = oraclebind.OracleIndex(image)
    for expansion in (16, 64):
        off = _search(index, queries, expansion, OFF, filter=allowed)
        on = _search(index, queries, expansion, ON, filter=allowed)
        _same(on, off, f"filtered, expansion {expansion}")
        assert on.stats.sketch_pruned > 0
        for q in range(0, QUERIES, 20):
            found, keys, distances, visited, computed = oracle.filtered_search(
                queries[q], K, lambda key: key >= n // 2, dtype="f16", expansion=expansion, lanes=index.lanes_per_row, counters=True)
            assert int(on.counts[q]) == found and np.array_equal(on.keys[q], keys) and util.same_float_bits(on.distances[q], distances)
            assert int(on.visited_per_query[q]) == visited and int(on.computed_per_query[q]) == computed


def test_extended_and_updated_index_keeps_a_valid_sketch():
    """Members appended to a built index get records under the directions it already has (the first append moves the records to a
    larger array, the second fits the room the first left); a member overwritten in place makes the sketch anew. After each step the
    snapshot itself must prune, answer with the sketch as without it, and answer as the same index loaded afresh does."""
    import usearch_amd
    ndim, first, step = 768, 4000, 300
    vectors = util.make_vectors(first + 2 * step, ndim, "f16", seed=47)
    built = usearch_amd.build(vectors[:first], "cos", "f16", keys=np.arange(first, dtype=np.uint64), seed=47)
    index = built.index
    queries = util.make_vectors(QUERIES, ndim, "f16", seed=48)
    replacements = util.make_vectors(3, ndim, "f16", seed=49)
    queries[:3] = replacements

    def check(what, members):
        assert len(index) == members and index.arrays.sketch == 1, what
        on, off = _search(index, queries, 64, ON), _search(index, queries, 64, OFF)
        _same(on, off, what)
        assert on.stats.sketch_pruned > 0 and off.stats.sketch_tested == 0, what
        fresh = usearch_amd.Index.restore(built.save_buffer())
        _same(_search(fresh, queries, 64, ON), on, f"{what}, against a fresh load")
        return on

    check("as built", first)
    built.extend(vectors[first:first + step], keys=np.arange(first, first + step, dtype=np.uint64))
    assert (check("extended once", first + step).keys >= first).any(), "the added members must be found"
    built.extend(vectors[first + step:], keys=np.arange(first + step, first + 2 * step, dtype=np.uint64))
    assert (check("extended twice", first + 2 * step).keys >= first + step).any()
    slots, renamed = np.array([5, 1000, first + 100], dtype=np.uint32), np.array([90005, 91000, 94100], dtype=np.uint64)
    built.update(slots, replacements, renamed)
    updated = check("three members overwritten", first + 2 * step)
    assert np.array_equal(updated.keys[:3, 0], renamed), "an overwritten member is found under its new row"
    built.close()


def test_index_extended_after_load_answers_like_a_fresh_load():
    """The drop-in ABI, the surface that adds to a LOADED index: the first addition rebuilds the graph on the device (a new sketch),
    additions after a search extend it in place (records appended). The result must answer as the same index loaded afresh does."""
    import usearch_amd
    from tests.test_gpu_dropin import METRIC, SCALAR, Options
    ndim, first, added = 768, 4000, 300
    vectors = util.make_vectors(first + added, ndim, "f16", seed=47)
    built = usearch_amd.build(vectors[:first], "cos", "f16", keys=np.arange(first, dtype=np.uint64), seed=47)
    image = built.save_buffer()
    built.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = C.CDLL(os.path.join(root, "usearch_amd", "lib", "libusearch_c.so"))
    err_p = C.POINTER(C.c_char_p)
    L.usearch_init.restype = C.c_void_p
    L.usearch_init.argtypes = [C.POINTER(Options), err_p]
    L.usearch_load_buffer.argtypes = L.usearch_save_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_reserve.argtypes = [C.c_void_p, C.c_size_t, err_p]
    L.usearch_change_expansion_search.argtypes = [C.c_void_p, C.c_size_t, err_p]
    L.usearch_add.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, err_p]
    L.usearch_serialized_length.restype = C.c_size_t
    L.usearch_serialized_length.argtypes = L.usearch_free.argtypes = [C.c_void_p, err_p]
    L.usearch_search_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, err_p]
    err = C.c_char_p()

    def ok():
        assert not err.value, err.value

    options = Options(METRIC["cos"], None, SCALAR["f16"], ndim, 16, 128, 64, False)
    handle = L.usearch_init(C.byref(options), C.byref(err)); ok()
    L.usearch_load_buffer(handle, C.c_void_p(image.ctypes.data), image.size, C.byref(err)); ok()
    L.usearch_change_expansion_search(handle, 64, C.byref(err)); ok()
    queries = util.make_vectors(QUERIES, ndim, "f16", seed=48)

    def search_many():
        keys, distances = np.zeros((QUERIES, K), dtype=np.uint64), np.zeros((QUERIES, K), dtype=np.float32)
        counts = np.zeros(QUERIES, dtype=np.uint64)
        L.usearch_search_many(handle, C.c_void_p(queries.ctypes.data), SCALAR["f16"], QUERIES, queries.strides[0], K,
                              C.c_void_p(keys.ctypes.data), keys.strides[0], C.c_void_p(distances.ctypes.data), distances.strides[0],
                              C.c_void_p(counts.ctypes.data), None, None, C.byref(err)); ok()
        return keys, distances, counts

    search_many()  # the loaded snapshot, sketch and all, exists before anything is added
    L.usearch_reserve(handle, first + added, C.byref(err)); ok()
    for i in range(first, first + added // 2):
        L.usearch_add(handle, i, C.c_void_p(vectors[i].ctypes.data), SCALAR["f16"], C.byref(err)); ok()
    search_many()  # links the first half: one build over everything
    for i in range(first + added // 2, first + added):
        L.usearch_add(handle, i, C.c_void_p(vectors[i].ctypes.data), SCALAR["f16"], C.byref(err)); ok()
    keys, distances, counts = search_many()  # links the second half: the graph is extended in place
    assert (keys >= first).any(), "the added members must be found"
    length = L.usearch_serialized_length(handle, C.byref(err)); ok()
    extended = np.zeros(length, dtype=np.uint8)
    L.usearch_save_buffer(handle, C.c_void_p(extended.ctypes.data), length, C.byref(err)); ok()
    L.usearch_free(handle, C.byref(err)); ok()

    fresh = usearch_amd.Index.restore(extended)
    assert len(fresh) == first + added and fresh.arrays.sketch == 1
    on, off = _search(fresh, queries, 64, ON), _search(fresh, queries, 64, OFF)
    _same(on, off, "fresh load of the extended index")
    assert on.stats.sketch_pruned > 0
    assert np.array_equal(keys, on.keys) and util.same_float_bits(distances, on.distances) and np.array_equal(counts, on.counts)
