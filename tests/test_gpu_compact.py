"""`isolate` and `compact` on the device (usearch_amd/csrc/compact.hip) against the plain model of tests/compact_model.py.

Every case: build on the device → `save_buffer` (image A) → remove → the operation → `save_buffer` (image B); both images are read
with the oracle's parser and B must be the model applied to A, list for list and in order, with the model's counts. After a
`compact` the searches must agree three ways: with the oracle on image B bit for bit, with the reference loaded from image B, and
with a fresh `Index.restore(B)`.

The shapes are the smallest at which each branch of the list kernel and of the row mover can go wrong."""
import numpy as np
import pytest

import usearch_amd
from oracle import refbind
from tests import compact_model, util
from tests import test_gpu_build_model as build_cases
from tests import test_gpu_search_parity as parity

pytestmark = pytest.mark.gpu

FREE = compact_model.FREE_KEY
K, EXPANSION = 10, 64


def scan_chunk() -> int:
    return int(usearch_amd.library().usearch_amd_compact_scan_chunk())


def random_slots(n: int, share: float, seed: int) -> np.ndarray:
    return np.sort(np.random.default_rng(seed).choice(n, int(n * share), replace=False)).astype(np.uint32)


def long_runs(n: int) -> np.ndarray:
    """Slots 0…199, the last slot and a run of 130 in the middle: runs that cross the scan's chunks, the first and the last slot."""
    return np.unique(np.concatenate([np.arange(200), np.arange(n // 2, n // 2 + 130), [n - 1]])).astype(np.uint32)


# name: (metric, dtype, ndim, n, M, M0, clusters, removed(n) → slots, staging rows (0 = default))
# (the two `ragged_stride` cases have rows of 388 and 33 bytes: the engine pads the pitch of stored rows to a multiple of 16 bytes, so
# the mover has no tail path — what they reach is a pitch that differs from the row's own length, moved through 3-row chunks)
CASES = {
    "narrow_lists": ("l2sq", "f32", 16, 500, 4, 8, 0, lambda n: np.arange(0, n, 2, dtype=np.uint32), 0),
    "one_wave_exactly": ("cos", "f32", 24, 600, 32, 64, 0, lambda n: random_slots(n, 0.30, 1), 0),
    "two_tiles": ("l2sq", "f32", 16, 900, 64, 128, 4, lambda n: random_slots(n, 0.30, 2), 0),
    "odd_base": ("ip", "f32", 40, 500, 16, 20, 0, lambda n: random_slots(n, 0.10, 3), 0),
    "inline_rows": ("hamming", "b1", 128, 700, 16, 32, 0, lambda n: random_slots(n, 0.25, 4), 0),
    "long_rows": ("cos", "f16", 768, 300, 8, 16, 0, lambda n: random_slots(n, 0.25, 5), 8),
    "ragged_stride_f32": ("cos", "f32", 97, 400, 8, 16, 0, lambda n: random_slots(n, 0.25, 6), 3),
    "ragged_stride_i8": ("cos", "i8", 33, 400, 8, 16, 0, lambda n: random_slots(n, 0.25, 7), 3),
    "long_runs": ("l2sq", "f32", 16, None, 8, 16, 0, long_runs, 0),  # n = 1 + 4 scan chunks
}


def case_inputs(name):
    metric, dtype, ndim, n, m, m0, clusters, removed, staging_rows = CASES[name]
    if n is None:
        n = 1 + 4 * scan_chunk()
    if dtype == "b1":
        vectors = util.make_vectors(n, ndim, dtype, seed=31)
    else:
        vectors = build_cases.case_vectors(metric, dtype, ndim, n, seed=2 if clusters else 31, clusters=clusters)
    return metric, dtype, ndim, n, m, m0, vectors, removed(n), staging_rows


def device_build(vectors, metric, dtype, m, m0):
    keys = np.arange(len(vectors), dtype=np.uint64) + 1000
    return usearch_amd.build(vectors, metric, dtype, keys=keys, connectivity=m, connectivity_base=m0, expansion_add=64)


def model_of(image_a, removed):
    """Image A with the removed members' keys turned into tombstones, as `remove` leaves them."""
    lists, levels, keys, entry, max_level = compact_model.read_image(image_a)
    for slot in removed:
        keys[int(slot)] = FREE
    return lists, levels, keys, entry, max_level


def assert_image_is(image, lists, keys, levels, entry, max_level, what):
    got_lists, got_levels, got_keys, got_entry, got_max_level = compact_model.read_image(image)
    assert got_keys == keys, f"{what}: keys differ"
    assert got_levels == levels, f"{what}: levels differ"
    for slot, (got, expected) in enumerate(zip(got_lists, lists)):
        assert got == expected, f"{what}: first difference at slot {slot}: the device wrote {got}, the model says {expected}"
    assert (got_entry, got_max_level) == (entry, max_level), f"{what}: entry point / top level"


def queries_for(vectors, dtype):
    """Stored rows, removed and surviving ones alike (the first hit of a survivor's row is itself), and rows between them."""
    rng = np.random.default_rng(77)
    picked = vectors[rng.choice(len(vectors), 48, replace=False)]
    if dtype in ("b1", "i8"):
        return np.ascontiguousarray(picked)
    mixed = (picked[:24].astype(np.float32) + picked[24:].astype(np.float32)) / 2
    return np.ascontiguousarray(np.concatenate([picked[:24], mixed.astype(picked.dtype)]))


def assert_searches_agree(built, image_b, vectors, metric, dtype, what):
    """After a compact: the oracle on image B bit for bit, the reference loaded from B, and a fresh restore of B."""
    queries = queries_for(vectors, dtype)
    got = parity.check_against_oracle(built.index, image_b, queries, K, dtype, EXPANSION)
    reference = refbind.RefIndex.from_buffer(image_b, dtype=dtype)
    assert len(reference) == len(built.index)
    reference.expansion_search = EXPANSION
    rkeys, rdists, rcounts, rvisited, rcomputed = reference.search(queries, K, dtype=dtype, threads=1)
    if util.exact_pair(metric, dtype):
        assert np.array_equal(got.keys, rkeys) and util.same_float_bits(got.distances, rdists), f"{what}: the reference disagrees"
        assert np.array_equal(got.counts, rcounts)
        assert np.array_equal(got.visited_per_query, rvisited) and np.array_equal(got.computed_per_query, rcomputed)
    else:
        util.assert_float_parity(got.keys, got.distances, got.counts,
                                 lambda batch, wanted: reference.search(batch, wanted, dtype=dtype, threads=1), queries, K, dtype, what=what)
    fresh = usearch_amd.Index.restore(image_b).search(queries, K, expansion=EXPANSION, dtype=dtype)
    assert fresh.keys.tobytes() == got.keys.tobytes() and fresh.distances.tobytes() == got.distances.tobytes(), \
        f"{what}: a fresh load of the saved image answers differently"
    assert np.array_equal(fresh.counts, got.counts)
    assert np.array_equal(fresh.visited_per_query, got.visited_per_query) and np.array_equal(fresh.computed_per_query, got.computed_per_query)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_isolate_equals_the_model_list_for_list(name):
    metric, dtype, ndim, n, m, m0, vectors, removed, _ = case_inputs(name)
    built = device_build(vectors, metric, dtype, m, m0)
    image_a = built.save_buffer()
    lists, levels, keys, entry, max_level = model_of(image_a, removed)
    expected, erased = compact_model.isolate(lists, keys)
    assert erased > 0, "the case removes nobody's neighbour"
    assert built.remove(removed) == len(removed)
    pruned = built.isolate()
    stats = built.index.compact_stats
    print(f"{name}: isolate erased {pruned} cells (model {erased}); {stats}")
    assert pruned == erased and stats["removed_members"] == len(removed) and stats["survivors"] == n - len(removed)
    assert_image_is(built.save_buffer(), expected, keys, levels, entry, max_level, f"{name}: isolate")
    assert built.isolate() == 0, "a second isolate finds nothing left to erase"


@pytest.mark.parametrize("name", list(CASES))
def test_compact_equals_the_model_and_searches_like_a_fresh_load(name):
    metric, dtype, ndim, n, m, m0, vectors, removed, staging_rows = case_inputs(name)
    built = device_build(vectors, metric, dtype, m, m0)
    image_a = built.save_buffer()
    model = compact_model.compact(*model_of(image_a, removed)[:4])
    if name == "two_tiles":  # the case is about lists wider than a wave that really fill
        assert max(len(per_level[0]) for per_level in model_of(image_a, [])[0]) > 64
    built.remove(removed)
    slot_map = built.compact(staging_bytes=staging_rows * built.index.row_stride, slot_map=True)
    stats = built.index.compact_stats
    print(f"{name}: {stats}")
    assert slot_map.tolist() == model["slot_map"]
    assert stats["pruned_edges"] == model["pruned_edges"] and stats["removed_members"] == model["removed_members"] == len(removed)
    assert stats["survivors"] == n - len(removed) == len(built.index)
    assert (stats["new_entry_slot"], stats["new_max_level"]) == (model["entry"], model["max_level"])
    if staging_rows:  # a bound this low makes a small index take many chunks
        first_moved = int(removed.min())
        assert stats["chunks"] == -(-(n - len(removed) - first_moved) // staging_rows) and stats["chunks"] > 10
    image_b = built.save_buffer()
    assert_image_is(image_b, model["lists"], model["keys"], model["levels"], model["entry"], model["max_level"], f"{name}: compact")
    survivors = np.setdiff1d(np.arange(n), removed)
    stored = np.frombuffer(image_b[8:8 + len(survivors) * vectors[0].nbytes].tobytes(), dtype=vectors.dtype).reshape(len(survivors), -1)
    assert np.array_equal(stored.view(np.uint8), vectors[survivors].view(np.uint8)), "the rows did not follow their members"
    assert built.index.inline_rows == (name == "inline_rows")
    assert_searches_agree(built, image_b, vectors, metric, dtype, name)


@pytest.mark.parametrize("name", ["narrow_lists", "long_rows"])
def test_compact_when_the_entry_point_and_the_whole_top_level_leave(name):
    metric, dtype, ndim, n, m, m0, vectors, _, staging_rows = case_inputs(name)
    built = device_build(vectors, metric, dtype, m, m0)
    image_a = built.save_buffer()
    lists, levels, keys, entry, max_level = compact_model.read_image(image_a)
    assert max_level >= 1
    removed = np.array([slot for slot in range(n) if levels[slot] == max_level], dtype=np.uint32)
    assert entry in removed.tolist()
    model = compact_model.compact(*model_of(image_a, removed)[:4])
    assert model["max_level"] < max_level, "the top level was removed whole"
    built.remove(removed)
    assert built.compact(staging_bytes=staging_rows * built.index.row_stride) == len(removed)
    stats = built.index.compact_stats
    assert (stats["new_entry_slot"], stats["new_max_level"]) == (model["entry"], model["max_level"])
    assert built.index.max_level == model["max_level"]
    image_b = built.save_buffer()
    assert_image_is(image_b, model["lists"], model["keys"], model["levels"], model["entry"], model["max_level"], f"{name}: entry removed")
    assert_searches_agree(built, image_b, vectors, metric, dtype, name)


def test_compact_of_nothing_moves_nothing():
    vectors = build_cases.case_vectors("cos", "f32", 24, 300, seed=41)
    built = device_build(vectors, "cos", "f32", 8, 16)
    image_a, arrays = built.save_buffer(), built.index.arrays
    before = (arrays.vectors, arrays.level0, arrays.keys)
    assert built.compact() == 0
    stats = built.index.compact_stats
    assert stats["survivors"] == 300 and stats["moved_bytes"] == 0 and stats["chunks"] == 0 and stats["pruned_edges"] == 0
    after = built.index.arrays
    assert before == (after.vectors, after.level0, after.keys), "a compact of nothing reallocated"
    assert built.save_buffer().tobytes() == image_a.tobytes()
    assert built.compact(slot_map=True).tolist() == list(range(300))


def test_compact_of_everything_leaves_an_index_that_takes_members_again():
    vectors = build_cases.case_vectors("cos", "f32", 24, 350, seed=42)
    built = device_build(vectors[:300], "cos", "f32", 8, 16)
    built.remove(np.arange(300, dtype=np.uint32))
    assert built.compact() == 300
    assert len(built.index) == 0
    empty = built.index.search(vectors[:4], K, expansion=EXPANSION)
    assert not empty.counts.any()
    built.extend(vectors[300:], keys=np.arange(50, dtype=np.uint64) + 5000)
    assert len(built.index) == 50
    image = built.save_buffer()
    got = parity.check_against_oracle(built.index, image, np.ascontiguousarray(vectors[300:320]), K, "f32", EXPANSION)
    assert np.array_equal(got.keys[:, 0], np.arange(20, dtype=np.uint64) + 5000)
    assert len(refbind.RefIndex.from_buffer(image, dtype="f32")) == 50


def test_extend_and_update_go_on_after_a_compact():
    vectors = build_cases.case_vectors("l2sq", "f32", 16, 600, seed=43)
    built = device_build(vectors[:500], "l2sq", "f32", 8, 16)
    removed = random_slots(500, 0.2, 8)
    built.remove(removed)
    built.compact()
    built.extend(vectors[500:], keys=np.arange(100, dtype=np.uint64) + 9000)
    built.update(np.array([3], dtype=np.uint32), vectors[499:500] + 0.25, np.array([77777], dtype=np.uint64))
    assert len(built.index) == 500
    image = built.save_buffer()
    got = parity.check_against_oracle(built.index, image, np.ascontiguousarray(vectors[500:540]), K, "f32", EXPANSION)
    assert (got.keys[:, 0] == np.arange(40, dtype=np.uint64) + 9000).mean() >= 0.9  # an approximate walk over thinned lists
    assert len(refbind.RefIndex.from_buffer(image, dtype="f32")) == 500


def test_compact_gives_the_fast_kernels_back():
    """With tombstones: the heap frontier and no build cut for plain batches. After `compact`: whatever a fresh device build of the
    survivors runs for the same batch."""
    vectors = build_cases.case_vectors("cos", "f32", 24, 600, seed=44)
    queries = np.ascontiguousarray(vectors[:256])
    built = device_build(vectors, "cos", "f32", 16, 32)
    removed = random_slots(600, 0.3, 9)
    built.remove(removed)
    with_tombstones = built.index.search(queries, K, expansion=EXPANSION)
    assert (with_tombstones.stats.frontier, with_tombstones.stats.plain) == (1, 0)
    built.compact()
    after = built.index.search(queries, K, expansion=EXPANSION)
    survivors = np.setdiff1d(np.arange(600), removed)
    fresh = device_build(np.ascontiguousarray(vectors[survivors]), "cos", "f32", 16, 32).index.search(queries, K, expansion=EXPANSION)
    print(f"tombstones: frontier {with_tombstones.stats.frontier} plain {with_tombstones.stats.plain}; compacted: frontier "
          f"{after.stats.frontier} plain {after.stats.plain}; fresh build: frontier {fresh.stats.frontier} plain {fresh.stats.plain}")
    assert (after.stats.frontier, after.stats.plain) == (fresh.stats.frontier, fresh.stats.plain)
    assert after.stats.frontier == 2, "a float pair without tombstones walks without a heap"


def test_compact_is_deterministic():
    metric, dtype, ndim, n, m, m0, vectors, removed, _ = case_inputs("one_wave_exactly")
    images = []
    for _ in range(2):
        built = device_build(vectors, metric, dtype, m, m0)
        built.remove(removed)
        built.compact(staging_bytes=5 * built.index.row_stride)
        images.append(built.save_buffer().tobytes())
    assert images[0] == images[1]


def test_a_restored_snapshot_compacts_too_and_old_filters_are_refused():
    """An index that came from an image with removed members (no builder behind it): `Index.compact` on the snapshot itself."""
    image, vectors, _ = util.build_image(500, 32, "cos", "f32", seed=45, connectivity=8, remove=range(1000, 1500, 3))
    index = usearch_amd.Index.restore(image)
    stale = index.filter_key_range(1000, 1200)
    lists, levels, keys, entry, _ = compact_model.read_image(image)
    model = compact_model.compact(lists, levels, keys, entry)
    queries = np.ascontiguousarray(vectors[:64])
    before = index.search(queries, K, expansion=EXPANSION)
    assert (before.stats.frontier, before.stats.plain) == (1, 0), "tombstones keep the index on the heap frontier"
    slot_map = index.compact(slot_map=True)
    assert slot_map.tolist() == model["slot_map"] and len(index) == len(model["keys"])
    assert index.compact_stats["pruned_edges"] == model["pruned_edges"]
    assert index.max_level == model["max_level"]
    # the brute-force scan sees exactly the survivors, each under its own key and with its own row
    exact = index.search(queries, K, exact=True)
    kept = np.array([keys[i] != FREE for i in range(64)])
    assert np.array_equal(exact.keys[kept, 0], np.array(keys[:64], dtype=np.uint64)[kept])
    assert not np.isin(exact.keys, 1000 + np.arange(0, 500, 3)).any(), "a removed member came back"
    after = index.search(queries, K, expansion=EXPANSION)
    assert after.stats.frontier == 2, "without tombstones a float pair walks without a heap"
    assert (after.keys == exact.keys).mean() > 0.9, "the compacted graph no longer finds the nearest members"
    with pytest.raises(RuntimeError):
        index.search(queries, K, filter=stale)
    fresh = index.filter_key_range(1000, 1200)
    filtered = index.search(queries, K, filter=fresh)
    found = filtered.keys[np.arange(K)[None, :] < filtered.counts[:, None]]
    assert len(found) and found.min() >= 1000 and found.max() <= 1200
